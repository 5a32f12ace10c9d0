"""Chunked admission of the continuous-batching scheduler (nanollama_amd/batch_serve.py, prefill_chunk > 0; --prefill-chunk):
every step is one forward_mixed_sample call -- the decoding requests as output rows, then up to N prompt tokens of the requests
being admitted -- so a running request gets a token in every step while prompts come in (go/main.go:160-166 feeds a prompt
before the first sample; go/serve.go:106-108 serves one request at a time).  A stand-in model records the calls.  No GPU."""
import threading
import time
from types import SimpleNamespace

import pytest

from nanollama_amd import cli
from nanollama_amd.batch_serve import BatchScheduler, RequestError
from nanollama_amd.engine import GenParams

EOS = 2


class FakeTokenizer:
    eos_id = EOS

    def encode(self, text, add_bos=True):
        return ([1] if add_bos else []) + [3 + (ord(c) % 40) for c in text]

    def decode_token_bytes(self, t):
        return bytes([97 + t % 26])


class FakeModel:
    """Records every call.  The id an output row samples is a function of the fed token alone (3 + (token + 1) % 40), so a
    greedy request's text does not depend on how its prompt reached the cache."""

    def __init__(self, max_streams=4, seq_len=128, max_rows=64, fail_call=None, delay=0.0):
        self.max_streams = max_streams
        self.config = SimpleNamespace(seq_len=seq_len, vocab_size=512)
        self.calls = []
        self.max_rows = max_rows
        self.fail_call = fail_call       # index of the mixed call that raises
        self.delay = delay
        self.n_mixed = 0

    @property
    def mixed_capacity(self):
        return self.max_rows, 64

    def reset(self, stream):
        self.calls.append(("reset", stream))

    def prefill(self, tokens, pos0=0, stream=0, want_logits=True):
        self.calls.append(("prefill", stream, list(tokens), pos0))

    def _sample(self, tokens, params, recents):
        ids = [3 + (t + 1) % 40 for t in tokens]
        return ids, [(list(r) + [i])[-p["rep_window"]:] if p["rep_window"] > 0 else [] for r, i, p in zip(recents, ids, params)]

    def forward_batch_sample(self, streams, tokens, pos, params, uniforms, recents):
        self.calls.append(("step", list(streams), list(tokens), list(pos)))
        return self._sample(tokens, params, recents)

    def forward_mixed_sample(self, streams, tokens, pos, n_out, params, uniforms, recents):
        if self.delay:
            time.sleep(self.delay)
        k, self.n_mixed = self.n_mixed, self.n_mixed + 1
        if k == self.fail_call:
            raise RuntimeError("injected engine failure")
        assert len(params) == len(uniforms) == len(recents) == n_out
        self.calls.append(("mixed", list(streams), list(tokens), list(pos), n_out))
        return self._sample(tokens[:n_out], params, recents)


def _serve(sched, prompts, params, stagger=None):
    """every prompt on its own thread; stagger(i): called before request i > 0 is submitted"""
    out, errs = [None] * len(prompts), [None] * len(prompts)

    def go(i):
        try:
            out[i] = sched.generate_quiet(prompts[i], params[i])
        except RequestError as exc:
            errs[i] = exc
    ths = []
    for i in range(len(prompts)):
        if i and stagger:
            stagger(i)
        ths.append(threading.Thread(target=go, args=(i,)))
        ths[-1].start()
    for t in ths:
        t.join(20)
    return out, errs


PROMPTS = ["abc", "hello", "x", "long prompt"]        # test_batch_serve.test_admission_prefill_and_rows_per_call's


def test_chunk_0_makes_the_calls_of_the_whole_prompt_scheduler():
    # one request after the other, so the order of the calls is fixed: reset, prefill of all but the last prompt token, then
    # one step per sampled id with the fed-back token
    tok = FakeTokenizer()
    m = FakeModel(max_streams=2)
    s = BatchScheduler(m, tok, 2, rep_penalty=1.15, rep_window=4, seed=5, prefill_chunk=0)
    want = []
    try:
        for i, p in enumerate(PROMPTS):
            text = s.generate_quiet(p, GenParams(max_tokens=3, temperature=0.0))
            assert len(text) == 3
            t = tok.encode(p)
            st = i % 2                                   # (a freed stream goes to the back of the free list)
            want += [("reset", st), ("prefill", st, t[:-1], 0)]
            fed, pos = t[-1], len(t) - 1
            for _ in range(3):
                want.append(("step", [st], [fed], [pos]))
                fed, pos = 3 + (fed + 1) % 40, pos + 1
    finally:
        s.close()
    assert m.calls == want
    assert s.prefill_chunk == 0 and s.steps == 12


def _audit(model, parallel, chunk):
    """the invariants of every mixed call and of a request's life; returns per stream the list of lives (dicts)"""
    lives, open_life, idx = [], {}, -1
    for c in model.calls:
        if c[0] == "reset":
            if c[1] in open_life:
                lives.append(open_life.pop(c[1]))
            open_life[c[1]] = dict(stream=c[1], fed=[], out=[])
            continue
        assert c[0] == "mixed", c
        _, streams, tokens, pos, n_out = c
        assert n_out <= parallel and len(streams) - n_out <= chunk
        assert len(set(streams[:n_out])) == n_out                       # output rows: one per request
        idx += 1
        for i, (s, t, p) in enumerate(zip(streams, tokens, pos)):
            life = open_life[s]
            if i < n_out:
                life["out"].append((idx, t, p))
            else:
                assert all(o[0] == idx for o in life["out"]), "a request that sampled in an earlier call has no prompt rows left"
                life["fed"].append((idx, t, p))
    lives += list(open_life.values())
    return lives


def test_chunk_8_feeds_every_prompt_token_once_and_keeps_decoding_rows_in_every_call():
    tok = FakeTokenizer()
    m = FakeModel(max_streams=3, delay=0.002)
    s = BatchScheduler(m, tok, 3, rep_penalty=1.15, rep_window=4, seed=5, prefill_chunk=8)
    long_prompt = "".join(chr(97 + i % 26) for i in range(49))          # 50 tokens with BOS
    prompts = ["ab", long_prompt, "xyz", "hijk"]

    def stagger(i):
        if i == 1:                                                      # the first request is decoding when the long prompt arrives
            t0 = time.time()
            while not any(c[0] == "mixed" for c in m.calls) and time.time() - t0 < 10:
                time.sleep(0.001)
    try:
        out, errs = _serve(s, prompts, [GenParams(max_tokens=40, temperature=0.0)] + [GenParams(max_tokens=5, temperature=0.0)] * 3, stagger)
    finally:
        s.close()
    assert errs == [None] * 4 and [len(o) for o in out] == [40, 5, 5, 5]
    assert not any(c[0] in ("prefill", "step") for c in m.calls)
    lives = _audit(m, 3, 8)
    assert len(lives) == 4
    by_prompt = {}
    for life in lives:
        # every prompt token but the last exactly once, at its own position, ascending and gap-free across calls
        toks = [t for _, t, _ in life["fed"]]
        assert [p for _, _, p in life["fed"]] == list(range(len(toks)))
        idxs = [i for i, _, _ in life["fed"]]
        assert idxs == sorted(idxs)
        whole = next(tok.encode(q) for q in prompts if tok.encode(q)[:-1] == toks)
        by_prompt[len(whole)] = life
        # the final prompt token is an output row in the call that feeds the last chunk
        first = life["out"][0]
        assert (first[1], first[2]) == (whole[-1], len(whole) - 1)
        if toks:
            assert first[0] == idxs[-1]
        # from then on an output row in EVERY call until its last, at consecutive positions
        calls = [i for i, _, _ in life["out"]]
        assert calls == list(range(calls[0], calls[0] + len(calls)))
        assert [p for _, _, p in life["out"]] == list(range(first[2], first[2] + len(calls)))
    # the 50-token prompt took ceil(49 / 8) = 7 calls, all of them while the first request decoded
    big, first_req = by_prompt[50], by_prompt[3]
    span = sorted({i for i, _, _ in big["fed"]})
    assert len(span) >= 7
    decoding_calls = {i for i, _, _ in first_req["out"]}
    assert set(span) <= decoding_calls
    # short prompts share one call's budget: "xyz" (3 rows) and "hijk" (4 rows) were fed beside other prompt rows
    mixed = [c for c in m.calls if c[0] == "mixed"]
    assert any(len(set(c[1][c[4]:])) >= 2 for c in mixed)
    assert s.max_step_gap_ms > 0.0


def test_greedy_texts_do_not_depend_on_the_chunk():
    tok = FakeTokenizer()
    texts = {}
    for chunk in (0, 8):
        m = FakeModel(max_streams=2)
        s = BatchScheduler(m, tok, 2, rep_penalty=1.15, rep_window=4, seed=5, prefill_chunk=chunk)
        try:
            out, errs = _serve(s, PROMPTS + ["a considerably longer prompt than the chunk"], [GenParams(max_tokens=7, temperature=0.0)] * 5)
        finally:
            s.close()
        assert errs == [None] * 5
        texts[chunk] = out
    assert texts[0] == texts[8] and all(len(t) == 7 for t in texts[0])


def test_sampled_rows_draw_uniforms_only_for_output_rows_with_temperature():
    class Rec(FakeModel):
        def forward_mixed_sample(self, streams, tokens, pos, n_out, params, uniforms, recents):
            self.us = getattr(self, "us", []) + [(float(u), p["temperature"]) for u, p in zip(uniforms, params)]
            return super().forward_mixed_sample(streams, tokens, pos, n_out, params, uniforms, recents)
    m = Rec(max_streams=2)
    s = BatchScheduler(m, FakeTokenizer(), 2, seed=5, prefill_chunk=8)
    try:
        out, errs = _serve(s, ["abcdefghijklmnop", "xy"], [GenParams(max_tokens=4, temperature=0.0), GenParams(max_tokens=4, temperature=0.9)])
    finally:
        s.close()
    assert errs == [None, None]
    assert all(u == 0.0 for u, t in m.us if t <= 0) and sum(1 for u, t in m.us if t > 0) == 4


def test_a_failing_mixed_call_fails_its_requests_and_the_next_is_served():
    tok = FakeTokenizer()
    m = FakeModel(max_streams=2, fail_call=2, delay=0.002)
    s = BatchScheduler(m, tok, 2, seed=5, prefill_chunk=8)

    def stagger(i):
        t0 = time.time()
        while m.n_mixed < 1 and time.time() - t0 < 10:
            time.sleep(0.001)
    try:
        # the first request decodes, the second is being admitted (30 rows: four calls) when call 2 raises
        out, errs = _serve(s, ["ab", "a prompt of thirty tokens, almost"], [GenParams(max_tokens=30, temperature=0.0)] * 2, stagger)
        assert [e.status for e in errs] == [500, 500] and "injected" in str(errs[0])
        assert len(s.generate_quiet("next", GenParams(max_tokens=3, temperature=0.0))) == 3
    finally:
        s.close()
    # close() fails what is pending
    gate = threading.Event()

    class Held(FakeModel):
        def forward_mixed_sample(self, *a):
            gate.wait(10)
            return super().forward_mixed_sample(*a)
    m = Held(max_streams=1)
    s = BatchScheduler(m, tok, 1, seed=5, prefill_chunk=8)
    res = []

    def go(p):
        try:
            res.append(s.generate_quiet(p, GenParams(max_tokens=50, temperature=0.0)))
        except RequestError as exc:
            res.append(exc)
    ths = [threading.Thread(target=go, args=(p,)) for p in ("one", "two")]
    for t in ths:
        t.start()
    time.sleep(0.05)
    closer = threading.Thread(target=s.close)
    closer.start()
    time.sleep(0.05)
    gate.set()
    closer.join(10)
    for t in ths:
        t.join(10)
    assert len(res) == 2 and all(isinstance(r, RequestError) and r.status == 500 for r in res)


def test_rows_of_one_step_must_fit_the_handle():
    with pytest.raises(ValueError, match="64"):
        BatchScheduler(FakeModel(max_streams=4, max_rows=64), FakeTokenizer(), 4, prefill_chunk=61)
    BatchScheduler(FakeModel(max_streams=4, max_rows=64), FakeTokenizer(), 4, prefill_chunk=60).close()
    with pytest.raises(ValueError):
        BatchScheduler(FakeModel(), FakeTokenizer(), 2, prefill_chunk=-1)


def test_cli_prefill_chunk_flag():
    ap = cli.build_parser()
    assert ap.parse_args(["--model", "m"]).prefill_chunk == 0
    args = ap.parse_args(["--model", "m", "--serve", "--parallel", "16", "--prefill-chunk", "64"])
    assert args.prefill_chunk == 64
    cli.check_prefill_chunk(args)
    cli.check_prefill_chunk(args, 320)
    with pytest.raises(RuntimeError, match="320"):
        cli.check_prefill_chunk(ap.parse_args(["--model", "m", "--serve", "--parallel", "16", "--prefill-chunk", "305"]), 320)
    with pytest.raises(RuntimeError, match="512"):
        cli.check_prefill_chunk(ap.parse_args(["--model", "m", "--serve", "--parallel", "16", "--prefill-chunk", "500"]))
    for argv in (["--model", "m", "--serve", "--prefill-chunk", "8"], ["--model", "m", "--parallel", "4", "--prefill-chunk", "8"],
                 ["--model", "m", "--serve", "--parallel", "1", "--prefill-chunk", "8"]):
        with pytest.raises(RuntimeError, match="--parallel"):
            cli.check_prefill_chunk(ap.parse_args(argv))
    # main() reports it like the other flag errors: exit status 1, no model is opened
    assert cli.main(["--model", "/nonexistent.gguf", "--serve", "--prefill-chunk", "8"]) == 1
