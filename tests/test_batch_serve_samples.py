"""Several samples of one prompt through the scheduler (BatchScheduler.generate_samples, "n" in POST /chat, --samples) with a
stand-in model that records every call, kv_fork included: one prefill and one fork per request, rows that share the first
step, generators in sample order, first-in-first-out admission of a request that needs several streams, failures, chunked
admission.  No GPU."""
import contextlib
import json
import threading
import time
import urllib.error
import urllib.request
from http.server import ThreadingHTTPServer
from types import SimpleNamespace

import pytest

from nanollama_amd import cli, serve
from nanollama_amd.batch_serve import BatchScheduler, RequestError
from nanollama_amd.engine import GenParams

EOS = 2
NOLOCK = contextlib.nullcontext()


class FakeTokenizer:
    eos_id = EOS

    def encode(self, text, add_bos=True):
        return ([1] if add_bos else []) + [3 + (ord(c) % 40) for c in text]

    def decode_token_bytes(self, t):
        return bytes([97 + t % 26])


class FakeModel:
    """Records every call.  A sampled row's id is 3 + the first digits of its uniform, a greedy row's is token + 1; a row
    whose stream is in `eos_once` samples EOS (once), and so does one whose stream's `hold` event is set."""

    def __init__(self, max_streams=4, seq_len=64, fail=None, delay=0.0):
        self.max_streams = max_streams
        self.config = SimpleNamespace(seq_len=seq_len, vocab_size=512, num_layers=1, embed_dim=8, num_heads=1,
                                      num_kv_heads=1, head_dim=8, interm_size=8, qk_norm=False, rope_conjugate=False)
        self.gamma = None
        self.calls = []
        self.fail = fail              # "prefill" / "kv_fork": that call raises once
        self.eos_once = set()
        self.delay = delay            # seconds per step: rows that decode "until released" stay far from the output cap
        self.gate = None              # threading.Event: a step waits for it
        self.hold = {}                # stream -> threading.Event: once set, the next step that carries the stream samples EOS on it
        self.mixed_capacity = (512, 64)

    def reset(self, stream):
        self.calls.append(("reset", stream))

    def prefill(self, tokens, pos0=0, stream=0, want_logits=True):
        if self.fail == "prefill":
            self.fail = None
            raise RuntimeError("injected prefill failure")
        self.calls.append(("prefill", stream, list(tokens), pos0))

    def kv_fork(self, src, dsts, n_pos):
        if self.fail == "kv_fork":
            self.fail = None
            raise RuntimeError("injected fork failure")
        self.calls.append(("kv_fork", src, list(dsts), n_pos))

    def _sample(self, streams, tokens, params, uniforms, recents):
        ids, outs = [], []
        for s, t, p, u, rec in zip(streams, tokens, params, uniforms, recents):
            if s in self.eos_once or (s in self.hold and self.hold[s].is_set()):
                self.eos_once.discard(s)
                self.hold.pop(s, None)                           # (the stream's next request decodes freely)
                nxt = EOS
            elif p["temperature"] > 0:
                nxt = 3 + int(float(u) * 1000) % 40
            else:
                nxt = 3 + (t + 1) % 40
            ids.append(nxt)
            outs.append((list(rec) + [nxt])[-p["rep_window"]:] if p["rep_window"] > 0 else [])
        return ids, outs

    def forward_batch_sample(self, streams, tokens, pos, params, uniforms, recents):
        if self.gate is not None:
            self.gate.wait(5)
        if self.delay:
            time.sleep(self.delay)
        assert len(set(streams)) == len(streams) <= self.max_streams
        self.calls.append(("step", list(streams), list(tokens), list(pos), [float(u) for u in uniforms]))
        return self._sample(streams, tokens, params, uniforms, recents)

    def forward_mixed_sample(self, streams, tokens, pos, n_out, params, uniforms, recents):
        assert len(params) == len(uniforms) == len(recents) == n_out
        self.calls.append(("mixed", list(streams), list(tokens), list(pos), n_out))
        return self._sample(streams[:n_out], tokens[:n_out], params, uniforms, recents)


def _sched(model, parallel=4, seed=5, **kw):
    return BatchScheduler(model, FakeTokenizer(), parallel, rep_penalty=1.15, rep_window=4, seed=seed, **kw)


def _wait(cond, seconds=5.0):
    t0 = time.time()
    while not cond() and time.time() - t0 < seconds:
        time.sleep(0.001)
    assert cond()


def test_three_samples_one_prefill_one_fork_and_a_shared_first_step():
    m = FakeModel()
    s = _sched(m)
    try:
        texts = s.generate_samples("hello", GenParams(max_tokens=5, temperature=0.8), 3)
    finally:
        s.close()
    toks = FakeTokenizer().encode("hello")
    n_prompt = len(toks)
    assert [c for c in m.calls if c[0] == "prefill"] == [("prefill", 0, toks[:-1], 0)]
    forks = [c for c in m.calls if c[0] == "kv_fork"]
    assert forks == [("kv_fork", 0, [1, 2], n_prompt - 1)]
    # reset and prefill of the leader, then the fork, then the steps; the siblings are never reset or prefilled by the scheduler
    assert m.calls[:3] == [("reset", 0), ("prefill", 0, toks[:-1], 0), forks[0]]
    assert [c for c in m.calls if c[0] == "reset"] == [("reset", 0)]
    first = m.calls[3]
    assert first[0] == "step" and first[1] == [0, 1, 2]
    assert first[2] == [toks[-1]] * 3 and first[3] == [n_prompt - 1] * 3
    assert len(set(first[4])) == 3                               # each row draws from its own generator
    assert isinstance(texts, list) and len(texts) == 3 and all(len(t) == 5 for t in texts)
    # sample order: text i is what stream i sampled (3 + the uniform's digits, as a letter)
    steps = [c for c in m.calls if c[0] == "step"]
    for i in range(3):
        ids = [3 + int(c[4][c[1].index(i)] * 1000) % 40 for c in steps if i in c[1]]
        assert texts[i] == "".join(chr(97 + t % 26) for t in ids)


def test_one_sample_makes_the_calls_of_a_single_request_and_shares_the_leaders_generator():
    toks = FakeTokenizer().encode("hello")
    p = GenParams(max_tokens=4, temperature=0.8)
    runs = {}
    for how in ("quiet", "n1", "n3"):
        m = FakeModel()
        s = _sched(m, seed=9)
        try:
            if how == "quiet":
                out = [s.generate_quiet("hello", p)]
            else:
                out = s.generate_samples("hello", p, 1 if how == "n1" else 3)
        finally:
            s.close()
        runs[how] = (m.calls, out)
    for how in ("quiet", "n1"):
        calls = runs[how][0]
        assert not [c for c in calls if c[0] == "kv_fork"]
        # the rule of a single request: reset, prefill of tokens 0 .. n_prompt - 2, then one one-row step per sampled id
        assert calls[:2] == [("reset", 0), ("prefill", 0, toks[:-1], 0)]
        assert [c[0] for c in calls[2:]] == ["step"] * 4
        assert [(c[1], c[3]) for c in calls[2:]] == [([0], [len(toks) - 1 + i]) for i in range(4)]
        assert calls[2][2] == [toks[-1]]
    assert runs["quiet"] == runs["n1"]
    lead = lambda calls: [c[4][c[1].index(0)] for c in calls if c[0] == "step"]
    assert lead(runs["n1"][0]) == lead(runs["n3"][0]) and len(lead(runs["n1"][0])) == 4
    assert runs["n1"][1][0] == runs["n3"][1][0]


def test_a_row_that_ends_early_frees_its_stream_while_its_siblings_go_on():
    m = FakeModel(max_streams=3, seq_len=10 ** 9, delay=0.001)
    m.eos_once = {1}                                          # sample 1 meets EOS in its first step
    m.hold = {0: threading.Event(), 2: threading.Event()}        # samples 0 and 2 decode until released
    s = _sched(m, parallel=3)
    res = {}
    try:
        a = threading.Thread(target=lambda: res.__setitem__("a", s.generate_samples("abc", GenParams(max_tokens=10 ** 6, temperature=0.0), 3)))
        a.start()
        _wait(lambda: any(c[0] == "step" for c in m.calls))
        # a waiting request gets stream 1 while samples 0 and 2 are still decoding
        b = s.generate_quiet("q", GenParams(max_tokens=2, temperature=0.0))
        assert len(b) == 2 and "a" not in res and a.is_alive()
        assert ("reset", 1) in m.calls
        shared = [c for c in m.calls if c[0] == "step" and 1 in c[1]][-1]
        assert 0 in shared[1] and 2 in shared[1]                 # ... in steps that also carry the siblings
        m.hold[0].set()
        _wait(lambda: any(c[0] == "step" and 0 not in c[1] and 2 in c[1] for c in m.calls))
        assert "a" not in res                                    # two rows done, one to go: the request has not returned
        m.hold[2].set()
        a.join(10)
    finally:
        for ev in list(m.hold.values()):
            ev.set()
        s.close()
    assert len(res["a"]) == 3 and res["a"][1] == ""              # the EOS is not emitted


def test_a_request_of_three_waits_for_three_streams_and_nothing_overtakes_it():
    m = FakeModel(max_streams=4, seq_len=10 ** 9, delay=0.001)
    m.hold = {0: threading.Event(), 1: threading.Event()}
    s = _sched(m, parallel=4)
    long = GenParams(max_tokens=10 ** 6, temperature=0.0)
    res = {}

    def go(key, fn):
        th = threading.Thread(target=lambda: res.__setitem__(key, fn()))
        th.start()
        return th
    try:
        r0 = go("r0", lambda: s.generate_quiet("a", long))
        _wait(lambda: ("reset", 0) in m.calls)
        r1 = go("r1", lambda: s.generate_quiet("b", long))
        _wait(lambda: ("reset", 1) in m.calls)
        big = go("big", lambda: s.generate_samples("cde", GenParams(max_tokens=3, temperature=0.0), 3))
        _wait(lambda: len(s._queue) == 1)
        small = go("small", lambda: s.generate_quiet("f", GenParams(max_tokens=2, temperature=0.0)))
        _wait(lambda: len(s._queue) == 2)
        n_steps = lambda: sum(1 for c in m.calls if c[0] == "step")
        k = n_steps()
        _wait(lambda: n_steps() >= k + 3)
        # two streams are free and the later one-row request would fit, but the head of the queue needs three: both wait
        assert len(s._queue) == 2 and not [c for c in m.calls if c[0] == "kv_fork"]
        assert [c for c in m.calls if c[0] == "reset"] == [("reset", 0), ("reset", 1)]
        m.hold[0].set()                                          # the first request ends: three streams are free
        big.join(10)
        small.join(10)
        # the request of three was admitted first (its leader's reset, its fork), the later request behind it
        order = [c for c in m.calls if c[0] in ("reset", "kv_fork")]
        assert [c[0] for c in order] == ["reset", "reset", "reset", "kv_fork", "reset"]
        assert order[3][1] == order[2][1] and sorted([order[3][1]] + order[3][2]) == [0, 2, 3]
        assert len(res["big"]) == 3 and all(len(t) == 3 for t in res["big"]) and len(res["small"]) == 2
        m.hold[1].set()
        r0.join(10)
        r1.join(10)
    finally:
        for ev in list(m.hold.values()):
            ev.set()
        s.close()


def test_bad_n_is_400_through_the_scheduler_and_over_http_and_responses_only_for_n_above_one():
    m = FakeModel()
    s = _sched(m, parallel=4)
    srv = ThreadingHTTPServer(("127.0.0.1", 0), serve.make_handler(s, GenParams(max_tokens=3, temperature=0.6)))
    th = threading.Thread(target=srv.serve_forever, daemon=True)
    th.start()
    base = f"http://127.0.0.1:{srv.server_address[1]}"

    def post(body):
        req = urllib.request.Request(base + "/chat", data=json.dumps(body).encode(), method="POST")
        try:
            with urllib.request.urlopen(req, timeout=10) as r:
                return r.status, json.loads(r.read())
        except urllib.error.HTTPError as exc:
            return exc.code, json.loads(exc.read())
    try:
        for bad in (5, 0, "x", -1, 2.0, True):
            with pytest.raises(RequestError) as ei:
                s.generate_samples("hi", GenParams(max_tokens=3), bad)
            assert ei.value.status == 400
            st, out = post({"messages": [{"role": "user", "content": "hi"}], "n": bad})
            assert st == 400 and set(out) == {"error"}, (bad, st, out)
        assert not m.calls                                       # nothing reached the engine
        st, out = post({"messages": [{"role": "user", "content": "hi"}], "n": 3})
        assert st == 200 and set(out) == {"response", "responses"}
        assert len(out["responses"]) == 3 and out["response"] == out["responses"][0] and all(len(t) == 3 for t in out["responses"])
        for body in ({"messages": [{"role": "user", "content": "hi"}]}, {"messages": [{"role": "user", "content": "hi"}], "n": 1}):
            st, out = post(body)
            assert st == 200 and set(out) == {"response"}
        with urllib.request.urlopen(base + "/health", timeout=10) as r:
            assert json.loads(r.read())["max_samples"] == 4
    finally:
        srv.shutdown()
        srv.server_close()
        s.close()
    # the serial server: one sample at a time, and the refusal says how to get more
    eng = SimpleNamespace(model=SimpleNamespace(voices={}), generate_quiet=lambda p, q: "echo")
    st, out = serve.handle_chat(eng, GenParams(), NOLOCK, b'{"messages":[{"content":"x"}],"n":2}')
    assert st == 400 and "--parallel" in out["error"]
    assert serve.handle_chat(eng, GenParams(), NOLOCK, b'{"messages":[{"content":"x"}],"n":1}') == (200, {"response": "echo"})


@pytest.mark.parametrize("what", ["prefill", "kv_fork"])
def test_a_failing_prefill_or_fork_is_a_500_that_frees_every_stream(what):
    m = FakeModel(max_streams=3, fail=what)
    s = _sched(m, parallel=3)
    try:
        with pytest.raises(RequestError) as ei:
            s.generate_samples("hello", GenParams(max_tokens=3, temperature=0.5), 3)
        assert ei.value.status == 500 and "injected" in str(ei.value)
        assert not [c for c in m.calls if c[0] == "step"]
        # all three streams are back: the next request of three is served
        texts = s.generate_samples("hello", GenParams(max_tokens=3, temperature=0.5), 3)
        assert len(texts) == 3 and all(len(t) == 3 for t in texts)
        assert sorted([c for c in m.calls if c[0] == "kv_fork"][-1][2] + [[c for c in m.calls if c[0] == "kv_fork"][-1][1]]) == [0, 1, 2]
    finally:
        s.close()


def test_chunked_admission_forks_behind_the_leaders_last_chunk():
    m = FakeModel()
    s = _sched(m, prefill_chunk=4)
    prompt = "a prompt!!"                                        # 11 tokens: chunks of 4, 4 and 2, the final token an output row
    toks = FakeTokenizer().encode(prompt)
    try:
        texts = s.generate_samples(prompt, GenParams(max_tokens=4, temperature=0.7), 3)
    finally:
        s.close()
    assert len(texts) == 3 and all(len(t) == 4 for t in texts)
    assert not [c for c in m.calls if c[0] in ("prefill", "step")]
    fork = [i for i, c in enumerate(m.calls) if c[0] == "kv_fork"]
    assert len(fork) == 1 and m.calls[fork[0]] == ("kv_fork", 0, [1, 2], len(toks) - 1)
    before, after = m.calls[fork[0] - 1], m.calls[fork[0] + 1]
    # the step before the fork carried the leader's last chunk, and its final prompt token as the only output row
    assert before[0] == "mixed" and before[4] == 1 and before[1][0] == 0 and before[3][0] == len(toks) - 1
    assert before[3][1:] == [8, 9] and set(before[1]) == {0}
    assert all(c[4] == 0 for c in m.calls[:fork[0] - 1] if c[0] == "mixed")
    # the siblings' first rows are in the step after it: the final prompt token at n_prompt - 1, next to the leader's second row
    assert after[0] == "mixed" and after[4] == 3 and after[1] == [0, 1, 2]
    assert after[2][1:] == [toks[-1]] * 2 and after[3] == [len(toks), len(toks) - 1, len(toks) - 1]
    # an injected fork failure behind the last chunk: 500, all streams free again
    m = FakeModel(max_streams=3, fail="kv_fork")
    s = _sched(m, parallel=3, prefill_chunk=4)
    try:
        with pytest.raises(RequestError) as ei:
            s.generate_samples(prompt, GenParams(max_tokens=4, temperature=0.7), 3)
        assert ei.value.status == 500
        assert len(s.generate_samples(prompt, GenParams(max_tokens=2, temperature=0.7), 3)) == 3
    finally:
        s.close()


def test_samples_flag_parsing_and_usage_errors(capsys):
    a = cli.build_parser().parse_args(["--model", "m.gguf", "--prompt", "hi"])
    assert a.samples == 1
    cli.check_samples(a)
    a = cli.build_parser().parse_args(["--model", "m.gguf", "--prompt", "hi", "--samples", "4", "--seed", "1"])
    assert a.samples == 4 and a.seed == 1
    cli.check_samples(a)
    for bad in (["--prompt", "hi", "--samples", "0"], ["--prompt", "hi", "--samples", "65"], ["--samples", "2"],
                ["--prompt", "hi", "--samples", "2", "--interactive"], ["--samples", "2", "--score", "t.txt"],
                ["--prompt", "hi", "--samples", "2", "--gpus", "2"], ["--prompt", "hi", "--samples", "2", "--serve"]):
        with pytest.raises(RuntimeError):
            cli.check_samples(cli.build_parser().parse_args(["--model", "m.gguf"] + bad))
    # a usage error ends main before the model is touched
    assert cli.main(["--model", "/nonexistent.gguf", "--prompt", "hi", "--samples", "2", "--interactive"]) == 1
    assert "--samples" in capsys.readouterr().err
    # --samples N prints the completions in order, each under its header
    eng = SimpleNamespace(model=FakeModel(), tokenizer=FakeTokenizer())
    eng.model.voices = {}
    a = cli.build_parser().parse_args(["--model", "m.gguf", "--prompt", "hi", "--samples", "3", "--seed", "1", "--max-tokens", "4"])
    cli.run_samples(eng, a.prompt, GenParams(max_tokens=4, temperature=0.8), a)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0::2] == ["--- sample 0 ---", "--- sample 1 ---", "--- sample 2 ---"] and all(len(t) == 4 for t in lines[1::2])
    assert len([c for c in eng.model.calls if c[0] == "prefill"]) == 1
