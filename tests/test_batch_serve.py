"""The continuous-batching scheduler behind POST /chat (nanollama_amd/batch_serve.py) driven with a stand-in model: admission,
stop rules, request settings, generators, errors, and the --parallel flag.  No GPU."""
import contextlib
import json
import threading
import urllib.request
from http.server import ThreadingHTTPServer
from types import SimpleNamespace

import numpy as np
import pytest

from nanollama_amd import cli, serve
from nanollama_amd.batch_serve import BatchScheduler, RequestError
from nanollama_amd.engine import GenParams

EOS = 2
NOLOCK = contextlib.nullcontext()


class FakeTokenizer:
    eos_id = EOS

    def __init__(self, piece_len=1):
        self.piece_len = piece_len

    def encode(self, text, add_bos=True):
        return ([1] if add_bos else []) + [3 + (ord(c) % 40) for c in text]

    def decode_token_bytes(self, t):
        return bytes([97 + t % 26]) * self.piece_len


class FakeModel:
    """Records every call; the id a row samples is a function of (stream, token, pos, uniform): EOS when the fed token is
    `eos_after`, else 3 + the uniform's first digits (sampled rows) or token + 1 (greedy rows)."""

    def __init__(self, max_streams=4, seq_len=64, vocab=512, eos_after=None, fail_prefill_len=None):
        self.max_streams = max_streams
        self.config = SimpleNamespace(seq_len=seq_len, vocab_size=vocab, num_layers=1, embed_dim=8, num_heads=1,
                                      num_kv_heads=1, head_dim=8, interm_size=8, qk_norm=False, rope_conjugate=False)
        self.gamma = None
        self.calls = []
        self.eos_after = eos_after
        self.fail_prefill_len = fail_prefill_len
        self.max_rows = 0
        self.gate = None          # threading.Event: forward_batch_sample waits for it (concurrency tests)

    def reset(self, stream):
        self.calls.append(("reset", stream))

    def prefill(self, tokens, pos0=0, stream=0, want_logits=True):
        if self.fail_prefill_len is not None and len(tokens) == self.fail_prefill_len:
            raise RuntimeError("injected engine failure")
        self.calls.append(("prefill", stream, list(tokens), pos0))

    def forward_batch_sample(self, streams, tokens, pos, params, uniforms, recents):
        if self.gate is not None:
            self.gate.wait(5)
        assert len(set(streams)) == len(streams) <= self.max_streams
        self.max_rows = max(self.max_rows, len(streams))
        self.calls.append(("step", list(streams), list(tokens), list(pos), [dict(p) for p in params],
                           [float(u) for u in uniforms]))
        ids, outs = [], []
        for t, p, u, rec, q in zip(tokens, params, uniforms, recents, pos):
            if self.eos_after is not None and t == self.eos_after:
                nxt = EOS
            elif p["temperature"] > 0:
                nxt = 3 + int(float(u) * 1000) % 40
            else:
                nxt = 3 + (t + 1) % 40
            ids.append(nxt)
            r = list(rec) + [nxt]
            outs.append(r[-p["rep_window"]:] if p["rep_window"] > 0 else [])
        return ids, outs


def _run(model, prompts, params, parallel=4, seed=5, tok=None):
    s = BatchScheduler(model, tok or FakeTokenizer(), parallel, rep_penalty=1.15, rep_window=4, seed=seed)
    try:
        out = [None] * len(prompts)
        errs = [None] * len(prompts)

        def go(i):
            try:
                out[i] = s.generate_quiet(prompts[i], params[i])
            except RequestError as exc:
                errs[i] = exc
        ths = [threading.Thread(target=go, args=(i,)) for i in range(len(prompts))]
        for t in ths:
            t.start()
        for t in ths:
            t.join(10)
        return out, errs
    finally:
        s.close()


def test_admission_prefill_and_rows_per_call():
    m = FakeModel(max_streams=2)
    prompts = ["abc", "hello", "x", "long prompt"]
    out, errs = _run(m, prompts, [GenParams(max_tokens=3, temperature=0.0)] * 4, parallel=2)
    assert errs == [None] * 4 and all(len(o) == 3 for o in out)
    assert m.max_rows <= 2
    tok = FakeTokenizer()
    for i, c in enumerate(m.calls):
        if c[0] == "prefill":                      # reset of that stream right before its prefill
            assert m.calls[i - 1] == ("reset", c[1])
    prefills = [c for c in m.calls if c[0] == "prefill"]
    assert sorted(len(c[2]) for c in prefills) == sorted(len(tok.encode(p)) - 1 for p in prompts)
    assert all(c[3] == 0 for c in prefills)
    # streams are reused (4 requests, 2 streams): every admission resets
    assert sum(1 for c in m.calls if c[0] == "reset") == 4
    # the first step after a stream's prefill feeds the request's last prompt token at position n_prompt - 1
    last = {}
    for c in m.calls:
        if c[0] == "prefill":
            last[c[1]] = c[2]
        elif c[0] == "step":
            for s, t, p in zip(c[1], c[2], c[3]):
                if s in last:
                    whole = next(tok.encode(q) for q in prompts if tok.encode(q)[:-1] == last[s])
                    assert (t, p) == (whole[-1], len(whole) - 1)
                    del last[s]


def test_stop_rules():
    # EOS ends the request and is not emitted
    m = FakeModel(eos_after=28)        # greedy ids from prompt "a" (last token 20): 24, 28, then EOS
    out, _ = _run(m, ["a"], [GenParams(max_tokens=50, temperature=0.0)])
    ids = []
    t = FakeTokenizer().encode("a")[-1]
    while True:
        nxt = EOS if t == m.eos_after else 3 + (t + 1) % 40
        if nxt == EOS or len(ids) == 50:
            break
        ids.append(nxt)
        t = nxt
    assert ids == [24, 28] and out[0] == "".join(chr(97 + i % 26) for i in ids)
    assert sum(len(c[1]) for c in m.calls if c[0] == "step") == 3          # the EOS was sampled, not emitted
    # max_tokens
    out, _ = _run(FakeModel(), ["ab"], [GenParams(max_tokens=5, temperature=0.0)])
    assert len(out[0]) == 5
    # the end of the context: positions up to seq_len - 2 are fed, as Engine.generate_ids samples seq_len - n_prompt ids
    m = FakeModel(seq_len=16)
    out, _ = _run(m, ["abcd"], [GenParams(max_tokens=500, temperature=0.0)])
    n_prompt = len(FakeTokenizer().encode("abcd"))
    assert len(out[0]) == 16 - n_prompt
    assert max(p for c in m.calls if c[0] == "step" for p in c[3]) == 16 - 2
    # the 8192-byte output cap: the piece that crosses it is the last
    out, _ = _run(FakeModel(seq_len=4096), ["a"], [GenParams(max_tokens=4000, temperature=0.0)], tok=FakeTokenizer(piece_len=1000))
    assert len(out[0]) == 9000


def test_request_overrides_and_400():
    m = FakeModel()
    s = BatchScheduler(m, FakeTokenizer(), 4, rep_penalty=1.3, rep_window=8, seed=1)
    try:
        d = GenParams(max_tokens=4, temperature=0.8, top_p=0.95, top_k=50)
        st, out = serve.handle_chat(s, d, NOLOCK, b'{"messages":[{"content":"x"}],"temperature":0.5,"max_tokens":2,"top_k":7}')
        assert st == 200 and len(out["response"]) == 2
        step = [c for c in m.calls if c[0] == "step"][-1]
        assert step[4][0] == dict(temperature=0.5, top_p=0.95, top_k=7, rep_penalty=np.float32(1.3), rep_window=8)
        # values <= 0 keep the server's (go/serve.go:94-103)
        st, out = serve.handle_chat(s, d, NOLOCK, b'{"messages":[{"content":"x"}],"temperature":0,"max_tokens":0,"top_k":-1}')
        assert st == 200 and len(out["response"]) == 4
        assert [c for c in m.calls if c[0] == "step"][-1][4][0]["temperature"] == 0.8
        # top_k > 1024 with top_p >= 1: the device sampler cannot serve it
        d1 = GenParams(max_tokens=4, temperature=0.8, top_p=1.0, top_k=50)
        st, out = serve.handle_chat(s, d1, NOLOCK, b'{"messages":[{"content":"x"}],"top_k":2000}')
        assert st == 400 and "top_k" in out
        st, out = serve.handle_chat(s, d1, NOLOCK, b'{"messages":[{"content":"x"}],"top_k":1024}')
        assert st == 200
    finally:
        s.close()


def test_same_seed_same_outputs_and_uniforms_only_when_sampling():
    params = [GenParams(max_tokens=6, temperature=0.9), GenParams(max_tokens=6, temperature=0.0),
              GenParams(max_tokens=6, temperature=0.7)]
    runs = []
    for seed in (11, 11, 12):
        m = FakeModel()
        m.gate = threading.Event()
        s = BatchScheduler(m, FakeTokenizer(), 4, rep_window=4, seed=seed)
        res = [None] * 3
        ths = []
        for i in range(3):                        # a fixed arrival order: each request queued before the next starts
            ths.append(threading.Thread(target=lambda i=i: res.__setitem__(i, s.generate_quiet("p%d" % i, params[i]))))
            ths[-1].start()
            for _ in range(400):                  # queued or admitted (an admission resets a stream)
                with s._cv:
                    if len(s._queue) + sum(1 for c in m.calls if c[0] == "reset") >= i + 1:
                        break
                threading.Event().wait(0.005)
        m.gate.set()
        for t in ths:
            t.join(10)
        s.close()
        runs.append(res)
        for c in m.calls:
            if c[0] == "step":
                for p, u in zip(c[4], c[5]):
                    if p["temperature"] <= 0:
                        assert u == 0.0
    assert runs[0] == runs[1]
    assert runs[0] != runs[2]


def test_one_failing_request_does_not_stop_the_others():
    tok = FakeTokenizer()
    bad = "zzz"
    m = FakeModel(fail_prefill_len=len(tok.encode(bad)) - 1)
    out, errs = _run(m, ["ab", bad, "abcdef", "q"], [GenParams(max_tokens=3, temperature=0.5)] * 4)
    assert errs[1] is not None and errs[1].status == 500 and out[1] is None
    assert [errs[i] for i in (0, 2, 3)] == [None] * 3 and all(len(out[i]) == 3 for i in (0, 2, 3))
    st, payload = serve.handle_chat(SimpleNamespace(generate_quiet=lambda p, q: (_ for _ in ()).throw(RequestError(500, "boom"))),
                                    GenParams(), NOLOCK, b'{"messages":[{"content":"x"}]}')
    assert (st, payload) == (500, "boom")


def test_parallel_flag():
    a = cli.build_parser().parse_args(["--model", "m.gguf", "--serve"])
    assert a.parallel == 1 and not cli.batched(a)           # the default: today's serial server
    cli.check_parallel(a)
    a = cli.build_parser().parse_args(["--model", "m.gguf", "--serve", "--parallel", "64"])
    assert cli.batched(a)
    cli.check_parallel(a)
    for bad in (["--parallel", "0"], ["--parallel", "65"], ["--parallel", "4", "--gpus", "2"],
                ["--parallel", "4", "--rep-window", "2000"]):
        with pytest.raises(RuntimeError):
            cli.check_parallel(cli.build_parser().parse_args(["--model", "m.gguf", "--serve"] + bad))
    assert cli.main(["--model", "/nonexistent.gguf", "--serve", "--parallel", "65"]) == 1
    assert not cli.batched(cli.build_parser().parse_args(["--model", "m.gguf", "--parallel", "8"]))   # (no --serve)
    with pytest.raises(ValueError):
        BatchScheduler(FakeModel(max_streams=2), FakeTokenizer(), 4)                  # more rows than streams
    with pytest.raises(ValueError):
        BatchScheduler(FakeModel(vocab=200000), FakeTokenizer(), 2)


def test_http_requests_run_concurrently_without_the_lock():
    m = FakeModel(max_streams=4)
    s = BatchScheduler(m, FakeTokenizer(), 4, seed=3)
    srv = ThreadingHTTPServer(("127.0.0.1", 0), serve.make_handler(s, GenParams(max_tokens=3, temperature=0.6)))
    th = threading.Thread(target=srv.serve_forever, daemon=True)
    th.start()
    port = srv.server_address[1]
    try:
        m.gate = threading.Event()
        res = [None] * 4

        def post(i):
            req = urllib.request.Request(f"http://127.0.0.1:{port}/chat", data=json.dumps(
                {"messages": [{"role": "user", "content": "hi %d" % i}]}).encode(), method="POST")
            with urllib.request.urlopen(req, timeout=10) as r:
                res[i] = (r.status, json.loads(r.read()))
        ths = [threading.Thread(target=post, args=(i,)) for i in range(4)]
        for t in ths:
            t.start()
        threading.Event().wait(0.3)
        m.gate.set()
        for t in ths:
            t.join(10)
        assert all(r is not None and r[0] == 200 and len(r[1]["response"]) == 3 for r in res)
        assert m.max_rows >= 2                     # requests shared decode steps
        with urllib.request.urlopen(f"http://127.0.0.1:{port}/health", timeout=10) as r:
            assert json.loads(r.read())["status"] == "ok"
    finally:
        srv.shutdown()
        srv.server_close()
        s.close()
