"""Host side of scoring (nanollama_amd/score.py, POST /score, BatchScheduler.score, --score) with a stand-in model whose
log-probability of a row is a known function of (input id, target id, position).  No GPU."""
import contextlib
import json
import math
import threading
from types import SimpleNamespace

import numpy as np
import pytest

from nanollama_amd import cli, score, serve
from nanollama_amd.batch_serve import BatchScheduler, RequestError
from nanollama_amd.engine import GenParams

NOLOCK = contextlib.nullcontext()


def lp_of(inp, tgt, pos):
    return -((inp * 31 + tgt * 7 + pos) % 97) / 16.0 - 0.25


class FakeModel:
    def __init__(self, seq_len=16, vocab=512, max_streams=2, fail_on=None):
        self.config = SimpleNamespace(seq_len=seq_len, vocab_size=vocab)
        self.max_streams = max_streams
        self.gamma = None
        self.calls = []
        self.fail_on = fail_on            # an input id whose presence makes score raise
        self.at_reset = {}

    def reset(self, stream):
        self.calls.append(("reset", stream))
        self.at_reset[stream] = True

    def score(self, tokens, targets, pos0=0, stream=0):
        assert len(tokens) == len(targets) and 0 < len(tokens) and pos0 + len(tokens) <= self.config.seq_len
        assert self.at_reset.pop(stream, False), "score without a reset of the stream"
        if self.fail_on is not None and self.fail_on in tokens:
            raise RuntimeError("injected engine failure")
        self.calls.append(("score", stream, list(tokens), list(targets), pos0))
        lp = np.array([lp_of(a, t, pos0 + i) if t >= 0 else 0.0 for i, (a, t) in enumerate(zip(tokens, targets))], dtype=np.float32)
        am = np.array([t if t >= 0 and (a + t) % 3 == 0 else 0 for a, t in zip(tokens, targets)], dtype=np.int32)
        return lp, am

    # what the scheduler needs for chat requests
    def prefill(self, tokens, pos0=0, stream=0, want_logits=True):
        self.calls.append(("prefill", stream))

    def forward_batch_sample(self, streams, tokens, pos, params, uniforms, recents):
        return [3 + (t + 1) % 40 for t in tokens], [list(r) for r in recents]


class FakeTokenizer:
    """One id per character, except that "ab" is a single piece (so a prompt ending in "a" merges with a continuation
    starting with "b")."""
    eos_id = 2

    def encode(self, text, add_bos=True):
        ids, i = ([1] if add_bos else []), 0
        while i < len(text):
            if text[i:i + 2] == "ab":
                ids.append(300)
                i += 2
            else:
                ids.append(3 + ord(text[i]) % 200)
                i += 1
        return ids

    def decode_token_bytes(self, t):
        return b"x"


def expected(ids, S, n_context):
    """every id from n_context on, once, with the input and position window arithmetic gives it"""
    return [lp_of(ids[j - 1], ids[j], (j - 1) % S) for j in range(max(n_context, 1), len(ids))]


@pytest.mark.parametrize("n_ids", [15, 16, 17, 32, 33])
@pytest.mark.parametrize("n_context", [1, 7, 16])
def test_window_arithmetic(n_ids, n_context):
    S = 16
    ids = [3 + (5 * i) % 200 for i in range(n_ids)]
    m = FakeModel(seq_len=S)
    r = score.score_ids(m, ids, n_context=n_context)
    want = [float(np.float32(v)) for v in expected(ids, S, n_context)]
    assert r.token_logprobs == want and r.n_tokens == max(n_ids - n_context, 0)
    assert r.logprob == float(np.sum(np.asarray(want, dtype=np.float64)))
    if r.n_tokens:
        assert r.nll == -r.logprob / r.n_tokens and r.ppl == math.exp(r.nll)
    else:                                        # (15 and 16 ids with 16 of context: nothing to score, nothing fed)
        assert r.nll == math.inf and not m.calls
    assert r.greedy_matches == sum((ids[j - 1] + ids[j]) % 3 == 0 for j in range(n_context, n_ids))
    calls = [c for c in m.calls if c[0] == "score"]
    # window k feeds ids[kS : (k + 1)S] at position 0 after a reset; no call without a target; nothing fed twice
    for _, stream, tokens, targets, pos0 in calls:
        assert pos0 == 0 and stream == 0 and any(t >= 0 for t in targets)
    fed = [t for c in calls for t in c[2]]
    live = [lo for lo in range(0, n_ids, S) if any(n_context <= j + 1 < n_ids for j in range(lo, min(lo + S, n_ids)))]
    assert fed == [t for lo in live for t in ids[lo:lo + S]]
    assert sum(t >= 0 for c in calls for t in c[3]) == max(n_ids - n_context, 0)


def test_windows_listing():
    assert score.windows(1, 16) == [] and score.windows(0, 16) == []
    assert score.windows(3, 16) == [(0, 3, [1, 2, -1])]
    assert score.windows(17, 16) == [(0, 16, list(range(1, 17)))]                 # the 17th id is only a target
    assert score.windows(18, 16) == [(0, 16, list(range(1, 17))), (16, 2, [17, -1])]
    assert score.windows(18, 16, n_context=16) == [(0, 16, [-1] * 15 + [16]), (16, 2, [17, -1])]
    assert score.windows(18, 16, n_context=17) == [(16, 2, [17, -1])]            # the first window is context only: not fed


def test_bits_per_byte_is_the_reference_expression():
    # nanollama/core_eval.py:47-52: loss_nats * num_tokens / num_bytes / ln 2 with loss the mean cross entropy
    lps = [-1.5, -0.25, -3.0]
    loss, num_tokens, num_bytes = -sum(lps) / 3, 3, 10
    assert math.isclose(score.bits_per_byte(sum(lps), num_bytes), loss * num_tokens / num_bytes / math.log(2), rel_tol=1e-15)
    tok, m = FakeTokenizer(), FakeModel(seq_len=64)
    text = "héllo"                                                               # 5 characters, 6 bytes
    r = score.score_text(m, tok, text)
    ids = tok.encode(text, True)
    want = sum(float(np.float32(v)) for v in expected(ids, 64, 1))
    assert r.n_tokens == 5 and r.n_bytes == 6 and math.isclose(r.bpb, -want / 6 / math.log(2), rel_tol=1e-12)
    short = score.score_text(FakeModel(), tok, "")                                   # fewer than 2 ids: inf, as there
    assert short.n_tokens == 0 and short.bpb == math.inf and short.nll == math.inf and short.ppl == math.inf


def test_continuation_whose_first_piece_merges_with_the_prompt():
    tok, m = FakeTokenizer(), FakeModel(seq_len=64)
    full, n_context = score.continuation_ids(tok, "xya", "bcd")
    assert full == tok.encode("xyabcd", True) and 300 in full
    assert n_context == 3                        # BOS x y are context; the merged piece "ab" is scored with the continuation
    r = score.score_continuation(m, tok, "xya", "bcd")
    assert r.n_tokens == len(full) - 3 and r.n_bytes == 3
    assert r.token_logprobs == [float(np.float32(v)) for v in expected(full, 64, 3)]
    plain = score.score_continuation(FakeModel(seq_len=64), tok, "xy", "cd")
    assert plain.n_tokens == 2
    assert score.continuation_ids(tok, "", "cd")[1] == 1                              # never below 1: BOS is not scored


def test_handle_score_bodies():
    eng = SimpleNamespace(model=FakeModel(seq_len=64), tokenizer=FakeTokenizer())
    lock = threading.Lock()
    st, out = serve.handle_score(eng, lock, json.dumps({"text": "hello"}).encode())
    ids = eng.tokenizer.encode("hello", True)
    want = sum(float(np.float32(v)) for v in expected(ids, 64, 1))
    assert st == 200 and set(out) == {"tokens", "logprob", "nll", "ppl", "bpb"} and out["tokens"] == 5
    assert math.isclose(out["logprob"], want) and math.isclose(out["bpb"], -want / 5 / math.log(2))
    st, out = serve.handle_score(eng, lock, json.dumps({"prompt": "he", "continuation": "llo", "details": True}).encode())
    assert st == 200 and out["tokens"] == 3 and len(out["token_logprobs"]) == 3
    assert math.isclose(out["bpb"], -sum(out["token_logprobs"]) / 3 / math.log(2))
    assert not lock.locked()
    for body in (b"{", b"[1]", b"{}", json.dumps({"text": 5}).encode(), json.dumps({"text": ""}).encode(),
                 json.dumps({"prompt": "a"}).encode(), json.dumps({"prompt": "a", "continuation": ""}).encode(),
                 json.dumps({"text": "a", "prompt": "b", "continuation": "c"}).encode(), b"\xff\xfe"):
        st, out = serve.handle_score(eng, lock, body)
        assert st == 400 and isinstance(out, str) and out.startswith("bad request"), body


def test_http_routes_for_score():
    import urllib.error
    import urllib.request
    from http.server import ThreadingHTTPServer
    eng = SimpleNamespace(model=FakeModel(seq_len=64), tokenizer=FakeTokenizer())
    srv = ThreadingHTTPServer(("127.0.0.1", 0), serve.make_handler(eng, GenParams()))
    th = threading.Thread(target=srv.serve_forever, daemon=True)
    th.start()
    try:
        url = f"http://127.0.0.1:{srv.server_address[1]}/score"
        req = urllib.request.Request(url, data=json.dumps({"text": "hello"}).encode(), headers={"Content-Type": "application/json"})
        with urllib.request.urlopen(req, timeout=10) as resp:
            assert resp.status == 200 and json.loads(resp.read())["tokens"] == 5
        with pytest.raises(urllib.error.HTTPError) as ei:
            urllib.request.urlopen(url, timeout=10)
        assert ei.value.code == 405
        with pytest.raises(urllib.error.HTTPError) as ei:
            urllib.request.urlopen(urllib.request.Request(url, data=b"{"), timeout=10)
        assert ei.value.code == 400
    finally:
        srv.shutdown()
        srv.server_close()


def test_scheduler_score_job_takes_and_returns_a_stream():
    m = FakeModel(seq_len=16, max_streams=2)
    s = BatchScheduler(m, FakeTokenizer(), 2, rep_window=4, seed=1)
    try:
        ids = [3 + i for i in range(20)]
        r = s.score(ids, 1)
        assert r.token_logprobs == [float(np.float32(v)) for v in expected(ids, 16, 1)]
        streams = {c[1] for c in m.calls if c[0] in ("reset", "score")}
        assert streams == {0}                                   # one stream taken ...
        r2 = s.score(ids, 5)                                    # ... and given back: the free list hands out 1, then 0 again
        r3 = s.score(ids, 5)
        assert r2.n_tokens == r3.n_tokens == 15
        assert [c[1] for c in m.calls if c[0] == "score"] == [0, 0, 1, 1, 0, 0]          # two windows per job
        # an engine error fails that job only; chat requests and later jobs go on
        m.fail_on = 77
        with pytest.raises(RequestError) as ei:
            s.score([3, 77, 5], 1)
        assert ei.value.status == 500 and "injected engine failure" in str(ei.value)
        m.fail_on = None
        assert s.generate_quiet("hi", GenParams(max_tokens=3, temperature=0.0)) != ""
        assert s.score(ids, 1).n_tokens == 19
        # through the handler: /score of the batched server routes to the scheduler
        st, out = serve.handle_score(s, NOLOCK, json.dumps({"text": "hello"}).encode())
        assert st == 200 and out["tokens"] == 5
        m.fail_on = 3 + ord("z") % 200
        st, out = serve.handle_score(s, NOLOCK, json.dumps({"text": "zz"}).encode())
        assert st == 500 and "injected engine failure" in out
    finally:
        s.close()
    with pytest.raises(RequestError):
        s.score([3, 4], 1)


def test_cli_score_flag_exclusions(tmp_path, capsys):
    ap = cli.build_parser()
    assert ap.parse_args(["--model", "m"]).score == ""
    for extra in (["--serve"], ["--interactive"], ["--prompt", "x"], ["--gpus", "2"]):
        with pytest.raises(RuntimeError):
            cli.check_score(ap.parse_args(["--model", "m", "--score", "t.txt"] + extra))
    cli.check_score(ap.parse_args(["--model", "m", "--score", "-"]))
    cli.check_score(ap.parse_args(["--model", "m", "--serve"]))
    # main() refuses before it loads anything
    assert cli.main(["--model", str(tmp_path / "none.gguf"), "--score", "t.txt", "--serve"]) == 1
    assert "--score cannot be combined with --serve" in capsys.readouterr().err
    # the line --score prints
    p = tmp_path / "t.txt"
    p.write_text("hello", encoding="utf-8")
    eng = SimpleNamespace(model=FakeModel(seq_len=64), tokenizer=FakeTokenizer())
    cli.run_score(eng, str(p))
    line = capsys.readouterr().out.split()
    assert line[0::2][:4] == ["tokens", "nll", "ppl", "bpb"] and line[1] == "5" and line[-1] == "tokens/s"
