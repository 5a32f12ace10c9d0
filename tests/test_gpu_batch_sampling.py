"""GPU tests of sampled decode batches: nl_forward_batch_sample (one decode step of n streams, then the n-row on-device sampler
of nanollama_amd/csrc/nl_sample.h with every row's own settings) against a shadow handle of the same model that returns the
logits of the same step (nl_forward_batch) and samples them on the host with tests/sampling_mirror.py -- ids and windows
equal at every step, KV state equal afterwards; the continuous-batching scheduler on top of it; the HTTP server with
--parallel."""
import json
import os
import socket
import subprocess
import sys
import threading
import time
import urllib.request

import numpy as np
import pytest

from nanollama_amd import gguf, synth
from nanollama_amd.engine import GenParams

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_mirror as sm  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def hip():
    from nanollama_amd import _lib, model
    if _lib.lib().nl_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return model


# the settings mix: greedy with a penalty, top-p at two temperatures, top-k (including a list as long as the device allows)
SETTINGS = [
    dict(temperature=0.0, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=8),
    dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=64),
    dict(temperature=1.3, top_p=1.0, top_k=40, rep_penalty=1.3, rep_window=16),
    dict(temperature=0.5, top_p=0.6, top_k=50, rep_penalty=1.0, rep_window=0),
    dict(temperature=0.7, top_p=1.0, top_k=1024, rep_penalty=1.2, rep_window=4),
    dict(temperature=2.0, top_p=0.99, top_k=50, rep_penalty=1.5, rep_window=5),
]


def host_pick(lg, p, recent, u, vocab):
    lg = sm.apply_penalty(lg, recent, p["rep_penalty"], vocab)
    if p["temperature"] <= 0:
        return int(np.argmax(lg))
    if p["top_p"] < 1.0:
        return sm.device_top_p(lg, p["temperature"], p["top_p"], u)[0]
    return sm.go_top_k(lg, p["temperature"], p["top_k"], u)


def _model_path(tmp_path, kind):
    if kind == "tiny_q8_0":
        return os.path.join(GOLDEN, "tiny_q8_0.gguf")
    shapes = {
        # Q4_0 with whole 256-column groups: dgemm_kernel layers and the dghead_kernel LM head (nl_dgemm.h)
        "q4_0_dgemm": (synth.ModelShape("bs_dg", 2, 256, 4, 2, 640, seq_len=320, interm=512), "q4_0"),
        # vocabulary 48000: the streamed select variants (vocab > 32768)
        "v48000": (synth.ModelShape("bs_v48", 1, 128, 4, 2, 48000, seq_len=320, interm=256), "q8_0"),
        # Q4_K: outside the batch path -- every row's single-token step, then the sampler on that row
        "q4_k": (synth.ModelShape("bs_qk", 1, 256, 4, 2, 512, seq_len=320, interm=512), "q4_k"),
    }
    shape, wt = shapes[kind]
    p = str(tmp_path / f"{kind}.gguf")
    synth.generate_gguf(p, shape, wt, 307)
    return p


# every row's mode rotates on every step (_drive(rotate=True)): argmax -> top-p -> top-k
ROTATE = [dict(temperature=0.0, top_p=0.9, top_k=50, rep_penalty=1.3),
          dict(temperature=0.9, top_p=0.9, top_k=50, rep_penalty=1.15),
          dict(temperature=1.1, top_p=1.0, top_k=50, rep_penalty=1.15)]


def _drive(hip, g, n, steps, start, seed, shadow_flags=0, dev_flags=0, switch_at=None, phases=None, rotate=False,
           go_rule=False, check_logits=None, tied=()):
    """n streams from prompt positions `start` for `steps` fed-back steps on a handle and its shadow; returns the ids.
    phases: row counts of successive runs of `steps` steps on the same two handles (rows = streams [0, m); a stream keeps its
    position, token and window from phase to phase; start then covers max(phases) streams); rotate: every row's settings
    rotate through ROTATE on every step; go_rule: top-p picks are also compared with the literal Go chain -- every difference
    at a boundary (margin < 5e-4), at most max(2, trials // 8) of them up to vocabulary 50000; check_logits(row logits): a
    precondition asserted on the shadow's logits of every row and step.  tied: ids whose logits are one value on every row
    (a crafted LM head): a difference where the device's or the Go chain's pick is one of them is a walk over thousands of
    equal terms, where the Go chain's float32 sum drifts by many of them -- the reason the cap stops at 50000 -- so it is held
    to the margin rule and counted apart, and the cap applies to the other differences."""
    phases = phases or [n]
    N = max(phases)
    vocab = g.meta.vocab_size
    dev = hip.load_llama_model(g, max_streams=max(N, 1), flags=dev_flags)
    sh = hip.load_llama_model(g, max_streams=max(N, 1), flags=shadow_flags)
    rng = np.random.Generator(np.random.PCG64(seed))
    try:
        prompts = [[int(t) for t in rng.integers(3, vocab, size=start[i] + 1)] for i in range(N)]
        for i in range(N):
            if start[i] > 0:
                dev.prefill(prompts[i][:start[i]], pos0=0, stream=i, want_logits=False)
                sh.prefill(prompts[i][:start[i]], pos0=0, stream=i, want_logits=False)
        params = [dict(SETTINGS[i % len(SETTINGS)]) for i in range(N)]
        # windows: empty, partial, full with repeated ids
        recents = []
        for i, p in enumerate(params):
            w = p["rep_window"]
            k = [0, w // 2, w][i % 3] if w else 0
            base = [int(t) for t in rng.integers(0, vocab, size=max(k, 1))]
            recents.append([base[j % 2] for j in range(k)] if i % 3 == 2 else base[:k])
        tokens = [prompts[i][start[i]] for i in range(N)]
        pos = list(start)
        all_ids = []
        go_trials = go_mism = go_tied = 0
        tied_set = set(tied)
        gstep = 0
        for m in phases:
            streams = list(range(m))
            for step in range(steps):
                if switch_at is not None and step == switch_at:   # other settings at the same n (no re-capture needed)
                    params = [dict(SETTINGS[(i + 1) % len(SETTINGS)], rep_window=params[i]["rep_window"]) for i in range(N)]
                    params = [dict(p, top_p=1.0 if p["top_p"] < 1.0 else 0.7) for p in params]
                cur = params[:m]
                if rotate:
                    cur = [dict(ROTATE[(i + gstep) % len(ROTATE)], rep_window=params[i]["rep_window"]) for i in range(m)]
                us = rng.random(m, dtype=np.float32)
                ids, new_rec = dev.forward_batch_sample(streams, tokens[:m], pos[:m], cur, us, recents[:m])
                _, lg = sh.forward_batch(streams, tokens[:m], pos[:m], want_logits=True)
                want_ids, want_rec = [], []
                for i in range(m):
                    if check_logits is not None:
                        check_logits(lg[i])
                    t = host_pick(lg[i], cur[i], recents[i], us[i], vocab)
                    want_ids.append(t)
                    want_rec.append(sm.push_recent(recents[i], t, cur[i]["rep_window"]) if cur[i]["rep_window"] > 0 else [])
                    if go_rule and cur[i]["temperature"] > 0 and cur[i]["top_p"] < 1.0:
                        plg = sm.apply_penalty(lg[i], recents[i], cur[i]["rep_penalty"], vocab)
                        go_trials += 1
                        go = sm.go_top_p(plg, cur[i]["temperature"], cur[i]["top_p"], us[i])
                        if t != go:
                            assert sm.device_top_p(plg, cur[i]["temperature"], cur[i]["top_p"], us[i])[1] < 5e-4, (m, step, i)
                            if t in tied_set or go in tied_set:
                                go_tied += 1
                            else:
                                go_mism += 1
                assert ids == want_ids, (m, step, ids, want_ids)
                assert new_rec == want_rec, (m, step)
                all_ids.append(ids)
                recents[:m], tokens[:m], pos[:m] = new_rec, ids, [q + 1 for q in pos[:m]]
                gstep += 1
        # the KV state is the same: the next step's logits are bitwise the shadow's
        streams = list(range(phases[-1]))
        _, a = dev.forward_batch(streams, tokens[:phases[-1]], pos[:phases[-1]], want_logits=True)
        _, b = sh.forward_batch(streams, tokens[:phases[-1]], pos[:phases[-1]], want_logits=True)
        assert a.tobytes() == b.tobytes()
        if go_rule:
            print(f"V={vocab}: {go_mism + go_tied} of {go_trials} top-p picks differ from the Go chain, {go_tied} of them "
                  f"on a tied id")
            if vocab <= 50000:
                assert go_mism <= max(2, go_trials // 8), (vocab, go_mism, go_trials)
        return all_ids
    finally:
        dev.close()
        sh.close()


def _starts(n, lo, hi, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    return [int(v) for v in r.integers(lo, hi, size=n)]


def test_exact_against_host_tiny(hip):
    g = gguf.load_gguf(os.path.join(GOLDEN, "tiny_q8_0.gguf"))   # (seq_len 64)
    for n in (1, 2, 3, 8, 64):
        _drive(hip, g, n, 20, _starts(n, 0, 40, n), 100 + n)


@pytest.mark.parametrize("kind", ["q4_0_dgemm", "v48000", "q4_k"])
def test_exact_against_host_synthetic(hip, tmp_path, kind):
    g = gguf.load_gguf(_model_path(tmp_path, kind))
    for n in ((1, 3, 8, 64) if kind != "v48000" else (2, 64)):
        start = _starts(n, 100, 140, n)              # rows on both sides of the 128-position split, crossing it while they run
        start[0] = 5
        _drive(hip, g, n, 20 if n < 64 else 12, start, 200 + n, switch_at=6)


def test_settings_change_between_calls(hip):
    g = gguf.load_gguf(os.path.join(GOLDEN, "tiny_q8_0.gguf"))
    _drive(hip, g, 8, 20, _starts(8, 0, 30, 3), 7, switch_at=10)


def test_no_graph_handle_gives_the_same_ids(hip, tmp_path):
    from nanollama_amd import _lib
    for path in (os.path.join(GOLDEN, "tiny_q8_0.gguf"), _model_path(tmp_path, "q4_0_dgemm")):
        g = gguf.load_gguf(path)
        start = _starts(16, 0, 40, 9)
        a = _drive(hip, g, 16, 8, start, 11)
        b = _drive(hip, g, 16, 8, start, 11, dev_flags=_lib.NL_FLAG_NO_GRAPH, shadow_flags=_lib.NL_FLAG_NO_GRAPH)
        assert a == b


ZERO_ROWS = 64


def _crafted_path(tmp_path, wt, vocab, dim):
    """A model whose LM head (output.weight) is crafted: ids [0, V/3) copy one row (exact ties on every stream), the ZERO_ROWS
    ids after them are zero rows (logits of exactly 0), id V - 2 is a row scaled x64 (dominant or far below, by the stream's
    sign), the rest are the drawn random rows."""
    shape = synth.ModelShape(f"bs_cr{vocab}", 1, dim, 4, 2, vocab, seq_len=128, interm=2 * dim)
    head = synth.draw_float(shape, 307, "output.weight", (vocab, dim), "matrix")
    third = vocab // 3
    head[:third] = head[vocab - 1]
    head[third:third + ZERO_ROWS] = 0.0
    head[vocab - 2] *= np.float32(64.0)
    p = str(tmp_path / f"crafted_{wt}_{vocab}.gguf")
    synth.generate_gguf(p, shape, wt, 307, overrides={"output.weight": head})
    return p


def _crafted_preconditions(vocab):
    third = vocab // 3

    def check(lg):
        # the edges are reached: >= V/3 - 1 bitwise-equal logits, the zero block exactly 0
        _, counts = np.unique(lg.view(np.uint32), return_counts=True)
        assert counts.max() >= third - 1, ("ties lost in the LM head", counts.max(), third)
        assert np.all(lg[third:third + ZERO_ROWS] == 0.0), "the zero rows do not give logits of 0"
    return check


@pytest.mark.parametrize("wt,vocab,dim", [("q8_0", 32768, 128), ("q8_0", 32769, 128), ("q8_0", 131072, 128),
                                          ("q4_0", 32768, 256)])
def test_crafted_logits_rotating_modes_and_row_counts(hip, tmp_path, wt, vocab, dim):
    # the batch path on logits with exact ties over a third of the vocabulary, a block of zeros and one token far above or
    # below the rest (q4_0 with whole 256-column groups: the dghead_kernel LM head); every row's mode rotates on every step and
    # the row counts on one handle go 64 -> 2 (below NL_BATCH_MIN: the per-row fallback) -> 17 (another captured graph) -> 64
    # (the handle's persistent sampler scratch again), with graphs and without
    from nanollama_amd import _lib
    g = gguf.load_gguf(_crafted_path(tmp_path, wt, vocab, dim))
    start = _starts(64, 0, 60, vocab)
    kw = dict(phases=[64, 2, 17, 64], rotate=True, go_rule=True, check_logits=_crafted_preconditions(vocab),
              tied=list(range(vocab // 3)) + [vocab - 1])
    a = _drive(hip, g, 64, 4, start, 31, **kw)
    b = _drive(hip, g, 64, 4, start, 31, dev_flags=_lib.NL_FLAG_NO_GRAPH, **kw)
    assert a == b


def test_argument_errors(hip):
    from nanollama_amd import _lib
    import ctypes as C
    g = gguf.load_gguf(os.path.join(GOLDEN, "tiny_q8_0.gguf"))
    dev = hip.load_llama_model(g, max_streams=4)
    L = _lib.lib()
    P = dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=8)

    def call(streams, tokens, pos, params, nrec=None, stride=8, n=None):
        n = len(streams) if n is None else n
        m = max(n, 1)
        ia = lambda v: (C.c_int * max(len(v), 1))(*v)
        ps = (_lib.NlSampleParams * m)(*[_lib.NlSampleParams(p["temperature"], p["top_p"], p["top_k"], p["rep_penalty"],
                                                              p["rep_window"]) for p in params[:m]])
        u = (C.c_float * m)(*([0.5] * m))
        rec = (C.c_int * (m * max(stride, 1)))()
        nr = ia(nrec if nrec is not None else [0] * m)
        ids = (C.c_int * m)()
        return L.nl_forward_batch_sample(dev._h, ia(streams), ia(tokens), ia(pos), n, ps, u, rec, stride, nr, ids)

    try:
        assert call([0, 1], [1, 2], [0, 0], [P, P]) == 0
        assert call([0, 0], [1, 2], [1, 1], [P, P]) == -1                       # a stream twice
        assert call([0, 1, 2, 3, 4], [1] * 5, [0] * 5, [P] * 5) == -1           # n > max_streams
        assert call([0], [1], [64], [P]) == -1                                  # pos >= seq_len
        assert call([0], [512], [1], [P]) == -1                                 # token out of range
        assert call([5], [1], [1], [P]) == -1                                   # stream out of range
        assert call([0], [1], [1], [dict(P, rep_window=2000)], stride=2000) == -1   # rep_window > 1024
        assert call([0], [1], [1], [dict(P, top_p=0.0)]) == -1                  # top_p <= 0
        assert call([0], [1], [1], [dict(P, top_p=1.0, top_k=2000)]) == -1      # top_k > 1024 in top-k mode
        assert call([0], [1], [1], [dict(P, top_p=1.0, top_k=0)]) == -1         # top_k < 1 in top-k mode
        assert call([0], [1], [1], [dict(P, rep_window=16)], stride=8) == -1    # recent_stride < rep_window
        assert call([0], [1], [1], [P], nrec=[9]) == -1                         # n_recent > rep_window
        assert call([0], [1], [1], [P], n=-1) == -1
        assert call([], [], [], [P], n=0) == 0
    finally:
        dev.close()
    # n > 64 per call
    dev = hip.load_llama_model(g, max_streams=65)
    try:
        assert call(list(range(65)), [1] * 65, [0] * 65, [P] * 65) == -1
        assert call(list(range(64)), [1] * 64, [0] * 64, [P] * 64) == 0
    finally:
        dev.close()


def test_unsupported_vocab_and_group(hip, tmp_path):
    from nanollama_amd import _lib
    shape = synth.ModelShape("bs_big", 1, 64, 2, 2, 131088, seq_len=32, interm=128)
    p = str(tmp_path / "big.gguf")
    synth.generate_gguf(p, shape, "q8_0", 5)
    dev = hip.load_llama_model(gguf.load_gguf(p), max_streams=2)
    try:
        with pytest.raises(_lib.NlError) as ei:
            dev.forward_batch_sample([0], [1], [0], [dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15,
                                                         rep_window=8)], [0.5], [[]])
        assert ei.value.code == -2
    finally:
        dev.close()
    g = gguf.load_gguf(os.path.join(GOLDEN, "tiny_q8_0.gguf"))
    grp = hip.load_llama_model(g, devices=[0, 0])
    try:
        with pytest.raises(_lib.NlError) as ei:
            grp.forward_batch_sample([0], [1], [0], [dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15,
                                                         rep_window=8)], [0.5], [[]])
        assert ei.value.code == -2
    finally:
        grp.close()


class CharTokenizer:
    """The tiny model's pieces for decoding; prompts become one id per character, so their lengths differ."""

    def __init__(self, tok, vocab):
        self.tok, self.vocab, self.eos_id = tok, vocab, tok.eos_id

    def encode(self, text, add_bos=True):
        return ([1] if add_bos else []) + [3 + ord(c) % (self.vocab - 3) for c in text]

    def decode_token_bytes(self, t):
        return self.tok.decode_token_bytes(t)


class Recorder:
    """The model as the scheduler sees it; every call is replayed on a shadow handle, forward_batch_sample as
    forward_batch(want_logits=True) + the host mirror, and the ids must agree."""

    def __init__(self, model, shadow):
        self.m, self.sh = model, shadow
        self.config, self.max_streams, self.gamma = model.config, model.max_streams, None
        self.steps, self.rows = 0, 0
        self.runs, self.cur = [], {}          # the ids of every admitted request, in admission order

    def reset(self, stream):
        self.m.reset(stream)
        self.sh.reset(stream)
        self.cur[stream] = []
        self.runs.append(self.cur[stream])

    def prefill(self, tokens, pos0=0, stream=0, want_logits=True):
        self.m.prefill(tokens, pos0=pos0, stream=stream, want_logits=want_logits)
        self.sh.prefill(tokens, pos0=pos0, stream=stream, want_logits=False)

    def forward_batch_sample(self, streams, tokens, pos, params, uniforms, recents):
        ids, rec = self.m.forward_batch_sample(streams, tokens, pos, params, uniforms, recents)
        _, lg = self.sh.forward_batch(streams, tokens, pos, want_logits=True)
        for i in range(len(streams)):
            want = host_pick(lg[i], params[i], recents[i], np.float32(uniforms[i]), self.config.vocab_size)
            assert ids[i] == want, (i, ids[i], want)
            self.cur[streams[i]].append(ids[i])
        self.steps += 1
        self.rows = max(self.rows, len(streams))
        return ids, rec


def test_scheduler_end_to_end(hip):
    from nanollama_amd.batch_serve import BatchScheduler
    from nanollama_amd.tokenizer import Tokenizer
    g = gguf.load_gguf(os.path.join(GOLDEN, "tiny_q8_0.gguf"))
    tok = CharTokenizer(Tokenizer(g.meta), g.meta.vocab_size)
    dev = hip.load_llama_model(g, max_streams=4)
    sh = hip.load_llama_model(g, max_streams=4)
    rec = Recorder(dev, sh)
    # an EOS id that occurs: the most frequent id of a first run
    s0 = BatchScheduler(rec, tok, 4, rep_penalty=1.15, rep_window=16, seed=1)
    prompts = ["a", "hello there", "x y z", "the quick brown fox", "ok", "sampling", "batch of seven"]
    gps = [GenParams(max_tokens=12, temperature=0.8, top_p=0.9, top_k=50), GenParams(max_tokens=20, temperature=0.0),
           GenParams(max_tokens=7, temperature=1.2, top_p=1.0, top_k=30), GenParams(max_tokens=30, temperature=0.5),
           GenParams(max_tokens=3, temperature=0.9, top_p=1.0, top_k=5), GenParams(max_tokens=64, temperature=0.7),
           GenParams(max_tokens=25, temperature=0.0, top_p=1.0)]
    try:
        s0.generate_quiet(prompts[1], gps[1])
        counts = np.bincount([t for v in rec.runs for t in v], minlength=g.meta.vocab_size)
    finally:
        s0.close()
    eos = int(np.argmax(counts))
    rec.runs = []
    s = BatchScheduler(rec, tok, 4, rep_penalty=1.15, rep_window=16, seed=2)
    s.eos_id = eos
    out = [None] * len(prompts)
    try:
        def go(i):
            out[i] = s.generate_quiet(prompts[i], gps[i])
        ths = [threading.Thread(target=go, args=(i,)) for i in range(len(prompts))]
        for t in ths:
            t.start()
        for t in ths:
            t.join(120)
        assert all(o is not None for o in out)
    finally:
        s.close()
        dev.close()
        sh.close()
    assert rec.rows >= 2 and len(rec.runs) == len(prompts)
    assert any(eos in run for run in rec.runs)              # the EOS occurred
    # each response = the pieces of its ids up to (not including) the EOS, the EOS only ever last
    want = []
    for run in rec.runs:
        assert eos not in run[:-1]
        ids = run[:-1] if run and run[-1] == eos else run
        want.append(b"".join(tok.decode_token_bytes(t) for t in ids).decode("utf-8", errors="replace"))
    assert sorted(want) == sorted(out)
    # and each request stopped by a rule: its max_tokens, the EOS or the end of the context
    lens = sorted(len(run) for run in rec.runs)
    caps = sorted(min(p.max_tokens, g.meta.seq_len - min(len(tok.encode(q, True)), g.meta.seq_len - 1))
                  for q, p in zip(prompts, gps))
    assert all(any(n == c for c in caps) or eos in run for n, run in zip(lens, sorted(rec.runs, key=len)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_http_server_parallel(tmp_path):
    port = _free_port()
    env = dict(os.environ, PYTHONPATH=ROOT)
    log = open(tmp_path / "server.log", "w")
    proc = subprocess.Popen([sys.executable, "-m", "nanollama_amd", "--model", os.path.join(GOLDEN, "tiny_q8_0.gguf"),
                             "--serve", "--parallel", "4", "--port", str(port), "--seed", "3", "--max-tokens", "16"],
                            cwd=ROOT, env=env, stdout=log, stderr=subprocess.STDOUT)
    try:
        for _ in range(300):
            try:
                with urllib.request.urlopen(f"http://127.0.0.1:{port}/health", timeout=2) as r:
                    health = json.loads(r.read())
                    break
            except OSError:
                if proc.poll() is not None:
                    break
                time.sleep(0.2)
        else:
            health = None
        assert health and health["status"] == "ok", open(tmp_path / "server.log").read()
        res = [None] * 8

        def post(i):
            req = urllib.request.Request(f"http://127.0.0.1:{port}/chat", data=json.dumps(
                {"messages": [{"role": "user", "content": "hello %d" % i}], "temperature": 0.1 * (i + 1)}).encode(),
                method="POST")
            with urllib.request.urlopen(req, timeout=60) as r:
                res[i] = (r.status, json.loads(r.read()))
        ths = [threading.Thread(target=post, args=(i,)) for i in range(8)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(90)
        assert all(r is not None and r[0] == 200 and isinstance(r[1]["response"], str) for r in res), res
    finally:
        proc.terminate()
        try:
            proc.wait(20)
        except subprocess.TimeoutExpired:
            proc.kill()
            proc.wait(10)
        log.close()
