"""GPU tests of voices (nl_set_voice / nl_stream_voice / nl_voice_info, include/nanollama_hip.h): several gamma essences
(go/gamma.go:272-290, go/model.go:503-505: embed[token] += gamma[token]) on one handle, one per KV stream.

The contract is bit for bit: a stream bound to voice v computes, on every entry point, what a fresh handle whose nl_set_gamma
received v's data computes.  Three essences A, B, C with different values and overlapping, different token lists; the prompts
hold ids listed in A only, in B only, in both and in none, so a row that read another voice's table cannot equal its
reference.  Every test also sees two voices differ (a comparison of equal things would prove nothing)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nanollama_amd import gguf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOGIT_TOL = 1e-4          # |gpu - oracle| <= 1e-4 * max(1, std(oracle logits))
NL_ERR_INVALID, NL_ERR_STATE = -1, -4
VOCAB, DIM, SEQ = 512, 128, 64

# ids 1, 301: A only; 9, 300: B only; 17, 45: A and B; 2, 33, 5, 77: neither (5, 77: C only)
IDX = {"A": [1, 17, 45, 301], "B": [17, 45, 9, 300], "C": [5, 17, 301, 77]}
PROMPT = [1, 17, 9, 301, 5, 45, 300, 2, 33]
# four streams' token lines (28 each): the same special ids in different orders, padded with ids no voice lists
LINES = [[PROMPT[(i * (s + 2) + s) % 9] if i % 3 != 2 else 100 + 7 * s + i for i in range(28)] for s in range(4)]
SAMP = dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=16)


@pytest.fixture(scope="module")
def hip():
    from nanollama_amd import _lib, model
    if _lib.lib().nl_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return model


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def g():
    return gguf.load_gguf(os.path.join(GOLDEN, "tiny_q8_0.gguf"))


def _essences(tmp, dtype):
    """A, B, C as gamma NPZ files read back through gamma.load_gamma, as the CLI does (f16 files stay f16)."""
    from nanollama_amd import gamma as gm
    rng = np.random.Generator(np.random.PCG64(4242))
    out = {}
    for name, idx in IDX.items():
        vals = (rng.standard_normal((len(idx), DIM)) * 0.3).astype(dtype)
        path = os.path.join(str(tmp), f"gamma_{name}_{np.dtype(dtype).name}.npz")
        np.savez(path, indices=np.array(idx, np.int32), values=vals, vocab_size=np.array(VOCAB), embed_dim=np.array(DIM))
        ge = gm.load_gamma(path)
        assert ge.is_f16 == (dtype == np.float16)
        out[name] = (ge.indices, ge.values)
    return out


def _voiced(hip, g, ess, **kw):
    """the handle under test: C through nl_set_gamma, A as voice 1, B as voice 2"""
    dev = hip.load_llama_model(g, **kw)
    dev.set_gamma(*ess["C"])
    dev.set_voice(1, *ess["A"])
    dev.set_voice(2, *ess["B"])
    return dev


def _single(hip, g, gam, **kw):
    ref = hip.load_llama_model(g, **kw)
    ref.set_gamma(*gam)
    return ref


VOICE_OF = {"A": 1, "B": 2, "C": 0}


def _kcache(dev, stream=0):
    return dev.debug_read("k_cache", 2 * 2 * SEQ * 32, stream=stream).tobytes()


def _every_entry_point(dev):
    """prefill, teacher-forced forward, decode_greedy (more steps than the 16 of a graph segment), sample_decode with fixed
    uniforms, score -- everything a single stream can be asked; each value as bytes or ids"""
    out = {}
    dev.reset()
    dev.prefill(PROMPT[:6])
    out["prefill"] = dev.state.logits.tobytes()
    for pos in range(6, 9):
        dev.forward(PROMPT[pos], pos)
        out[f"forward{pos}"] = dev.state.logits.tobytes()
    first = int(np.argmax(dev.state.logits))
    out["argmax"] = dev.forward_argmax(PROMPT[8], 8)
    out["greedy"] = dev.decode_greedy(first, 9, 20)
    out["greedy_logits"] = dev.debug_read("logits", VOCAB).tobytes()
    out["k_greedy"] = _kcache(dev)
    dev.reset()
    dev.prefill(PROMPT)
    us = np.random.Generator(np.random.PCG64(7)).random(8, dtype=np.float32)
    out["sampled"] = dev.sample_decode(9, 8, SAMP["temperature"], SAMP["top_p"], SAMP["top_k"], SAMP["rep_penalty"],
                                       SAMP["rep_window"], us, [])
    out["k_sampled"] = _kcache(dev)
    dev.reset()
    lp, am = dev.score(PROMPT, PROMPT[1:] + [-1])
    out["score_lp"], out["score_am"] = lp.tobytes(), am.tobytes()
    out["k_score"] = _kcache(dev)
    return out


def _same(got, want, what):
    for k in want:
        assert got[k] == want[k], f"{what}: {k} differs from the handle whose nl_set_gamma received this voice's data"


def _differ(a, b):
    return any(a[k] != b[k] for k in a)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_one_stream_every_entry_point_is_bitwise_the_single_gamma_handle(hip, g, tmp_path, dtype):
    ess = _essences(tmp_path, dtype)
    refs = {}
    for name in "ABC":
        ref = _single(hip, g, ess[name])
        refs[name] = _every_entry_point(ref)
        ref.close()
    assert _differ(refs["A"], refs["B"]) and _differ(refs["A"], refs["C"]) and _differ(refs["B"], refs["C"])
    assert refs["A"]["prefill"] != refs["B"]["prefill"] and refs["A"]["k_greedy"] != refs["C"]["k_greedy"]
    dev = _voiced(hip, g, ess)
    assert dev.voice_info(0) == {"voice": 0, "defined": 3}
    for name in ("A", "B", "C", "A"):
        dev.stream_voice(0, VOICE_OF[name])
        assert dev.voice_info(0)["voice"] == VOICE_OF[name]
        _same(_every_entry_point(dev), refs[name], f"voice {name} ({np.dtype(dtype).name})")     # (resets inside: the binding outlives them)
    dev.close()


def _rows_of_one_step(dev):
    """four streams: prefills of different lengths, then a logits batch, a sampled batch, a mixed step (two decode rows + one
    stream's 8-token chunk) and a sampled mixed step.  Returns per stream the values of its rows."""
    out = {s: {} for s in range(4)}
    pos = [3, 5, 4, 6]
    for s in range(4):
        dev.reset(s)
        dev.prefill(LINES[s][:pos[s]], stream=s, want_logits=False)
    streams = [0, 1, 2, 3]
    ids, lg = dev.forward_batch(streams, [LINES[s][pos[s]] for s in streams], pos, want_logits=True)
    for s in streams:
        out[s]["batch"] = (ids[s], lg[s].tobytes())
    pos = [p + 1 for p in pos]
    us = np.random.Generator(np.random.PCG64(11)).random(16, dtype=np.float32)
    ids, rec = dev.forward_batch_sample(streams, [LINES[s][pos[s]] for s in streams], pos, [SAMP] * 4, us[:4], [[]] * 4)
    for s in streams:
        out[s]["batch_sample"] = (ids[s], rec[s])
    pos = [p + 1 for p in pos]
    # mixed: streams 0 and 1 decode, stream 2 feeds 8 prompt tokens
    rs = [0, 1] + [2] * 8
    rt = [LINES[0][pos[0]], LINES[1][pos[1]]] + LINES[2][pos[2]:pos[2] + 8]
    rp = [pos[0], pos[1]] + list(range(pos[2], pos[2] + 8))
    ids, lg = dev.forward_mixed(rs, rt, rp, 2, want_logits=True)
    out[0]["mixed"], out[1]["mixed"] = (ids[0], lg[0].tobytes()), (ids[1], lg[1].tobytes())
    pos = [pos[0] + 1, pos[1] + 1, pos[2] + 8, pos[3]]
    # sampled mixed: streams 2 and 3 decode (2 right behind its chunk), stream 0 feeds 8 prompt tokens
    rs = [2, 3] + [0] * 8
    rt = [LINES[2][pos[2]], LINES[3][pos[3]]] + LINES[0][pos[0]:pos[0] + 8]
    rp = [pos[2], pos[3]] + list(range(pos[0], pos[0] + 8))
    ids, rec = dev.forward_mixed_sample(rs, rt, rp, 2, [SAMP] * 2, us[4:6], [[], []])
    out[2]["mixed_sample"], out[3]["mixed_sample"] = (ids[0], rec[0]), (ids[1], rec[1])
    for s in streams:
        out[s]["k"] = _kcache(dev, s)          # chunk rows leave no logits: their K rows are their witnesses
    return out


@pytest.mark.parametrize("mixed_attn_min", [None, "0"])
def test_rows_of_one_step_each_follow_their_own_streams_voice(hip, g, tmp_path, monkeypatch, mixed_attn_min):
    if mixed_attn_min is not None:
        monkeypatch.setenv("NL_MIXED_ATTN_MIN", mixed_attn_min)     # the segment-tile attention for the 8-token chunks
    ess = _essences(tmp_path, np.float32)
    refs = {}
    for name in "ABC":          # every reference runs all four streams: the same step geometry
        ref = _single(hip, g, ess[name], max_streams=4)
        refs[name] = _rows_of_one_step(ref)
        ref.close()
    dev = _voiced(hip, g, ess, max_streams=4)
    bound = ["A", "B", "C", "A"]
    for s, name in enumerate(bound):
        dev.stream_voice(s, VOICE_OF[name])
    got = _rows_of_one_step(dev)
    for s, name in enumerate(bound):
        _same(got[s], refs[name][s], f"stream {s} as voice {name}")
    # ... and the voices are told apart on every stream: another voice's rows are not these
    for s, name in enumerate(bound):
        for other in "ABC":
            if other != name:
                assert _differ(got[s], refs[other][s]), (s, name, other)
    dev.close()


def test_rebinding_mid_sequence_against_the_oracle(hip, orc, g, tmp_path):
    # positions below p under voice 1 (A), from p on under voice 2 (B); the oracle's gamma is swapped at p
    ess = _essences(tmp_path, np.float32)
    dev = _voiced(hip, g, ess)
    ref = orc.OracleModel(g)
    only_a = orc.OracleModel(g)
    only_a.set_gamma(*ess["A"])
    p, diff_seen, want = 5, False, None
    dev.stream_voice(0, 1)
    ref.set_gamma(*ess["A"])
    for pos, t in enumerate(PROMPT):
        if pos == p:
            dev.stream_voice(0, 2)
            ref.set_gamma(*ess["B"])
        dev.forward(t, pos)
        want = ref.forward(t, pos)
        d = float(np.abs(dev.state.logits - want).max()) / max(1.0, float(want.std()))
        assert d <= LOGIT_TOL, (pos, d)
        stay = only_a.forward(t, pos)
        diff_seen |= pos >= p and bool(np.abs(want - stay).max() > 1e-3)
    assert diff_seen                                   # the rebind really changes what follows
    tok, want_ids = int(orc.argmax(want)), []
    first = tok
    for k in range(20):
        tok = int(orc.argmax(ref.forward(tok, len(PROMPT) + k)))
        want_ids.append(tok)
    assert int(np.argmax(dev.state.logits)) == first
    assert dev.decode_greedy(first, len(PROMPT), 20) == want_ids
    dev.close(); ref.close(); only_a.close()


def test_cached_graphs_follow_a_rebind(hip, g, tmp_path):
    # bind, step, rebind, step again through the same cached step graphs and 16-step decode graphs: a graph that had baked a
    # table in would repeat the first voice
    ess = _essences(tmp_path, np.float32)
    refs = {}
    for name in "AB":
        ref = _single(hip, g, ess[name])
        refs[name] = _every_entry_point(ref)
        ref.close()
    assert _differ(refs["A"], refs["B"]) and refs["A"]["greedy_logits"] != refs["B"]["greedy_logits"]
    dev = _voiced(hip, g, ess)
    for name in ("A", "B", "A", "B"):
        dev.stream_voice(0, VOICE_OF[name])
        _same(_every_entry_point(dev), refs[name], f"round of voice {name}")
    # a redefinition under the same id is data as well: voice 1 now holds B's table
    dev.stream_voice(0, 0)
    dev.set_voice(1, *ess["B"])
    dev.stream_voice(0, 1)
    _same(_every_entry_point(dev), refs["B"], "voice 1 redefined with B's data")
    dev.close()


def _code(hip, fn):
    from nanollama_amd import _lib
    with pytest.raises(_lib.NlError) as exc:
        fn()
    return exc.value.code


def test_errors_and_lifecycle(hip, g, tmp_path):
    ess = _essences(tmp_path, np.float32)
    dev = hip.load_llama_model(g, max_streams=2)
    plain = hip.load_llama_model(g)
    for s in (0, 1):                                                  # (whatever a first step allocates is in the baseline)
        dev.forward(1, 0, stream=s)
        dev.reset(s)
    state0 = dev.memory_usage()["state"]
    assert dev.voice_info(1) == {"voice": 0, "defined": 0}
    dev.stream_voice(0, 0)                                            # voice 0 is always legal, gamma or not
    assert _code(hip, lambda: dev.stream_voice(0, 1)) == NL_ERR_INVALID          # not defined
    assert _code(hip, lambda: dev.stream_voice(0, 64)) == NL_ERR_INVALID         # voice out of range
    assert _code(hip, lambda: dev.stream_voice(0, -1)) == NL_ERR_INVALID
    assert _code(hip, lambda: dev.stream_voice(2, 0)) == NL_ERR_INVALID          # stream out of range
    assert _code(hip, lambda: dev.set_voice(64, *ess["A"])) == NL_ERR_INVALID
    assert _code(hip, lambda: dev.set_voice(-1, *ess["A"])) == NL_ERR_INVALID
    assert _code(hip, lambda: dev.voice_info(2)) == NL_ERR_INVALID
    with pytest.raises(ValueError):
        dev.set_voice(1, [1], np.zeros((1, 64), np.float32))          # embed_dim mismatch, as set_gamma
    dev.set_voice(1, *ess["A"])
    state1 = dev.memory_usage()["state"]
    assert state1 - state0 == VOCAB * 4 + len(IDX["A"]) * DIM * 4     # the row map and the values
    dev.set_voice(63, *ess["B"])
    assert dev.voice_info(0) == {"voice": 0, "defined": 2}
    dev.stream_voice(1, 1)
    assert _code(hip, lambda: dev.set_voice(1, [], np.zeros((0, DIM), np.float32))) == NL_ERR_STATE    # removing a bound voice
    assert _code(hip, lambda: dev.set_voice(1, *ess["B"])) == NL_ERR_STATE                             # redefining it
    dev.reset(1)
    assert dev.voice_info(1)["voice"] == 1                            # the binding outlives nl_reset
    # nl_set_gamma with n == 0 while voices exist leaves them intact
    dev.set_gamma(*ess["C"])
    dev.set_gamma([], np.zeros((0, DIM), np.float32))
    assert dev.voice_info(1) == {"voice": 1, "defined": 2}
    ref = _single(hip, g, ess["A"])
    for pos, t in enumerate(PROMPT):
        dev.forward(t, pos, stream=1); a = dev.state.logits.tobytes()
        ref.forward(t, pos); plain.forward(t, pos)
        assert a == ref.state.logits.tobytes(), pos                   # stream 1 still speaks as A
        dev.forward(t, pos, stream=0)
        assert dev.state.logits.tobytes() == plain.state.logits.tobytes(), pos   # stream 0: voice 0, no gamma -- the plain model
    assert ref.state.logits.tobytes() != plain.state.logits.tobytes()
    # out-of-range ids are dropped, the rows in range apply (as nl_set_gamma)
    wide = np.concatenate([ess["B"][0], np.array([100000, -3], np.int32)])
    dev.set_voice(63, wide, np.concatenate([ess["B"][1], np.ones((2, DIM), np.float32)]))
    refb = _single(hip, g, ess["B"])
    dev.stream_voice(0, 63)
    for pos, t in enumerate(PROMPT):
        dev.forward(t, pos); refb.forward(t, pos)
        assert dev.state.logits.tobytes() == refb.state.logits.tobytes(), pos
    dev.stream_voice(0, 0)
    # removing an unbound voice: binding to it is an error again, and the state shrinks back
    dev.stream_voice(1, 0)
    dev.set_voice(1, [], np.zeros((0, DIM), np.float32))
    dev.set_voice(63, [], np.zeros((0, DIM), np.float32))
    assert _code(hip, lambda: dev.stream_voice(1, 1)) == NL_ERR_INVALID
    assert dev.memory_usage()["state"] == state0 and dev.voice_info(0)["defined"] == 0
    # before nl_finalize: the ABI takes a definition on a handle that has no tensors yet
    import ctypes as C
    from nanollama_amd import _lib
    L, m = _lib.lib(), g.meta
    cfg = _lib.NlConfig(m.num_layers, m.embed_dim, m.num_heads, m.num_kv_heads, m.head_dim, m.interm_size, m.vocab_size, m.seq_len,
                        m.rms_norm_eps, m.rope_theta, int(m.qk_norm), int(m.rope_conjugate), 1, 0, 0, 1, 0)
    h = C.c_void_p()
    assert L.nl_create(C.byref(cfg), C.byref(h)) == 0
    idx, vals = ess["A"]
    assert L.nl_set_voice(h, 5, idx.ctypes.data_as(C.POINTER(C.c_int32)), int(idx.size), vals.ctypes.data, 0) == 0
    assert L.nl_stream_voice(h, 0, 5) == 0 and L.nl_stream_voice(h, 0, 6) == NL_ERR_INVALID
    L.nl_destroy(h)
    dev.close(); plain.close(); ref.close(); refb.close()


GROUP_WORKER = r"""
import sys
import numpy as np
sys.path.insert(0, {root!r})
from nanollama_amd import gguf, model, synth
g = gguf.load_gguf(sys.argv[1])
vocab = g.meta.vocab_size
rng = np.random.Generator(np.random.PCG64(5))
idx_a, idx_b = np.array([1, 17, 45, 301], np.int32), np.array([17, 45, 9, 300], np.int32)
va = (rng.standard_normal((4, 512)) * 0.3).astype(np.float32)
vb = (rng.standard_normal((4, 512)) * 0.3).astype(np.float32)
toks = [1, 17, 9, 301, 5, 45, 300, 2]
def run(m):
    out = []
    m.reset()
    for pos, t in enumerate(toks):
        m.forward(t, pos)
        out.append(m.state.logits.tobytes())
    out.append(m.decode_greedy(int(np.argmax(m.state.logits)), len(toks), 20))
    return out
want = {{}}
for name, (i, v) in (("a", (idx_a, va)), ("b", (idx_b, vb))):
    ref = model.load_llama_model(g, devices=[0, 0])
    ref.set_gamma(i, v)
    want[name] = run(ref)
    ref.close()
assert want["a"] != want["b"]
grp = model.load_llama_model(g, devices=[0, 0])
grp.set_voice(1, idx_a, va)
grp.set_voice(2, idx_b, vb)
assert grp.voice_info(0) == {{"voice": 0, "defined": 2}}
for name, v in (("a", 1), ("b", 2), ("a", 1)):
    grp.stream_voice(0, v)
    assert run(grp) == want[name], name
try:
    grp.set_voice(1, [], np.zeros((0, 512), np.float32))
    raise SystemExit("removing a bound voice must fail on a group handle too")
except model._lib.NlError as exc:
    assert exc.code == -4, exc
assert run(grp) == want["a"]
grp.close()
print("group voices ok")
"""


def test_group_handle_broadcasts_voices_to_every_rank(hip, tmp_path):
    # 2 ranks on device 0, as tests/test_gpu_group.py: a bound voice is bitwise the group handle whose nl_set_gamma got the data
    from nanollama_amd import synth
    shape = synth.ModelShape("grp_voices", 2, 512, 8, 4, 1024, seq_len=64, interm=1024)
    p = tmp_path / "m.gguf"
    synth.generate_gguf(str(p), shape, "q4_0", 77, mode="qrand")
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8", NL_P2P_TIMEOUT_MS="5000")
    r = subprocess.run([sys.executable, "-c", GROUP_WORKER.format(root=ROOT), str(p)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "group voices ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
