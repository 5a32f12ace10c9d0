"""GPU: every norm, SwiGLU and fragment path against the float64 forward of tests/attn_cases.py on the models of
tests/scale_cases.py -- residual streams at rms 2^-14 .. 2^15, an rms that rises 2^4 at every seam or 2^8 / 2^12 at one (the folded
norm's power-of-two pre-scale is then the stale one of the token's previous norm), SiLU pre-activations to +-550, three massive
channels that own the rms.  Random synth models reach none of these.

Bound: max|gpu - f64| <= 1e-4 * std(f64 logits of the step) at every checked step -- this work's metric has no floor of 1 under the
standard deviation (eps and outlier have logits of std ~0.02) -- and every logit finite.  tests/test_scale_cases_cpu.py holds the CPU
oracle to half of that on the same models, so a failure here is not the input's fault.  Every test asserts that the kernel it is
about served the steps (launch kinds of the plan, plan_info, persist_info, the block-major weight copies dgemm_kernel builds, or a
bitwise difference from the route that would have served them otherwise) and prints its worst value and where it occurred.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_cases as ac  # noqa: E402
import scale_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = sc.GPU_TOL
KV_TOL = 2e-5            # single ops, DESIGN section 5: |d| <= 2e-5 * (1 + |v|)
ALL = sc.ALL


@pytest.fixture(scope="module")
def hip():
    from nanollama_amd import _lib, model
    if _lib.lib().nl_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return model


_cases = {}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """(loaded GGUF, token sequence, float64 model, float64 run over the sequence) of a (shape, weight type, case): built once"""
    def get(shape_key, wtype, name):
        key = (shape_key, wtype, name)
        assert key in sc.CASES, f"{key} is not pinned by test_scale_cases_cpu.py"
        if key not in _cases:
            g = sc.build_case(str(tmp_path_factory.mktemp("scale") / "m.gguf"), shape_key, wtype, name)
            toks = sc.tokens(shape_key)
            f64 = ac.F64Model(g)
            _cases[key] = (g, toks, f64, f64.forward(toks))
        return _cases[key]
    return get


class Worst:
    """the largest max|gpu - f64| / std of a test, and where"""

    def __init__(self, what):
        self.what, self.err, self.at = what, 0.0, None

    def see(self, got, want64, at):
        assert np.isfinite(got).all(), (self.what, at, "inf / nan in the logits")
        e = sc.rel_err(got, want64)
        if e > self.err:
            self.err, self.at = e, at
        return e

    def close(self):
        print(f"\n{self.what}: max|gpu-f64|/std = {self.err:.2e} (at {self.at})")
        assert self.err <= TOL, (self.what, self.err, self.at)


def _kinds(dev, pos):
    return {k: c for k, (ms, c) in dev.profile_forward(5, pos, iters=1).items() if c}


def _teacher_forced(dev, toks, run, w):
    for pos, t in enumerate(toks):
        dev.forward(t, pos)
        w.see(dev.state.logits, run.logits[pos], pos)


# ---- 1. the general five-launch plan: rmsnorm in the GEMV prologues, SiLU in the gate/up GEMV (nl_kernels.h) ----------------------

@pytest.mark.parametrize("wtype,name", [("q8_0", c) for c in ALL] + [(t, c) for t in ("q4_0", "f16") for c in ("hi", "jump12", "gate")])
def test_general_five_launch_plan(hip, case, monkeypatch, wtype, name):
    g, toks, _, run = case("gqa", wtype, name)
    monkeypatch.setenv("NL_FUSED_ATTN", "0")
    monkeypatch.setenv("NL_PERSIST", "0")
    dev = hip.load_llama_model(g)
    assert dev.plan_info()["fused_mode"] == 0 and not dev.persist_info()["ready"], (dev.plan_info(), dev.persist_info())
    w = Worst(f"general plan gqa/{wtype}/{name}")
    _teacher_forced(dev, toks, run, w)
    L = g.meta.num_layers
    k = _kinds(dev, 20)
    assert (k.get("attention"), k.get("wo_resid"), k.get("gate_up_swiglu"), k.get("down_resid")) == (L,) * 4 and k.get("qkv_rope"), k
    assert "attn_block" not in k and "ffn_block" not in k, k
    dev.close()
    w.close()


# ---- 2. the fused block plan: attn_block_kernel + ffn_block_kernel (nl_block.h) --------------------------------------------------

@pytest.mark.parametrize("wtype,name", [("q8_0", c) for c in ALL] + [("q4_0", c) for c in ("lo", "gate")])
def test_fused_block_plan(hip, case, monkeypatch, wtype, name):
    g, toks, _, run = case("gqa", wtype, name)
    monkeypatch.setenv("NL_FUSED_FFN", "1")
    monkeypatch.setenv("NL_PERSIST", "0")                      # (the 256-wide shapes would otherwise go to the resident session)
    dev = hip.load_llama_model(g)
    info = dev.plan_info()
    assert info["fused_mode"] == 1 and info["fused_max_pos"] >= len(toks) and not dev.persist_info()["ready"], info
    w = Worst(f"fused block gqa/{wtype}/{name}")
    _teacher_forced(dev, toks, run, w)
    L = g.meta.num_layers
    for pos in (5, 40):     # (the last layer keeps the two GEMV launches so that the LM head reads a complete residual stream)
        k = _kinds(dev, pos)
        assert k.get("attn_block") == L and k.get("ffn_block") == L - 1 and "attention" not in k and "wo_resid" not in k, (pos, k)
    assert dev.last_error() == ""                              # (no exchange timed out: the blocks did serve every step)
    dev.close()
    w.close()


# ---- 3. the wide tier: tp_attn_kernel + wide_ffn_kernel with the matrix-pipe digits (mf_*) or the vector pipe; mode 2 --------------

_wide_bits = {}


def _wide(hip, g, toks, run, monkeypatch, what, mode, mfma):
    monkeypatch.setenv("NL_WIDE_FFN", "2")       # (the one-launch feed-forward half on this 64-block grid: by default it waits for grids that fill the chip)
    if mfma is not None:
        monkeypatch.setenv("NL_MFMA_DOT", mfma)
    if mode == 2:
        monkeypatch.setenv("NL_ATTN_WO", "0")
    dev = hip.load_llama_model(g)
    assert dev.plan_info()["fused_mode"] == mode, dev.plan_info()
    w = Worst(what)
    out = []
    for pos, t in enumerate(toks):
        dev.forward(t, pos)
        w.see(dev.state.logits, run.logits[pos], pos)
        out.append(dev.state.logits.copy())
    L = g.meta.num_layers
    k = _kinds(dev, 20)
    assert k.get("attn_block") == L and "qkv_rope" not in k and "attention" not in k, k
    if mode == 4:
        assert k.get("ffn_block") == L and "gate_up_swiglu" not in k and "wo_resid" not in k, k
    else:
        assert k.get("wo_resid") == L, k
    assert dev.last_error() == ""
    dev.close()
    w.close()
    return np.stack(out)


@pytest.mark.parametrize("name", ALL)
def test_wide_tier_matrix_pipe_feed_forward(hip, case, monkeypatch, name):
    g, toks, _, run = case("wide", "q4_0", name)
    _wide_bits[name] = _wide(hip, g, toks, run, monkeypatch, f"wide tier, mode 4, matrix pipe q4_0/{name}", 4, None)


@pytest.mark.parametrize("name", ["hi", "lo", "gate"])
def test_wide_tier_vector_pipe_feed_forward(hip, case, monkeypatch, name):
    g, toks, _, run = case("wide", "q4_0", name)
    got = _wide(hip, g, toks, run, monkeypatch, f"wide tier, mode 4, NL_MFMA_DOT=0 q4_0/{name}", 4, "0")
    if name not in _wide_bits:          # (run alone)
        monkeypatch.delenv("NL_MFMA_DOT")
        _wide_bits[name] = _wide(hip, g, toks, run, monkeypatch, f"wide tier, mode 4, matrix pipe q4_0/{name}", 4, None)
    assert got.tobytes() != _wide_bits[name].tobytes()         # the two pipes are not each other's bits: both did run


@pytest.mark.parametrize("name", ["hi", "jump12"])
def test_wide_tier_projection_attention_launch_wo_own_launch(hip, case, monkeypatch, name):
    g, toks, _, run = case("wide", "q4_0", name)
    _wide(hip, g, toks, run, monkeypatch, f"wide tier, mode 2 q4_0/{name}", 2, None)


# ---- 4. a tensor-parallel rank: tp_attn_kernel + tp_ffn_kernel (its SiLU carries u * inv), the shards of an in-process group --------

@pytest.mark.parametrize("name", ["hi", "lo", "gate", "jump12"])
def test_tensor_parallel_rank(hip, case, name):
    g, toks, _, run = case("wide", "q4_0", name)
    grp = hip.LocalTPGroup(g, 2, fused=True)                   # both ranks on device 0
    try:
        info = grp.shards[0].plan_info()
        assert info["fused_mode"] == 3 and info["launches_fused"] == 2 * g.meta.num_layers + 3, info
        w = Worst(f"tensor-parallel rank, tp 2 wide/q4_0/{name}")
        for pos, t in enumerate(toks):
            w.see(grp.forward(t, pos), run.logits[pos], pos)
        for s in grp.shards:                                   # (the fused plan was never retired)
            assert not s.last_error() and s.plan_info()["fused_mode"] == 3
    finally:
        grp.close()
    w.close()


# ---- 5. the persistent decode: pd_limbs / pd_inv_rms / pd_exp (nl_persist.h) through the resident session and nl_decode_greedy -----

class _PlacementMiss(Exception):
    pass


def _no_warning(dev):
    err = dev.last_error()
    if "not placed 32 per XCD" in err:       # a property of the moment on the device (nl_persist.h): the chunk was redone on the
        raise _PlacementMiss(err)            # launch plans, so the run did not test the persistent path
    return err == ""


def _persistent(hip, g, toks, f64, run, what):
    dev = hip.load_llama_model(g)
    try:
        info = dev.persist_info()
        assert info["ready"] and info["max_pos"] == 320, info
        # (a) the resident session: per-call Forward over the whole sequence
        w = Worst(f"persistent decode, resident session {what}")
        _teacher_forced(dev, toks, run, w)
        info = dev.persist_info()          # (one resident launch unless the host paused longer than the idle limit)
        assert _no_warning(dev) and info["tokens"] == len(toks) and 1 <= info["launches"] <= 4, info
        # (b) chained greedy steps: the device picks its own tokens; the float64 forward is fed the ids it produced
        dev.reset()
        n0, steps = sc.PERSIST_PROMPT, sc.PERSIST_STEPS
        dev.prefill(toks[:n0])
        tok = int(np.argmax(dev.state.logits))
        fed, rows = [], []
        for i in range(steps):
            fed.append(tok)
            (tok,) = dev.decode_greedy(tok, n0 + i, 1)
            rows.append(dev.debug_read("logits", g.meta.vocab_size))
        info2 = dev.persist_info()
        assert _no_warning(dev) and info2["tokens"] - info["tokens"] == steps, (info, info2)
    finally:
        dev.close()
    seq = list(toks[:n0]) + fed
    want = f64.forward(seq)
    # the inputs' condition on the sequence the device chose (test_scale_cases_cpu.py pins it on the oracle's own chain): the CPU
    # oracle, teacher-forced with the device's ids, stays within REF_CAP of float64 there too
    errs, oracle_ids = sc.oracle_errs(g, seq, want)
    picked = fed[1:] + [tok]
    same = sum(picked[i] == oracle_ids[n0 + i] for i in range(steps))
    print(f"\npersistent decode, greedy chain {what}: max|oracle-f64|/std on the device's ids = {max(errs):.2e}; "
          f"{same} of {steps} device ids are the oracle's")
    assert max(errs) <= sc.REF_CAP, max(errs)
    wg = Worst(f"persistent decode, greedy chain {what}")
    for i in range(steps):
        wg.see(rows[i], want.logits[n0 + i], n0 + i)
    w.close()
    wg.close()


@pytest.mark.parametrize("shape_key,wtype,name", sc.PERSIST_CASES, ids=["-".join(c) for c in sc.PERSIST_CASES])
def test_persistent_decode(hip, case, shape_key, wtype, name):
    g, toks, f64, run = case(shape_key, wtype, name)
    what = f"{shape_key}/{wtype}/{name}"
    try:
        _persistent(hip, g, toks, f64, run, what)
    except _PlacementMiss as exc:                              # one retry with a fresh handle; a second miss in a row fails
        print(f"\n[retry] {what}: {exc}")
        _persistent(hip, g, toks, f64, run, what)


# ---- 6. decode batches: dgemm_kernel + dghead_kernel, the split-K head, split-K + bnorm + bswiglu -------------------------------------

# 16 streams whose histories end 3 positions apart; 3 steps: every position 0 .. 47 of the sequence is a row of exactly one step
BATCH_NS, BATCH_STEPS = 16, 3
BATCH_START = [3 * s for s in range(BATCH_NS)]


def _batch_steps(hip, g, toks, monkeypatch, knobs):
    """the three steps on a fresh handle under `knobs`: (logits [step, stream, vocab], bytes of weight copies the steps built)"""
    with monkeypatch.context() as mp:
        for k, v in knobs.items():
            mp.setenv(k, v)
        dev = hip.load_llama_model(g, max_streams=BATCH_NS)
        for s in range(BATCH_NS):
            for pos in range(BATCH_START[s]):                  # histories on single-token steps: the batch steps are the subject
                dev.forward(toks[pos], pos, stream=s)
        w0 = dev.memory_usage()["weights"]
        out = []
        for k in range(BATCH_STEPS):
            pos = [BATCH_START[s] + k for s in range(BATCH_NS)]
            _, lg = dev.forward_batch(list(range(BATCH_NS)), [toks[p] for p in pos], pos, want_logits=True)
            out.append(lg.copy())
        grew = dev.memory_usage()["weights"] - w0
        assert dev.last_error() == ""
        dev.close()
    return np.stack(out), grew


def _check_batch(out, run, what):
    w = Worst(what)
    for k in range(BATCH_STEPS):
        for s in range(BATCH_NS):
            w.see(out[k, s], run.logits[BATCH_START[s] + k], BATCH_START[s] + k)
    w.close()


_HEAD0 = ("hi", "lo", "jump12")
_SPLIT_K = ("hi", "lo", "ramp", "gate", "outlier")


@pytest.mark.parametrize("name", ALL)
def test_decode_batches_on_dgemm(hip, case, monkeypatch, name):
    g, toks, _, run = case("gqa", "q4_0", name)
    assert sorted(BATCH_START[s] + k for s in range(BATCH_NS) for k in range(BATCH_STEPS)) == list(range(len(toks)))
    dg, grew = _batch_steps(hip, g, toks, monkeypatch, {})
    assert grew > 0                                            # dgemm's block-major weight copies were built: it took the steps
    _check_batch(dg, run, f"decode batch, dgemm + dghead gqa/q4_0/{name}")
    sk, grew = _batch_steps(hip, g, toks, monkeypatch, {"NL_DGEMM": "0"})
    assert grew == 0 and sk.tobytes() != dg.tobytes()          # the split-K launches are the other route: other bits
    if name in _SPLIT_K:
        _check_batch(sk, run, f"decode batch, NL_DGEMM=0 gqa/q4_0/{name}")
    if name in _HEAD0:
        h0, grew = _batch_steps(hip, g, toks, monkeypatch, {"NL_DGEMM_HEAD": "0"})
        assert grew > 0 and h0.tobytes() != dg.tobytes() and h0.tobytes() != sk.tobytes()
        _check_batch(h0, run, f"decode batch, dgemm, NL_DGEMM_HEAD=0 gqa/q4_0/{name}")


@pytest.mark.parametrize("name", _SPLIT_K)
def test_decode_batches_on_split_k_q8_0(hip, case, monkeypatch, name):
    g, toks, _, run = case("gqa", "q8_0", name)
    sk, grew = _batch_steps(hip, g, toks, monkeypatch, {"NL_DGEMM": "0"})
    assert grew == 0
    _check_batch(sk, run, f"decode batch, split-K + bnorm + bswiglu gqa/q8_0/{name}")
    # the multi-token step served the batches: a handle held to single-token steps gives other bits
    single, _ = _batch_steps(hip, g, toks, monkeypatch, {"NL_NO_BATCH_PATH": "1"})
    assert single.tobytes() != sk.tobytes()


# ---- 7. a short prompt: 48 tokens in one nl_prefill ----------------------------------------------------------------------------------

PREFIXES = (3, 16, 17, 33, 48)           # a prompt's logits are its last row's: the edges of the 16-token tiles, and the whole sequence


def _prompt(hip, g, toks, run, monkeypatch, knobs, what):
    m = g.meta
    hd, S = m.head_dim, m.seq_len
    nkv = m.num_layers * m.num_kv_heads * S * hd
    with monkeypatch.context() as mp:
        for k, v in knobs.items():
            mp.setenv(k, v)
        dev = hip.load_llama_model(g)
        w0 = dev.memory_usage()["weights"]
        w = Worst(what)
        last = []
        for n in PREFIXES:
            dev.reset()
            dev.prefill(toks[:n])
            last.append(dev.state.logits.copy())
            w.see(last[-1], run.logits[n - 1], n - 1)
        grew = dev.memory_usage()["weights"] - w0
        # every row of the prompt: the K / V rows of layer 1 are behind layer 0's two norms, its SwiGLU and both its writers
        kv_worst = 0.0
        for which, want in (("k_cache", run.k), ("v_cache", run.v)):
            got = dev.debug_read(which, nkv).reshape(m.num_layers, m.num_kv_heads, S, hd)[:, :, :len(toks)]
            assert np.isfinite(got).all(), which
            d = float((np.abs(got.astype(np.float64) - want) / (1.0 + np.abs(want))).max())
            print(f"\n{which} {what}: max|gpu-f64|/(1+|v|) = {d:.2e}")
            kv_worst = max(kv_worst, d)
        assert dev.last_error() == ""
        dev.close()
    w.close()
    assert kv_worst <= KV_TOL, kv_worst
    return np.stack(last), grew


@pytest.mark.parametrize("name", ALL)
def test_short_prompt(hip, case, monkeypatch, name):
    g, toks, _, run = case("gqa", "q4_0", name)
    assert len(toks) == PREFIXES[-1]
    dg, grew = _prompt(hip, g, toks, run, monkeypatch, {}, f"short prompt, dgemm gqa/q4_0/{name}")
    assert grew > 0
    if name in ("hi", "lo", "jump12", "gate"):
        sk, grew = _prompt(hip, g, toks, run, monkeypatch, {"NL_DGEMM": "0"}, f"short prompt, NL_DGEMM=0 gqa/q4_0/{name}")
        assert grew == 0 and sk.tobytes() != dg.tobytes()


# ---- 8. the long-run folded path: qgemm2_kernel producing the next GEMM's fragments under the previous norm's pre-scale -----------

@pytest.mark.parametrize("name", sc.FOLD_CASES)
def test_long_run_folded_norm(hip, case, monkeypatch, name):
    # scale_cases.SHAPES["fold"]: D = I = 1664 x 320 tokens, the smallest two-layer shape whose WO / down / Q|K|V / gate grids all
    # reach 128 workgroups unsplit at <= 320 tokens -- NL_FOLD_NORM 1 and 0 differ bitwise there (asserted below)
    g, toks, _, run = case("fold", "q4_0", name)
    m = g.meta
    hd, S, n = m.head_dim, m.seq_len, len(toks)
    nkv = m.num_layers * m.num_kv_heads * S * hd
    outs = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("NL_FOLD_NORM", knob)
        dev = hip.load_llama_model(g)
        w0 = dev.memory_usage()["weights"]
        dev.prefill(toks)
        outs[knob] = dev.state.logits.copy()
        assert dev.memory_usage()["weights"] == w0            # (not dgemm_kernel: D is no whole number of 256-column groups)
        w = Worst(f"long-run GEMM, NL_FOLD_NORM={knob} fold/q4_0/{name}")
        w.see(outs[knob], run.logits[n - 1], n - 1)
        for which, want in (("k_cache", run.k), ("v_cache", run.v)):      # every row of the prompt, behind layer 0's folded norms
            got = dev.debug_read(which, nkv).reshape(m.num_layers, m.num_kv_heads, S, hd)[:, :, :n]
            assert np.isfinite(got).all(), (knob, which)
            d = float((np.abs(got.astype(np.float64) - want) / (1.0 + np.abs(want))).max())
            print(f"\n{which} NL_FOLD_NORM={knob} fold/q4_0/{name}: max|gpu-f64|/(1+|v|) = {d:.2e}")
            assert d <= KV_TOL, (knob, which, d)
        assert dev.last_error() == ""
        dev.close()
        w.close()
    assert outs["1"].tobytes() != outs["0"].tobytes()          # (the folded path is the one that ran)


# ---- 9. a mixed step: 8 decode rows beside a 32-token chunk of a prompt ------------------------------------------------------------------

MIX_DECODE = [3 + 5 * s for s in range(8)]                     # streams 0 .. 7 stand at positions 3 .. 38; stream 8 takes the prompt


def _mixed(hip, g, toks, monkeypatch, knobs):
    """step A: the decode rows + prompt rows 0 .. 31; step B: the decode rows one further + rows 32 .. 46 + the final prompt token as
    an output row.  Returns [(logits of the output rows, their positions)]."""
    with monkeypatch.context() as mp:
        for k, v in knobs.items():
            mp.setenv(k, v)
        dev = hip.load_llama_model(g, max_streams=9)
        w0 = dev.memory_usage()["weights"]                     # (before the histories: their prefills are multi-token steps too)
        for s, p in enumerate(MIX_DECODE):
            dev.prefill(toks[:p], stream=s, want_logits=False)
        got = []
        for k, (p0, p1) in enumerate(((0, 32), (32, 47))):
            out = [(s, p + k) for s, p in enumerate(MIX_DECODE)] + ([(8, 47)] if p1 == 47 else [])
            rows = out + [(8, p) for p in range(p0, p1)]
            _, lg = dev.forward_mixed([s for s, _ in rows], [toks[p] for _, p in rows], [p for _, p in rows], len(out), want_logits=True)
            got.append((lg.copy(), [p for _, p in out]))
        grew = dev.memory_usage()["weights"] - w0
        assert dev.last_error() == ""
        dev.close()
    return got, grew


@pytest.mark.parametrize("name", ["hi", "lo", "jump12", "gate"])
def test_mixed_step(hip, case, monkeypatch, name):
    g, toks, _, run = case("gqa", "q4_0", name)
    bits = {}
    for route, knobs in (("dgemm", {}), ("NL_DGEMM=0", {"NL_DGEMM": "0"})):
        got, grew = _mixed(hip, g, toks, monkeypatch, knobs)
        assert (grew > 0) == (route == "dgemm"), (route, grew)
        w = Worst(f"mixed step, {route} gqa/q4_0/{name}")
        for lg, pos in got:
            for i, p in enumerate(pos):
                w.see(lg[i], run.logits[p], p)
        w.close()
        bits[route] = np.concatenate([lg for lg, _ in got]).tobytes()
    assert bits["dgemm"] != bits["NL_DGEMM=0"]


# ---- 10. nl_score: the prompt path with the LM head over every row, each row reduced on the device ---------------------------------------

@pytest.mark.parametrize("name", ["hi", "lo"])
def test_score(hip, case, name):
    # reference: float64 log-softmax of the float64 logits.  |d logprob| <= |d x_t| + |d lse| <= 2 max|d x| (tests/test_gpu_score.py),
    # on this work's metric: 2 * 1e-4 * std(f64 row)
    g, toks, _, run = case("gqa", "q4_0", name)
    targets = list(toks[1:]) + [toks[0]]
    want = sc.log_softmax64(run.logits)[np.arange(len(toks)), targets]
    dev = hip.load_llama_model(g)
    w0 = dev.memory_usage()["weights"]
    lp, am = dev.score(toks, targets)
    assert dev.memory_usage()["weights"] > w0 and dev.last_error() == ""       # (the 48-token step ran on dgemm_kernel)
    dev.close()
    assert np.isfinite(lp).all()
    std = run.logits.std(axis=1)
    rel = np.abs(lp.astype(np.float64) - want) / (2 * TOL * std)
    at = int(rel.argmax())
    print(f"\nnl_score gqa/q4_0/{name}: max|gpu-f64| = {float(rel.max()):.3f} of the bound 2e-4 * std (row {at})")
    assert (rel <= 1.0).all(), (at, float(rel.max()))
    top2 = np.partition(run.logits, -2, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 10 * TOL * std
    assert clear.sum() >= 0.9 * len(toks) and (am[clear] == run.logits.argmax(axis=1)[clear]).all()
