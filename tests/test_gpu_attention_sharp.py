"""GPU: every softmax-attention path against the float64 forward of tests/attn_cases.py on inputs in which one key dominates
the softmax (sharp / self / anti / shift, see attn_cases.py) -- the accumulator rescales by alpha -> 0, the split merges in which
every split but one weighs e^-60 or underflows, the maximum that lives in split 0 while the step is in split 2, the -inf guards
next to a finite but enormous gap.  Random synth models reach none of these.

Bound (DESIGN section 5's standing one, here against float64): max|gpu - f64| <= 1e-4 * max(1, std(f64 logits)) at every checked
step.  tests/test_attn_cases_cpu.py holds the CPU oracle to half of that on the same inputs, so a failure here is not the
input's fault.  Every test asserts that the kernel it is about served the steps (launch kinds of the plan, plan_info,
persist_info, or a bitwise difference from the route that would have served them otherwise) and prints its worst value.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_cases as ac  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = ac.GPU_TOL
KV_TOL = 2e-5            # single ops, DESIGN section 5: |d| <= 2e-5 * (1 + |v|)
THREE = ("sharp", "self", "anti")
SHIFT = ("shift_pos", "shift_neg")


@pytest.fixture(scope="module")
def hip():
    from nanollama_amd import _lib, model
    if _lib.lib().nl_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return model


_cases = {}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """(loaded GGUF, token sequence, float64 run over it) of a (shape, weight type, case): built once per module"""
    def get(shape_key, wtype, name):
        key = (shape_key, wtype, name)
        assert key in ac.CASES, f"{key} is not pinned by test_attn_cases_cpu.py"
        if key not in _cases:
            g = ac.build_case(str(tmp_path_factory.mktemp("sharp") / "m.gguf"), shape_key, wtype, name)
            toks = ac.tokens(shape_key)
            _cases[key] = (g, toks, ac.F64Model(g), ac.forward_f64(g, toks))
        g, toks, f64, run = _cases[key]
        return g, toks, f64, run
    return get


class Worst:
    """the largest max|gpu - f64| / max(1, std) of a test, and where"""

    def __init__(self, what):
        self.what, self.err, self.at = what, 0.0, None

    def see(self, got, want64, at):
        e = ac.rel_err(got, want64)
        if e > self.err:
            self.err, self.at = e, at
        return e

    def close(self, run=None):
        note = ""
        if run is not None and isinstance(self.at, int):
            note = f", smallest top-two margin of that step {float(run.top2_gap[self.at].min()):.2f} nats"
        print(f"\n{self.what}: max|gpu-f64|/max(1,std) = {self.err:.2e} (at {self.at}{note})")
        assert self.err <= TOL, (self.what, self.err, self.at)


def _kinds(dev, pos):
    return {k: c for k, (ms, c) in dev.profile_forward(5, pos, iters=1).items() if c}


def _teacher_forced(dev, toks, run, w):
    for pos, t in enumerate(toks):
        dev.forward(t, pos)
        w.see(dev.state.logits, run.logits[pos], pos)


# ---- 1. the general single-token plan: attn_kernel, its 128-key splits and the merge in the WO GEMV's prologue ------------------

@pytest.mark.parametrize("shape_key,wtype,name",
                         [("gqa", "q8_0", c) for c in THREE] + [("gqa", "f16", c) for c in THREE]
                         + [("gqa_bias", "q8_0", c) for c in SHIFT] + [("hd32_g3", "q8_0", "sharp")])
def test_general_single_token_plan(hip, case, monkeypatch, shape_key, wtype, name):
    g, toks, _, run = case(shape_key, wtype, name)
    monkeypatch.setenv("NL_FUSED_ATTN", "0")
    monkeypatch.setenv("NL_PERSIST", "0")
    dev = hip.load_llama_model(g)
    assert dev.plan_info()["fused_mode"] == 0 and not dev.persist_info()["ready"], (dev.plan_info(), dev.persist_info())
    w = Worst(f"general plan {shape_key}/{wtype}/{name}")
    _teacher_forced(dev, toks, run, w)                         # positions 0 .. 299: one split, two, three
    for pos in (20, 200, 290):
        k = _kinds(dev, pos)
        assert k.get("attention") == g.meta.num_layers and k.get("wo_resid") == g.meta.num_layers and "attn_block" not in k, (pos, k)
    dev.close()
    w.close(run)


# ---- 2. the fused block plan: attn_block_kernel across its 128-position pass boundary ------------------------------------------

@pytest.mark.parametrize("shape_key,wtype,name",
                         [("mha3", "q8_0", c) for c in THREE] + [("gqa", "q4_0", "sharp")] + [("gqa_bias", "q8_0", c) for c in SHIFT])
def test_fused_block_plan(hip, case, monkeypatch, shape_key, wtype, name):
    g, toks, _, run = case(shape_key, wtype, name)
    monkeypatch.setenv("NL_FUSED_MAX_POS", "4096")
    monkeypatch.setenv("NL_PERSIST", "0")                      # (the 256-wide shapes would otherwise go to the resident session)
    dev = hip.load_llama_model(g)
    info = dev.plan_info()
    assert info["fused_mode"] == 1 and info["fused_max_pos"] == 4096 and not dev.persist_info()["ready"], info
    w = Worst(f"fused block {shape_key}/{wtype}/{name}")
    _teacher_forced(dev, toks, run, w)
    for pos in (20, 200, 290):
        k = _kinds(dev, pos)
        assert k.get("attn_block") == g.meta.num_layers and "attention" not in k and "qkv_rope" not in k and "wo_resid" not in k, (pos, k)
    assert dev.last_error() == ""                              # (no exchange timed out: the block did serve every step)
    dev.close()
    w.close(run)


# ---- 3. the wide tier: qkv_attn_kernel (projection + attention, WO its own launch) and tp_attn_kernel (WO in the launch) ---------

@pytest.mark.parametrize("wo", ["wo_own_launch", "wo_in_the_launch"])
@pytest.mark.parametrize("name", THREE)
def test_wide_tier_projection_attention_launch(hip, case, monkeypatch, name, wo):
    g, toks, _, run = case("wide", "q4_0", name)
    if wo == "wo_own_launch":
        monkeypatch.setenv("NL_ATTN_WO", "0")
    monkeypatch.setenv("NL_FUSED_MAX_POS", "4096")
    dev = hip.load_llama_model(g)
    assert dev.plan_info()["fused_mode"] == (2 if wo == "wo_own_launch" else 4), dev.plan_info()
    w = Worst(f"wide tier {wo} q4_0/{name}")
    _teacher_forced(dev, toks, run, w)                         # 160 positions: across the launch's 128-position pass boundary
    for pos in (20, 150):
        k = _kinds(dev, pos)
        assert k.get("attn_block") == g.meta.num_layers and "qkv_rope" not in k and "attention" not in k, (pos, k)
        assert k.get("wo_resid") == (g.meta.num_layers if wo == "wo_own_launch" else None), (pos, k)
    assert dev.last_error() == ""
    dev.close()
    w.close(run)


# ---- 4. the persistent decode: pd_decode_kernel through nl_decode_greedy and through the resident session -----------------------

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
        # (a) the resident session: per-call Forward over the whole sequence, passes of 128 keys from position 128 and 256 on
        w = Worst(f"persistent decode, resident session {what}")
        _teacher_forced(dev, toks, run, w)
        info = dev.persist_info()          # (one resident launch unless the host paused longer than the idle limit)
        assert _no_warning(dev) and info["tokens"] == len(toks) and 1 <= info["launches"] <= 4, info
        # (b) chained greedy steps at positions 100 .. 159: below 128 a head's single record, above it the merge of the records
        # in LDS.  The device picks its own tokens; the float64 forward is fed the ids it produced.
        dev.reset()
        n0, steps = ac.PERSIST_PROMPT, ac.PERSIST_STEPS
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
    # the inputs' condition on the sequence the device chose (test_attn_cases_cpu.py pins it on the oracle's own chain): the CPU
    # oracle, teacher-forced with the device's ids, stays within REF_CAP of float64 there too
    errs, oracle_ids = ac.oracle_errs(g, seq, want)
    picked = fed[1:] + [tok]                                         # the id the device chose at positions n0 .. n0 + steps - 1
    same = sum(picked[i] == oracle_ids[n0 + i] for i in range(steps))
    print(f"\npersistent decode, greedy chain {what}: max|oracle-f64| on the device's ids = {max(errs):.2e}; "
          f"{same} of {steps} device ids are the oracle's (all: the device followed the oracle's own chain)")
    assert max(errs) <= ac.REF_CAP, max(errs)
    wg = Worst(f"persistent decode, greedy chain {what}")
    for i in range(steps):
        wg.see(rows[i], want.logits[n0 + i], n0 + i)
    if what.endswith("/self"):             # on the ids the device chose the newest key still wins every row
        cov = ac.coverage(want, range(n0, n0 + steps))
        assert cov["max_is_newest_key"] == cov["rows"], cov
    w.close(run)
    wg.close(want)


@pytest.mark.parametrize("shape_key", ["mha4", "gqa"])        # the kv = 4 and the kv = 2 instantiation
@pytest.mark.parametrize("name", THREE)
def test_persistent_decode(hip, case, name, shape_key):
    g, toks, f64, run = case(shape_key, "q8_0", name)
    what = f"{shape_key}/q8_0/{name}"
    try:
        _persistent(hip, g, toks, f64, run, what)
    except _PlacementMiss as exc:                              # one retry with a fresh handle; a second miss in a row fails
        print(f"\n[retry] {what}: {exc}")
        _persistent(hip, g, toks, f64, run, what)


# ---- 5. decode batches: attn_kernel with items, its FIN variant, attn_rope_prologue and battn_merge_kernel ----------------------------

# Five streams at ragged positions, five steps each.  A step's attention grid has as many 128-key splits as its deepest row needs
# (batched_step, nl_engine.hip), and the engine rotates q / k inside the attention launch (attn_rope_prologue, which also adds the
# biases and stores the K / V rows) only while that is at most two and the Q|K|V GEMM is the plain one (Q8_0 / F16 files; a Q4_0
# file's short steps go to dgemm_kernel, which rotates in its own epilogue):
#   one_split     every position below 128: attn_kernel<FIN> writes the WO fragments itself, no merge launch;  NL_ROPE_IN_ATTN acts
#   two_splits    positions 3 .. 204, two streams cross 128: items + battn_merge_kernel over two partials;      NL_ROPE_IN_ATTN acts
#   three_splits  positions 3 .. 294, straddling 128 and 256: items + battn_merge_kernel over three partials; the knob is inert (the
#                 brope_kv launch rotates whatever it says), both values run because the step graph is keyed on it
BATCH_STARTS = {"one_split": [0, 3, 60, 100, 122], "two_splits": [3, 100, 124, 126, 200], "three_splits": [3, 125, 127, 254, 290]}
BATCH_STEPS = 5
_Q8_BATCH = [("gqa", "q8_0", c) for c in THREE] + [("gqa_bias", "q8_0", c) for c in SHIFT] + [("gqa_conj", "q8_0", "sharp")]


@pytest.mark.parametrize("layout,shape_key,wtype,name",
                         [(lay,) + c for lay in ("one_split", "two_splits") for c in _Q8_BATCH]
                         + [("three_splits",) + c for c in _Q8_BATCH[:5] + [("gqa_conj", "q4_0", "sharp")]])
def test_decode_batches(hip, case, monkeypatch, layout, shape_key, wtype, name):
    g, toks, _, run = case(shape_key, wtype, name)
    start = BATCH_STARTS[layout]
    ns = len(start)
    assert max(start) + BATCH_STEPS - 1 < {"one_split": 128, "two_splits": 256, "three_splits": 300}[layout]
    assert layout == "one_split" or any(s < 128 <= s + BATCH_STEPS - 1 for s in start)

    def steps(dev):
        for s in range(ns):
            if start[s]:
                dev.prefill(toks[:start[s]], stream=s, want_logits=False)
        out = []
        for k in range(BATCH_STEPS):
            pos = [start[s] + k for s in range(ns)]
            ids, lg = dev.forward_batch(list(range(ns)), [toks[p] for p in pos], pos, want_logits=True)
            out.append(lg.copy())
        return np.stack(out)

    outs = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("NL_ROPE_IN_ATTN", knob)
        dev = hip.load_llama_model(g, max_streams=ns)
        outs[knob] = steps(dev)
        dev.close()
        w = Worst(f"decode batch {layout} NL_ROPE_IN_ATTN={knob} {shape_key}/{wtype}/{name}")
        for k in range(BATCH_STEPS):
            for s in range(ns):
                w.see(outs[knob][k, s], run.logits[start[s] + k], start[s] + k)
        w.close(run)
    # attn_rope_prologue and brope_kv_kernel do the same arithmetic in the same order (test_gpu_parity.py): equal bits.  No counter
    # tells the two apart, so which of them ran is the engine's rule above, not something this test observes; on three_splits the
    # equality is trivial.
    assert np.array_equal(outs["1"], outs["0"])
    # What IS observed: the multi-token step served the batches -- a handle held to single-token steps (NL_NO_BATCH_PATH) gives
    # other bits.  That handle differs in its GEMVs as well, so this shows the batched step ran, of which attn_kernel with items
    # (and the merge from two splits on) is the only attention route for rows of different streams; it does not single them out.
    monkeypatch.setenv("NL_NO_BATCH_PATH", "1")
    single = hip.load_llama_model(g, max_streams=ns)
    assert steps(single).tobytes() != outs["1"].tobytes()
    single.close()


# ---- 6. prompts: attn_tile16_kernel with prebuilt fp16 hi / lo K/V images and with per-chunk conversion --------------------------

@pytest.mark.parametrize("shape_key,wtype,name",
                         [("gqa", "q4_0", "sharp")] + [("gqa", "f16", c) for c in THREE] + [("gqa_bias", "q8_0", c) for c in SHIFT])
def test_prompts(hip, case, monkeypatch, shape_key, wtype, name):
    g, toks, _, run = case(shape_key, wtype, name)
    m = g.meta
    hd, S = m.head_dim, m.seq_len
    nkv = m.num_layers * m.num_kv_heads * S * hd
    last, cache = {}, {}
    for kv16_min in (16, 1 << 30):                             # images built once per layer for every prefix / converted per chunk
        monkeypatch.setenv("NL_KV16_MIN_TOKENS", str(kv16_min))
        dev = hip.load_llama_model(g)
        w = Worst(f"prompt, images from {kv16_min} tokens {shape_key}/{wtype}/{name}")
        for n in (130, 257, 300):                              # a prompt's logits are its last row's: three prefixes
            dev.reset()
            dev.prefill(toks[:n])
            last[kv16_min, n] = dev.state.logits.copy()
            w.see(last[kv16_min, n], run.logits[n - 1], n - 1)
        kv_worst = 0.0
        for which, want in (("k_cache", run.k), ("v_cache", run.v)):
            got = dev.debug_read(which, nkv).reshape(m.num_layers, m.num_kv_heads, S, hd)[:, :, :300]
            cache[kv16_min, which] = got
            d = float((np.abs(got.astype(np.float64) - want) / (1.0 + np.abs(want))).max())
            print(f"\n{which} {shape_key}/{wtype}/{name}, images from {kv16_min}: max|gpu-f64|/(1+|v|) = {d:.2e}")
            kv_worst = max(kv_worst, d)
        dev.close()
        w.close(run)
        assert kv_worst <= KV_TOL, kv_worst
    # The images hold the fp16 hi / lo halves the per-chunk conversion computes and the chunks are folded in the same order: the
    # two variants agree to the last bit.  (So no bit tells which of them ran; NL_KV16_MIN_TOKENS is what selects it.)
    for n in (130, 257, 300):
        assert last[16, n].tobytes() == last[1 << 30, n].tobytes(), n
    for which in ("k_cache", "v_cache"):
        assert cache[16, which].tobytes() == cache[1 << 30, which].tobytes(), which
    # Observed: the multi-token step served the prompt -- single-token steps (NL_NO_BATCH_PATH) give other bits.  Within that step
    # a run of 8 or more rows of one stream has no attention route but the tile kernel (attn_tile_supported(2)); the difference
    # itself also comes from the GEMMs and does not single the kernel out.
    monkeypatch.setenv("NL_NO_BATCH_PATH", "1")
    single = hip.load_llama_model(g)
    single.prefill(toks[:130])
    assert single.state.logits.tobytes() != last[16, 130].tobytes()
    single.close()


# ---- 7. mixed steps: attn_seg_kernel for the prompt chunk, the per-token route as the other ---------------------------------------

def _mixed_steps(toks, chunk):
    """a 200-token prompt (stream 2) beside two decode rows that stand at 130 and 260.  chunk 199: ONE step carries the whole
    prompt -- a single segment of 199 rows (seven query tiles of 32, tiles that straddle key 128) and its final token as an output
    row; chunk 64: the same prompt admitted as 64 / 64 / 64 / 7 rows (segments that start at a position > 0, a short last one)."""
    steps, a, b = [], 130, 260
    bounds = [(p0, min(p0 + chunk, 199)) for p0 in range(0, 199, chunk)]
    for k, (p0, p1) in enumerate(bounds):
        out = [(0, a + k), (1, b + k)] + ([(2, 199)] if p1 == 199 else [])      # the final prompt token joins as an output row
        rows = out + [(2, p) for p in range(p0, p1)]
        steps.append(([s for s, _ in rows], [toks[p] for _, p in rows], [p for _, p in rows], len(out)))
    k = len(bounds)
    steps.append(([0, 1, 2], [toks[a + k], toks[b + k], toks[200]], [a + k, b + k, 200], 3))   # a decode step over the chunk's K / V
    return steps


def _mixed_run(hip, g, toks, chunk, knob, monkeypatch):
    """the steps of _mixed_steps on a fresh handle: (logits of the output rows per step, their positions)"""
    monkeypatch.setenv("NL_MIXED_ATTN", knob)
    dev = hip.load_llama_model(g, max_streams=3)
    dev.prefill(toks[:130], stream=0, want_logits=False)
    dev.prefill(toks[:260], stream=1, want_logits=False)
    got = []
    for streams, tk, pos, n_out in _mixed_steps(toks, chunk):
        ids, lg = dev.forward_mixed(streams, tk, pos, n_out, want_logits=True)
        got.append((lg.copy(), pos[:n_out]))
    dev.close()
    return got


@pytest.mark.parametrize("chunk", [199, 64])
@pytest.mark.parametrize("shape_key,wtype,name", [("gqa", "q8_0", c) for c in THREE] + [("gqa_bias", "q8_0", c) for c in SHIFT])
def test_mixed_steps(hip, case, monkeypatch, shape_key, wtype, name, chunk):
    g, toks, _, run = case(shape_key, wtype, name)
    monkeypatch.setenv("NL_MIXED_ATTN_MIN", "0")               # (the default threshold keeps steps this small on the per-token kernel)
    outs = {}
    for knob in ("1", "0"):
        w = Worst(f"mixed steps, chunks of {chunk}, NL_MIXED_ATTN={knob} {shape_key}/{wtype}/{name}")
        got = _mixed_run(hip, g, toks, chunk, knob, monkeypatch)
        for lg, pos in got:
            for i, p in enumerate(pos):
                w.see(lg[i], run.logits[p], p)
        outs[knob] = np.concatenate([lg for lg, _ in got])
        w.close(run)
    # The segment-tile kernel did take the chunks: other bits than the per-token route (the two handles differ in nothing else).
    # Which route serves a step depends on the knobs and the step's rows, not on the weights; under `self` every softmax is one-hot
    # to the last bit and both routes return the newest V row exactly, so there the same steps on the `sharp` file of the shape
    # are the witness.
    if name == "self":
        gs, _, _, _ = case(shape_key, wtype, "sharp")
        outs = {knob: np.concatenate([lg for lg, _ in _mixed_run(hip, gs, toks, chunk, knob, monkeypatch)]) for knob in ("1", "0")}
    assert outs["1"].tobytes() != outs["0"].tobytes()
