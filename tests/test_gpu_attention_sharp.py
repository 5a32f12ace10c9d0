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
KV_TOL = ac.KV_TOL       # single ops, DESIGN section 5: |d| <= 2e-5 * (1 + |v|)
THREE = ("sharp", "self", "anti")
SHIFT = ("shift_pos", "shift_neg")
# the bound, the witnesses and the layouts live beside forward_f64: tests/test_gpu_attention_geometry.py runs them over every
# (head_dim, GQA group) instantiation
Worst, _kinds, _teacher_forced = ac.Worst, ac.kinds, ac.teacher_forced


@pytest.fixture(scope="module")
def hip():
    from nanollama_amd import _lib, model
    if _lib.lib().nl_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return model


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """(loaded GGUF, token sequence, float64 run over it) of a (shape, weight type, case): built once per session"""
    def get(shape_key, wtype, name):
        return ac.cached_case(lambda: tmp_path_factory.mktemp("sharp"), (shape_key, wtype, name))
    return get


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

_PlacementMiss, _no_warning = ac.PlacementMiss, ac.no_warning
_persistent = ac.persistent_run


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

# the layouts (five streams at ragged positions, five steps each) and what each of them reaches: attn_cases.BATCH_STARTS
BATCH_STARTS, BATCH_STEPS = ac.BATCH_STARTS, ac.BATCH_STEPS
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
        return ac.batch_run(dev, toks, start)

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
    last, cache = {}, {}
    for kv16_min in (16, 1 << 30):                             # images built once per layer for every prefix / converted per chunk
        monkeypatch.setenv("NL_KV16_MIN_TOKENS", str(kv16_min))
        dev = hip.load_llama_model(g)
        w = Worst(f"prompt, images from {kv16_min} tokens {shape_key}/{wtype}/{name}")
        lg, kv, kv_worst = ac.prompt_run(dev, g, toks, run, w, f"{shape_key}/{wtype}/{name}, images from {kv16_min}")
        for n in ac.PROMPT_PREFIXES:
            last[kv16_min, n] = lg[n]
        for which in ("k_cache", "v_cache"):
            cache[kv16_min, which] = kv[which]
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

_mixed_steps, _mixed_run = ac.mixed_steps, ac.mixed_run


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
