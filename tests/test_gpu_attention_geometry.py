"""GPU: every (head_dim, GQA group) instantiation of the attention kernels against the float64 forward of tests/attn_cases.py.

nl_create admits head_dim 32 / 64 x 1, 2, 3, 4, 6, 8 query heads per kv head, and every attention kernel is a template over that
pair: attn_kernel<HD, G, FIN, ROPE> takes all six group sizes; attn_tile16_kernel, attn_tile_kernel and attn_seg_kernel<HD, G, QT>
take G in {1, 2, 3, 4, 8} with QT = 64 / 32 / 16 / 16 / 8 rows (the prebuilt K/V images double that); Kv16Image / kv16_build_kernel
depend on head_dim; the fused launches need head_dim 64; G = 6 has no tile kernel, its prompts go to attn_kernel per token.  A wrong
row-to-head mapping, a partial last query tile or a bad kv-head offset shows only at the geometry that instantiates it, and only on
inputs whose softmax bookkeeping does real work: tests/test_gpu_attention_sharp.py reaches those branches at (64, 2); this file runs
the same routes over all twelve geometries (attn_cases.GEO: two-layer models with two kv heads, D = hd * 2G), `sharp` and `anti`.

Bounds -- the standing ones: logits max|gpu - f64| <= 1e-4 * max(1, std(f64 logits)) at every checked step, K / V rows within
2e-5 * (1 + |v|).  tests/test_attn_cases_cpu.py holds the CPU oracle to half the first on every case.  Every test prints its worst
value and where, and asserts that the route it is about served the steps: launch kinds, plan_info, persist_info, or a bitwise
difference from the route that would otherwise have served them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attn_cases as ac  # noqa: E402
import attn_geometry_worker as worker  # noqa: E402

pytestmark = pytest.mark.gpu

KV_TOL = ac.KV_TOL
Worst = ac.Worst
GEOS = ac.GEOMETRIES
TILE_GROUPS = (1, 2, 3, 4, 8)            # attn_tile_supported (nl_engine.hip): the G the tile, tile16 and segment kernels exist for
TWO = ("sharp", "anti")


def _gid(v):
    return f"hd{v[0]}-g{v[1]}" if isinstance(v, tuple) else str(v)


geos = pytest.mark.parametrize("geo", GEOS, ids=_gid)


@pytest.fixture(scope="module")
def hip():
    from nanollama_amd import _lib, model
    if _lib.lib().nl_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    for k in PROCESS_KNOBS:                  # read once per process: this process must be on the default routes
        assert k not in os.environ, k
    return model


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """(loaded GGUF, token sequence, F64Model, float64 run) of a geometry's (weight type, case): built once per session"""
    def get(geo, wtype, name):
        key = (ac.GEO[geo], wtype, name)
        g, toks, f64, run = ac.cached_case(lambda: tmp_path_factory.mktemp("geo"), key)
        m = g.meta
        assert (m.head_dim or m.embed_dim // m.num_heads, m.num_heads // m.num_kv_heads, m.num_kv_heads) == (geo[0], geo[1], 2)
        return g, toks, f64, run, f"hd{geo[0]} g{geo[1]} {'/'.join(key)}"
    return get


# ---- 1. the general single-token plan: attn_kernel<HD, G>, one to three 128-key splits, the merge in the WO GEMV's prologue ------

@pytest.mark.parametrize("name", TWO)
@geos
def test_general_single_token_plan(hip, case, monkeypatch, geo, name):
    g, toks, _, run, what = case(geo, "q8_0", name)
    monkeypatch.setenv("NL_FUSED_ATTN", "0")
    monkeypatch.setenv("NL_PERSIST", "0")
    dev = hip.load_llama_model(g)
    assert dev.plan_info()["fused_mode"] == 0 and not dev.persist_info()["ready"], (dev.plan_info(), dev.persist_info())
    w = Worst(f"general plan {what}")
    ac.teacher_forced(dev, toks, run, w)                       # positions 0 .. 299: one split, two, three
    for pos in (20, 200, 290):
        k = ac.kinds(dev, pos)
        assert k.get("attention") == g.meta.num_layers and k.get("wo_resid") == g.meta.num_layers and "attn_block" not in k, (pos, k)
    dev.close()
    w.close(run)


# ---- 2. decode batches: attn_kernel<HD, G> with items, its FIN variant, attn_rope_prologue and battn_merge_kernel ----------------

@pytest.mark.parametrize("layout,geo,wtype",
                         [(lay, geo, "q8_0") for lay in ("one_split", "two_splits", "three_splits") for geo in GEOS]
                         + [("three_splits", geo, "q4_0") for geo in ac.GEO_Q4], ids=_gid)
def test_decode_batches(hip, case, monkeypatch, layout, geo, wtype):
    # (what each layout reaches: attn_cases.BATCH_STARTS; a Q4_0 file's steps rotate in dgemm_kernel's epilogue)
    g, toks, _, run, what = case(geo, wtype, "sharp")
    start = ac.BATCH_STARTS[layout]
    ns = len(start)
    assert max(start) + ac.BATCH_STEPS - 1 < ac.BATCH_BELOW[layout]
    assert layout == "one_split" or any(s < 128 <= s + ac.BATCH_STEPS - 1 for s in start)
    outs = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("NL_ROPE_IN_ATTN", knob)
        dev = hip.load_llama_model(g, max_streams=ns)
        outs[knob] = ac.batch_run(dev, toks, start)
        dev.close()
        w = Worst(f"decode batch {layout} NL_ROPE_IN_ATTN={knob} {what}")
        ac.batch_see(w, outs[knob], run, start)
        w.close(run)
    # attn_rope_prologue and brope_kv_kernel do the same arithmetic in the same order: equal bits (on three_splits trivially)
    assert np.array_equal(outs["1"], outs["0"])
    # the multi-token step served the batches: a handle held to single-token steps (NL_NO_BATCH_PATH) gives other bits
    monkeypatch.setenv("NL_NO_BATCH_PATH", "1")
    single = hip.load_llama_model(g, max_streams=ns)
    assert ac.batch_run(single, toks, start).tobytes() != outs["1"].tobytes()
    single.close()


# ---- 3. prompts: attn_tile16_kernel<HD, G, QT> with prebuilt fp16 hi / lo K/V images (Kv16Image<HD>, twice the rows) and without --

def _prompts(hip, g, toks, run, what, monkeypatch, kv16_min):
    if kv16_min is None:
        monkeypatch.delenv("NL_KV16_MIN_TOKENS", raising=False)
    else:
        monkeypatch.setenv("NL_KV16_MIN_TOKENS", str(kv16_min))
    dev = hip.load_llama_model(g)
    w = Worst(f"prompt, images from {kv16_min} tokens {what}")
    last, cache, kv_worst = ac.prompt_run(dev, g, toks, run, w, f"{what}, images from {kv16_min}")
    dev.close()
    w.close(run)
    assert kv_worst <= KV_TOL, kv_worst
    return last, cache


@pytest.mark.parametrize("name", TWO)
@geos
def test_prompts(hip, case, monkeypatch, geo, name):
    # Prefixes 130, 257 and 300: at every QT (8, 16, 32, 64 and their doubles) a partial last query tile and a tile across key 128.
    # G = 6: attn_tile_supported(6) is false (nl_engine.hip) -- no tile kernel is instantiated for it, so the rows of a G = 6 prompt
    # attend on attn_kernel<HD, 6> per token with as many splits as the deepest row needs, behind the same multi-token GEMMs, and
    # NL_KV16_MIN_TOKENS selects nothing.  The result is held to float64 all the same.
    g, toks, _, run, what = case(geo, "q8_0", name)
    last, cache = {}, {}
    for kv16_min in (16, 1 << 30):                             # images built once per layer for every prefix / converted per chunk
        last[kv16_min], cache[kv16_min] = _prompts(hip, g, toks, run, what, monkeypatch, kv16_min)
    # the images hold the fp16 hi / lo halves the per-chunk conversion computes, the chunks are folded in the same order: equal bits
    for n in ac.PROMPT_PREFIXES:
        assert last[16][n].tobytes() == last[1 << 30][n].tobytes(), n
    for which in ("k_cache", "v_cache"):
        assert cache[16][which].tobytes() == cache[1 << 30][which].tobytes(), which
    # the multi-token step served the prompt: single-token steps (NL_NO_BATCH_PATH) give other bits.  Within that step a run of 8 or
    # more rows of one stream has no attention route but the tile kernel where attn_tile_supported(G)
    monkeypatch.setenv("NL_NO_BATCH_PATH", "1")
    single = hip.load_llama_model(g)
    single.prefill(toks[:130])
    assert single.state.logits.tobytes() != last[16][130].tobytes()
    single.close()


# ---- 4. mixed steps: attn_seg_kernel<HD, G, QT> for the prompt chunk, the per-token route as the other ---------------------------

@pytest.mark.parametrize("chunk", [199, 64])
@pytest.mark.parametrize("name", TWO)
@geos
def test_mixed_steps(hip, case, monkeypatch, geo, name, chunk):
    g, toks, _, run, what = case(geo, "q8_0", name)
    monkeypatch.setenv("NL_MIXED_ATTN_MIN", "0")               # (the default threshold keeps steps this small on the per-token kernel)
    outs = {}
    for knob in ("1", "0"):
        w = Worst(f"mixed steps, chunks of {chunk}, NL_MIXED_ATTN={knob} {what}")
        got = ac.mixed_run(hip, g, toks, chunk, knob, monkeypatch)
        for lg, pos in got:
            for i, p in enumerate(pos):
                w.see(lg[i], run.logits[p], p)
        outs[knob] = np.concatenate([lg for lg, _ in got])
        w.close(run)
    if geo[1] in TILE_GROUPS:
        # the segment-tile kernel did take the chunks: other bits than the per-token route (the two handles differ in nothing else)
        assert outs["1"].tobytes() != outs["0"].tobytes()
    else:
        # G = 6: nl_forward_mixed builds the segment work list only if `mixed_attn && attn_tile_supported(gqa)`; with no list every
        # row of the step attends on attn_kernel<HD, 6>, whatever NL_MIXED_ATTN says -- the two handles run the same launches
        assert geo[1] == 6 and outs["1"].tobytes() == outs["0"].tobytes()


# ---- 5. the fused launches and the persistent decode: head_dim 64 only -----------------------------------------------------------

# What nl_finalize admits for each geometry model when loaded with NL_FUSED_MAX_POS=4096 and NL_PERSIST=0: plan_info's fused_mode by
# default and under NL_ATTN_WO=0, and whether the persistent decode is ready (max_pos 320) with neither knob set.
#   mode 1  attn_block_kernel, one workgroup per (head, member)         mode 2  qkv_attn_kernel, WO its own launch
#   mode 4  the same launch with WO inside it (tp_attn_kernel's attention half on one GPU)
# 0 / False rows are the pairs the engine does NOT admit, asserted below: the fused launches need head_dim 64 and a G the tile
# kernels exist for (nl_finalize: `if (!attn_tile_supported(gqa)) fused_mode = 0`), D 128 .. 512 is mode 1's tier and D 1024 the
# projection + attention launch's; pd_decode_kernel is instantiated for D 256 / I 512 with 2 or 4 kv heads (and nano's shape)
# only, which of these models is (64, 2) alone.  A change that admits another pair fails here until this file covers it.
ADMITTED = {  # geometry: (fused_mode, fused_mode under NL_ATTN_WO=0, persistent decode ready)
    (32, 1): (0, 0, False), (32, 2): (0, 0, False), (32, 3): (0, 0, False),
    (32, 4): (0, 0, False), (32, 6): (0, 0, False), (32, 8): (0, 0, False),
    (64, 1): (1, 1, False), (64, 2): (1, 1, True), (64, 3): (1, 1, False),
    (64, 4): (1, 1, False), (64, 6): (0, 0, False), (64, 8): (4, 2, False),
}


def _fused_env(monkeypatch, attn_wo0):
    monkeypatch.setenv("NL_FUSED_MAX_POS", "4096")
    monkeypatch.setenv("NL_PERSIST", "0")
    if attn_wo0:
        monkeypatch.setenv("NL_ATTN_WO", "0")
    else:
        monkeypatch.delenv("NL_ATTN_WO", raising=False)


@geos
def test_modes_not_admitted(hip, case, monkeypatch, geo):
    g, _, _, _, what = case(geo, "q8_0", "sharp")
    seen = []
    for attn_wo0 in (False, True):
        _fused_env(monkeypatch, attn_wo0)
        dev = hip.load_llama_model(g)
        seen.append(dev.plan_info()["fused_mode"])
        assert not dev.persist_info()["ready"]
        dev.close()
    for k in ("NL_FUSED_MAX_POS", "NL_PERSIST", "NL_ATTN_WO"):
        monkeypatch.delenv(k, raising=False)
    dev = hip.load_llama_model(g)
    info = dev.persist_info()
    seen.append(bool(info["ready"]))
    assert not info["ready"] or info["max_pos"] == 320, info
    dev.close()
    print(f"\nadmitted {what}: fused_mode {seen[0]}, under NL_ATTN_WO=0 {seen[1]}, persistent decode ready {seen[2]}")
    assert tuple(seen) == ADMITTED[geo], (geo, seen, ADMITTED[geo])
    if geo[0] == 32 or geo[1] not in TILE_GROUPS:
        assert tuple(seen) == (0, 0, False)


_FUSED = [(geo, wo0) for geo in GEOS for wo0 in (False, True) if ADMITTED[geo][wo0] and (not wo0 or ADMITTED[geo][1] != ADMITTED[geo][0])]


@pytest.mark.parametrize("name", TWO)
@pytest.mark.parametrize("geo,attn_wo0", _FUSED, ids=_gid)
def test_fused_launches(hip, case, monkeypatch, geo, attn_wo0, name):
    # (NL_ATTN_WO=0 is run where it selects another mode than the default: on the mode 1 models it selects nothing)
    g, toks, _, run, what = case(geo, "q8_0", name)
    _fused_env(monkeypatch, attn_wo0)
    dev = hip.load_llama_model(g)
    info, mode = dev.plan_info(), ADMITTED[geo][attn_wo0]
    assert info["fused_mode"] == mode and info["fused_max_pos"] >= len(toks) and not dev.persist_info()["ready"], info
    w = Worst(f"fused mode {mode} {what}")
    ac.teacher_forced(dev, toks, run, w)                       # 300 positions: across the launches' 128- and 256-position passes
    L = g.meta.num_layers
    for pos in (20, 200, 290):
        k = ac.kinds(dev, pos)
        assert k.get("attn_block") == L and "attention" not in k and "qkv_rope" not in k, (pos, k)
        assert k.get("wo_resid") == (L if mode == 2 else None), (pos, k)      # (mode 2: WO its own launch)
    assert dev.last_error() == ""                              # (no exchange timed out: the launch did serve every step)
    dev.close()
    w.close(run)


@pytest.mark.parametrize("name", TWO)
@pytest.mark.parametrize("geo", [geo for geo in GEOS if ADMITTED[geo][2]], ids=_gid)
def test_persistent_decode(hip, case, geo, name):
    g, toks, f64, run, what = case(geo, "q8_0", name)
    try:
        ac.persistent_run(hip, g, toks, f64, run, what)
    except ac.PlacementMiss as exc:                            # one retry with a fresh handle; a second miss in a row fails
        print(f"\n[retry] {what}: {exc}")
        ac.persistent_run(hip, g, toks, f64, run, what)


# ---- 6. the routes that process knobs select: one child process per knob ---------------------------------------------------------

PROCESS_KNOBS = ("NL_ATTN_F32", "NL_NO_ATTN_TILE", "NL_NO_ATTN_FIN")
CHILD_TIMEOUT = 240
_dead_child = []                         # an abort, a segmentation fault or a time-out of a child: no further child is started


def _child(knob, which, geo_list):
    if _dead_child:
        pytest.fail(f"not started: the child of {_dead_child[0]} aborted, faulted or timed out")
    env = {k: v for k, v in os.environ.items() if k not in PROCESS_KNOBS}
    env[knob] = "1"
    cmd = [sys.executable, os.path.join(HERE, "attn_geometry_worker.py"), which, json.dumps([list(x) for x in geo_list])]
    try:
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _dead_child.append(knob)
        raise
    if out.returncode in (-6, -11, 134, 139):
        _dead_child.append(knob)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert sorted(res) == sorted(f"{hd},{grp}" for hd, grp in geo_list)
    for r in res.values():
        print("\n" + r["line"] + (f"; K / V rows {r['kv']:.2e}" if "kv" in r else ""))
    for name, r in res.items():
        assert r["err"] <= ac.GPU_TOL, (knob, name, r)
        assert r.get("kv", 0.0) <= KV_TOL, (knob, name, r)
    return {tuple(int(v) for v in name.split(",")): r for name, r in res.items()}


def _default_prompts(hip, case, geo_list):
    """the same prefixes on this process's default route"""
    out = {}
    for geo in geo_list:
        case(geo, "q8_0", "sharp")
        out[geo] = worker.prompts(hip, (ac.GEO[geo], "q8_0", "sharp"), f"prompts, default route hd{geo[0]} g{geo[1]}")
    return out


def test_knob_attn_f32(hip, case):
    # NL_ATTN_F32=1: prompts on attn_tile_kernel<HD, G, QT>, the f32-MFMA tile kernel, for every G it is instantiated for
    tile = [geo for geo in GEOS if geo[1] in TILE_GROUPS]
    got = _child("NL_ATTN_F32", "prompts", tile)
    ref = _default_prompts(hip, case, tile)
    for geo in tile:
        assert ref[geo]["err"] <= ac.GPU_TOL and ref[geo]["kv"] <= KV_TOL, (geo, ref[geo])
        assert got[geo]["logits_sha"] != ref[geo]["logits_sha"], geo        # not attn_tile16_kernel's bits: the other kernel ran
        assert got[geo]["kv_sha"] != ref[geo]["kv_sha"], geo                # (nor are layer 1's K / V rows, which follow layer 0's attention)


def test_knob_no_attn_tile(hip, case):
    # NL_NO_ATTN_TILE=1: a prompt's rows on attn_kernel<HD, G> per token -- other bits than the tile kernel's where one exists; on
    # the G = 6 models that is the route already (attn_tile_supported(6) is false), so the knob changes no bit
    geo_list = [(32, 8), (64, 1), (64, 2), (32, 6), (64, 6)]
    got = _child("NL_NO_ATTN_TILE", "prompts", geo_list)
    ref = _default_prompts(hip, case, geo_list)
    for geo in geo_list:
        assert ref[geo]["err"] <= ac.GPU_TOL and ref[geo]["kv"] <= KV_TOL, (geo, ref[geo])
        assert (got[geo]["logits_sha"] == ref[geo]["logits_sha"]) == (geo[1] == 6), geo
        assert (got[geo]["kv_sha"] == ref[geo]["kv_sha"]) == (geo[1] == 6), geo       # (layer 1's K / V rows follow layer 0's attention)


def test_knob_no_attn_fin(hip, case):
    # NL_NO_ATTN_FIN=1: the one-split attention of a decode batch writes its partial and keeps the battn_merge_kernel launch.
    # Observed: the same bits as the default route.  That is the design -- attn_finalize (nl_batch.h) is "the ns == 1 arithmetic of
    # battn_merge_kernel": both sum the workgroup's partial rows in the same order, the merge's only weight is exp(0) = 1 and its
    # L = 1 * l, so both store s * (1 / l).  No bit tells the two apart, so that the knob route ran is the engine's rule
    # (fin_attn = ... && !no_fin, batched_step), not something this test observes; what it holds is that the route stays
    # within the bound and stays equal to the FIN kernel at every geometry it runs.
    geo_list = [(32, 2), (64, 3), (64, 8)]
    got = _child("NL_NO_ATTN_FIN", "batches", geo_list)
    same = {}
    for geo in geo_list:
        case(geo, "q8_0", "sharp")
        ref = worker.batches(hip, (ac.GEO[geo], "q8_0", "sharp"), f"batches one_split, default route hd{geo[0]} g{geo[1]}")
        assert ref["err"] <= ac.GPU_TOL, (geo, ref)
        same[geo] = got[geo]["logits_sha"] == ref["logits_sha"]
        print(f"\nNL_NO_ATTN_FIN=1 against the FIN kernel, hd{geo[0]} g{geo[1]}: {'the same' if same[geo] else 'other'} bits")
    assert all(same.values()), same
