"""Known-answer tests of the decode GEMV (gemv_kernel) in every launch geometry and of every multi-token GEMM
instantiation nl_op_matmul_batch can reach, on matrices whose products are exact in float32 in any summation order
(tests/exact_mats.py): the assertions are equalities with float32(W @ x) computed in float64.  Run with `pytest -m gpu`.

A GEMV geometry is (tw, kw): tw 16-row tiles per workgroup, kw wavefronts per tile.  It decides which 256-column groups
a wavefront walks (kw_index + n * kw), how they split between the two-group rounds and the one-group tail rounds, which
tiles of the last workgroup are dead, and how red[] is summed -- all of it indexing, none of it visible to a relative
bound on random weights unless a shape is lucky.

Part C runs whole models under forced geometries: the RMSNorm / attention-merge prologues and the SwiGLU / RoPE + KV /
residual epilogues exist only inside a model, at the one geometry its shapes pick.
"""
import os
import sys

import numpy as np
import pytest

from nanollama_amd import gguf, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_mats as em  # noqa: E402
from test_gpu_parity import LOGIT_TOL, _rand_blocks, _rand_matrix  # noqa: E402

pytestmark = pytest.mark.gpu


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


# Every (tw, kw) with tw * kw <= 8 (a workgroup holds at most 8 wavefronts): 17 pairs.
# choose_geometry picks, from the shape and NL_WAVES alone, (1..4, 1), (1..2, 2) and (1, 3..8): kw = min(ceil(2048 /
# tiles), groups, 8), tw = max(1, 4 // kw) clamped to the tile count.  The rest -- (2, 3), (2, 4), (3, 2), (4, 2),
# (8, 1) -- is what tools/sweep_*.sh can set through NL_TW / NL_KW.
GEOMETRIES = [(tw, kw) for tw in (1, 2, 3, 4, 8) for kw in range(1, 9) if tw * kw <= 8]
assert len(GEOMETRIES) == 17
KQUANTS = ("q4_k", "q6_k")


def _geometries(cols):
    """the pairs a matrix of `cols` columns admits: production clamps kw to the number of 256-column groups"""
    groups = (cols + 255) // 256
    return [(tw, kw) for tw, kw in GEOMETRIES if kw <= groups]


def _set_geometry(monkeypatch, tw, kw):
    monkeypatch.setenv("NL_TW", str(tw))      # handle knobs: nl_op_matmul's temporary engine reads them on every call
    monkeypatch.setenv("NL_KW", str(kw))


# rows x cols: what the shape exercises (16-row tiles; 64-column pairs; 256-column groups of 4 pairs; Q8_0 / Q4_0 /
# Q5_0 / F16 / Q4_K / Q6_K wavefronts take two groups per round while two are left, then one per tail round; F32 one)
SHAPES = [
    # 2304 / 256 = 9 groups.  Wavefront i of kw walks groups i, i + kw, ...: kw = 1: 9 groups = 4 two-group rounds + 1
    # tail; kw = 2: 5 and 4 groups (2 rounds + 1 tail | 2 rounds); kw = 3: 3 each (1 + 1); kw = 4: 3, 2, 2, 2 (1 + 1 | 1
    # round); kw = 5..8: 2 or 1 groups (one round | one tail) -- every kw mixes the two round kinds differently per
    # wavefront.  40 rows = 3 tiles, the last with 8 live rows; tw = 2 leaves a dead tile (tw = 4, 8 clamp to 3 tiles).
    (40, 2304, em.KINDS),
    # 2208 / 32 = 69 blocks = 35 pairs, the last with one block (half its columns); 35 = 8 groups of 4 + one of 3
    # pairs.  100 rows = 7 tiles (the last with 4 live rows): tw = 2, 3, 4, 8 all end in a partial workgroup.
    (100, 2208, tuple(k for k in em.KINDS if k not in KQUANTS)),
    # 151 rows = 10 tiles (the last with 7 live rows): the last workgroup holds 1 of 3, 2 of 4, 2 of 8 tiles.  Two groups.
    (151, 512, em.KINDS),
    # 768 / 256 = 3 groups: kw = 1 is one two-group round + one tail round (the K-quants' tail case: their columns come in
    # whole groups), kw = 2 splits 2 | 1, kw = 3 is one tail round each.  33 rows = 3 tiles, the last with 1 live row.
    (33, 768, em.KINDS),
    # one row; one block (half a pair) / one pair.  One group, so kw = 1 only; tw clamps to the single tile.
    (1, 32, tuple(k for k in em.KINDS if k not in KQUANTS)),
    (1, 64, tuple(k for k in em.KINDS if k not in KQUANTS)),
]
CASES = [(kind, rows, cols) for rows, cols, kinds in SHAPES for kind in kinds]


@pytest.mark.parametrize("kind,rows,cols", CASES, ids=[f"{k}-{r}x{c}" for k, r, c in CASES])
def test_gemv_exact_in_every_geometry(hip, monkeypatch, kind, rows, cols):
    rng = np.random.Generator(np.random.PCG64(rows * 7919 + cols * 13 + em.KINDS.index(kind)))
    raw, W = em.build(kind, rows, cols, rng)
    t = em.GGML_TYPE[kind]
    probes = em.probe(cols, rng)
    want = [em.exact_product(W, x) for x in probes]
    zero = np.zeros(cols, np.float32)
    for tw, kw in _geometries(cols):
        _set_geometry(monkeypatch, tw, kw)
        for i, x in enumerate(probes):
            got = hip.op_matmul(raw, t, x, rows, cols)
            bad = np.flatnonzero(got != want[i])
            assert bad.size == 0, (kind, (tw, kw), f"probe {i}", bad[:8], got[bad[:8]], want[i][bad[:8]])
        assert np.all(hip.op_matmul(raw, t, zero, rows, cols) == 0), (kind, (tw, kw), "zero x")


def _rand_raw(rng, rows, cols, wtype):
    return _rand_blocks(rng, rows, cols, wtype) if wtype in ("q5_0",) + KQUANTS else _rand_matrix(rng, rows, cols, wtype)


RAND_CASES = [(k, 151, 512) for k in em.KINDS] + [(k, 100, 2208) for k in em.KINDS if k not in KQUANTS]


@pytest.mark.parametrize("wtype,rows,cols", RAND_CASES, ids=[f"{k}-{r}x{c}" for k, r, c in RAND_CASES])
def test_gemv_random_weights_across_geometries(hip, orc, monkeypatch, wtype, rows, cols):
    # Random float weights and Gaussian x, as test_gemv_matches_oracle draws them: no exactness here.  Two assertions
    # without a tolerance of their own:
    #  * the summation order depends on kw alone (a wavefront's groups are kw_index + n * kw, red[] is added in j
    #    order); across tw only the workgroup that owns a tile changes -- so for each kw the outputs under every
    #    admissible tw are bitwise identical;
    #  * every geometry stays within the project's GEMV bound 2e-5 * (1 + |want|) of the oracle.
    rng = np.random.Generator(np.random.PCG64(rows * 131 + cols + em.KINDS.index(wtype)))
    raw = _rand_raw(rng, rows, cols, wtype)
    x = rng.standard_normal(cols, dtype=np.float32)
    t = synth.WTYPES[wtype]
    want = orc.matmul(raw, t, x, rows, cols)
    first = {}
    for tw, kw in _geometries(cols):
        _set_geometry(monkeypatch, tw, kw)
        got = hip.op_matmul(raw, t, x, rows, cols)
        err = np.abs(got - want) / (1 + np.abs(want))
        assert err.max() <= 2e-5, ((tw, kw), err.max(), int(err.argmax()))
        if kw in first:
            assert np.array_equal(got.view(np.uint32), first[kw][1].view(np.uint32)), (kw, first[kw][0], tw)
        else:
            first[kw] = (tw, got)
    assert len(first) == min(8, (cols + 255) // 256)


# ---- Part B: the multi-token GEMM instantiations ------------------------------------------------------------------
#
# launch_qgemm's rules (tiles = ceil(rows / 16), token tiles = ceil(tokens / 64), NL_QG2_MIN_TOKENS = 128 by default):
#   Q4_0 with tokens >= NL_QG2_MIN_TOKENS and ceil(tiles / 4) * token tiles >= 128 -> qgemm2_kernel, with row blocks =
#     ceil(tiles / 4): <Q4_0, 4, 2, 8> (256-token tiles) if row blocks * ceil(tokens / 256) >= 512, else <Q4_0, 4, 1, 4>;
#   otherwise qgemm_kernel: 8 wavefronts (128 rows) per workgroup if ceil(tiles / 8) * token tiles >= 128, else 4;
#     one token tile computes 1 / 2 / 4 sixteen-token tiles for tokens <= 16 / <= 32 / more; no split-K without a
#     partial buffer, which nl_op_matmul_batch does not pass.
# Q5_0 is expanded to the Q8_0 layout at upload and runs the Q8_0 instantiations.
NEVER = str(1 << 30)
GEMM_KINDS = ("q4_0", "q8_0", "q5_0", "f16")
GEMM_CASES = [
    # 20 tiles: ceil(20 / 8) * token tiles <= 3 * 3 < 128 -> 4 wavefronts; Q4_0: ceil(20 / 4) * 3 = 15 < 128 -> no qgemm2
    (320, 320, 1, None),      # one 16-token tile, a single token
    (320, 320, 16, None),     # one 16-token tile, full
    (320, 320, 17, None),     # two 16-token tiles, the second with one token
    (320, 320, 32, None),     # two, full
    (320, 320, 33, None),     # four, the third with one token
    (320, 320, 64, None),     # four, full: a whole 64-token workgroup tile
    (320, 320, 65, None),     # two 64-token tiles, the second with one token
    (320, 320, 130, None),    # three 64-token tiles, the last with two tokens
    (100, 96, 3, None),       # 7 tiles, the last with 4 live rows; 3 blocks = one partial K chunk
    # 352 tiles, 3 token tiles: ceil(352 / 8) * 3 = 132 >= 128 -> the 8-wavefront qgemm_kernel.  (Q4_0 at the default
    # NL_QG2_MIN_TOKENS would take qgemm2 -- 130 >= 128 tokens and ceil(352 / 4) * 3 = 264 >= 128 -- so these two cases
    # switch qgemm2 off; the 5632-row case runs once more with it on below.)
    (5632, 256, 130, NEVER),
    (5639, 256, 130, NEVER),  # 353 tiles, the last with 7 live rows: ceil(353 / 8) * 3 = 135
]


def _token_rows(rng, probes, ntok, cols):
    """[ntok, cols]: the integer probes first, then rows that differ per token (random integers in -2..2)"""
    X = rng.integers(-2, 3, size=(ntok, cols)).astype(np.float32)
    for i, p in enumerate(probes[:ntok]):
        X[i] = p
    assert np.abs(X).max() <= em.XMAX and (ntok < 5 or len({X[i].tobytes() for i in range(ntok)}) == ntok)
    return X


def _gemm_exact(hip, kind, rows, cols, ntok, seed=0):
    rng = np.random.Generator(np.random.PCG64(rows * 31 + cols * 7 + ntok + em.KINDS.index(kind) + seed))
    raw, W = em.build(kind, rows, cols, rng)
    X = _token_rows(rng, em.probe(cols, rng), ntok, cols)
    got = hip.op_matmul_batch(raw, em.GGML_TYPE[kind], X, rows, cols)
    want = em.exact_product(W, X)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (kind, rows, cols, ntok, len(bad), bad[:6].tolist())
    return got


@pytest.mark.parametrize("kind", GEMM_KINDS)
@pytest.mark.parametrize("rows,cols,ntok,qg2_min", GEMM_CASES, ids=[f"{r}x{c}x{n}" for r, c, n, _ in GEMM_CASES])
def test_gemm_exact_on_qgemm_kernel(hip, monkeypatch, kind, rows, cols, ntok, qg2_min):
    if qg2_min is not None:
        monkeypatch.setenv("NL_QG2_MIN_TOKENS", qg2_min)      # a step knob: nl_op_matmul_batch reads it on every call
    _gemm_exact(hip, kind, rows, cols, ntok)


def test_gemm_exact_q4_0_8_wavefront_shape_on_qgemm2_by_default(hip, monkeypatch):
    # 5632 x 256 x 130 with NL_QG2_MIN_TOKENS at its default: 130 >= 128 and ceil(352 / 4) * 3 = 264 >= 128 -> qgemm2;
    # 88 row blocks * ceil(130 / 256) = 88 < 512 -> <Q4_0, 4, 1, 4>, three token tiles, the last with two tokens.
    # Same seed as the qgemm_kernel case above, and the two kernels must agree bitwise.
    monkeypatch.delenv("NL_QG2_MIN_TOKENS", raising=False)
    a = _gemm_exact(hip, "q4_0", 5632, 256, 130)
    monkeypatch.setenv("NL_QG2_MIN_TOKENS", NEVER)
    assert np.array_equal(a.view(np.uint32), _gemm_exact(hip, "q4_0", 5632, 256, 130).view(np.uint32))


def test_gemm_exact_qgemm2_64_token_tiles_and_cross_check(hip, monkeypatch):
    # qgemm2_kernel<Q4_0, 4, 1, 4>: 2064 rows = 129 tiles -> 33 row blocks of four tiles, the last holding one; 224
    # columns = 7 blocks = two K chunks of four, the second with three; 250 tokens = 4 token tiles, the last with 58:
    # 33 * 4 = 132 >= 128 -> qgemm2, 33 * ceil(250 / 256) = 33 < 512 -> 64-token tiles.
    monkeypatch.setenv("NL_QG2_MIN_TOKENS", "1")
    a = _gemm_exact(hip, "q4_0", 2064, 224, 250)
    # The default (128) takes the same kernel: 250 >= 128 tokens.
    monkeypatch.delenv("NL_QG2_MIN_TOKENS", raising=False)
    b = _gemm_exact(hip, "q4_0", 2064, 224, 250)
    # With qgemm2 switched off the case runs on qgemm_kernel (ceil(129 / 8) * 4 = 68 < 128 -> 4 wavefronts) and must
    # equal the qgemm2 result bitwise, as nl_qgemm2.h claims.
    monkeypatch.setenv("NL_QG2_MIN_TOKENS", NEVER)
    c = _gemm_exact(hip, "q4_0", 2064, 224, 250)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a.view(np.uint32), c.view(np.uint32))


def test_gemm_exact_qgemm2_256_token_tiles(hip, monkeypatch):
    # qgemm2_kernel<Q4_0, 4, 2, 8>: 32760 rows = 2048 tiles (the last with 8 live rows) -> 512 row blocks; 200 tokens =
    # one ragged 256-token tile: 512 * ceil(200 / 64) >= 128 -> qgemm2, 512 * ceil(200 / 256) = 512 >= 512 -> 256-token
    # tiles.  160 columns = 5 blocks = two K chunks, the second with one block.
    monkeypatch.setenv("NL_QG2_MIN_TOKENS", "1")
    _gemm_exact(hip, "q4_0", 32760, 160, 200)


# ---- Part C: prologues and epilogues under forced geometries ------------------------------------------------------
#
# dim 512 = two 256-column groups; vocab 1000 = 62.5 tiles: the LM head's last tile is half full; interm 1120 = 17.5
# pairs: the down projection has 5 groups, the last with 2 pairs of which the second holds one block (the K-quants need
# whole groups: interm 1280).  136 positions cross the 128-position attention split: from position 128 on the WO
# prologue merges two partials.
MODEL_GEOMETRIES = [(4, 1), (2, 1), (1, 1), (2, 2), (1, 3), (1, 4), (1, 8)]
N_POS = 136
CHECK_POS = (0, 1, 5, 127, 128, 135)


# (dim 384 = 1.5 groups, one more model: the lanes past the last column of the RMSNorm prologue's input must stay out of
# its sum of squares -- with whole groups, and through nl_op_matmul, whose padding weights are zero, they cannot show)
@pytest.mark.parametrize("wtype,dim,heads", [("q8_0", 512, 8), ("q4_0", 512, 8), ("f16", 512, 8), ("q6_k", 512, 8), ("q4_0", 384, 6)])
def test_model_logits_under_forced_geometries(hip, orc, tmp_path, monkeypatch, wtype, dim, heads):
    shape = synth.ModelShape("geom", 2, dim, heads, 2, 1000, seq_len=192, interm=1280 if wtype in KQUANTS else 1120)
    p = tmp_path / "geom.gguf"
    synth.generate_gguf(str(p), shape, wtype, 11)
    g = gguf.load_gguf(str(p))
    toks = synth.prompt_ids(N_POS, shape.vocab, seed=4)
    orc.set_threads(min(16, os.cpu_count() or 1))
    ref = orc.OracleModel(g)
    want = {}
    for pos, tok in enumerate(toks):
        lg = ref.forward(int(tok), pos)
        if pos in CHECK_POS:
            want[pos] = np.array(lg, np.float32, copy=True)
    ref.close()
    monkeypatch.setenv("NL_FUSED_ATTN", "0")     # the five-launch plan only: every GEMV is gemv_kernel
    monkeypatch.setenv("NL_PERSIST", "0")
    got = {}
    for tw, kw in MODEL_GEOMETRIES:
        _set_geometry(monkeypatch, tw, kw)
        dev = hip.load_llama_model(g)
        assert dev.plan_info()["fused_mode"] == 0
        assert not dev.persist_info()["ready"]
        got[tw, kw] = {}
        for pos, tok in enumerate(toks):
            dev.forward(int(tok), pos)
            if pos in CHECK_POS:
                got[tw, kw][pos] = dev.state.logits.copy()
        dev.close()
    for geom in MODEL_GEOMETRIES:
        for pos in CHECK_POS:
            worst, scale = float(np.abs(got[geom][pos] - want[pos]).max()), max(1.0, float(want[pos].std()))
            print(f"{wtype} {geom} pos {pos}: max|gpu-oracle|={worst:.2e} (logit std {scale:.2f})")
            assert worst <= LOGIT_TOL * scale, (geom, pos, worst, scale)
    for geom in [(2, 1), (1, 1)]:                # kw = 1 throughout: the same sums, other workgroups
        for pos in CHECK_POS:
            assert np.array_equal(got[geom][pos].view(np.uint32), got[4, 1][pos].view(np.uint32)), (geom, pos)
