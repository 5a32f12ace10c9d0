"""The exact-matrix builder (tests/exact_mats.py) against the oracle and the hand-built K-quant super blocks: its own
numpy decoders and the oracle's must agree bit for bit, and the oracle's left-to-right float32 matmul must reproduce
the float64 product exactly -- the property the GPU tests (test_gpu_gemv_exact.py) assert of every kernel geometry."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_mats as em  # noqa: E402
import kquant_kat as kat  # noqa: E402
from oracle import oracle as orc  # noqa: E402

SHAPES = [(40, 256), (23, 1792), (17, 2048)]


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("kind", em.KINDS)
def test_oracle_reproduces_the_exact_matrices_bit_for_bit(kind, rows, cols):
    rng = np.random.Generator(np.random.PCG64(rows * 1000 + cols + len(kind)))
    raw, W = em.build(kind, rows, cols, rng)
    t = em.GGML_TYPE[kind]
    assert raw.dtype == np.uint8 and raw.size == rows * cols // em.BLOCK[kind][0] * em.BLOCK[kind][1]
    assert W.dtype == np.float64 and W.shape == (rows, cols)
    assert np.array_equal(orc.dequant(raw, t, rows * cols).reshape(rows, cols).astype(np.float64), W)
    for x in em.probe(cols, rng):
        assert np.array_equal(orc.matmul(raw, t, x, rows, cols), em.exact_product(W, x))


@pytest.mark.parametrize("kind", ["q8_0", "q4_0", "q5_0", "q4_k", "q6_k"])
def test_builder_draws_the_whole_range(kind):
    # negative and zero scales, and both ends of the quant range, do occur: the matrices are not accidentally tame
    rng = np.random.Generator(np.random.PCG64(3))
    raw, W = em.build(kind, 40, 2304 if kind in ("q4_k", "q6_k") else 2208, rng)
    per, nbytes = em.BLOCK[kind]
    b = raw.reshape(-1, nbytes)
    d = b[:, 208:210] if kind == "q6_k" else b[:, 0:2]
    dv = np.ascontiguousarray(d).view(np.float16)[:, 0]
    assert (dv < 0).any() and (dv == 0).any() and (dv > 0).any()
    assert (W > 0).any() and (W < 0).any()
    body = b[:, :208] if kind == "q6_k" else b[:, 2:]
    assert body.min() == 0 and body.max() == 255
    if kind == "q4_k":
        assert (b[:, 4:12] >> 6).max() == 3      # the two-bit tops of the second 6-bit packing are in use


def test_builder_decoders_reproduce_the_hand_built_super_blocks():
    raw, exp = kat.q4_k_block()
    assert np.array_equal(em.decode_q4_k(np.frombuffer(raw, np.uint8), 1)[0], np.array(exp, np.float64))
    raw, exp = kat.q6_k_block()
    assert np.array_equal(em.decode_q6_k(np.frombuffer(raw, np.uint8), 1)[0], np.array(exp, np.float64))


def test_unit_is_the_smallest_power_of_two_step():
    assert em.unit(np.array([[0.0, 0.75, -6.0]])) == 0.25
    assert em.unit(np.array([[8.0, 0.0]])) == 8.0
    assert em.unit(np.array([[3.0 * 2.0 ** -9, 1.0]])) == 2.0 ** -9
    assert em.unit(np.zeros((2, 2))) == 1.0


def test_exactness_assertion_raises_for_a_too_long_row():
    # ones in units of 1/64 over 2^20 columns: 2^26 units against |x| = 1, 2^27 against XMAX
    W = np.ones((1, 1 << 20))
    W[0, 0] = 1.0 / 64
    with pytest.raises(ValueError):
        em.check_exact(W, 1)
    with pytest.raises(ValueError):
        em.check_exact(W)
    em.check_exact(W[:, :1 << 16])               # 2^16 * 64 * 2 = 2^23 units: fine
    # and through build(): k / 64 with E|k| = 32 over 2^20 columns is ~2^26 units
    with pytest.raises(ValueError):
        em.build("f32", 1, 1 << 20, np.random.Generator(np.random.PCG64(1)))
