"""Weight matrices of every supported format whose products with small-integer inputs are exact in float32 in ANY
summation order (a helper module, not a test; no oracle import).

build(kind, rows, cols, rng) draws the raw ggml blocks -- quants uniformly over the format's whole range (the Q5_0
high bits, all twelve Q4_K scale bytes so both 6-bit packings occur, Q6_K's int8 sub-scales), the fp16 scales d /
dmin per block from a short list of powers of two with a negative entry and 0 -- and decodes them with its own numpy
restatement of the published block layouts (ggml-quants.c: block_q8_0, block_q4_0, block_q5_0, block_q4_K +
get_scale_min_k4, block_q6_K) into the dense float64 matrix W.  f16 / f32 weights are k / 64 with integer |k| <= 64.
(A zero scale is harmless in every one of these formulas: the block -- or, for Q4_K, one of its two terms -- is 0.)

probe(cols, rng) hands out the input vectors; every element is an integer with |x_j| <= XMAX.

Why equality may be asserted: let u be the smallest power of two dividing every element of W.  build() requires
    max_i sum_j |W_ij| * XMAX  <  2^24 * u
and raises ValueError otherwise.  Every product w_ij * x_j, every partial sum of them in any order, and every block sum
before or after its power-of-two scale is then an integer multiple of u (or of a larger power of two) below 2^24 of its
units: a float32 value, so no addition, no fused multiply-add and no scaling ever rounds.  Small integers are exact in
fp16 as well (the device's fp16 nibble trick, the hi half of the matrix-core path's hi/lo split of x; k / 64 in an f16
weight).  The device and the oracle must therefore reproduce float32(W @ x) bit for bit.
"""
import numpy as np

KINDS = ("f32", "f16", "q8_0", "q4_0", "q5_0", "q4_k", "q6_k")
GGML_TYPE = {"f32": 0, "f16": 1, "q4_0": 2, "q5_0": 6, "q8_0": 8, "q4_k": 12, "q6_k": 14}
BLOCK = {"f32": (1, 4), "f16": (1, 2), "q8_0": (32, 34), "q4_0": (32, 18), "q5_0": (32, 22), "q4_k": (256, 144),
         "q6_k": (256, 210)}          # kind -> (elements, bytes) per block
XMAX = 2

# fp16 scales per block (all exact in fp16).  Largest element in units of the smallest step: Q8_0 128 * 4, Q4_0 8 * 4,
# Q5_0 16 * 4, Q4_K (63 * 15 + 63) * 4, Q6_K 128 * 32 * 2.  The Q6_K list stops at two units: its average element is
# 64 * 16 = 1024 sub-scale x quant steps, so a 2304-column row whose blocks all drew the largest scale still sums to
# 1024 * 2 * XMAX * 2304 = 9.4e6 < 2^24 units; with four it would not.  check_exact() decides, not this estimate.
_D = {"q8_0": [2.0 ** -6, 2.0 ** -5, -(2.0 ** -6), 2.0 ** -4, 0.0],
      "q4_0": [2.0 ** -6, 2.0 ** -5, -(2.0 ** -6), 2.0 ** -4, 0.0],
      "q5_0": [2.0 ** -6, 2.0 ** -5, -(2.0 ** -6), 2.0 ** -4, 0.0],
      "q4_k": [2.0 ** -9, 2.0 ** -8, -(2.0 ** -9), 2.0 ** -7, 0.0],
      "q6_k": [2.0 ** -9, 2.0 ** -8, -(2.0 ** -9), -(2.0 ** -8), 0.0]}
_DMIN = [2.0 ** -9, 2.0 ** -8, -(2.0 ** -8), 2.0 ** -7, 0.0]


def _draw_f16(rng, values, n):
    """n scales drawn from `values`: (fp16 bytes [n, 2], float64 [n])"""
    v = np.asarray(values, np.float64)[rng.integers(0, len(values), size=n)]
    h = v.astype(np.float16)
    assert np.array_equal(h.astype(np.float64), v)
    return h.view(np.uint8).reshape(n, 2), v


def _f16_field(b):
    """two byte columns [n, 2] -> float64 [n]"""
    return np.ascontiguousarray(b).view(np.float16)[:, 0].astype(np.float64)


def decode_q8_0(raw, nblk):
    b = raw.reshape(nblk, 34)
    return _f16_field(b[:, 0:2])[:, None] * b[:, 2:34].view(np.int8).astype(np.float64)


def decode_q4_0(raw, nblk):
    b = raw.reshape(nblk, 18)
    qs = b[:, 2:18].astype(np.int64)
    q = np.concatenate([qs & 0xF, qs >> 4], axis=1) - 8          # elements 0..15: low nibbles, 16..31: high nibbles
    return _f16_field(b[:, 0:2])[:, None] * q.astype(np.float64)


def decode_q5_0(raw, nblk):
    b = raw.reshape(nblk, 22)
    qh = np.ascontiguousarray(b[:, 2:6]).view("<u4")[:, 0].astype(np.int64)[:, None]
    qs = b[:, 6:22].astype(np.int64)
    j = np.arange(16)[None, :]
    lo = (qs & 0xF) | (((qh >> j) & 1) << 4)                     # fifth bit of element j: bit j of qh
    hi = (qs >> 4) | (((qh >> (j + 16)) & 1) << 4)               # of element j + 16: bit j + 16
    return _f16_field(b[:, 0:2])[:, None] * (np.concatenate([lo, hi], axis=1) - 16).astype(np.float64)


def decode_q4_k(raw, nblk):
    b = raw.reshape(nblk, 144)
    d, dmin = _f16_field(b[:, 0:2]), _f16_field(b[:, 2:4])
    sc = b[:, 4:16].astype(np.int64)
    s, m = np.empty((nblk, 8), np.int64), np.empty((nblk, 8), np.int64)
    s[:, :4], m[:, :4] = sc[:, 0:4] & 63, sc[:, 4:8] & 63        # get_scale_min_k4, j < 4
    s[:, 4:] = (sc[:, 8:12] & 0xF) | ((sc[:, 0:4] >> 6) << 4)    # j >= 4: low nibble of byte j + 4, top bits of byte j - 4
    m[:, 4:] = (sc[:, 8:12] >> 4) | ((sc[:, 4:8] >> 6) << 4)     #         high nibble of byte j + 4, top bits of byte j
    qs = b[:, 16:144].astype(np.int64).reshape(nblk, 4, 32)      # 64 elements: low nibbles of 32 bytes, then the high ones
    q = np.stack([qs & 0xF, qs >> 4], axis=2).reshape(nblk, 8, 32)
    w = (d[:, None] * s)[:, :, None] * q - (dmin[:, None] * m)[:, :, None]
    return w.reshape(nblk, 256)


def decode_q6_k(raw, nblk):
    b = raw.reshape(nblk, 210)
    ql = b[:, 0:128].astype(np.int64).reshape(nblk, 2, 2, 32)    # [half][first / second 32 bytes][l]
    qh = b[:, 128:192].astype(np.int64).reshape(nblk, 2, 32)
    sc = b[:, 192:208].view(np.int8).astype(np.int64).reshape(nblk, 2, 8)
    d = _f16_field(b[:, 208:210])
    # element 128 * half + 32 * k + l: k = 0, 1 low nibbles of ql[l], ql[l + 32]; k = 2, 3 their high nibbles;
    # bits 2k, 2k + 1 of qh[l] on top; sub-scale index 8 * half + 2 * k + l // 16
    q = np.stack([(ql[:, :, 0] & 0xF) | (((qh >> 0) & 3) << 4), (ql[:, :, 1] & 0xF) | (((qh >> 2) & 3) << 4),
                  (ql[:, :, 0] >> 4) | (((qh >> 4) & 3) << 4), (ql[:, :, 1] >> 4) | (((qh >> 6) & 3) << 4)], axis=2) - 32
    scl = np.repeat(sc.reshape(nblk, 2, 4, 2), 16, axis=3)       # [half][k][l] -> sc[half][2 k + l // 16]
    return (d[:, None, None, None] * scl * q).reshape(nblk, 256)


DECODERS = {"q8_0": decode_q8_0, "q4_0": decode_q4_0, "q5_0": decode_q5_0, "q4_k": decode_q4_k, "q6_k": decode_q6_k}


def unit(W):
    """the smallest power of two dividing every element of W (1.0 for an all-zero matrix)"""
    nz = np.asarray(W, np.float64)
    nz = nz[nz != 0]
    if nz.size == 0:
        return 1.0
    mant, exp = np.frexp(np.abs(nz))
    mi = (mant * 2.0 ** 53).astype(np.int64)                     # exact: a float64 mantissa has 53 bits
    low = (mi & -mi).astype(np.float64)                          # lowest set bit, a power of two
    return float(2.0 ** int((np.log2(low).astype(np.int64) + exp - 53).min()))


def check_exact(W, xmax=XMAX):
    """raise ValueError unless every row's sum_j |W_ij| * xmax stays below 2^24 units of unit(W)"""
    u = unit(W)
    worst = float(np.abs(np.asarray(W, np.float64)).sum(axis=1).max()) * xmax
    if not worst < 2.0 ** 24 * u:
        raise ValueError(f"not exact in float32: a row reaches {worst / u:.4g} units of {u:g}, the limit is 2^24")
    return worst / u


def build(kind, rows, cols, rng):
    """(raw ggml bytes as a flat uint8 array, dense float64 W[rows, cols]); raises ValueError if a product of W with
    integers |x_j| <= XMAX could round in float32"""
    per, nbytes = BLOCK[kind]
    if cols % per:
        raise ValueError(f"{kind}: cols must be a multiple of {per}")
    if kind in ("f32", "f16"):
        W = rng.integers(-64, 65, size=(rows, cols)).astype(np.float64) / 64.0
        raw = W.astype(np.float32 if kind == "f32" else np.float16)
        assert np.array_equal(raw.astype(np.float64), W)
        raw = raw.view(np.uint8).reshape(-1)
    else:
        nblk = rows * cols // per
        b = rng.integers(0, 256, size=(nblk, nbytes), dtype=np.uint8)
        if kind == "q6_k":
            b[:, 208:210] = _draw_f16(rng, _D[kind], nblk)[0]
        else:
            b[:, 0:2] = _draw_f16(rng, _D[kind], nblk)[0]
        if kind == "q4_k":
            b[:, 2:4] = _draw_f16(rng, _DMIN, nblk)[0]
        raw = np.ascontiguousarray(b).reshape(-1)
        W = DECODERS[kind](raw, nblk).reshape(rows, cols)
    check_exact(W)
    return raw, W


def probe(cols, rng):
    """the input vectors (float32, integers with |x_j| <= XMAX): random, the pattern (j % 5) - 2, all ones"""
    xs = [rng.integers(-2, 3, size=cols).astype(np.float32), ((np.arange(cols) % 5) - 2).astype(np.float32),
          np.ones(cols, np.float32)]
    assert all(np.abs(x).max() <= XMAX for x in xs)
    return xs


def exact_product(W, x):
    """float32(W @ x) for one vector x[cols] (-> [rows]) or a batch x[n, cols] (-> [n, rows]), in float64"""
    x = np.asarray(x, np.float64)
    return (W @ x if x.ndim == 1 else x @ W.T).astype(np.float32)
