"""GPU tests of score_rows_kernel (nanollama_amd/csrc/nl_score.h) through nl_op_score_rows: per logits row the log-sum-exp,
the log-probability of a target id and the greedy id, against float64 numpy on the same float32 rows.

Tolerance, derived: the kernel sums exp(x - max) in float64, so the only float32 roundings are those of the returned lse and
of the returned logprob: 2^-24 relative each, doubled for the difference between the device's float64 exp / log chain and
libm: |d| <= 2^-22 * max(1, |x_t|, |lse|) for both outputs.  The greedy id must be numpy's argmax (first of equals, the rule
of go/main.go:400-408), and a second call on the same input must be bitwise equal.

Vocabularies: 1, 2, 63, 64, 65 (one wavefront and its edges), 255, 1023, 1024, 1025 (one workgroup: 1024 threads; head and
tail of the 16-byte loads, since a row of an odd vocabulary starts off a 16-byte boundary), 4099 (several strides), 32000 and
150001 (above the sampler's 131072).  Rows: 1, 3, 64, 65, 130 (with NL_SCORE_SLAB=64: one slab of rows, a ragged second, a third)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VOCABS = (1, 2, 63, 64, 65, 255, 1023, 1024, 1025, 4099, 32000, 150001)
ROWS = (1, 3, 64, 65, 130)
N_PATTERNS = 12
TOL = 2.0 ** -22


@pytest.fixture(scope="module")
def hip():
    from nanollama_amd import _lib, model
    if _lib.lib().nl_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return model


def _row(pattern, V, rng):
    """(float32 row, target, expected logprob is -inf)"""
    t = int(rng.integers(0, V))
    neg_inf = False
    if pattern == 0:
        x = rng.standard_normal(V)
    elif pattern == 1:
        x = 30.0 * rng.standard_normal(V)
    elif pattern == 2:                       # all equal: log(1 / V), greedy id 0
        x = np.full(V, 0.5)
    elif pattern in (3, 4):                  # one entry +1e4, the rest -1e4: target on it / elsewhere (-2e4, nothing overflows)
        x = np.full(V, -1e4)
        hot = int(rng.integers(0, V))
        x[hot] = 1e4
        t = hot if pattern == 3 else (hot + 1 + int(rng.integers(0, max(V - 1, 1)))) % V
    elif pattern == 5:                       # all near +3e4
        x = 3e4 + rng.standard_normal(V)
    elif pattern in (6, 7):                  # -inf everywhere but two entries: target on one of them / on a -inf entry
        x = np.full(V, -np.inf)
        keep = rng.choice(V, size=min(2, V), replace=False)
        x[keep] = rng.standard_normal(keep.size) * 3.0
        t = int(keep[0])
        if pattern == 7 and V >= 3:
            t = int(rng.choice(np.setdiff1d(np.arange(min(V, 64)), keep)))
            neg_inf = True
    elif pattern == 8:
        x, t = rng.standard_normal(V), 0
    elif pattern == 9:
        x, t = rng.standard_normal(V), V - 1
    elif pattern == 10:                      # exact ties of the maximum at several indices: the lowest wins
        x = rng.standard_normal(V).astype(np.float32).astype(np.float64)
        at = rng.choice(V, size=min(5, V), replace=False)
        x[at] = np.float32(x.max() + 1.0)
    else:                                    # target -1: not scored, exactly 0.0f; lse and greedy id still right
        x, t = rng.standard_normal(V), -1
    return x.astype(np.float32), t, neg_inf


def _case(V, n, first_pattern, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    rows, tg, ninf = zip(*[_row((first_pattern + i) % N_PATTERNS, V, rng) for i in range(n)])
    return np.stack(rows), np.asarray(tg, dtype=np.int32), np.asarray(ninf)


def _reference(x, t):
    x64 = x.astype(np.float64)
    m = x64.max(axis=1)
    with np.errstate(divide="ignore"):
        lse = m + np.log(np.exp(x64 - m[:, None]).sum(axis=1))
    xt = x64[np.arange(len(t)), np.maximum(t, 0)]
    return np.where(t >= 0, xt - lse, 0.0), lse, xt, x.argmax(axis=1)


def _check(hip, x, t, ninf, what):
    lp, lse, am = hip.op_score_rows(x, t)
    want_lp, want_lse, xt, want_am = _reference(x, t)
    bound = TOL * np.maximum(1.0, np.maximum(np.where(np.isfinite(xt), np.abs(xt), 0.0), np.abs(want_lse)))
    d_lse = np.abs(lse.astype(np.float64) - want_lse)
    fin = np.isfinite(want_lp)
    d_lp = np.abs(lp.astype(np.float64)[fin] - want_lp[fin])
    print(f"{what}: max|d lse| / bound = {float((d_lse / bound).max()):.3f}, max|d logprob| / bound = "
          f"{float((d_lp / bound[fin]).max()) if fin.any() else 0.0:.3f}")
    assert (d_lse <= bound).all(), (what, "lse", int(np.argmax(d_lse / bound)))
    assert (d_lp <= bound[fin]).all(), (what, "logprob", int(np.argmax(d_lp / bound[fin])))
    assert (~fin == ninf).all(), what                         # the reference is -inf exactly where the case says so ...
    assert (lp[~fin] == -np.inf).all(), (what, lp[~fin])      # ... and so is the device
    assert (lp[t < 0] == 0.0).all() and not np.signbit(lp[t < 0]).any(), what
    assert (am == want_am).all(), (what, np.nonzero(am != want_am)[0][:8])
    lp2, lse2, am2 = hip.op_score_rows(x, t)
    assert lp2.tobytes() == lp.tobytes() and lse2.tobytes() == lse.tobytes() and am2.tobytes() == am.tobytes(), what


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("n", ROWS)
def test_score_rows_match_float64(hip, monkeypatch, V, n):
    monkeypatch.setenv("NL_SCORE_SLAB", "64")      # (nl_score's default is 512 rows per launch: test_one_launch_for_all_rows)
    # calls of fewer rows than there are patterns start at every pattern in turn
    for first in (range(0, N_PATTERNS, n) if n < N_PATTERNS else (V % N_PATTERNS,)):
        x, t, ninf = _case(V, n, first, seed=1000 * n + V + first)
        _check(hip, x, t, ninf, f"vocab {V} rows {n} first pattern {first}")


@pytest.mark.parametrize("V", (65, 1025, 32000))
def test_one_launch_for_all_rows(hip, V):
    x, t, ninf = _case(V, 130, 0, seed=77 + V)
    _check(hip, x, t, ninf, f"vocab {V} rows 130, default slab")


def test_argument_checks(hip):
    from nanollama_amd import _lib
    x = np.zeros((2, 8), dtype=np.float32)
    for bad in ([0, 8], [-2, 0]):
        with pytest.raises(_lib.NlError) as ei:
            hip.op_score_rows(x, bad)
        assert ei.value.code == -1
    lp, lse, am = hip.op_score_rows(x, [7, -1])
    assert lp[1] == 0.0 and abs(float(lp[0]) + np.log(8.0)) <= TOL * np.log(8.0) and list(am) == [0, 0]
