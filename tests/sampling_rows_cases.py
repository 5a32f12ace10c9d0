"""The seeded edge catalogue of the n-row sampler tests (tests/test_gpu_sampling_rows.py) and the float64 reference of their
distribution check, shared with the CPU tests that hold the catalogue and the reference to the host mirrors alone
(tests/test_sampling_rows_cpu.py)."""
import bisect

import numpy as np

import sampling_mirror as sm

F = np.float32
U_TOP = float(F(1.0) - F(2.0 ** -24))          # the largest float32 below 1

# every row draws its own logits from these
LOGIT_KINDS = ["normal0.7", "normal3", "normal8", "flat", "two", "ties", "peak", "neg", "plateau300", "twomax"]


def logits_of(kind, V, rng):
    if kind.startswith("normal"):
        return (rng.standard_normal(V) * float(kind[6:])).astype(F)
    if kind == "flat":
        return np.full(V, 0.25, F)
    if kind == "two":                                                  # two distinct values
        return np.where(rng.random(V) < 0.5, F(0.25), F(-0.5)).astype(F)
    if kind == "ties":                                                 # two thirds of the ids share the logit 1.0
        lg = (rng.standard_normal(V) * 3.0).astype(F)
        lg[rng.permutation(V)[: (V * 2) // 3]] = F(1.0)
        return lg
    if kind == "peak":                                                 # one dominant token
        lg = rng.standard_normal(V).astype(F)
        lg[int(rng.integers(0, V))] = F(40.0)
        return lg
    if kind == "neg":                                                  # negatives, denormals, scattered -inf
        lg = -np.abs(rng.standard_normal(V) * 3.0).astype(F)
        lg[::97] = F(-1e-41)
        lg[5::101] = -np.inf
        return lg
    if kind == "plateau300":                                           # equal logits straddling the 50th place
        lg = (rng.standard_normal(V) * 2.0).astype(F)
        lg[rng.choice(V, min(300, V // 3), replace=False)] = F(np.sort(lg)[-50])
        return lg
    if kind == "twomax":                                               # two equal maxima
        lg = rng.standard_normal(V).astype(F)
        a, b = rng.choice(V, 2, replace=False)
        lg[a] = lg[b] = F(lg.max() + 1.0)
        return lg
    raise ValueError(kind)


# settings cycled through the rows: argmax with a penalty, top-p at two temperatures and three top_p, top-k at four k
# (k = 1024 exceeds V = 300; the call rejects k > 1024 in top-k mode)
SETTINGS = ([dict(temperature=0.0, top_p=0.9, top_k=50, rep_penalty=1.5)]
            + [dict(temperature=t, top_p=p, top_k=50) for t in (0.8, 1.5) for p in (0.02, 0.5, 0.9)]
            + [dict(temperature=t, top_p=1.0, top_k=k) for t, k in ((0.9, 1), (1.3, 7), (0.7, 50), (1.1, 1024))])
PENALTIES = (1.0, 1.15, 1.3)
UNIFORMS = (0.0, 0.37, U_TOP, None)                                    # None: a random draw
# The edges at float32's last step below 1 -- top_p = 1 - 2^-24 and, on a top-p row, u = 1 - 2^-24 -- put the cut or the
# pick on the last candidate, where the Go chain's float32 normaliser decides by its own rounding: there it differs from the
# exact sums on most rows (every such pick is still held to device_top_p exactly and must pass rule (d)'s margin).  So that
# the Go-chain cap stays a statement about ordinary rows, a call carries them on a few rows only: top_p = 1 - 2^-24 at both
# temperatures on rows NEAR1_ROWS, u = 1 - 2^-24 on the first top-p row that draws it; other top-p rows take 0.37 instead.
NEAR1_ROWS = (5, 40)


def mode_of(p):
    return "argmax" if p["temperature"] <= 0 else ("top_p" if p["top_p"] < 1.0 else "top_k")


def _window(kind, V, rng, must):
    """empty / partial / full at 1024; a non-empty window holds ids 0 and V - 1, one id three times, and `must`"""
    if kind == 0:
        return 16, ([] if must is None else [must])
    size, win = (int(rng.integers(10, 41)), 64) if kind == 1 else (1024, 1024)
    ids = [int(t) for t in rng.integers(0, V, size=size)]
    rep = int(rng.integers(0, V))
    ids[0], ids[1], ids[2], ids[5], ids[-1] = 0, rep, rep, V - 1, rep
    if must is not None:
        ids[3] = must
    return win, ids


def rows_case(V, n, seed, kinds=None):
    """n rows of vocabulary V: (logits [n, V] float32, settings per row, uniforms float32 [n], windows, logit kind per row)"""
    rng = np.random.default_rng(seed)
    lgs, params, us, recents, kind_of = [], [], [], [], []
    u_top_taken = False
    for r in range(n):
        kind = kinds[r] if kinds is not None else LOGIT_KINDS[(r + seed) % len(LOGIT_KINDS)]
        lg = logits_of(kind, V, rng)
        p = dict(SETTINGS[(r + 3 * seed) % len(SETTINGS)])          # (11 settings, 10 kinds: the pairing moves every row)
        if r in NEAR1_ROWS:
            p = dict(temperature=(0.8, 1.5)[NEAR1_ROWS.index(r)], top_p=U_TOP, top_k=50)
        if mode_of(p) != "argmax":
            p["rep_penalty"] = PENALTIES[(r // 2) % len(PENALTIES)]
        must = int(np.argmax(lg)) if mode_of(p) == "argmax" else None
        p["rep_window"], rec = _window((r + seed // 3) % 3, V, rng, must)
        u = UNIFORMS[(r // 3 + seed) % len(UNIFORMS)]
        if u == U_TOP and mode_of(p) == "top_p":
            u, u_top_taken = (0.37 if u_top_taken else U_TOP), True
        lgs.append(lg)
        params.append(p)
        us.append(F(rng.random()) if u is None else F(u))
        recents.append(rec)
        kind_of.append(kind)
    return np.stack(lgs), params, np.array(us, F), recents, kind_of


# (vocabulary, rows of each call): 64 rows mostly, 1, 2, 17 and 63 besides
CATALOGUE = [(300, (64, 1)), (4096, (64, 17)), (32000, (64,)), (32768, (64, 2)), (32769, (64, 63)), (50000, (64,)),
             (128256, (64,)), (131072, (64,))]
CAP_VOCAB = 50000                          # the Go-chain mismatch cap applies up to here


def catalogue_calls():
    """every call of the edge catalogue: (V, n, seed).  The Go chain's float32 sums drift by about V * 2^-24 over a flat or
    two-valued row, as far as the 1 / V between its boundaries from V ~ 32000 on, so whether a catalogue meets the cap under
    the mirrors alone depends on its seeds (about half of them at V = 50000): these were chosen so that it does, and
    tests/test_sampling_rows_cpu.py keeps that true."""
    return [(V, n, 1000 * V % 9973 + 30 + i) for V, ns in CATALOGUE for i, n in enumerate(ns)]


def go_cap(trials):
    return max(2, trials // 8)


# ---- the distribution check: 4096 uniforms on a grid against a float64 reference ----
GRID = 4096
GRID_U = np.array([F((k + 0.5) / GRID) for k in range(GRID)], F)
DIST_VOCABS = (4096, 32768, 32769, 131072)
DIST_LOGITS = ("normal1", "normal3", "ties")
DIST_TOP_P = ((0.8, 0.9), (1.5, 0.5), (0.7, 0.02))                    # (temperature, top_p)
DIST_TOP_K = ((50, 0.8), (1024, 1.3))                                  # (k, temperature)
COUNT_BOUND = 2.0
CUT_SLACK = 1e-5


def dist_configs():
    """(V, logit kind, mode, temperature, top_p or k)"""
    out = []
    for V in DIST_VOCABS:
        for kind in DIST_LOGITS:
            out += [(V, kind, "top_p", t, p) for t, p in DIST_TOP_P]
            out += [(V, kind, "top_k", t, k) for k, t in DIST_TOP_K]
    return out


def dist_logits(V, kind):
    return logits_of(kind, V, np.random.default_rng(V * 7 + len(kind)))


def reference_q(lg, mode, temp, arg):
    """float64 from the float32 logits: p_i = exp((l_i - max) / T), order p descending / id ascending, the set (top-p: the
    shortest prefix whose share of the mass is >= top_p; top-k: the first k), q = p renormalised inside it.
    Returns (q, the id just after the cut or -1, whether the cumulative share at the cut is within CUT_SLACK of top_p)."""
    l64 = lg.astype(np.float64)
    p = np.exp((l64 - l64.max()) / temp)
    order = np.lexsort((np.arange(lg.size), -p))
    if mode == "top_p":
        share = np.cumsum(p[order]) / p.sum()
        cut = min(int(np.searchsorted(share, arg, side="left")), lg.size - 1)
        near = abs(share[cut] - arg) <= CUT_SLACK
    else:
        cut, near = min(arg, lg.size) - 1, False
    inside = order[:cut + 1]
    q = np.zeros(lg.size)
    q[inside] = p[inside] / p[inside].sum()
    nxt = int(order[cut + 1]) if cut + 1 < lg.size else -1
    return q, nxt, near


def check_counts(counts, q, nxt, near):
    """(worst |count - GRID q|, ids outside the set that were drawn); the id after the cut is allowed only when `near`"""
    dev = np.abs(counts - GRID * q)
    out = np.nonzero((q == 0) & (counts > 0))[0]
    if near:
        out = out[out != nxt]
    return float(dev.max()), [int(i) for i in out]


def device_top_p_grid(lg, temp, top_p, us):
    """sampling_mirror.device_top_p for many uniforms at once (one order, one exact integer prefix sum)"""
    p = sm._probs(lg, temp)
    order = np.argsort(-p, kind="stable")
    w = np.floor(p[order].astype(np.float64) * 2.0 ** 45).astype(np.int64)
    cs = [int(c) for c in np.cumsum(w)]
    xcut = max(1, sm._ceil_mul(top_p, cs[-1]))
    cut = bisect.bisect_left(cs, xcut)
    return [int(order[bisect.bisect_left(cs, max(1, sm._ceil_mul(float(u), cs[cut])))]) for u in us]


def go_top_k_grid(lg, temp, k, us):
    """sampling_mirror.go_top_k for many uniforms at once"""
    k = min(k, lg.size)
    order = np.argsort(-lg, kind="stable")[:k]
    vals = lg[order]
    probs = np.exp(((vals - vals[0]) / F(temp)).astype(np.float32).astype(np.float64)).astype(np.float32)
    cs = np.cumsum(probs, dtype=np.float32)
    r = (np.asarray(us, F) * cs[-1]).astype(F)
    j = np.searchsorted(cs, r, side="left")
    return [int(order[i]) if i < k else int(order[0]) for i in j]
