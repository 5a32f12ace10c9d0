"""The n-row sampler of sampled decode batches (nl_op_sample_rows: the launches of nl_forward_batch_sample on host logits, on a
scratch whose per-row slabs are poisoned first) at its edges, row by row:
  (a) an edge catalogue on every row of 64-row calls (and 1, 2, 17, 63 rows) -- the penalty, the window, argmax, top-k held
      to the mirrors exactly, top-p to device_top_p exactly and to the Go chain by rule (d);
  (b) row isolation -- an n-row call is n single-row calls, reversing the rows reverses the results, neighbours do not matter;
  (c) the distribution of 4096 grid uniforms against a float64 reference that depends on neither mirror.
The catalogue and the reference live in tests/sampling_rows_cases.py; tests/test_sampling_rows_cpu.py holds them to the
mirrors on the CPU."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_mirror as sm  # noqa: E402
import sampling_rows_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from nanollama_amd import _lib, model
    if _lib.lib().nl_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return model


def _check_row(V, lg_in, p, u, rec_in, pick, lg_out, rec_out):
    """one row against the mirrors; returns (top-p row, differs from the Go chain)"""
    want_lg = sm.apply_penalty(lg_in, rec_in, p["rep_penalty"], V)
    assert lg_out.tobytes() == want_lg.tobytes()                          # the in-place penalty, bit for bit
    assert rec_out == sm.push_recent(rec_in, pick, p["rep_window"])
    mode = rc.mode_of(p)
    if mode == "argmax":
        assert pick == int(np.argmax(want_lg))                              # lowest index of the maximum
        return False, False
    if mode == "top_k":
        assert pick == sm.go_top_k(want_lg, p["temperature"], p["top_k"], u)
        return False, False
    want, margin = sm.device_top_p(want_lg, p["temperature"], p["top_p"], u)
    assert pick == want
    if pick != sm.go_top_p(want_lg, p["temperature"], p["top_p"], u):     # rule (d): only at a boundary
        assert margin < 5e-4, margin
        return True, True
    return True, False


@pytest.mark.parametrize("V", [V for V, _ in rc.CATALOGUE])
def test_edge_catalogue_on_every_row(hip, V):
    t0 = time.time()
    trials = mism = 0
    for V2, n, seed in rc.catalogue_calls():
        if V2 != V:
            continue
        lgs, params, us, recents, kinds = rc.rows_case(V, n, seed)
        picks, lg_out, rec_out = hip.op_sample_rows(lgs, params, us, recents)
        for r in range(n):
            try:
                top_p, differs = _check_row(V, lgs[r], params[r], float(us[r]), recents[r], picks[r], lg_out[r], rec_out[r])
            except AssertionError as e:
                raise AssertionError(f"V={V} n={n} seed={seed} row {r}: {kinds[r]} {params[r]} u={float(us[r])!r} "
                                     f"pick {picks[r]}: {e}") from None
            trials += top_p
            mism += differs
    print(f"V={V}: {mism} of {trials} top-p rows differ from the Go chain ({time.time() - t0:.1f} s)")
    if V <= rc.CAP_VOCAB:
        assert mism <= rc.go_cap(trials), (V, mism, trials)


def _single_rows(hip, lgs, params, us, recents):
    out = [hip.op_sample(lgs[r], p["temperature"], p["top_p"], p["top_k"], p["rep_penalty"], p["rep_window"], float(us[r]),
                         recents[r]) for r, p in enumerate(params)]
    return [o[0] for o in out], np.stack([o[1] for o in out]), [o[2] for o in out]


@pytest.mark.parametrize("V", [300, 32768, 32769, 131072])
def test_rows_are_isolated(hip, V):
    _, n, seed = next(c for c in rc.catalogue_calls() if c[0] == V and c[1] == 64)
    lgs, params, us, recents, _ = rc.rows_case(V, n, seed)
    picks, lg_out, rec_out = hip.op_sample_rows(lgs, params, us, recents)
    # one n-row call = n single-row calls, bitwise
    p1, lg1, rec1 = _single_rows(hip, lgs, params, us, recents)
    assert picks == p1
    assert lg_out.tobytes() == lg1.tobytes()
    assert rec_out == rec1
    # the rows reversed: the results reversed
    pr, lgr, recr = hip.op_sample_rows(lgs[::-1], params[::-1], us[::-1], recents[::-1])
    assert pr == picks[::-1] and lgr.tobytes() == lg_out[::-1].tobytes() and recr == rec_out[::-1]
    # a row's result does not depend on its neighbours: the odd rows switch between the plateau and random logits
    for neighbour in ("ties", "normal3"):
        kinds = [None if r % 2 == 0 else neighbour for r in range(n)]
        lgs2, params2, us2, recents2, _ = rc.rows_case(V, n, seed + 1, kinds=[k or "normal0.7" for k in kinds])
        for r in range(0, n, 2):          # the even rows are the first call's
            lgs2[r], params2[r], us2[r], recents2[r] = lgs[r], params[r], us[r], recents[r]
        p2, lg2, rec2 = hip.op_sample_rows(lgs2, params2, us2, recents2)
        assert [p2[r] for r in range(0, n, 2)] == [picks[r] for r in range(0, n, 2)], neighbour
        assert lg2[0::2].tobytes() == lg_out[0::2].tobytes()
        assert [rec2[r] for r in range(0, n, 2)] == [rec_out[r] for r in range(0, n, 2)]


@pytest.mark.parametrize("V", list(rc.DIST_VOCABS))
def test_distribution_against_float64(hip, V):
    # Every config: the same logits in all 64 rows, uniforms u_k = f32((k + 0.5) / 4096) over 64 calls, the picks counted per
    # token against q of the float64 reference (sampling_rows_cases.reference_q): |count - 4096 q| <= 2 for every token, no
    # count outside the set but the id after the cut when the float64 share at the cut is within 1e-5 of top_p.  The grid
    # alone bounds the error below 1 (the mirrors in place of the device reach 0.992 at worst, test_sampling_rows_cpu); 2
    # still catches an interval moved by 5e-4 of the mass -- a swapped order, a wrong cut, another row's slab.
    rows = 64
    worst_all = 0.0
    for V2, kind, mode, temp, arg in rc.dist_configs():
        if V2 != V:
            continue
        lg = rc.dist_logits(V, kind)
        p = dict(temperature=temp, top_p=arg if mode == "top_p" else 1.0, top_k=arg if mode == "top_k" else 50,
                 rep_penalty=1.0, rep_window=0)
        block = np.tile(lg, (rows, 1))
        picks = []
        for c in range(rc.GRID // rows):
            got, _, _ = hip.op_sample_rows(block, [p] * rows, rc.GRID_U[c * rows:(c + 1) * rows], [[] for _ in range(rows)])
            picks += got
        counts = np.bincount(picks, minlength=V)
        q, nxt, near = rc.reference_q(lg, mode, temp, arg)
        worst, outside = rc.check_counts(counts, q, nxt, near)
        worst_all = max(worst_all, worst)
        print(f"V={V} {kind} {mode} T={temp} {arg}: worst |count - 4096 q| = {worst:.3f}, outside the set {outside}")
        assert worst <= rc.COUNT_BOUND and not outside, (V, kind, mode, temp, arg, worst, outside)
    print(f"V={V}: worst deviation {worst_all:.3f}")


def test_argument_errors(hip):
    from nanollama_amd import _lib
    import ctypes as C
    L = _lib.lib()
    P = dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=8)

    def call(n, params, vocab=64, stride=8, nrec=None):
        m = max(n, 1)
        lg = np.zeros((m, max(vocab, 1)), np.float32)
        ps = (_lib.NlSampleParams * m)(*[_lib.NlSampleParams(p["temperature"], p["top_p"], p["top_k"], p["rep_penalty"],
                                                              p["rep_window"]) for p in params[:m]])
        u = (C.c_float * m)(*([0.5] * m))
        rec = (C.c_int * (m * max(stride, 1)))()
        nr = (C.c_int * m)(*(nrec if nrec is not None else [0] * m))
        ids = (C.c_int * m)()
        return L.nl_op_sample_rows(0, lg.ctypes.data_as(C.POINTER(C.c_float)), vocab, n, ps, u, rec, stride, nr, ids)

    assert call(2, [P, P]) == 0
    assert call(64, [P] * 64) == 0
    assert call(0, [P]) == -1                                                # n < 1
    assert call(65, [P] * 65) == -1                                          # n > 64
    assert call(1, [P], vocab=0) == -1
    assert call(1, [P], vocab=131073) == -2                                  # beyond on-device sampling
    assert call(1, [dict(P, rep_window=2000)], stride=2000) == -1            # rep_window > 1024
    assert call(1, [dict(P, top_p=0.0)]) == -1                               # top_p <= 0
    assert call(1, [dict(P, top_p=1.0, top_k=2000)]) == -1                   # top_k > 1024 in top-k mode
    assert call(1, [dict(P, top_p=1.0, top_k=0)]) == -1                      # top_k < 1 in top-k mode
    assert call(1, [dict(P, rep_window=16)], stride=8) == -1                 # recent_stride < rep_window
    assert call(1, [P], nrec=[9]) == -1                                      # n_recent > rep_window
