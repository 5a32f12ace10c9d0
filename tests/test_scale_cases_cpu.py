"""Pins tests/scale_cases.py (no GPU): for every (shape, weight type, case) tests/test_gpu_scale_cases.py uses,
(a) the CPU oracle stays within REF_CAP = 5e-5 of the float64 forward at EVERY step of the token sequence, on this work's metric
    max|oracle - f64| / std(f64 logits of the step) (no floor of 1) -- half the GPU bound, so a GPU failure against float64
    cannot be the input's fault.  The cap is a condition on the inputs: a case that breaks it gets a lower exponent
    (scale_cases.LOWERED), never a higher cap, and no step is left out;
(b) the float64 run contains what the case exists for:
      eps      mean(x^2) < eps / 10 at every norm input of every step
      ramp     the rms rises 16 x 16 over the two seams of each layer, within a factor 2 (median over the steps), and by more than
      jump     one binade at every seam of every step; jump: 2^8 / 2^12 over layer 0 within a factor 2, its first seam (attention
               norm -> feed-forward norm) carrying at least 2^-4 of that at every step and no other seam more than 8
      gate     >= 20 % of the pre-activations below -88.8, >= 20 % above +88.8, >= 85 % beyond +-17
      outlier  every outlier channel >= 2^9 x the median channel (rms over the steps) at every norm input

    On ramp / jump: a writer multiplied by 2^p does not raise the rms by 2^p at its own seam, because the two writers of a
    layer have different gains at unit scale -- attn_output writes a softmax average of V rows (rms 0.15 .. 0.35 of the stream:
    the seam shows 2^p x that), ffn_down a SwiGLU of I terms (rms 2 .. 4).  Their product is ~1, so the factor-2 window is
    asserted where it can hold, over a layer's two seams; the single seams are held to the binade / 2^-4 floors above.
    Measured medians per seam, gqa q8_0: ramp 5.6 / 44 / 8.2 / 30, jump8 89 / 3.0, jump12 1420 / 3.0.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_cases as ac  # noqa: E402
import scale_cases as sc  # noqa: E402

_runs = {}


def _run(tmp_path_factory, key):
    """(loaded file, float64 run, oracle error of every step) of one model, computed once per session"""
    if key not in _runs:
        shape_key, wtype, case = key
        g = sc.build_case(str(tmp_path_factory.mktemp("scale") / "m.gguf"), shape_key, wtype, case)
        toks = sc.tokens(shape_key)
        run = ac.forward_f64(g, toks)
        errs, _ = sc.oracle_errs(g, toks, run)
        _runs[key] = (g, run, errs)
    return _runs[key]


def test_the_gpu_file_uses_exactly_these_models():
    assert len(set(sc.CASES)) == len(sc.CASES)
    assert set(sc.PERSIST_CASES) <= set(sc.CASES)
    assert set(sc.LOWERED) <= set(sc.CASES)


@pytest.mark.parametrize("shape_key,wtype,case", sc.CASES, ids=["-".join(c) for c in sc.CASES])
def test_oracle_is_within_the_cap_of_float64_and_the_case_is_what_it_claims(tmp_path_factory, shape_key, wtype, case):
    g, run, errs = _run(tmp_path_factory, (shape_key, wtype, case))
    T, L = run.logits.shape[0], g.meta.num_layers
    assert len(errs) == T == sc.n_tokens(shape_key) and run.norm_ms.shape == (T, 2 * L + 1) and run.gate.shape[:2] == (T, L)
    worst = int(np.argmax(errs))
    std = run.logits.std(axis=1)
    rms = np.sqrt(run.norm_ms)
    seam = rms[:, 1:] / rms[:, :-1]                       # [T, 2L]: rise of the rms from one norm to the next
    print(f"\n{shape_key}/{wtype}/{case}: max|oracle-f64|/std = {errs[worst]:.2e} (step {worst}); logit std {std.min():.4f} .. "
          f"{std.max():.4f}; norm input rms {rms.min():.3g} .. {rms.max():.3g}; median rise per seam "
          f"{[float(f'{v:.3g}') for v in np.median(seam, axis=0)]}; max|g| {np.abs(run.gate).max():.0f}")
    assert np.isfinite(run.logits).all() and errs[worst] <= sc.REF_CAP
    assert std.min() > 1e-3                               # no step's logits collapse (the metric divides by this)
    eps = float(np.float32(g.meta.rms_norm_eps))
    if case == "eps":
        assert run.norm_ms.max() < eps / 10
    else:
        assert run.norm_ms.min() > 10 * eps or case == "lo"       # (lo: rms 2^-6, mean square ~25 eps at the embedding)
    if case in ("lo", "hi"):
        want = sc.LOWERED.get((shape_key, wtype, case), sc.STREAM_SCALE[case])
        assert (rms > want / 2).all() and (rms < want * 8).all()
    if case == "ramp":
        layer = np.median(seam[:, 0::2] * seam[:, 1::2], axis=0)
        assert ((layer > 128) & (layer < 512)).all(), layer
        assert seam.min() > 2.0, seam.min()               # the pre-scale of every token is stale at every seam
    if case in ("jump8", "jump12"):
        p = 2.0 ** int(case[4:])
        layer0 = float(np.median(seam[:, 0] * seam[:, 1]))
        assert p / 2 < layer0 < p * 2, layer0
        assert seam[:, 0].min() >= p / 16 and seam[:, 1:].max() < 8.0, (seam[:, 0].min(), seam[:, 1:].max())
    if case == "gate":
        gt = run.gate
        lo, hi, sat = float(np.mean(gt < -88.8)), float(np.mean(gt > 88.8)), float(np.mean(np.abs(gt) > 17.0))
        print(f"  pre-activations below -88.8: {lo:.3f}, above +88.8: {hi:.3f}, beyond +-17: {sat:.3f}")
        assert lo >= 0.20 and hi >= 0.20 and sat >= 0.85
    if case == "outlier":
        ch = np.sqrt(run.chan_ms)                         # [2L + 1, D]
        ratio = ch[:, list(sc.OUTLIER_COLS)].min(axis=1) / np.median(ch, axis=1)
        print(f"  outlier channel / median channel per norm input: {[float(f'{v:.0f}') for v in ratio]}")
        assert (ratio >= 2.0 ** 9).all()


@pytest.mark.parametrize("shape_key,wtype,case", sc.PERSIST_CASES, ids=["-".join(c) for c in sc.PERSIST_CASES])
def test_the_cap_holds_on_the_greedy_chain_of_the_persistent_decode_too(tmp_path_factory, shape_key, wtype, case):
    # the persistent decode picks its own tokens: the oracle's greedy continuation of the prompt is the sequence the device
    # reproduces unless two logits tie within its error; the cap must hold there as on the fixed sequence
    from oracle import oracle
    g, _, _ = _run(tmp_path_factory, (shape_key, wtype, case))
    toks = sc.tokens(shape_key)[:sc.PERSIST_PROMPT]
    ref = oracle.OracleModel(g)
    rows = [ref.forward(t, pos).copy() for pos, t in enumerate(toks)]
    seq = list(toks)
    for i in range(sc.PERSIST_STEPS):
        seq.append(int(oracle.argmax(rows[-1])))
        rows.append(ref.forward(seq[-1], len(seq) - 1).copy())
    ref.close()
    run = ac.forward_f64(g, seq)
    errs = [sc.rel_err(rows[pos], run.logits[pos]) for pos in range(len(seq))]
    print(f"\n{shape_key}/{wtype}/{case}, greedy chain: max|oracle-f64|/std = {max(errs):.2e}; {len(set(seq[sc.PERSIST_PROMPT:]))} distinct ids")
    assert max(errs) <= sc.REF_CAP
