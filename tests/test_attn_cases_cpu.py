"""Pins tests/attn_cases.py (no GPU): for every (shape, weight type, case) tests/test_gpu_attention_sharp.py and
tests/test_gpu_attention_geometry.py use,
(a) the CPU oracle stays within REF_CAP = 5e-5 of the float64 forward at every step of the token sequence -- half the project's
    logits tolerance, so a GPU failure against float64 cannot be the input's fault.  The cap is a condition on the inputs, not
    a measurement: a case that breaks it gets a lower sigma, never a higher cap;
(b) the float64 score rows of the steps the GPU tests check do contain what the cases exist for: a maximum in split 0 and one in
    the last split at pos >= 256, a maximum that is the newest key, a split whose float32 merge weight underflows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_cases as ac  # noqa: E402

_runs = {}
# random synth models: the winner is ~3 nats over the row's median key.  At SIGMA the scores are SIGMA times as wide (a lower sigma
# of a case scales the demand with it)
OVER_MEDIAN_MIN = 15.0


def _run(tmp_path_factory, key):
    """(float64 run, worst oracle error, step of the worst) of one case, computed once per session"""
    if key not in _runs:
        from oracle import oracle
        shape_key, wtype, case = key
        g = ac.build_case(str(tmp_path_factory.mktemp("attn") / "m.gguf"), shape_key, wtype, case)
        toks = ac.tokens(shape_key)
        run = ac.forward_f64(g, toks)
        ref = oracle.OracleModel(g)
        oracle.set_threads(min(8, os.cpu_count() or 1))
        errs = [ac.rel_err(ref.forward(t, pos), run.logits[pos]) for pos, t in enumerate(toks)]
        oracle.set_threads(1)
        ref.close()
        _runs[key] = (run, errs)
    return _runs[key]


@pytest.mark.parametrize("shape_key,wtype,case", ac.CASES, ids=["-".join(c) for c in ac.CASES])
def test_oracle_is_within_the_cap_of_float64_and_the_case_is_what_it_claims(tmp_path_factory, shape_key, wtype, case):
    run, errs = _run(tmp_path_factory, (shape_key, wtype, case))
    worst = int(np.argmax(errs))
    cov = ac.coverage(run)
    late = run.max_score[ac.SPLIT:]
    print(f"\n{shape_key}/{wtype}/{case}: max|oracle-f64|/max(1,std) = {errs[worst]:.2e} (step {worst}); scores up to "
          f"{np.abs(late).max():.1f}, median winning margin {np.median(run.top2_gap[ac.SPLIT:]):.1f} nats; {cov}")
    assert errs[worst] <= ac.REF_CAP
    T = len(errs)
    pos = np.arange(T)[:, None, None]
    if case == "self":          # the newest key wins every row, by tens of nats: every step rescales, earlier splits weigh ~e^-60
        assert (run.argmax == pos).all()
        assert np.median(run.top2_gap[1:]) > 30.0
        assert np.nanmin(run.split_gap[ac.SPLIT:, :, :, 0]) < -40.0
    elif case == "anti":        # the newest key is never the winner
        assert (run.argmax[1:] != pos[1:]).all()
    else:                       # one key dominates, somewhere: the typical row's winner is far ahead of the row's median key
        over = float(np.median(run.over_median[ac.SPLIT:]))
        print(f"  median over the rows from position {ac.SPLIT} on of (winner - median key): {over:.1f} nats")
        assert over > OVER_MEDIAN_MIN * ac.sigma_of((shape_key, wtype, case)) / ac.SIGMA
        assert np.abs(late).max() > 25.0


def test_the_checked_rows_cover_every_bookkeeping_branch(tmp_path_factory):
    # counted over every case, on the rows the GPU tests compare (the teacher-forced ones compare every step)
    total = {}
    for key in ac.CASES:
        run, _ = _run(tmp_path_factory, key)
        for k, v in ac.coverage(run).items():
            total[k] = total.get(k, 0) + v
    print(f"\ncoverage over {len(ac.CASES)} cases: {total}")
    for k in ("max_in_split0_at_pos_ge_256", "max_in_last_split_at_pos_ge_256", "max_is_newest_key", "split_weight_underflows"):
        assert total[k] >= 1, k
    # and on the 256/4/2 q8_0 models alone, which most paths run (anti underflows at positions 128 and 256, where the last split
    # holds nothing but the newest, lowest key)
    for case, need in (("sharp", ("max_in_split0_at_pos_ge_256", "max_in_last_split_at_pos_ge_256")),
                       ("self", ("max_is_newest_key",)), ("anti", ("split_weight_underflows",))):
        cov = ac.coverage(_run(tmp_path_factory, ("gqa", "q8_0", case))[0])
        for k in need:
            assert cov[k] >= 1, (case, k)


@pytest.mark.parametrize("shape_key", ["mha4", "gqa"])
@pytest.mark.parametrize("case", ["sharp", "self", "anti"])
def test_the_cap_holds_on_the_greedy_chain_of_the_persistent_decode_too(tmp_path_factory, shape_key, case):
    # the persistent decode picks its own tokens: the oracle's greedy continuation of the prompt is the sequence the device
    # reproduces unless two logits tie within its error; the cap must hold there as on the fixed sequence
    from oracle import oracle
    g = ac.build_case(str(tmp_path_factory.mktemp("attn") / "m.gguf"), shape_key, "q8_0", case)
    toks = ac.tokens(shape_key)[:ac.PERSIST_PROMPT]
    ref = oracle.OracleModel(g)
    rows = [ref.forward(t, pos).copy() for pos, t in enumerate(toks)]
    seq = list(toks)
    for i in range(ac.PERSIST_STEPS):
        seq.append(int(oracle.argmax(rows[-1])))
        rows.append(ref.forward(seq[-1], len(seq) - 1).copy())
    ref.close()
    run = ac.forward_f64(g, seq)
    errs = [ac.rel_err(rows[pos], run.logits[pos]) for pos in range(len(seq))]
    cov = ac.coverage(run, range(ac.PERSIST_PROMPT, len(seq)))
    print(f"\n{shape_key}/q8_0/{case}, greedy chain: max|oracle-f64|/max(1,std) = {max(errs):.2e}; {len(set(seq[ac.PERSIST_PROMPT:]))} distinct ids; {cov}")
    assert max(errs) <= ac.REF_CAP
