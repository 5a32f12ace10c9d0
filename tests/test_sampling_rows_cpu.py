"""CPU checks behind the n-row sampler tests (tests/test_gpu_sampling_rows.py): their seeded catalogue meets the Go-chain
mismatch cap under the host mirrors alone, their float64 reference holds the mirrors within its bound, and the crafted-model
argument of synth.generate_gguf leaves the files it wrote before unchanged."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_mirror as sm  # noqa: E402
import sampling_rows_cases as rc  # noqa: E402
from nanollama_amd import synth  # noqa: E402


def test_catalogue_meets_the_go_chain_cap_under_the_mirrors():
    # the cap of the GPU test's rule for top-p rows (every pick that differs from go_top_p has a margin < 5e-4 and equals
    # device_top_p; at most max(2, trials // 8) of them per vocabulary up to 50000) must hold for the mirrors themselves,
    # or the GPU test could fail on a correct device
    for V, _ in rc.CATALOGUE:
        if V > rc.CAP_VOCAB:
            continue
        trials = mism = 0
        for V2, n, seed in rc.catalogue_calls():
            if V2 != V:
                continue
            lgs, params, us, recents, _ = rc.rows_case(V, n, seed)
            for r in range(n):
                p = params[r]
                if rc.mode_of(p) != "top_p":
                    continue
                lg = sm.apply_penalty(lgs[r], recents[r], p["rep_penalty"], V)
                trials += 1
                dev, margin = sm.device_top_p(lg, p["temperature"], p["top_p"], float(us[r]))
                if dev != sm.go_top_p(lg, p["temperature"], p["top_p"], float(us[r])):
                    mism += 1
                    assert margin < 5e-4, (V, seed, r, margin)
        print(f"V={V}: {mism} of {trials} top-p rows differ from the Go chain (cap {rc.go_cap(trials)})")
        assert trials >= 8
        assert mism <= rc.go_cap(trials), (V, mism, trials)


def test_catalogue_reaches_every_mode_kind_and_window():
    for V, n, seed in rc.catalogue_calls():
        if n < 64:
            continue
        _, params, us, recents, kinds = rc.rows_case(V, n, seed)
        assert set(kinds) == set(rc.LOGIT_KINDS)
        assert {rc.mode_of(p) for p in params} == {"argmax", "top_p", "top_k"}
        assert {len(r) for r in recents} >= {0, 1024}
        assert {float(u) for u in us} >= {0.0, float(np.float32(0.37)), rc.U_TOP}
        for p, rec in zip(params, recents):
            assert len(rec) <= p["rep_window"] <= 1024
            if len(rec) > 1:
                assert 0 in rec and V - 1 in rec and max(rec.count(t) for t in rec) >= 3


def test_grid_restatements_equal_the_mirrors():
    rng = np.random.default_rng(3)
    for V in (300, 4096, 32769):
        lg = rc.logits_of("ties", V, rng)
        us = [0.0, 0.37, rc.U_TOP] + [float(u) for u in rng.random(5, dtype=np.float32)]
        for temp, top_p in rc.DIST_TOP_P:
            assert rc.device_top_p_grid(lg, temp, top_p, us) == [sm.device_top_p(lg, temp, top_p, u)[0] for u in us]
        for k, temp in rc.DIST_TOP_K + ((1, 0.9),):
            assert rc.go_top_k_grid(lg, temp, k, us) == [sm.go_top_k(lg, temp, k, u) for u in us]


@pytest.mark.parametrize("V", rc.DIST_VOCABS)
def test_float64_reference_holds_the_mirrors(V):
    # the distribution check of the GPU test with the mirrors in place of the device (device_top_p for top-p, go_top_k for
    # top-k): 4096 grid uniforms, |count - 4096 q| <= 2 for every token, nothing drawn outside the set
    for V2, kind, mode, temp, arg in rc.dist_configs():
        if V2 != V:
            continue
        lg = rc.dist_logits(V, kind)
        if mode == "top_p":
            picks = rc.device_top_p_grid(lg, temp, arg, rc.GRID_U)
        else:
            picks = rc.go_top_k_grid(lg, temp, arg, rc.GRID_U)
        counts = np.bincount(picks, minlength=V)
        q, nxt, near = rc.reference_q(lg, mode, temp, arg)
        worst, outside = rc.check_counts(counts, q, nxt, near)
        print(f"V={V} {kind} {mode} T={temp} {arg}: worst |count - 4096 q| = {worst:.3f}, outside {outside}")
        assert worst <= rc.COUNT_BOUND and not outside, (V, kind, mode, temp, arg, worst, outside)


# sha256 of the files generate_gguf wrote before it took `overrides` (recorded once with that code)
_PARENT_SHA = {
    "q8_0": "b4db7bf5bdaaa6620d29830fd4c7f0a1282cdb3a2c48da438e778a48b3cd36e7",
    "q4_0": "7814b38c1f16cae4e62714f68b50530af8eb623163e575577173f0c6fde2226e",
    "q4_k": "1f2dfd03463618b6be54765624b2aaa3f14f456f6ad949d13cd293e277280c78",
}
_HASH_SHAPE = synth.ModelShape("hash", 1, 64, 2, 2, 300, seq_len=32, interm=128)


@pytest.mark.parametrize("wt", sorted(_PARENT_SHA))
def test_generate_gguf_without_overrides_is_unchanged(tmp_path, wt):
    p = str(tmp_path / "m.gguf")
    synth.generate_gguf(p, _HASH_SHAPE, wt, 5)
    with open(p, "rb") as fh:
        assert hashlib.sha256(fh.read()).hexdigest() == _PARENT_SHA[wt]


def test_generate_gguf_overrides_replace_one_tensor(tmp_path):
    from nanollama_amd import gguf
    a, b = str(tmp_path / "a.gguf"), str(tmp_path / "b.gguf")
    fa = synth.generate_gguf(a, _HASH_SHAPE, "q8_0", 5, keep_float=True)
    head = np.zeros((300, 64), np.float32)
    head[7] = 0.5
    fb = synth.generate_gguf(b, _HASH_SHAPE, "q8_0", 5, keep_float=True, overrides={"output.weight": head})
    assert np.array_equal(fb["output.weight"], head)
    assert all(np.array_equal(fa[k], fb[k]) for k in fa if k != "output.weight")
    ga, gb = gguf.load_gguf(a), gguf.load_gguf(b)
    assert ga.tensors.keys() == gb.tensors.keys()
    with pytest.raises(ValueError):
        synth.generate_gguf(b, _HASH_SHAPE, "q8_0", 5, overrides={"output.weight": head[:10]})
    with pytest.raises(ValueError):
        synth.generate_gguf(b, _HASH_SHAPE, "q8_0", 5, overrides={"no.such": head})
