"""The per-token launch plans of nanollama_amd/csrc/nl_engine.hip after the code that builds them was folded into one maker per op
and one filler per family of parameter structs (build_plan reads as the list of a layer's ops per mode): every change is meant to
leave every parameter value, launch and bit where it was.
tests/golden/plan_parent_hashes.json holds what the commit BEFORE those changes computed (tools/plan_hashes.py, recorded twice with
equal results: per step the sha256 of the logits and the argmax id, the chain's ids, plan_info(), persist_info() and the launches
per kind of every plan of the handle); this file asserts that the same procedure gives the same record, path by path.
Cases (CASES of the tool), each on a two-layer model, 9 + 12 per-call steps and a greedy chain of 24, NL_PERSIST=0: the five-launch
plan on seven models (Q8_0, Q4_0, F16, biases, conjugate RoPE, head_dim 32 with three query heads per kv head, qk-norm), again eager
and under the forced tensor-parallel seams; mode 1 with and without the feed-forward block; mode 2; mode 4 on the matrix pipe, on
the vector pipe, with GEMVs behind it, with every NL_PREFETCH branch, in Q8_0, and across the second attention pass with and without
helper blocks; mode 3 on the shards of an in-process group (tp_ffn_kernel in Q4_0 and Q8_0, wide_ffn_kernel) and the plain group;
two rank processes over the push seams on the five-launch and on the two-launch plan; one rank in loopback; the designed give-up of
modes 1 and 4."""
import importlib.util
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_single = _load("single_entry_bits", "tests", "test_gpu_single_entry_bits.py")      # its one-retry wrapper and its path-by-path diff
sys.modules["single_entry_hashes"] = _single.seh                                    # (the wrapper catches THAT module's Unforced)
ph = _load("plan_hashes", "tools", "plan_hashes.py")

with open(os.path.join(ROOT, "tests", "golden", "plan_parent_hashes.json")) as _fh:
    GOLDEN = json.load(_fh)


@pytest.fixture(scope="module")
def hip():
    from nanollama_amd import _lib, model
    if _lib.lib().nl_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return model


def test_the_fixture_holds_every_case():
    assert sorted(k for k in GOLDEN if k != "_build") == sorted(ph.CASES)
    assert GOLDEN["_build"]["lib_src_sha16"]


def test_the_fixtures_variants_are_not_one_plan():
    # the matrix pipe's sums are not the vector pipe's bits; warming a cache changes none; a retired plan's are the general plan's
    first = {name: next(iter(GOLDEN[name].values()))["logits_sha256"] for name in ph.CASES if name.startswith("mode4_")}
    assert first["mode4_matrix_pipe"] != first["mode4_vector_pipe"]
    assert all(first[name] == first["mode4_matrix_pipe"] for name in first if name.startswith("mode4_prefetch_"))
    for key, rec in GOLDEN["give_up_mode1"].items():
        assert rec["logits_sha256"] == GOLDEN["general"][key]["logits_sha256"] and rec["ids"] == GOLDEN["general"][key]["ids"]


@pytest.mark.parametrize("name", list(ph.CASES))
@_single._retry_unforced
def test_every_plan_reproduces_the_parents_bits(hip, tmp_path, name):
    got = json.loads(json.dumps(ph.run_case(hip, name, str(tmp_path))))     # (lists and strings, as the fixture holds them)
    diff = _single._diff(got, GOLDEN[name])
    assert not diff, diff
