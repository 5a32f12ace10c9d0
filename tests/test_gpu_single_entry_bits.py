"""The single-stream entry points (nl_forward, nl_forward_argmax, nl_decode_greedy, nl_sample_decode, nl_profile_forward,
nl_group_forward) and the op-level entry points (nl_op_*) of nanollama_amd/csrc/nl_engine.hip after their host-side scaffolding was
folded into shared helpers -- one per-call ladder, one redo loop, one fused-plan retirement, one chained loop, one holder of a group
call's per-rank results, one op scratch: every change is meant to leave every bit where it was.
tests/golden/single_entry_parent_hashes.json holds what the commit BEFORE those changes computed (tools/single_entry_hashes.py: ids,
windows and n_recent as lists, the sha256 of logits and K / V bytes, and for every handle the counters of persist_info() and
plan_info(), which say which rung of the ladder served it); this file asserts that the same procedure gives the same record.
Cases (CASES of the tool), on the small persistent instantiations (2 layers, dim 256, 4 heads, 2 and 4 KV heads, Q8_0 and Q4_0)
behind a 9-token prompt: six per-call steps on every rung (resident session, one-step persistent launch, call box, control copy +
synchronise, DMA read-back, eager launches, the forced tensor-parallel plan), the designed give-ups (NL_PERSIST_SPIN_LIMIT=0,
NL_FUSED_SPIN_LIMIT=0), a session interrupted by a stream switch and by forward / forward_argmax alternations, a step above the
high-water mark; greedy chains of 40 steps on the launch plans, on the persistent launch, handed over inside the chain, eager,
clipped at seq_len, redone; sampled chains with the three settings, re-captured, eager, with the plan's embed launch, redone;
profile_forward; the in-process shard group plain, fused and redone; a group handle; every op-level function and its argument
check."""
import functools
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("single_entry_hashes", os.path.join(ROOT, "tools", "single_entry_hashes.py"))
seh = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(seh)

with open(os.path.join(ROOT, "tests", "golden", "single_entry_parent_hashes.json")) as _fh:
    GOLDEN = json.load(_fh)


def _retry_unforced(fn):
    """A placement miss of the persistent launch or a fused launch whose cluster exchange timed out, where the case's own knobs did
    not force it, is a property of the moment on the device, not of the code under test, and the handle has left the rung the case
    is meant to hold: no valid comparison.  One retry with fresh handles (the note is printed); a second in a row fails the test."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        try:
            return fn(*args, **kwargs)
        except seh.Unforced as exc:
            print(f"\n[retry] {fn.__name__}: {exc}")
        return fn(*args, **kwargs)
    return wrapper


@pytest.fixture(scope="module")
def hip():
    from nanollama_amd import _lib, model
    if _lib.lib().nl_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return model


def test_the_fixture_holds_every_case():
    assert sorted(k for k in GOLDEN if k != "_build") == sorted(seh.CASES)


def _diff(got, want, path=""):
    """paths at which two records differ"""
    if isinstance(want, dict) and isinstance(got, dict):
        return [d for k in sorted(set(want) | set(got)) for d in
                (_diff(got[k], want[k], f"{path}/{k}") if k in got and k in want else [f"{path}/{k}: missing on one side"])]
    return [] if got == want else [f"{path}: {got!r} != {want!r}"]


@pytest.mark.parametrize("name", list(seh.CASES))
@_retry_unforced
def test_every_case_reproduces_the_parents_bits(hip, tmp_path, name):
    got = json.loads(json.dumps(seh.run_case(hip, name, str(tmp_path))))     # (lists and strings, as the fixture holds them)
    diff = _diff(got, GOLDEN[name])
    assert not diff, diff
