"""The persistent decode (nanollama_amd/csrc/nl_persist.h) after its h hand-off moved to 16-byte granules and its attention and
logits tails were shortened: every change is meant to leave every bit where it was.  tests/golden/persist_parent_hashes.json holds
what the commit BEFORE those changes computed (tools/persist_step_hashes.py: sha256 of every one-token step's logits, the ids, the
ids and last logits of one long chunk); this file asserts that the same procedure gives the same record.  Cases (CASES of the
tool): the D 256 / I 512 shape (two values per granule) with 13 layers (one- and two-slot XCDs; the chunk runs to position 140:
the single-record attention tail below 128, helpers and the merge from 128 on), with 2 kv heads and 5 layers (XCDs 5-7 carry
LM-head rows only), with 1 layer, as a Q4_0 file (the packer's other block types through the new row map), and nano's true shape
(three values per granule).  Then the resident session against the oracle, and the soak of the in-XCD 16-byte store form."""
import ctypes as C
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

from nanollama_amd import gguf, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("persist_step_hashes", os.path.join(ROOT, "tools", "persist_step_hashes.py"))
psh = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(psh)

with open(os.path.join(ROOT, "tests", "golden", "persist_parent_hashes.json")) as _fh:
    GOLDEN = json.load(_fh)

LOGIT_TOL = 1e-4      # the engine's stated tolerance (tests/test_gpu_persist.py)


class _PlacementMiss(Exception):
    """the persistent launch found its workgroups placed otherwise than 32 per XCD (observed, never assumed: nl_persist.h) -- the
    chunk was redone on the launch plans and the results are right, but the run did not test the persistent path"""


def _no_warning(dev):
    err = dev.last_error()
    if "not placed 32 per XCD" in err:
        raise _PlacementMiss(err)
    return err == ""


def _retry_placement(fn):
    """A placement miss is a property of the moment on the device, not of the code under test: one retry with fresh handles (the
    note is printed); a second miss in a row fails the test."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        try:
            return fn(*args, **kwargs)
        except (_PlacementMiss, psh.PlacementMiss) as exc:
            print(f"\n[retry] {fn.__name__}: {exc}")
        return fn(*args, **kwargs)
    return wrapper


@pytest.fixture(scope="module")
def hip():
    from nanollama_amd import _lib, model
    if _lib.lib().nl_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return model


@pytest.mark.parametrize("name", list(psh.CASES))
@_retry_placement
def test_every_step_reproduces_the_parents_bits(hip, tmp_path, name):
    want = GOLDEN[name]
    got = psh.run_case(hip, name, str(tmp_path))
    assert got["first"] == want["first"]
    assert got["step_ids"] == want["step_ids"]
    diff = [i for i, (a, b) in enumerate(zip(got["step_logits_sha256"], want["step_logits_sha256"])) if a != b]
    assert not diff and len(got["step_logits_sha256"]) == len(want["step_logits_sha256"]), f"steps whose logits bytes differ: {diff}"
    assert got["chunk_ids"] == want["chunk_ids"]
    assert got["chunk_last_logits_sha256"] == want["chunk_last_logits_sha256"]


@_retry_placement
def test_resident_session_still_delivers_every_steps_logits(hip, tmp_path):
    # per-step logits must still reach nl_host_logits (dev.state.logits) and the device buffer where a caller reads them
    from oracle import oracle as orc
    shape = psh.CASES["small_13"][0]
    p = tmp_path / "m.gguf"
    synth.generate_gguf(str(p), shape, "q8_0", 211)
    g = gguf.load_gguf(str(p))
    tokens = synth.prompt_ids(20, shape.vocab, seed=21)
    ref = orc.OracleModel(g)
    orc.set_threads(min(16, os.cpu_count() or 1))
    want = [ref.forward(t, pos).copy() for pos, t in enumerate(tokens)]
    orc.set_threads(1)
    ref.close()
    dev = hip.load_llama_model(g)
    assert dev.persist_info()["ready"]
    worst = 0.0
    for pos, t in enumerate(tokens):
        dev.forward(t, pos)
        lg = dev.state.logits
        worst = max(worst, float(np.abs(lg - want[pos]).max()) / max(1.0, float(want[pos].std())))
        assert int(np.argmax(lg)) == int(orc.argmax(want[pos])), pos
    info = dev.persist_info()
    print(f"\nresident session, 20 forced tokens: max|gpu-oracle| = {worst:.2e}; launches {info['launches']}")
    assert worst <= LOGIT_TOL and _no_warning(dev)
    assert info["launches"] == 1 and info["tokens"] == 20, info
    # the launch leaves when another entry point needs the stream; the device buffer holds the last step's logits
    dl = dev.debug_read("logits", shape.vocab)
    assert float(np.abs(dl - want[-1]).max()) / max(1.0, float(want[-1].std())) <= LOGIT_TOL
    dev.close()


def test_in_xcd_16_byte_granules_are_never_torn(hip):
    # the store and load forms of the h hand-off (pd_publish16 / pd_gather16), writer and reader on the same XCD
    from nanollama_amd import _lib
    torn, seen = C.c_ulonglong(0), C.c_ulonglong(0)
    rc = _lib.lib().nl_op_gran16_soak_local(0, 16, 20000, C.byref(torn), C.byref(seen))
    assert rc == 0
    print(f"\nin-XCD 16-byte granules: {seen.value} copies read, {torn.value} torn")
    assert seen.value > 0 and torn.value == 0
