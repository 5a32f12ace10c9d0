"""The persistent decode (nanollama_amd/csrc/nl_persist.h) after the work the compiler had sunk between a phase's barrier and its
publishing store was taken off the hand-off chain (1 / rms under the operand latency, one dead-flag check per layer slot, the
unit products' scale reads with their digit rows, one hand-off arena): no arithmetic operation or order changed, so every bit
stays where it was.  tests/golden/persist_chain_parent_hashes.json holds what the commit BEFORE those changes computed for the
instantiations tests/golden/persist_parent_hashes.json does not reach (CHAIN_CASES of tools/persist_step_hashes.py): the GAMMA
kernel of the D 256 / I 512 shape, a Q5_0 file, nano's shape with 3 kv heads (2 layers each), and the resident session -- per-call
forward over 12 positions on the 13-layer small shape, every step's host logits hashed.  Then one give-up case: with the dead flag
looked at once per layer slot, a launch whose every poll gives up at once still ends, the chunk is redone on the launch plans and
the handle retires the path."""
import functools
import importlib.util
import json
import os

import pytest

from nanollama_amd import gguf, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("persist_step_hashes", os.path.join(ROOT, "tools", "persist_step_hashes.py"))
psh = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(psh)

with open(os.path.join(ROOT, "tests", "golden", "persist_chain_parent_hashes.json")) as _fh:
    GOLDEN = json.load(_fh)


def _retry_placement(fn):
    """A placement miss (the launch's workgroups not 32 per XCD: observed, never assumed) is a property of the moment on the
    device, not of the code under test: one retry with fresh handles (the note is printed); a second miss in a row fails."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        try:
            return fn(*args, **kwargs)
        except psh.PlacementMiss as exc:
            print(f"\n[retry] {fn.__name__}: {exc}")
        return fn(*args, **kwargs)
    return wrapper


@pytest.fixture(scope="module")
def hip():
    from nanollama_amd import _lib, model
    if _lib.lib().nl_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return model


@pytest.mark.parametrize("name", list(psh.CHAIN_CASES))
@_retry_placement
def test_every_step_reproduces_the_parents_bits(hip, tmp_path, name):
    want = GOLDEN[name]
    got = psh.run_chain_case(hip, name, str(tmp_path))
    assert sorted(got) == sorted(want)
    for key in ("first", "tokens", "step_ids"):
        if key in want:
            assert got[key] == want[key], key
    diff = [i for i, (a, b) in enumerate(zip(got["step_logits_sha256"], want["step_logits_sha256"])) if a != b]
    assert not diff and len(got["step_logits_sha256"]) == len(want["step_logits_sha256"]), f"steps whose logits bytes differ: {diff}"
    if "chunk_ids" in want:
        assert got["chunk_ids"] == want["chunk_ids"]
        assert got["chunk_last_logits_sha256"] == want["chunk_last_logits_sha256"]


@_retry_placement
def test_a_launch_whose_polls_all_give_up_ends_and_is_redone(hip, tmp_path, monkeypatch):
    # spin limit 0: every poll of the launch leaves at once with whatever it read, and the units run on to the next dead-flag check
    # (one per layer slot, one at the LM head) through phases that compute on stale granules -- none of which is used as an address.
    # The launch ends, the host redoes the 20-token chunk on the launch plans (the oracle's ids) and retires the persistent path.
    from oracle import oracle as orc
    shape = synth.ModelShape("pdc_giveup", 13, 256, 4, 4, 1024, seq_len=96, interm=512)
    p = tmp_path / "m.gguf"
    synth.generate_gguf(str(p), shape, "q8_0", 257)
    g = gguf.load_gguf(str(p))
    prompt = synth.prompt_ids(6, shape.vocab, seed=13)
    ref = orc.OracleModel(g)
    orc.set_threads(min(16, os.cpu_count() or 1))
    lg = None
    for pos, t in enumerate(prompt):
        lg = ref.forward(t, pos)
    want = [int(orc.argmax(lg))]          # the first decode token, then the 20 the chunk must return
    for i in range(20):
        want.append(int(orc.argmax(ref.forward(want[-1], len(prompt) + i))))
    orc.set_threads(1)
    ref.close()
    monkeypatch.setenv("NL_PERSIST_SPIN_LIMIT", "0")
    monkeypatch.setenv("NL_QUIET", "1")
    dev = hip.load_llama_model(g)
    try:
        assert dev.persist_info()["ready"]
        dev.prefill(prompt)
        assert dev.decode_greedy(want[0], len(prompt), 20) == want[1:21]
        err = dev.last_error()
        if "not placed 32 per XCD" in err:
            raise psh.PlacementMiss(err)
        assert "persistent decode launch gave up" in err and "a hand-off poll timed out" in err, err
        assert not dev.persist_info()["ready"]
    finally:
        dev.close()
