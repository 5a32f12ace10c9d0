"""GPU tests of gamma inside the persistent decode (nanollama_amd/csrc/nl_persist.h, the GAMMA instantiations of
pd_decode_kernel): a handle with a gamma essence -- through nl_set_gamma or through a bound voice -- keeps the
one-launch-per-chunk path and the resident session instead of falling back to the launch plans.  Reference lines:
go/model.go:503-505 (embed[token] += gamma[token]), go/main.go:173-219 (the greedy loop).  The launch plans of a handle
with the same gamma (NL_PERSIST=0) are the witness of the ids, the oracle of the logits."""
import os
import sys

import numpy as np
import pytest

from nanollama_amd import gguf, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_persist import LOGIT_TOL, _no_warning, _retry_placement  # noqa: E402  (placement retry: a miss is the moment's, not the code's)

pytestmark = pytest.mark.gpu

SHAPE = synth.ModelShape("pd_voices", 13, 256, 4, 4, 1024, seq_len=192, interm=512)      # the small instantiation, nano's layer split


@pytest.fixture(scope="module")
def hip():
    from nanollama_amd import _lib, model
    if _lib.lib().nl_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return model


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def g(tmp_path_factory):
    p = tmp_path_factory.mktemp("pd_voices") / "m.gguf"
    synth.generate_gguf(str(p), SHAPE, "q8_0", 171)
    return gguf.load_gguf(str(p))


def _essence(seed, first):
    """every second token id from `first` on: whatever the greedy chain picks, about half of the in-launch embeddings take a
    gamma row and half do not"""
    rng = np.random.Generator(np.random.PCG64(seed))
    idx = np.arange(first, SHAPE.vocab, 2, dtype=np.int32)
    return idx, (rng.standard_normal((idx.size, SHAPE.dim)) * 0.3).astype(np.float32)


GA, GB = _essence(31, 0), _essence(32, 1)
PROMPT = synth.prompt_ids(9, SHAPE.vocab, seed=3)


def _with_gamma(hip, g, how, gam):
    dev = hip.load_llama_model(g)
    if how == "gamma":
        dev.set_gamma(*gam)
    else:
        dev.set_voice(3, *gam)
        dev.stream_voice(0, 3)
    return dev


def _rel(a, b):
    return float(np.abs(a - b).max()) / max(1.0, float(b.std()))


@pytest.mark.parametrize("how", ["gamma", "voice"])
@_retry_placement
def test_gamma_keeps_the_persistent_decode(hip, orc, g, monkeypatch, how):
    monkeypatch.setenv("NL_PERSIST", "0")
    plain = _with_gamma(hip, g, how, GA)
    bare = hip.load_llama_model(g)
    assert not plain.persist_info()["ready"]
    monkeypatch.delenv("NL_PERSIST")
    plain.prefill(PROMPT); bare.prefill(PROMPT)
    first = int(np.argmax(plain.state.logits))
    want = plain.decode_greedy(first, len(PROMPT), 60)
    assert want != bare.decode_greedy(first, len(PROMPT), 60)        # the gamma really changes the chain

    dev = _with_gamma(hip, g, how, GA)
    assert dev.persist_info()["ready"]
    dev.prefill(PROMPT)
    assert int(np.argmax(dev.state.logits)) == first
    base = dev.persist_info()
    got = dev.decode_greedy(first, len(PROMPT), 60)
    assert _no_warning(dev), dev.last_error()
    info = dev.persist_info()
    assert info["ready"] and info["launches"] == base["launches"] + 1 and info["tokens"] == base["tokens"] + 60, (base, info)
    assert got == want, (got[:12], want[:12])

    # the resident session: consecutive per-call steps on ONE launch, teacher-forced logits against the oracle with the gamma
    ref = orc.OracleModel(g)
    ref.set_gamma(*GA)
    orc.set_threads(min(16, os.cpu_count() or 1))
    tokens = PROMPT + want[:21]
    dev.reset()
    base = dev.persist_info()
    worst = 0.0
    for pos, t in enumerate(tokens):
        dev.forward(t, pos)
        worst = max(worst, _rel(dev.state.logits, ref.forward(t, pos)))
    orc.set_threads(1)
    ref.close()
    info = dev.persist_info()
    print(f"\nresident session with gamma ({how}): {len(tokens)} forced tokens, max|gpu-oracle| = {worst:.2e}")
    assert worst <= LOGIT_TOL and _no_warning(dev)
    assert info["launches"] == base["launches"] + 1 and info["tokens"] == base["tokens"] + len(tokens), (base, info)
    dev.reset()
    base = dev.persist_info()
    tok, chain = None, []
    for pos in range(30):                      # the prompt teacher-forced, then its own ids
        tok = dev.forward_argmax(PROMPT[pos] if pos < len(PROMPT) else tok, pos)
        chain.append(tok)
    info = dev.persist_info()
    assert _no_warning(dev) and info["tokens"] == base["tokens"] + 30 and info["launches"] == base["launches"] + 1, (base, info)
    assert chain[len(PROMPT) - 1] == first and chain[len(PROMPT):] == want[:30 - len(PROMPT)]
    dev.close(); plain.close(); bare.close()


@_retry_placement
def test_a_rebind_between_two_chunks_is_honoured(hip, g, monkeypatch):
    def run(dev, rebind):
        dev.reset()
        dev.stream_voice(0, 1)
        dev.prefill(PROMPT)
        ids = dev.decode_greedy(int(np.argmax(dev.state.logits)), len(PROMPT), 30)
        if rebind:
            dev.stream_voice(0, 2)
        return ids + dev.decode_greedy(ids[-1], len(PROMPT) + 30, 30)

    monkeypatch.setenv("NL_PERSIST", "0")
    plain = hip.load_llama_model(g)
    monkeypatch.delenv("NL_PERSIST")
    dev = hip.load_llama_model(g)
    for m in (plain, dev):
        m.set_voice(1, *GA)
        m.set_voice(2, *GB)
    assert dev.persist_info()["ready"] and not plain.persist_info()["ready"]
    want, stay = run(plain, True), run(plain, False)
    assert want[:30] == stay[:30] and want[30:] != stay[30:]          # the second voice really changes the second chunk
    base = dev.persist_info()
    assert run(dev, True) == want
    info = dev.persist_info()
    assert _no_warning(dev) and info["launches"] == base["launches"] + 2 and info["tokens"] == base["tokens"] + 60, (base, info)
    assert run(dev, False) == stay
    dev.close(); plain.close()
