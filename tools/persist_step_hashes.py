"""Bit-level record of the persistent decode (nanollama_amd/csrc/nl_persist.h): for each case below, one-token chunks with the
sha256 of every step's logits bytes (debug_read("logits")) and the ids, then one long chunk with its ids and the sha256 of
its last logits.  Run at a commit whose results are to be kept, the output is the fixture the next commit is held to
(tests/golden/persist_parent_hashes.json, tests/test_gpu_persist_handoff.py imports CASES and run_case from here).
A second table, CHAIN_CASES / run_chain_case, covers the instantiations and entry points CASES does not reach (the GAMMA kernels, a
Q5_0 file, nano's shape with 3 kv heads, the resident session's per-call logits): tests/golden/persist_chain_parent_hashes.json,
tests/test_gpu_persist_chain.py.
usage: python tools/persist_step_hashes.py OUT.json            (CASES)
       python tools/persist_step_hashes.py --chain OUT.json    (CHAIN_CASES)"""
import hashlib
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanollama_amd import gguf, synth

# name: (shape, weight type, seed, generator mode, prompt length, prompt seed, one-token steps, long chunk)
_SMALL = dict(dim=256, n_head=4, vocab=1024, seq_len=192, interm=512)
CASES = {
    # D 256 / I 512: two values per granule; 13 layers = one- and two-slot XCDs.  The chunk runs to position 140: a single attention
    # record below 128, helpers from 128 on
    "small_13": (synth.ModelShape("pdh_13", 13, n_kv_head=4, **_SMALL), "q8_0", 211, "float", 5, 9, 12, 124),
    "small_kv2_5": (synth.ModelShape("pdh_kv2_5", 5, n_kv_head=2, **_SMALL), "q8_0", 223, "float", 5, 9, 12, 124),   # XCDs 5-7: LM-head rows only
    "small_1": (synth.ModelShape("pdh_1", 1, n_kv_head=4, **_SMALL), "q8_0", 227, "float", 5, 9, 12, 124),
    "small_13_q4_0": (synth.ModelShape("pdh_13q4", 13, n_kv_head=4, **_SMALL), "q4_0", 229, "float", 5, 9, 12, 124),     # the packer's other block types
    # nano's true shape: the only one with three values per granule
    "nano": (synth.TIERS["nano"], "q8_0", synth.TIER_SEED["nano"], "qrand", 8, 7, 4, 32),
}

# A second table (CASES is what tests/test_gpu_persist_handoff.py parametrises over and stays as it is).  Chunk cases have CASES' fields
# plus the seed of a gamma essence (None: no gamma); the session case is per-call forward() over forced tokens.
CHAIN_CASES = {
    # the GAMMA instantiation of the D 256 / I 512 kernel: every second token id takes a gamma row (go/model.go:503-505)
    "small_gamma_2": ("chunk", synth.ModelShape("pdc_gamma_2", 2, n_kv_head=4, **_SMALL), "q8_0", 233, "float", 5, 9, 12, 124, 31),
    # (the seed is one whose greedy chain moves: most random two-layer Q5_0 files fall into one token or a pair after a few steps)
    "small_q5_0_2": ("chunk", synth.ModelShape("pdc_q5_2", 2, n_kv_head=4, **_SMALL), "q5_0", 277, "qrand", 5, 9, 12, 124, None),
    # nano's shape with grouped-query attention (three query heads per kv head): the <18, 48, 3> instantiation
    "nano_kv3_2": ("chunk", synth.ModelShape("pdc_nano_kv3_2", 2, 576, 9, 3, 1024, seq_len=192, interm=1536), "q8_0", 241, "float", 5, 9, 12, 124, None),
    # the resident session (go/main.go:173-219: Forward once per token): (kind, shape, type, seed, mode, forced tokens, their seed)
    "session_13": ("session", synth.ModelShape("pdc_sess_13", 13, n_kv_head=4, **_SMALL), "q8_0", 251, "float", 12, 11),
}


class PlacementMiss(Exception):
    """the launch found its workgroups placed otherwise than 32 per XCD: the chunk was redone on the launch plans"""


def _check(dev):
    err = dev.last_error()
    if "not placed 32 per XCD" in err:
        raise PlacementMiss(err)
    if err:
        raise RuntimeError(err)


def gamma_essence(seed, vocab, dim):
    """every second token id: whatever the greedy chain picks, about half of the in-launch embeddings take a gamma row"""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(seed))
    idx = np.arange(0, vocab, 2, dtype=np.int32)
    return idx, (rng.standard_normal((idx.size, dim)) * 0.3).astype(np.float32)


def run_case(model, name, workdir):
    """-> {"first", "step_ids", "step_logits_sha256", "chunk_ids", "chunk_last_logits_sha256"} of CASES[name]"""
    return _run_chunks(model, name, workdir, *CASES[name], None)


def run_chain_case(model, name, workdir):
    """the record of CHAIN_CASES[name]: run_case's for a chunk case, {"tokens", "step_logits_sha256"} for the session"""
    kind, *rest = CHAIN_CASES[name]
    return _run_chunks(model, name, workdir, *rest) if kind == "chunk" else _run_session(model, name, workdir, *rest)


def _run_session(model, name, workdir, shape, wtype, seed, mode, ntok, tseed):
    path = os.path.join(workdir, f"{name}.gguf")
    if not os.path.exists(path):
        synth.generate_gguf(path, shape, wtype, seed, mode=mode)
    dev = model.load_llama_model(gguf.load_gguf(path))
    try:
        if not dev.persist_info()["ready"]:
            raise RuntimeError(f"{name}: the persistent decode is not available for this shape")
        tokens = synth.prompt_ids(ntok, shape.vocab, seed=tseed)
        hashes = []
        for pos, t in enumerate(tokens):
            dev.forward(t, pos)
            _check(dev)
            hashes.append(hashlib.sha256(dev.state.logits.tobytes()).hexdigest())
        info = dev.persist_info()
        if info["launches"] != 1 or info["tokens"] != ntok:
            raise RuntimeError(f"{name}: not every call was served by one resident launch: {info}")
    finally:
        dev.close()
    return {"tokens": [int(t) for t in tokens], "step_logits_sha256": hashes}


def _run_chunks(model, name, workdir, shape, wtype, seed, mode, plen, pseed, nsteps, nchunk, gseed):
    import numpy as np
    path = os.path.join(workdir, f"{name}.gguf")
    if not os.path.exists(path):
        synth.generate_gguf(path, shape, wtype, seed, mode=mode)
    g = gguf.load_gguf(path)
    dev = model.load_llama_model(g)
    try:
        if gseed is not None:
            dev.set_gamma(*gamma_essence(gseed, shape.vocab, shape.dim))
        if not dev.persist_info()["ready"]:
            raise RuntimeError(f"{name}: the persistent decode is not available for this shape")
        prompt = synth.prompt_ids(plen, shape.vocab, seed=pseed)
        dev.prefill(prompt)
        first = int(np.argmax(dev.state.logits))
        tok, pos, ids, hashes = first, plen, [], []
        for _ in range(nsteps):
            (tok,) = dev.decode_greedy(tok, pos, 1)
            _check(dev)
            ids.append(int(tok))
            hashes.append(hashlib.sha256(dev.debug_read("logits", shape.vocab).tobytes()).hexdigest())
            pos += 1
        chunk = [int(t) for t in dev.decode_greedy(tok, pos, nchunk)]
        _check(dev)
        last = hashlib.sha256(dev.debug_read("logits", shape.vocab).tobytes()).hexdigest()
        info = dev.persist_info()
        if info["launches"] != nsteps + 1 or info["tokens"] != nsteps + nchunk:
            raise RuntimeError(f"{name}: not every chunk ran on the persistent launch: {info}")
    finally:
        dev.close()
    return {"first": first, "step_ids": ids, "step_logits_sha256": hashes, "chunk_ids": chunk, "chunk_last_logits_sha256": last}


def main():
    from nanollama_amd import _lib, model
    out = {}
    chain = sys.argv[1:2] == ["--chain"]
    cases, run = (CHAIN_CASES, run_chain_case) if chain else (CASES, run_case)
    with tempfile.TemporaryDirectory() as tmp:
        for name in cases:
            try:
                out[name] = run(model, name, tmp)
            except PlacementMiss as exc:
                print(f"[retry] {name}: {exc}")
                out[name] = run(model, name, tmp)
            print(name, out[name].get("step_ids", ""), out[name]["step_logits_sha256"][-1][:16])
    out["_build"] = _lib.build_info()
    with open(sys.argv[-1], "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
