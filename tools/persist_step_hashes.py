"""Bit-level record of the persistent decode (nanollama_amd/csrc/nl_persist.h): for each case below, one-token chunks with the
sha256 of every step's logits bytes (debug_read("logits")) and the ids, then one long chunk with its ids and the sha256 of
its last logits.  Run at a commit whose results are to be kept, the output is the fixture the next commit is held to
(tests/golden/persist_parent_hashes.json, tests/test_gpu_persist_handoff.py imports CASES and run_case from here).
usage: python tools/persist_step_hashes.py OUT.json"""
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


class PlacementMiss(Exception):
    """the launch found its workgroups placed otherwise than 32 per XCD: the chunk was redone on the launch plans"""


def _check(dev):
    err = dev.last_error()
    if "not placed 32 per XCD" in err:
        raise PlacementMiss(err)
    if err:
        raise RuntimeError(err)


def run_case(model, name, workdir):
    """-> {"first", "step_ids", "step_logits_sha256", "chunk_ids", "chunk_last_logits_sha256"} of CASES[name]"""
    import numpy as np
    shape, wtype, seed, mode, plen, pseed, nsteps, nchunk = CASES[name]
    path = os.path.join(workdir, f"{name}.gguf")
    if not os.path.exists(path):
        synth.generate_gguf(path, shape, wtype, seed, mode=mode)
    g = gguf.load_gguf(path)
    dev = model.load_llama_model(g)
    try:
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
    with tempfile.TemporaryDirectory() as tmp:
        for name in CASES:
            try:
                out[name] = run_case(model, name, tmp)
            except PlacementMiss as exc:
                print(f"[retry] {name}: {exc}")
                out[name] = run_case(model, name, tmp)
            print(name, out[name]["step_ids"], out[name]["chunk_last_logits_sha256"][:16])
    out["_build"] = _lib.build_info()
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
