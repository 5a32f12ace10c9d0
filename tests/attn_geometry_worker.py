"""Child process of tests/test_gpu_attention_geometry.py: one attention route that a process knob selects (NL_ATTN_F32,
NL_NO_ATTN_TILE, NL_NO_ATTN_FIN -- the library reads them once per process, so the parent sets them in this child's environment),
over the geometry cases the parent names, in sequence.  argv: "prompts" or "batches", a JSON list of [head_dim, group] pairs.
Prints one JSON line: per geometry the worst values against the float64 forward (the parent holds them to the bounds) and the
SHA-256 of the result's bytes (the parent compares them with the default route's)."""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import attn_cases as ac  # noqa: E402


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def prompts(model, key, what, mkdir=None):
    """the prefixes of ac.PROMPT_PREFIXES on one handle: worst logits value, worst K / V row value, digests"""
    g, toks, _, run = ac.cached_case(mkdir, key)      # (mkdir None: the caller has built the case)
    dev = model.load_llama_model(g)
    w = ac.Worst(what)
    last, cache, kv_worst = ac.prompt_run(dev, g, toks, run, w, what)
    dev.close()
    return {"err": w.err, "at": w.at, "kv": kv_worst, "line": w.line(run),
            "logits_sha": sha(*[last[n] for n in ac.PROMPT_PREFIXES]), "kv_sha": sha(cache["k_cache"], cache["v_cache"])}


def batches(model, key, what, mkdir=None, layout="one_split"):
    """the decode batches of a layout on one handle: worst logits value, digest"""
    g, toks, _, run = ac.cached_case(mkdir, key)      # (mkdir None: the caller has built the case)
    start = ac.BATCH_STARTS[layout]
    dev = model.load_llama_model(g, max_streams=len(start))
    out = ac.batch_run(dev, toks, start)
    dev.close()
    w = ac.Worst(what)
    ac.batch_see(w, out, run, start)
    return {"err": w.err, "at": w.at, "line": w.line(run), "logits_sha": sha(out)}


if __name__ == "__main__":
    from nanollama_amd import model
    which, geos = sys.argv[1], [tuple(x) for x in json.loads(sys.argv[2])]
    knobs = " ".join(f"{k}={os.environ[k]}" for k in ("NL_ATTN_F32", "NL_NO_ATTN_TILE", "NL_NO_ATTN_FIN") if k in os.environ)
    res = {}
    with tempfile.TemporaryDirectory() as root:
        for hd, grp in geos:
            key = (ac.GEO[hd, grp], "q8_0", "sharp")
            what = f"{which} under {knobs} hd{hd} g{grp} {'/'.join(key)}"
            res[f"{hd},{grp}"] = (prompts if which == "prompts" else batches)(model, key, what, lambda: tempfile.mkdtemp(dir=root))
    print(json.dumps(res))
