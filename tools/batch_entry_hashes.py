"""Bit-level record of the five batched entry points (nl_prefill, nl_score, nl_forward_batch, nl_forward_batch_sample,
nl_forward_mixed / nl_forward_mixed_sample, nanollama_amd/csrc/nl_engine.hip): for each case below the returned ids, the sha256
of the returned logits bytes, for sampled calls the ids and the windows, for score the sha256 of the log-prob bytes and the
argmax list.  Run at a commit whose results are to be kept, the output is the fixture the next commit is held to
(tests/golden/batch_entry_parent_hashes.json, tests/test_gpu_batch_entry_bits.py imports CASES and run_case from here).
usage: python tools/batch_entry_hashes.py OUT.json"""
import contextlib
import hashlib
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanollama_amd import gguf, synth

BE_A = synth.ModelShape("be_a", 2, 256, 4, 2, 512, seq_len=320, interm=512)        # MX_A of tests/test_gpu_mixed.py
BE_K = synth.ModelShape("be_k", 1, 256, 4, 2, 512, seq_len=320, interm=512)        # the Q4_K file: outside the batch path
BE_WRAP = synth.ModelShape("be_wrap", 1, 256, 4, 2, 512, seq_len=72, interm=512)   # a ring of 72 control blocks
SEED = 307
SETTINGS = [dict(temperature=0.0, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=8),       # greedy
            dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=64),      # top-p
            dict(temperature=1.3, top_p=1.0, top_k=40, rep_penalty=1.3, rep_window=16)]       # top-k


class FusedTimeout(Exception):
    """a fused launch's cluster exchange timed out and the call was redone on the general plan, which the handle keeps: the
    results are right, but the run is no valid recording or comparison"""


def _sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _Ctx:
    def __init__(self, model, workdir):
        self.model, self.workdir, self.devs = model, workdir, []

    def load(self, shape, wtype, max_streams):
        path = os.path.join(self.workdir, f"{shape.name}_{wtype}.gguf")
        if not os.path.exists(path):
            synth.generate_gguf(path, shape, wtype, SEED)
        dev = self.model.load_llama_model(gguf.load_gguf(path), max_streams=max_streams)
        self.devs.append(dev)
        return dev

    def close(self):
        errs = [dev.last_error() for dev in self.devs]
        for dev in self.devs:
            dev.close()
        return errs

    def finish(self):
        for err in self.close():
            if "fused-launch cluster exchange timed out" in err:
                raise FusedTimeout(err)
            if err:
                raise RuntimeError(err)


def _decode_setup(ctx, shape, wtype, n, steps=3):
    """n streams standing at positions drawn over 0..139 (their history through prefill) -> (dev, rng, start, toks)"""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(21))
    start = [int(v) for v in rng.integers(0, 140, size=n)]
    toks = [[int(t) for t in rng.integers(3, shape.vocab, size=start[s] + steps)] for s in range(n)]
    dev = ctx.load(shape, wtype, n)
    for s in range(n):
        if start[s]:
            dev.prefill(toks[s][:start[s]], stream=s, want_logits=False)
    return dev, rng, start, toks


def _forward_batch(ctx, n, wtype="q4_0", shape=BE_A):
    # step 0 twice (the second call replays the first call's graph), step 1 (the graph with new data), step 2 for ids alone
    dev, _, start, toks = _decode_setup(ctx, shape, wtype, n, steps=3)
    out = {"ids": [], "logits_sha256": []}
    for k in (0, 0, 1):
        ids, lg = dev.forward_batch(list(range(n)), [toks[s][start[s] + k] for s in range(n)], [start[s] + k for s in range(n)],
                                    want_logits=True)
        out["ids"].append(ids)
        out["logits_sha256"].append(_sha(lg))
    ids, _ = dev.forward_batch(list(range(n)), [toks[s][start[s] + 2] for s in range(n)], [start[s] + 2 for s in range(n)])
    out["ids"].append(ids)
    return out


def _sampler_args(rng, vocab, m, shift):
    import numpy as np
    params = [SETTINGS[(i + shift) % 3] for i in range(m)]
    us = rng.random(m, dtype=np.float32)
    recents = [[int(t) for t in rng.integers(0, vocab, size=params[i]["rep_window"] // 2)] for i in range(m)]    # half-filled windows
    return params, us, recents


def _forward_batch_sample(ctx, n, wtype="q4_0", shape=BE_A):
    # two consecutive calls with different settings per row on one handle: the second replays the graph with new data
    dev, rng, start, toks = _decode_setup(ctx, shape, wtype, n, steps=2)
    out = {"ids": [], "windows": []}
    for k in range(2):
        params, us, recents = _sampler_args(rng, shape.vocab, n, k)
        ids, rec = dev.forward_batch_sample(list(range(n)), [toks[s][start[s] + k] for s in range(n)],
                                            [start[s] + k for s in range(n)], params, us, recents)
        out["ids"].append(ids)
        out["windows"].append(rec)
    return out


def _mixed_steps(shape):
    """(dev setup, steps) of the mixed cases: streams 0-2 decode from 5, 126 and 200.  Step A: the three decode rows and the final
    token of stream 3's 40-token prompt as output rows, then the 39 rows before it and the first 9 rows of stream 4.  Step B
    (stream 4 fed to 105 in between): the decode rows of streams 0-3 and stream 4's final token (149) as output rows, then its
    rows 105..148 -- across position 128 -- and the first 4 rows of stream 5."""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(11))
    seqs = [[int(t) for t in rng.integers(3, shape.vocab, size=220)] for _ in range(6)]

    def rows(out, chunks):
        r = list(out) + [(s, p) for s, p0, cnt in chunks for p in range(p0, p0 + cnt)]
        return [s for s, _ in r], [seqs[s][p] for s, p in r], [p for _, p in r], len(out)

    step_a = rows([(0, 5), (1, 126), (2, 200), (3, 39)], [(3, 0, 39), (4, 0, 9)])
    step_b = rows([(0, 6), (1, 127), (2, 201), (3, 40), (4, 149)], [(4, 105, 44), (5, 0, 4)])
    return seqs, step_a, step_b


def _mixed(ctx, sampled, wtype="q4_0", shape=BE_A):
    import numpy as np
    seqs, step_a, step_b = _mixed_steps(shape)
    dev = ctx.load(shape, wtype, 6)
    for s, p0 in ((0, 5), (1, 126), (2, 200)):
        dev.prefill(seqs[s][:p0], stream=s, want_logits=False)
    rng = np.random.Generator(np.random.PCG64(31))
    out = {"ids": [], "logits_sha256": [], "windows": []}

    def run(step, shift):
        streams, tokens, pos, n_out = step
        for _ in range(2):         # capture, then replay
            if sampled:
                params, us, recents = _sampler_args(rng, shape.vocab, n_out, shift)
                ids, rec = dev.forward_mixed_sample(streams, tokens, pos, n_out, params, us, recents)
                out["windows"].append(rec)
            else:
                ids, lg = dev.forward_mixed(streams, tokens, pos, n_out, want_logits=True)
                out["logits_sha256"].append(_sha(lg))
            out["ids"].append(ids)

    run(step_a, 0)
    dev.prefill(seqs[4][9:105], pos0=9, stream=4, want_logits=False)
    run(step_b, 1)
    # what the non-output rows left behind: stream 4's K / V rows
    L, KV, hd, S = shape.n_layer, shape.n_kv_head, shape.head_dim, shape.seq_len
    for which in ("k_cache", "v_cache"):
        out[which + "_sha256"] = _sha(dev.debug_read(which, L * KV * S * hd, stream=4).reshape(L, KV, S, hd)[:, :, :150])
    return out


def _mixed_no_output_rows(ctx):
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(13))
    toks = [int(t) for t in rng.integers(3, BE_A.vocab, size=21)]
    dev = ctx.load(BE_A, "q4_0", 6)
    ids, _ = dev.forward_mixed([3] * 20, toks[:20], list(range(20)), 0)
    dev.forward(toks[20], 20, stream=3)          # the rows' K / V through the next token's logits
    return {"ids": ids, "next_logits_sha256": _sha(dev.state.logits)}


def _prompt_setup(ctx, shape, wtype, n, pos0):
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(17))
    toks = [int(t) for t in rng.integers(3, shape.vocab, size=pos0 + n + 1)]
    dev = ctx.load(shape, wtype, 1)
    if pos0:
        dev.prefill(toks[:pos0], want_logits=False)
    return dev, toks


def _kv(dev, shape, upto):
    L, KV, hd, S = shape.n_layer, shape.n_kv_head, shape.head_dim, shape.seq_len
    return {which + "_sha256": _sha(dev.debug_read(which, L * KV * S * hd).reshape(L, KV, S, hd)[:, :, :upto])
            for which in ("k_cache", "v_cache")}


def _prefill(ctx, n, pos0, wtype="q4_0", shape=BE_A):
    dev, toks = _prompt_setup(ctx, shape, wtype, n, pos0)
    dev.prefill(toks[pos0:pos0 + n], pos0=pos0)
    out = {"logits_sha256": _sha(dev.state.logits), "device_logits_sha256": _sha(dev.debug_read("logits", shape.vocab))}
    out.update(_kv(dev, shape, pos0 + n))
    return out


def _score(ctx, n, pos0, wtype="q4_0", shape=BE_A):
    dev, toks = _prompt_setup(ctx, shape, wtype, n, pos0)
    targets = toks[pos0 + 1:pos0 + n + 1]
    targets[n // 2] = -1                         # a row that is not scored
    lp, am = dev.score(toks[pos0:pos0 + n], targets, pos0=pos0)
    out = {"logprob_sha256": _sha(lp), "argmax": [int(v) for v in am], "device_logits_sha256": _sha(dev.debug_read("logits", shape.vocab))}
    out.update(_kv(dev, shape, pos0 + n))
    return out


def _prefill_then_forward(ctx):
    # the last tile's copies keep the single-token state coherent: the next token's step, and the greedy id behind it
    dev, toks = _prompt_setup(ctx, BE_A, "q4_0", 71, 0)
    dev.prefill(toks[:70])
    out = {"prefill_logits_sha256": _sha(dev.state.logits)}
    dev.forward(toks[70], 70)
    out["forward_logits_sha256"] = _sha(dev.state.logits)
    out["forward_argmax"] = dev.forward_argmax(toks[71], 71)
    return out


def _q4_k_mixed_sample(ctx):
    # rows in an order that differs from (stream, position) order: the fallback's stable sort matters
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(19))
    seqs = [[int(t) for t in rng.integers(3, BE_K.vocab, size=16)] for _ in range(3)]
    dev = ctx.load(BE_K, "q4_k", 3)
    dev.prefill(seqs[2][:10], stream=2, want_logits=False)
    r = [(2, 10), (0, 3), (0, 0), (0, 1), (0, 2)]
    params, us, recents = _sampler_args(rng, BE_K.vocab, 2, 1)
    ids, rec = dev.forward_mixed_sample([s for s, _ in r], [seqs[s][p] for s, p in r], [p for _, p in r], 2, params, us, recents)
    ids2, lg = dev.forward_mixed([s for s, _ in r], [seqs[s][p] for s, p in r], [p for _, p in r], 2, want_logits=True)
    return {"ids": [ids, ids2], "windows": rec, "logits_sha256": _sha(lg)}


def _ring_wrap(ctx):
    # 81 single-token steps through a ring of max(seq_len, max_streams) = 72 control blocks: slot 0 is reused
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(23))
    seqs = [[int(t) for t in rng.integers(3, BE_WRAP.vocab, size=41)] for _ in range(2)]
    dev = ctx.load(BE_WRAP, "q4_k", 2)
    r = [(0, 40)] + [(s, p) for s in (0, 1) for p in range(40)]
    ids, lg = dev.forward_mixed([s for s, _ in r], [seqs[s][p] for s, p in r], [p for _, p in r], 1, want_logits=True)
    dev.forward(seqs[1][40], 40, stream=1)       # the last rows' K / V through the next token's logits
    return {"ids": ids, "logits_sha256": _sha(lg), "next_logits_sha256": _sha(dev.state.logits)}


MIXED_ENV = {"NL_MIXED_ATTN_MIN": "0"}            # as the autouse fixture of tests/test_gpu_mixed.py
NO_GRAPH = {"NL_NO_GRAPH": "1"}

# name: (environment of the case, function of a _Ctx -> record)
CASES = {
    "forward_batch_2": ({}, lambda c: _forward_batch(c, 2)),                       # below NL_BATCH_MIN = 3: the row loop
    "forward_batch_3": ({}, lambda c: _forward_batch(c, 3)),                       # the first batched step
    "forward_batch_37": ({}, lambda c: _forward_batch(c, 37)),                     # nsplit 2 in the key
    "forward_batch_37_q8_0": ({}, lambda c: _forward_batch(c, 37, "q8_0")),        # split-K
    "forward_batch_65": ({}, lambda c: _forward_batch(c, 65)),                     # two LM-head chunks
    "forward_batch_37_no_graph": (NO_GRAPH, lambda c: _forward_batch(c, 37)),
    "forward_batch_sample_2": ({}, lambda c: _forward_batch_sample(c, 2)),
    "forward_batch_sample_3": ({}, lambda c: _forward_batch_sample(c, 3)),
    "forward_batch_sample_37": ({}, lambda c: _forward_batch_sample(c, 37)),
    "forward_batch_sample_37_q8_0": ({}, lambda c: _forward_batch_sample(c, 37, "q8_0")),
    "forward_batch_sample_37_no_graph": (NO_GRAPH, lambda c: _forward_batch_sample(c, 37)),
    "forward_mixed": (MIXED_ENV, lambda c: _mixed(c, False)),
    "forward_mixed_q8_0": (MIXED_ENV, lambda c: _mixed(c, False, "q8_0")),
    "forward_mixed_sample": (MIXED_ENV, lambda c: _mixed(c, True)),
    "forward_mixed_no_graph": ({**MIXED_ENV, **NO_GRAPH}, lambda c: _mixed(c, False)),
    "forward_mixed_no_output_rows": (MIXED_ENV, _mixed_no_output_rows),
    "forward_mixed_per_token_attention": ({**MIXED_ENV, "NL_MIXED_ATTN": "0"}, lambda c: _mixed(c, False)),    # n_work = 0
    "prefill_2": ({}, lambda c: _prefill(c, 2, 0)),                                # the row loop
    "prefill_70_at_100": ({}, lambda c: _prefill(c, 70, 100)),                     # one tile, across position 128
    "prefill_70_at_100_q8_0": ({}, lambda c: _prefill(c, 70, 100, "q8_0")),
    "score_2": ({}, lambda c: _score(c, 2, 0)),
    "score_70_at_100": ({}, lambda c: _score(c, 70, 100)),
    "score_70_at_100_q8_0": ({}, lambda c: _score(c, 70, 100, "q8_0")),
    "prefill_then_forward": ({}, _prefill_then_forward),
    "q4_k_forward_batch_5": ({}, lambda c: _forward_batch(c, 5, "q4_k", BE_K)),
    "q4_k_forward_batch_sample_5": ({}, lambda c: _forward_batch_sample(c, 5, "q4_k", BE_K)),
    "q4_k_forward_mixed_sample_5": (MIXED_ENV, _q4_k_mixed_sample),
    "q4_k_prefill_5": ({}, lambda c: _prefill(c, 5, 3, "q4_k", BE_K)),
    "q4_k_score_5": ({}, lambda c: _score(c, 5, 3, "q4_k", BE_K)),
    "ring_wrap_forward_mixed": (MIXED_ENV, _ring_wrap),
}


def run_case(model, name, workdir):
    """-> the record of CASES[name] (ids, windows, argmax lists, sha256 of logits / log-prob / K / V bytes); FusedTimeout when a
    handle of the case retired its fused plan"""
    env, fn = CASES[name]
    with _env(env):
        ctx = _Ctx(model, workdir)
        try:
            out = fn(ctx)
        except Exception:
            ctx.close()
            raise
        ctx.finish()
    return out


def main():
    from nanollama_amd import _lib, model
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in CASES:
            try:
                out[name] = run_case(model, name, tmp)
            except FusedTimeout as exc:
                print(f"[retry] {name}: {exc}")
                out[name] = run_case(model, name, tmp)
            print(name, json.dumps(out[name])[:120])
    out["_build"] = _lib.build_info()
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
