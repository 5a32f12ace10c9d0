"""Developer tool: what a gamma essence / a voice costs.  One JSON line per measurement.

  nano    nano Q8_0 greedy decode (decode_greedy chunks from position 8) without a gamma, with one through nl_set_gamma and --
          where the library has voices -- with one through a bound voice; tok/s and whether the persistent launch served it
  batch   goldie Q4_0 x 64 streams, one sampled decode step at positions 8.. (the shape of tools/bench_batch_sampling.py) with
          no voice defined, one voice on every row, and 8 voices spread over the rows; ms/step (device timer)

    python tools/bench_voices.py                 # both
    python tools/bench_voices.py nano [label]    # label: copied into every line (e.g. "parent r1" in an alternating run)

The tool also runs on a tree from before voices (set_gamma only): the lines it cannot measure there are left out.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from nanollama_amd import gguf, model, synth

DEFAULTS = dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=64)


def _model(tier, wtype):
    path = os.path.join(os.environ.get("NL_BENCH_DIR", "/tmp"), f"nl_bench_{tier}_{wtype}_qrand.gguf")
    if not os.path.exists(path):
        synth.generate_gguf(path + ".tmp", synth.TIERS[tier], wtype, mode="qrand")
        os.replace(path + ".tmp", path)
    return gguf.load_gguf(path)


def _essence(g, seed, first=0, step=2):
    """every `step`-th token id from `first` on, values of the size of a trained essence's (0.3 sigma)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    idx = np.arange(first, g.meta.vocab_size, step, dtype=np.int32)
    return idx, (rng.standard_normal((idx.size, g.meta.embed_dim)) * 0.3).astype(np.float32)


def _emit(label, **kw):
    print(json.dumps(dict(label=label, **kw)), flush=True)


def nano(label, steps=512, runs=3):
    g = _model("nano", "q8_0")
    forms = ["none", "gamma"] + (["voice"] if hasattr(model.LlamaModel, "set_voice") else [])
    for form in forms:
        dev = model.load_llama_model(g)
        if form == "gamma":
            dev.set_gamma(*_essence(g, 1))
        elif form == "voice":
            dev.set_voice(1, *_essence(g, 1))
            dev.stream_voice(0, 1)
        prompt = synth.prompt_ids(8, g.meta.vocab_size, seed=3)
        rates = []
        for r in range(runs + 1):                     # (the first run warms: graphs, clocks)
            dev.reset()
            dev.prefill(prompt)
            first = int(np.argmax(dev.state.logits))
            base = dev.persist_info()["tokens"]
            dev.synchronize()
            t0 = time.perf_counter()
            ids = dev.decode_greedy(first, len(prompt), steps)
            dt = time.perf_counter() - t0
            if r:
                rates.append(len(ids) / dt)
        persistent = dev.persist_info()["tokens"] - base
        _emit(label, bench="nano_q8_0_greedy", gamma=form, steps=steps, tok_s=[round(x, 1) for x in rates],
              tok_s_median=round(float(np.median(rates)), 1), persistent_tokens_last_run=persistent, note=dev.last_error())
        dev.close()


def batch(label, ns=64, pos0=8, steps=24):
    g = _model("goldie", "q4_0")
    V = g.meta.vocab_size
    forms = [0] + ([1, 8] if hasattr(model.LlamaModel, "set_voice") else [])
    for nv in forms:
        dev = model.load_llama_model(g, max_streams=ns)
        for v in range(1, nv + 1):
            dev.set_voice(v, *_essence(g, 10 + v, first=v % 2))
        rng = np.random.Generator(np.random.PCG64(3))
        streams = list(range(ns))
        for s in streams:
            dev.reset(s)
            if nv:
                dev.stream_voice(s, 1 + s % nv)
        ids = [int(t) for t in rng.integers(3, V, size=ns)]
        recents = [[] for _ in streams]
        for p in range(max(0, pos0 - 6), pos0):
            ids, _ = dev.forward_batch(streams, ids, [p] * ns)
        dev.forward_batch_sample(streams, ids, [pos0] * ns, [DEFAULTS] * ns, rng.random(ns, dtype=np.float32), recents)
        dev.synchronize()
        dev.timer_start()
        t0 = time.perf_counter()
        for k in range(steps):
            ids, recents = dev.forward_batch_sample(streams, ids, [pos0 + k] * ns, [DEFAULTS] * ns,
                                                    rng.random(ns, dtype=np.float32), recents)
        dt = time.perf_counter() - t0
        ev = dev.timer_stop()
        _emit(label, bench=f"goldie_q4_0_x{ns}_sampled_pos{pos0}", voices=nv, ms_step_device=round(ev / steps, 4),
              ms_step_wall=round(dt / steps * 1e3, 4))
        dev.close()


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    label = sys.argv[2] if len(sys.argv) > 2 else ""
    if which in ("nano", "both"):
        nano(label)
    if which in ("batch", "both"):
        batch(label)
