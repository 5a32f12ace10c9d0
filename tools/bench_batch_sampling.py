"""Developer tool: per-step device time (nl_timer_*) of a decode batch in three forms --
  greedy      forward_batch (argmax ids only),
  sampled     forward_batch_sample at the reference defaults (temp 0.8, top-p 0.9, repetition penalty 1.15 over 64 tokens,
              go/main.go:29-34), every row on the device,
  host        forward_batch(want_logits=True) + the host sampler per row (a few steps, for scale: n x vocab logits read back)
for goldie Q4_0 and nano Q8_0 at 16 and 64 streams, positions 8 and 1000.

    python tools/bench_batch_sampling.py                      # the whole table
    python tools/bench_batch_sampling.py goldie q4_0 64 8     # one line (e.g. under rocprofv3 --kernel-trace --stats)
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

from nanollama_amd import gguf, model, synth

DEFAULTS = dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=64)


def one(tier, wtype, ns, pos0, steps=24, host_steps=3, forms=("greedy", "sampled", "host")):
    import sampling_mirror as sm
    path = os.path.join(os.environ.get("NL_BENCH_DIR", "/tmp"), f"nl_bench_{tier}_{wtype}_qrand.gguf")
    if not os.path.exists(path):
        synth.generate_gguf(path + ".tmp", synth.TIERS[tier], wtype, mode="qrand")
        os.replace(path + ".tmp", path)
    g = gguf.load_gguf(path)
    V = g.meta.vocab_size
    dev = model.load_llama_model(g, max_streams=ns)
    rng = np.random.Generator(np.random.PCG64(3))
    streams = list(range(ns))
    start = [int(t) for t in rng.integers(3, V, size=ns)]
    res = {}
    for form in forms:
        for s in streams:
            dev.reset(s)
        ids = list(start)
        recents = [[] for _ in streams]
        p0 = max(0, pos0 - 6)
        for p in range(p0, pos0):                       # warm: KV rows below pos0, step graphs captured
            ids, _ = dev.forward_batch(streams, ids, [p] * ns)
        n = host_steps if form == "host" else steps
        if form == "sampled":                           # (capture of the sampled step's graph outside the timing)
            dev.forward_batch_sample(streams, ids, [pos0] * ns, [DEFAULTS] * ns, rng.random(ns, dtype=np.float32), recents)
        dev.synchronize()
        dev.timer_start()
        t0 = time.perf_counter()
        for k in range(n):
            pos = [pos0 + k] * ns
            if form == "greedy":
                ids, _ = dev.forward_batch(streams, ids, pos)
            elif form == "sampled":
                ids, recents = dev.forward_batch_sample(streams, ids, pos, [DEFAULTS] * ns, rng.random(ns, dtype=np.float32), recents)
            else:
                _, lg = dev.forward_batch(streams, ids, pos, want_logits=True)
                us = rng.random(ns, dtype=np.float32)
                nxt = []
                for i in range(ns):
                    x = sm.apply_penalty(lg[i], recents[i], DEFAULTS["rep_penalty"], V)
                    t = sm.go_top_p(x, DEFAULTS["temperature"], DEFAULTS["top_p"], us[i])
                    nxt.append(t)
                    recents[i] = sm.push_recent(recents[i], t, DEFAULTS["rep_window"])
                ids = nxt
        dt = time.perf_counter() - t0
        ev = dev.timer_stop()
        res[form] = (ev / n, dt / n * 1e3)
        print(f"{tier} {wtype} x {ns} streams, positions {pos0}..: {form:8s} {ev / n:.3f} ms/step device, "
              f"{dt / n * 1e3:.3f} ms/step wall, {ns * n / dt:.0f} tok/s aggregate", flush=True)
    if "greedy" in res and "sampled" in res:
        print(f"{tier} {wtype} x {ns} @ {pos0}: sampled / greedy = {res['sampled'][0] / res['greedy'][0]:.3f} (device)", flush=True)
    dev.close()
    return res


if __name__ == "__main__":
    if len(sys.argv) > 4:
        forms = sys.argv[5].split(",") if len(sys.argv) > 5 else ("greedy", "sampled", "host")
        one(sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), forms=forms)
    else:
        for tier, wtype in (("goldie", "q4_0"), ("nano", "q8_0")):
            for ns in (16, 64):
                for pos0 in (8, 1000):
                    one(tier, wtype, ns, pos0)
