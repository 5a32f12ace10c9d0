"""Developer tool: device time (nl_timer_*) of one mixed step -- 48 decode rows beside one chunk of a prompt -- against the two
calls it replaces, goldie Q4_0 and nano Q8_0:

  mixed       forward_mixed_sample: the 48 decode rows (output rows) + the chunk's rows in one step,
  separate    prefill of the chunk (nl_prefill) + forward_batch_sample of the 48 rows: what whole-prompt admission runs, the
              decode rows waiting for the prefill,
  tile        the mixed step under NL_MIXED_ATTN_MIN=0 (the chunk on the segment-tile kernel whatever its size),
  per-token   the mixed step under NL_MIXED_ATTN=0 (every row on the per-token attention kernel).

Shapes: decode rows at positions ~8 and ~500; a chunk of 16 / 64 / 192 tokens whose stream stands at position 0 and at 512.
Every figure is the median of `repeats` timed runs of `steps` steps; each shape runs in a child process under its own time
limit, so one that hangs does not hold the others.

    python tools/bench_mixed_step.py                          # the whole table
    python tools/bench_mixed_step.py goldie q4_0 500 64 512   # one shape: decode position, chunk rows, chunk position
"""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ND = 48
DEFAULTS = dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=64)


def one(tier, wtype, dpos, chunk, cpos, steps=8, repeats=5):
    from nanollama_amd import gguf, model, synth
    path = os.path.join(os.environ.get("NL_BENCH_DIR", "/tmp"), f"nl_bench_{tier}_{wtype}_qrand.gguf")
    if not os.path.exists(path):
        synth.generate_gguf(path + ".tmp", synth.TIERS[tier], wtype, mode="qrand")
        os.replace(path + ".tmp", path)
    g = gguf.load_gguf(path)
    V = g.meta.vocab_size
    dev = model.load_llama_model(g, max_streams=ND + 1)
    rng = np.random.Generator(np.random.PCG64(3))
    dec = list(range(ND))
    # K / V below the positions of the timed steps: every step of a run rewrites the same rows (same positions each time)
    for s in dec:
        dev.prefill([int(t) for t in rng.integers(3, V, size=dpos)], stream=s, want_logits=False)
    if cpos:
        dev.prefill([int(t) for t in rng.integers(3, V, size=cpos)], stream=ND, want_logits=False)
    dtok = [int(t) for t in rng.integers(3, V, size=ND)]
    ctok = [int(t) for t in rng.integers(3, V, size=chunk)]
    us = rng.random(ND, dtype=np.float32)
    recents = [[] for _ in dec]
    streams = dec + [ND] * chunk
    tokens = dtok + ctok
    pos = [dpos] * ND + list(range(cpos, cpos + chunk))

    def mixed():
        dev.forward_mixed_sample(streams, tokens, pos, ND, [DEFAULTS] * ND, us, recents)

    def separate():
        dev.prefill(ctok, pos0=cpos, stream=ND, want_logits=False)
        dev.forward_batch_sample(dec, dtok, [dpos] * ND, [DEFAULTS] * ND, us, recents)

    def timed(fn):
        fn()                                              # graphs captured, weight copies built
        runs = []
        for _ in range(repeats):
            dev.synchronize()
            dev.timer_start()
            for _ in range(steps):
                fn()
            runs.append(dev.timer_stop() / steps)
        return float(np.median(runs)), (max(runs) - min(runs)) / float(np.median(runs))

    res = {}
    res["mixed"] = timed(mixed)
    res["separate"] = timed(separate)
    for name, knob in (("tile", "NL_MIXED_ATTN_MIN"), ("per-token", "NL_MIXED_ATTN")):
        os.environ[knob] = "0"                            # step knobs: read per call
        res[name] = timed(mixed)
        del os.environ[knob]
    dev.close()
    m, s, f, t = res["mixed"], res["separate"], res["tile"], res["per-token"]
    print(f"{tier} {wtype}: {ND} decode rows @ {dpos} + {chunk:3d}-token chunk @ {cpos:3d}: mixed {m[0]:.3f} ms (spread {m[1] * 100:.1f} %), "
          f"prefill + batch {s[0]:.3f} ms (spread {s[1] * 100:.1f} %), mixed / separate {m[0] / s[0]:.3f}; "
          f"NL_MIXED_ATTN_MIN=0 {f[0]:.3f} ms, NL_MIXED_ATTN=0 {t[0]:.3f} ms (tile / per-token {f[0] / t[0]:.3f})", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 5:
        one(sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    else:
        for tier, wtype in (("goldie", "q4_0"), ("nano", "q8_0")):
            for dpos in (8, 500):
                for cpos in (0, 512):
                    for chunk in (16, 64, 192):
                        try:
                            rc = subprocess.run([sys.executable, os.path.abspath(__file__), tier, wtype, str(dpos), str(chunk), str(cpos)],
                                                timeout=120).returncode
                        except subprocess.TimeoutExpired:
                            rc = "time limit"
                        if rc:                            # a failed shape: stop, nothing more is started on the GPU
                            print(f"{tier} {wtype} {dpos} {chunk} {cpos}: failed ({rc})", flush=True)
                            sys.exit(1)
