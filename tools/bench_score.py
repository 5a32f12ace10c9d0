"""Developer tool: what scoring 2047 tokens costs on mini / goldie Q4_0.  Three routes over the same ids on the same build:

  score    nl_score: the prompt path with an LM head over every row and the device reduction (no logits leave the device)
  prefill  nl_prefill of the same ids (what the score costs on top of it is the LM head over all rows + the reduction)
  host     the route without nl_score: nl_forward_mixed in steps of 64 output rows, the logits to the host, a float64 numpy
           log-softmax there

score and prefill are timed with the handle's device events (nl_timer_*) and with the host clock around the call (which ends in
a synchronise); the host route with the host clock only, since its numpy half is not device work.  The rounds alternate the
routes; the median and the minimum of the rounds are printed.  Every slab size (NL_SCORE_SLAB) runs in a fresh child, so each
allocates its own scratch and no size inherits another's warm state.

    python3 tools/bench_score.py [--tiers mini goldie] [--slabs 64 128 256 512] [--rounds 7] [--host-rounds 3]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

N_TOKENS = 2047


def host_route(dev, ids, targets):
    """log P(targets[i]) by the route a caller has without nl_score"""
    out = np.zeros(len(ids), dtype=np.float64)
    for t0 in range(0, len(ids), 64):
        n = min(64, len(ids) - t0)
        _, lg = dev.forward_mixed([0] * n, ids[t0:t0 + n], list(range(t0, t0 + n)), n, want_logits=True)
        x = lg.astype(np.float64)
        m = x.max(axis=1)
        lse = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
        out[t0:t0 + n] = x[np.arange(n), targets[t0:t0 + n]] - lse
    return out


def child(tier, path, rounds, host_rounds):
    from nanollama_amd import gguf, model, synth
    g = gguf.load_gguf(path)
    dev = model.load_llama_model(g)
    ids = synth.prompt_ids(N_TOKENS + 1, g.meta.vocab_size)
    toks, targets = ids[:-1], ids[1:]

    def timed(fn):
        dev.reset()
        dev.synchronize()
        dev.timer_start()
        t0 = time.perf_counter()
        r = fn()
        wall = (time.perf_counter() - t0) * 1e3
        return r, dev.timer_stop(), wall

    run_score = lambda: dev.score(toks, targets)[0]
    run_prefill = lambda: dev.prefill(toks, want_logits=False)
    for fn in (run_score, run_prefill):          # warm-up: code objects, the handle's scratch
        timed(fn)
    ev = {"score": [], "prefill": []}
    wall = {"score": [], "prefill": [], "host": []}
    lp = None
    for _ in range(rounds):
        for name, fn in (("prefill", run_prefill), ("score", run_score)):
            r, e, w = timed(fn)
            ev[name].append(e)
            wall[name].append(w)
            lp = r if name == "score" else lp
    diff = None
    if host_rounds:
        timed(lambda: host_route(dev, toks, targets))
        for _ in range(host_rounds):
            r, _, w = timed(lambda: host_route(dev, toks, targets))
            wall["host"].append(w)
        diff = float(np.abs(r - lp.astype(np.float64)).max())
    dev.close()
    stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v))} if v else None
    print(json.dumps({"tier": tier, "slab": int(os.environ.get("NL_SCORE_SLAB", "512")), "tokens": N_TOKENS,
                      "event_ms": {k: stat(v) for k, v in ev.items()}, "wall_ms": {k: stat(v) for k, v in wall.items()},
                      "logprob_sum": float(lp.astype(np.float64).sum()), "max_abs_host_minus_device": diff}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiers", nargs="+", default=["mini", "goldie"])
    ap.add_argument("--slabs", nargs="+", type=int, default=[64, 128, 256, 512])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--child", nargs=2, metavar=("TIER", "PATH"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.rounds, args.host_rounds)
        return 0
    from nanollama_amd import synth
    for tier in args.tiers:
        path = os.path.join(tempfile.gettempdir(), f"nl_modes_{tier}_q4_0.gguf")
        if not os.path.exists(path):
            synth.generate_gguf(path, synth.TIERS[tier], "q4_0", mode="qrand")
        for k, slab in enumerate(args.slabs):
            env = dict(os.environ, NL_SCORE_SLAB=str(slab))
            cmd = [sys.executable, os.path.abspath(__file__), "--child", tier, path, "--rounds", str(args.rounds),
                   "--host-rounds", str(args.host_rounds if k == 0 else 0)]        # the host route does not depend on the slab
            out = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if out.returncode != 0:
                print(out.stderr[-2000:], file=sys.stderr)
                return out.returncode
            r = json.loads(out.stdout.strip().splitlines()[-1])
            e, w = r["event_ms"], r["wall_ms"]
            line = (f"{tier} q4_0 {N_TOKENS} tokens, slab {slab}: score {e['score']['median']:.3f} ms (min {e['score']['min']:.3f}), "
                    f"prefill {e['prefill']['median']:.3f} ms (min {e['prefill']['min']:.3f}) on device events; "
                    f"host clock score {w['score']['median']:.3f}, prefill {w['prefill']['median']:.3f}")
            if w["host"]:
                line += (f", host route {w['host']['median']:.1f} ms (min {w['host']['min']:.1f}); "
                         f"max|host - device logprob| {r['max_abs_host_minus_device']:.2e}")
            print(line + f"; logprob sum {r['logprob_sum']:.4f}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
