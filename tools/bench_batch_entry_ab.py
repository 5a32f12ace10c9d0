"""Developer tool: A/B of two builds of libnanollama_hip.so on the host side of the batched entry points -- the single-token row
loop (forward_batch, forward_batch_sample, prefill and score of 2 rows: below NL_BATCH_MIN), small decode batches and a short
prompt -- nano Q8_0, wall clock per call around calls that end in a device synchronise.  The builds alternate (NL_LIB_PATH), the
first of a round changing every round; per row and build the median of the rounds and their min..max; the bar a change of host
code is held to: its median inside the other build's min..max.

    python tools/bench_batch_entry_ab.py PARENT.so PR.so [rounds=6] [FILTER]   # the table (FILTER: only the rows whose name holds it)
    python tools/bench_batch_entry_ab.py rows [FILTER]                         # one build's rows (what the driver starts per round)

rows: per row 3 windows of 2000 calls after 50 warm-up calls, the median window; then, without FILTER, `tools/bench_prefill.py
tokens=64 nano`."""
import os, re, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS = 2000
SETTINGS = dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=64)


def rows(only=""):
    import numpy as np
    from nanollama_amd import model
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_modes as b
    g = b.gen("nano", "q8_0")
    dev = model.load_llama_model(g, max_streams=64)
    rng = np.random.Generator(np.random.PCG64(3))
    toks = [int(t) for t in rng.integers(3, g.meta.vocab_size, size=65)]
    us = rng.random(2, dtype=np.float32)
    table = [("forward_batch x 2 (row loop)", CALLS, lambda: dev.forward_batch([0, 1], toks[:2], [4, 4])),
             ("forward_batch_sample x 2 (row loop)", CALLS, lambda: dev.forward_batch_sample([0, 1], toks[:2], [4, 4], [SETTINGS] * 2, us, [[], []])),
             ("prefill 2 tokens (row loop)", CALLS, lambda: dev.prefill(toks[:2])),
             ("score 2 tokens (row loop)", CALLS, lambda: dev.score(toks[:2], toks[1:3]))]
    for ns in (3, 8, 64):
        table.append((f"forward_batch x {ns}", CALLS, lambda ns=ns: dev.forward_batch(list(range(ns)), toks[:ns], [4] * ns)))
    table.append(("prefill 64 tokens", CALLS, lambda: dev.prefill(toks[:64])))
    table.append(("score 64 tokens", CALLS, lambda: dev.score(toks[:64], toks[1:65])))
    for name, calls, fn in table:
        if only not in name:
            continue
        for _ in range(50):
            fn()
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            runs.append((time.perf_counter() - t0) / calls * 1e3)
        print(f"ROW {name}, {calls} calls: {sorted(runs)[1]:.4f} ms", flush=True)
    if dev.last_error():
        print("NOTE", dev.last_error())
    dev.close()


def main():
    builds = {"parent": os.path.abspath(sys.argv[1]), "pr": os.path.abspath(sys.argv[2])}
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    only = sys.argv[4] if len(sys.argv) > 4 else ""
    children = [[sys.executable, os.path.abspath(__file__), "rows", only]]
    if not only:
        children.append([sys.executable, os.path.join(ROOT, "tools", "bench_prefill.py"), "tokens=64", "nano"])
    got = {}
    for r in range(rounds):
        for build in (("parent", "pr") if r % 2 == 0 else ("pr", "parent")):
            for cmd in children:
                p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, NL_LIB_PATH=builds[build]), timeout=240, capture_output=True, text=True)
                if p.returncode:         # a failed child: stop, nothing more is started on the GPU
                    print(f"failed ({p.returncode}): {build} {cmd}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", flush=True)
                    sys.exit(1)
                for line in p.stdout.splitlines():
                    m = re.match(r"ROW (.*): ([\d.]+) ms", line) or re.match(r"(\S+ q4_0 \d+-token prompt, \S+): ([\d.]+) ms", line)
                    if m:
                        name = m.group(1) if line.startswith("ROW") else "bench_prefill.py " + m.group(1) + ", best of 5"
                        got.setdefault(name, {}).setdefault(build, []).append(float(m.group(2)))
    print(f"{rounds} rounds, builds alternating; ms per call, median (min..max)")
    print(f"{'row':58s} {'parent':>28s} {'pr':>28s}  pr median in the parent's range")
    for name, by in got.items():
        a, b = by["parent"], by["pr"]
        ma, mb = statistics.median(a), statistics.median(b)
        print(f"{name:58s} {ma:8.4f} ({min(a):.4f}..{max(a):.4f}) {mb:8.4f} ({min(b):.4f}..{max(b):.4f})  "
              f"{'yes' if min(a) <= mb <= max(a) else ('below' if mb < min(a) else 'ABOVE')}", flush=True)


if __name__ == "__main__":
    rows(*sys.argv[2:3]) if sys.argv[1:2] == ["rows"] else main()
