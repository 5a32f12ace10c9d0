"""Developer tool: A/B of two builds of libnanollama_hip.so on the host side of the single-stream entry points -- per-call forward
with logits and forward_argmax on the resident session, forward_argmax on the one-step persistent launch (NL_PERSIST_SESSION=0) and
on the call box (NL_PERSIST=0), decode_greedy and sample_decode of 256 tokens -- nano Q8_0, wall clock per call, and bench.py's
headline; and of the launch plans' closures, which the host runs wherever no graph replays them: forward_argmax with eager launches
(NL_PERSIST=0 NL_NO_GRAPH=1), a step of the in-process shard group on the two-launch rank plan (LocalTPGroup(fused=True), tp 2, a
three-layer D 1024 Q4_0 model), and load_llama_model itself (plan building and graph capture).  The builds alternate (NL_LIB_PATH), the first of a round changing every round; per row and build the median of the
rounds and their min..max; the bar a change of host code is held to: its median inside the other build's min..max.

    python tools/bench_single_entry_ab.py PARENT.so PR.so [rounds=5]    # the table
    python tools/bench_single_entry_ab.py rows                          # one build's rows (what the driver starts per round)

rows: per-call rows 3 windows of 1000 calls (positions 8 .. 1007 of a reset stream) after a warm-up window, chains 3 windows of 8
calls, group steps 3 windows of 300 (positions 0 .. 299), loads 3 after a first; the median window."""
import json, os, re, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETTINGS = dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=64)


def rows():
    import numpy as np
    from nanollama_amd import model
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_modes as b
    g = b.gen("nano", "q8_0")
    rng = np.random.Generator(np.random.PCG64(3))
    toks = [int(t) for t in rng.integers(3, g.meta.vocab_size, size=1024)]
    us = rng.random(256, dtype=np.float32)

    def per_call(dev, call):
        def window():
            dev.reset()
            dev.prefill(toks[:8], want_logits=False)
            t0 = time.perf_counter()
            for pos in range(8, 1008):
                call(toks[pos], pos)
            return (time.perf_counter() - t0) / 1000 * 1e3
        return window

    def chain(dev, call):
        def window():
            t0 = time.perf_counter()
            for _ in range(8):
                call()
            return (time.perf_counter() - t0) / 8 * 1e3
        return window

    table = [("forward with logits, session", {}, lambda d: per_call(d, d.forward)),
             ("forward_argmax, session", {}, lambda d: per_call(d, d.forward_argmax)),
             ("forward_argmax, one-step persistent launch", {"NL_PERSIST_SESSION": "0"}, lambda d: per_call(d, d.forward_argmax)),
             ("forward_argmax, call box", {"NL_PERSIST": "0"}, lambda d: per_call(d, d.forward_argmax)),
             ("forward with logits, call box", {"NL_PERSIST": "0"}, lambda d: per_call(d, d.forward)),
             ("forward_argmax, eager launch plans", {"NL_PERSIST": "0", "NL_NO_GRAPH": "1"}, lambda d: per_call(d, d.forward_argmax)),
             ("decode_greedy x 256", {}, lambda d: chain(d, lambda: d.decode_greedy(toks[8], 8, 256))),
             ("decode_greedy x 256, launch plans", {"NL_PERSIST": "0"}, lambda d: chain(d, lambda: d.decode_greedy(toks[8], 8, 256))),
             ("sample_decode x 256", {}, lambda d: chain(d, lambda: d.sample_decode(8, 256, uniforms=us, recent=[], **SETTINGS)))]
    for name, env, make in table:
        os.environ.update(env)                 # (handle knobs: read when the handle is made)
        dev = model.load_llama_model(g)
        for k in env:
            del os.environ[k]
        dev.prefill(toks[:8])
        window = make(dev)
        window()
        runs = sorted(window() for _ in range(3))
        print(f"ROW {name}: {runs[1]:.4f} ms", flush=True)
        if dev.last_error():
            print("NOTE", name, dev.last_error(), flush=True)
        dev.close()

    def row(name, window):
        window()
        runs = sorted(window() for _ in range(3))
        print(f"ROW {name}: {runs[1]:.4f} ms", flush=True)

    from nanollama_amd import gguf, synth
    shape = synth.ModelShape("ab_tp2", 3, 1024, 16, 4, 4096, seq_len=320, interm=2048)      # gqa4 of tests/test_gpu_tp_fused.py
    path = "/tmp/nl_ab_tp2_q4_0.gguf"
    if not os.path.exists(path):
        synth.generate_gguf(path, shape, "q4_0", 1004, mode="qrand")
    grp = model.LocalTPGroup(gguf.load_gguf(path), 2, fused=True)

    def group_window():
        t0 = time.perf_counter()
        for pos in range(300):
            grp.forward(toks[pos] % shape.vocab, pos)
        return (time.perf_counter() - t0) / 300 * 1e3
    row("LocalTPGroup(fused=True) step, tp 2", group_window)
    if grp.shards[0].plan_info()["fused_mode"] != 3 or grp.shards[0].last_error():
        print("NOTE group", grp.shards[0].plan_info(), grp.shards[0].last_error(), flush=True)
    grp.close()

    def load_window():
        t0 = time.perf_counter()
        dev = model.load_llama_model(g)
        dt = time.perf_counter() - t0
        dev.close()
        return dt * 1e3
    row("load_llama_model, nano q8_0", load_window)


def main():
    builds = {"parent": os.path.abspath(sys.argv[1]), "pr": os.path.abspath(sys.argv[2])}
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    children = [[sys.executable, os.path.abspath(__file__), "rows"],
                [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "512", "--warmup", "64"]]
    got = {}
    for r in range(rounds):
        for build in (("parent", "pr") if r % 2 == 0 else ("pr", "parent")):
            for cmd in children:
                p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, NL_LIB_PATH=builds[build]), timeout=240, capture_output=True, text=True)
                if p.returncode:         # a failed child: stop, nothing more is started on the GPU
                    print(f"failed ({p.returncode}): {build} {cmd}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", flush=True)
                    sys.exit(1)
                print(f"round {r} {build}: {os.path.basename(cmd[1])} done", flush=True)
                for line in p.stdout.splitlines():
                    m = re.match(r"ROW (.*): ([\d.]+) ms", line)
                    if m:
                        got.setdefault(m.group(1) + " (ms)", {}).setdefault(build, []).append(float(m.group(2)))
                    elif line.startswith("NOTE"):
                        print(f"round {r} {build}: {line}", flush=True)
                    elif line.startswith("{") and '"value"' in line:
                        got.setdefault("bench.py headline (tokens/s)", {}).setdefault(build, []).append(float(json.loads(line)["value"]))
    print(f"{rounds} rounds, builds alternating; median (min..max)")
    print(f"{'row':52s} {'parent':>30s} {'pr':>30s}  pr median in the parent's range")
    for name, by in got.items():
        a, b = by["parent"], by["pr"]
        ma, mb = statistics.median(a), statistics.median(b)
        print(f"{name:52s} {ma:9.4f} ({min(a):.4f}..{max(a):.4f}) {mb:9.4f} ({min(b):.4f}..{max(b):.4f})  "
              f"{'yes' if min(a) <= mb <= max(a) else ('below' if mb < min(a) else 'ABOVE')}", flush=True)


if __name__ == "__main__":
    rows() if sys.argv[1:2] == ["rows"] else main()
