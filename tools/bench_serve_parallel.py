"""Developer tool: the HTTP server end to end -- C concurrent POST /chat clients against `--serve --parallel N` on a synthetic
model, aggregate generated tokens per second (each response's tokens counted by re-encoding is unreliable, so the server runs
with EOS effectively absent from random weights and every request asks for --max-tokens; the count is requests x max_tokens).

    python tools/bench_serve_parallel.py goldie q4_0 1 64      # --parallel 1 (today's serial server), 64 clients
    python tools/bench_serve_parallel.py goldie q4_0 64 64
    python tools/bench_serve_parallel.py goldie q4_0 64 64 --prefill-chunk 64    # long prompts arriving while others decode:
                                                                                  # chunk 0, then chunk N, of the same build

With --prefill-chunk N the workload is `clients` short requests that decode while clients / 8 requests with long prompts
(about a thousand characters) arrive 50 ms apart; for chunk 0 (whole prompts at admission) and chunk N it prints the aggregate tok/s and the
scheduler's max_step_gap_ms -- the longest interval between two consecutive steps that both carried a decoding row, i.e. how
long the running requests waited for an admission.
"""
import json
import os
import socket
import subprocess
import sys
import threading
import time
import urllib.request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(tier, wtype, parallel, clients, max_tokens=64, prefill_chunk=None):
    from nanollama_amd import synth
    path = os.path.join(os.environ.get("NL_BENCH_DIR", "/tmp"), f"nl_bench_{tier}_{wtype}_qrand.gguf")
    if not os.path.exists(path):
        synth.generate_gguf(path + ".tmp", synth.TIERS[tier], wtype, mode="qrand")
        os.replace(path + ".tmp", path)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    extra = ["--prefill-chunk", str(prefill_chunk)] if prefill_chunk else []
    proc = subprocess.Popen([sys.executable, "-m", "nanollama_amd", "--model", path, "--serve", "--parallel", str(parallel),
                             "--port", str(port), "--seed", "1", "--max-tokens", str(max_tokens)] + extra, cwd=ROOT,
                            stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    try:
        for _ in range(600):
            try:
                urllib.request.urlopen(f"http://127.0.0.1:{port}/health", timeout=2).read()
                break
            except OSError:
                if proc.poll() is not None:
                    raise RuntimeError("server exited")
                time.sleep(0.2)

        def post(i, out, text=None):
            req = urllib.request.Request(f"http://127.0.0.1:{port}/chat", data=json.dumps(
                {"messages": [{"role": "user", "content": text or "hello number %d" % i}]}).encode(), method="POST")
            with urllib.request.urlopen(req, timeout=600) as r:
                out[i] = r.status

        post(0, [None])                                  # warm: graphs captured, dgemm weights built
        n_long = max(1, clients // 8) if prefill_chunk is not None else 0
        if n_long:                                       # warm the admission path too (step graphs of the chunked steps)
            post(0, [None], "warm " * 180)
        out = [None] * clients
        ths = [threading.Thread(target=post, args=(i, out)) for i in range(clients - n_long)]
        ths += [threading.Thread(target=post, args=(clients - n_long + j, out, "a long prompt %d " % j * 60)) for j in range(n_long)]
        t0 = time.perf_counter()
        for i, t in enumerate(ths):
            if i >= clients - n_long and n_long:
                time.sleep(0.05)                         # the long prompts arrive while the short requests decode
            t.start()
        for t in ths:
            t.join()
        dt = time.perf_counter() - t0
        ok = sum(1 for v in out if v == 200)
        health = json.loads(urllib.request.urlopen(f"http://127.0.0.1:{port}/health", timeout=10).read())
        print(f"{tier} {wtype} --parallel {parallel}" + (f" --prefill-chunk {prefill_chunk}" if prefill_chunk is not None else "") +
              f", {len(ths)} clients x {max_tokens} tokens" + (f" ({n_long} with long prompts)" if n_long else "") +
              f": {dt:.2f} s, {ok * max_tokens / dt:.0f} tok/s aggregate ({ok}/{len(ths)} ok)" +
              (f", max_step_gap_ms {health.get('max_step_gap_ms')}, {health.get('steps')} steps" if "steps" in health else ""), flush=True)
    finally:
        proc.terminate()
        try:
            proc.wait(30)
        except subprocess.TimeoutExpired:
            proc.kill()
            proc.wait(10)


if __name__ == "__main__":
    if "--prefill-chunk" in sys.argv:
        chunk = int(sys.argv[sys.argv.index("--prefill-chunk") + 1])
        for c in (0, chunk):
            main(sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), prefill_chunk=c)
    else:
        main(sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
