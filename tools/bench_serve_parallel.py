"""Developer tool: the HTTP server end to end -- C concurrent POST /chat clients against `--serve --parallel N` on a synthetic
model, aggregate generated tokens per second (each response's tokens counted by re-encoding is unreliable, so the server runs
with EOS effectively absent from random weights and every request asks for --max-tokens; the count is requests x max_tokens).

    python tools/bench_serve_parallel.py goldie q4_0 1 64      # --parallel 1 (today's serial server), 64 clients
    python tools/bench_serve_parallel.py goldie q4_0 64 64
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


def main(tier, wtype, parallel, clients, max_tokens=64):
    from nanollama_amd import synth
    path = os.path.join(os.environ.get("NL_BENCH_DIR", "/tmp"), f"nl_bench_{tier}_{wtype}_qrand.gguf")
    if not os.path.exists(path):
        synth.generate_gguf(path + ".tmp", synth.TIERS[tier], wtype, mode="qrand")
        os.replace(path + ".tmp", path)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    proc = subprocess.Popen([sys.executable, "-m", "nanollama_amd", "--model", path, "--serve", "--parallel", str(parallel),
                             "--port", str(port), "--seed", "1", "--max-tokens", str(max_tokens)], cwd=ROOT,
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

        def post(i, out):
            req = urllib.request.Request(f"http://127.0.0.1:{port}/chat", data=json.dumps(
                {"messages": [{"role": "user", "content": "hello number %d" % i}]}).encode(), method="POST")
            with urllib.request.urlopen(req, timeout=600) as r:
                out[i] = r.status

        post(0, [None])                                  # warm: graphs captured, dgemm weights built
        out = [None] * clients
        ths = [threading.Thread(target=post, args=(i, out)) for i in range(clients)]
        t0 = time.perf_counter()
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        dt = time.perf_counter() - t0
        ok = sum(1 for v in out if v == 200)
        print(f"{tier} {wtype} --parallel {parallel}, {clients} clients x {max_tokens} tokens: {dt:.2f} s, "
              f"{ok * max_tokens / dt:.0f} tok/s aggregate ({ok}/{clients} ok)", flush=True)
    finally:
        proc.terminate()
        try:
            proc.wait(30)
        except subprocess.TimeoutExpired:
            proc.kill()
            proc.wait(10)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
