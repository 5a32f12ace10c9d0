"""Developer tool: what nl_kv_fork costs and what it saves.  One JSON line per measurement.

  copy     nl_kv_fork on goldie Q4_0 and nano Q8_0: n_pos 64 / 512 / 1000 / 2047 into 1 / 15 / 63 destinations, device events,
           median of 7; achieved bytes/s from (1 + n_dst) * 2 * L * KV * n_pos * hd * 4, for each cache policy of the kernel
           (NL_FORK_POLICY 0 / 1 / 2: plain, non-temporal stores, non-temporal loads and stores)
  samples  time from request to the first sampled token of all rows for n = 16 and 64 samples of a 1000-token prompt through
           the scheduler: one generate_samples(n) request (one prefill, one fork) against n generate_quiet requests that each
           prefill (what a tree without nl_kv_fork has to do), alternated, three rounds

    python tools/bench_fork.py                     # both
    python tools/bench_fork.py copy [tier ...]     # tiers: goldie nano
    python tools/bench_fork.py samples
"""
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from nanollama_amd import gguf, model, synth
from nanollama_amd.engine import GenParams

TIERS = {"goldie": "q4_0", "nano": "q8_0"}


def _model(tier, wtype):
    path = os.path.join(os.environ.get("NL_BENCH_DIR", "/tmp"), f"nl_bench_{tier}_{wtype}_qrand.gguf")
    if not os.path.exists(path):
        synth.generate_gguf(path + ".tmp", synth.TIERS[tier], wtype, mode="qrand")
        os.replace(path + ".tmp", path)
    return gguf.load_gguf(path)


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def copy(tiers):
    for tier in tiers:
        g = _model(tier, TIERS[tier])
        m = g.meta
        per_pos = 2 * m.num_layers * m.num_kv_heads * m.head_dim * 4           # bytes per position and stream, K and V
        for policy in (0, 1, 2):
            os.environ["NL_FORK_POLICY"] = str(policy)
            dev = model.load_llama_model(g, max_streams=64)
            top = min(2047, dev.config.seq_len - 1)
            dev.prefill(synth.prompt_ids(top, m.vocab_size, seed=3), stream=0, want_logits=False)
            for n_pos in (64, 512, 1000, top):
                for n_dst in (1, 15, 63):
                    dst = list(range(1, 1 + n_dst))
                    ms = []
                    for r in range(8):                                         # (the first call warms)
                        dev.synchronize()
                        dev.timer_start()
                        dev.kv_fork(0, dst, n_pos)
                        t = dev.timer_stop()
                        if r:
                            ms.append(t)
                    nbytes = (1 + n_dst) * per_pos * n_pos
                    med = float(np.median(ms))
                    _emit(bench="kv_fork", tier=tier, policy=policy, n_pos=n_pos, n_dst=n_dst, bytes=nbytes,
                          us=[round(x * 1e3, 1) for x in ms], us_median=round(med * 1e3, 1), tb_s=round(nbytes / (med * 1e-3) / 1e12, 3))
            dev.close()
        os.environ.pop("NL_FORK_POLICY", None)


class FixedTokenizer:
    """every prompt is the same 1000 ids; pieces are one byte"""
    eos_id = -1

    def __init__(self, ids):
        self.ids = ids

    def encode(self, text, add_bos=True):
        return list(self.ids)

    def decode_token_bytes(self, t):
        return b"a"


def samples(rounds=3, n_prompt=1000):
    from nanollama_amd.batch_serve import BatchScheduler
    g = _model("goldie", "q4_0")
    dev = model.load_llama_model(g, max_streams=64)
    tok = FixedTokenizer(synth.prompt_ids(n_prompt, g.meta.vocab_size, seed=5))
    sched = BatchScheduler(dev, tok, 64, seed=1)
    p = GenParams(max_tokens=1, temperature=0.8, top_p=0.9, top_k=50)          # done at the first sampled token of every row
    try:
        sched.generate_samples("warm", p, 64)                                  # graphs, clocks
        for n in (16, 64):
            sched.generate_samples("warm", p, n)
            for r in range(rounds):
                t0 = time.perf_counter()
                sched.generate_samples("x", p, n)
                forked = time.perf_counter() - t0
                ths = [threading.Thread(target=sched.generate_quiet, args=("x", p)) for _ in range(n)]
                t0 = time.perf_counter()
                for t in ths:
                    t.start()
                for t in ths:
                    t.join()
                separate = time.perf_counter() - t0
                _emit(bench="first_token_of_all_rows", tier="goldie", n=n, n_prompt=n_prompt, round=r,
                      one_request_ms=round(forked * 1e3, 2), n_requests_ms=round(separate * 1e3, 2))
    finally:
        sched.close()
        dev.close()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "both"
    if what in ("copy", "both"):
        copy(sys.argv[2:] or list(TIERS))
    if what in ("samples", "both"):
        samples()
