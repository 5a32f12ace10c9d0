"""Bit-level record of the single-stream entry points (nl_forward, nl_forward_argmax, nl_decode_greedy, nl_sample_decode,
nl_profile_forward, nl_group_forward) and of the op-level entry points (nl_op_*, nanollama_amd/csrc/nl_engine.hip): for each case
below the returned ids, windows and n_recent as lists, the sha256 of logits and K / V bytes, and HOW the case was served -- the
counters of persist_info() (ready, launches, tokens) and plan_info() of every handle, so that a case cannot silently run on
another rung of the ladder than the one it is meant to hold.  Run at a commit whose results are to be kept, the output is the
fixture the next commit is held to (tests/golden/single_entry_parent_hashes.json; tests/test_gpu_single_entry_bits.py imports CASES
and run_case from here).  Knobs of a case are set before its handles are made (they are read in nl_create).
usage: python tools/single_entry_hashes.py OUT.json        (python tools/single_entry_hashes.py --group-worker GGUF: the group case's child)"""
import contextlib
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nanollama_amd import gguf, synth

# the small persistent instantiations (pd_decode_kernel<8, 16, 2 / 4>) of tests/test_gpu_persist.py and tools/batch_entry_hashes.py
SE_KV2 = synth.ModelShape("se_kv2", 2, 256, 4, 2, 512, seq_len=320, interm=512)
SE_KV4 = synth.ModelShape("se_kv4", 2, 256, 4, 4, 512, seq_len=320, interm=512)
MODELS = ((SE_KV2, "q8_0"), (SE_KV4, "q4_0"))
SE_FUSED = synth.ModelShape("se_fused", 3, 192, 3, 3, 1024, seq_len=96)            # fb_fallback of tests/test_gpu_parity.py: a fused plan
SE_TP = synth.ModelShape("se_tp", 3, 1024, 16, 4, 4096, seq_len=320, interm=2048)  # gqa4 of tests/test_gpu_tp_fused.py
SE_GRP = synth.ModelShape("se_grp", 3, 1024, 16, 4, 4096, seq_len=64, interm=2048)  # grp_probe (n = 2) of tests/test_gpu_group.py
SEED = 311
PROMPT = 9
SETTINGS = [dict(temperature=0.0, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=8),       # greedy
            dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=64),      # top-p
            dict(temperature=1.3, top_p=1.0, top_k=40, rep_penalty=1.3, rep_window=16)]       # top-k

PD_NOTE = "the persistent decode launch gave up"
FUSED_NOTE = "fused-launch cluster exchange timed out"


class Unforced(Exception):
    """a handle of the case carries a note that the case's own knobs did not force (a placement miss of the persistent launch, a
    fused launch whose cluster exchange timed out): the results are right, but the run is no valid recording or comparison"""


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
    def __init__(self, model, workdir, note):
        self.model, self.workdir, self.note, self.devs = model, workdir, note, []

    def gguf(self, shape, wtype, **kw):
        path = os.path.join(self.workdir, f"{shape.name}_{wtype}.gguf")
        if not os.path.exists(path):
            synth.generate_gguf(path, shape, wtype, SEED, **kw)
        return path

    def load(self, shape, wtype, max_streams=1, **kw):
        dev = self.model.load_llama_model(gguf.load_gguf(self.gguf(shape, wtype, **kw)), max_streams=max_streams)
        self.devs.append(dev)
        return dev

    def close(self):
        errs = [dev.last_error() for dev in self.devs]
        for dev in self.devs:
            dev.close()
        return errs

    def finish(self):
        """every note a handle carries is the one the case forces (and then at least one handle carries it)"""
        errs = self.close()
        for err in errs:
            if err and not (self.note and self.note in err):
                raise Unforced(err) if (PD_NOTE in err or FUSED_NOTE in err) else RuntimeError(err)
        if self.note and not any(self.note in err for err in errs):
            raise RuntimeError(f"no handle of the case reported: {self.note}")


def _served(dev):
    """which rung served the handle's calls: [persistent path ready, its launches, its tokens], [fused mode, its position limit,
    launches per token of the fused and of the general plan]"""
    pi, pl = dev.persist_info(), dev.plan_info()
    return {"persist": [int(pi["ready"]), pi["launches"], pi["tokens"]],
            "plan": [pl["fused_mode"], pl["fused_max_pos"], pl["launches_fused"], pl["launches_general"]]}


def _tokens(shape, n, seed=29):
    import numpy as np
    return [int(t) for t in np.random.Generator(np.random.PCG64(seed)).integers(3, shape.vocab, size=n)]


def _kv(dev, shape, upto, stream=0):
    L, KV, hd, S = shape.n_layer, shape.n_kv_head, shape.head_dim, shape.seq_len
    return {which + "_sha256": _sha(dev.debug_read(which, L * KV * S * hd, stream=stream).reshape(L, KV, S, hd)[:, :, :upto])
            for which in ("k_cache", "v_cache")}


def _each_model(fn, models=MODELS):
    """the case on every model of `models`: {"<shape>_<wtype>": record}"""
    def run(ctx):
        return {f"{shape.name}_{wtype}": fn(ctx, shape, wtype) for shape, wtype in models}
    return run


# ---- per-call nl_forward / nl_forward_argmax ------------------------------------------------------------------------------
def _per_call(ctx, shape, wtype, steps=6, **kw):
    """six consecutive positions behind a 9-token prompt: nl_forward (logits) on one handle, nl_forward_argmax on another"""
    toks = _tokens(shape, PROMPT + steps)
    out = {}
    dev = ctx.load(shape, wtype, **kw)
    out["plan_at_start"] = _served(dev)["plan"]
    dev.prefill(toks[:PROMPT], want_logits=False)
    out["logits_sha256"] = []
    for pos in range(PROMPT, PROMPT + steps):
        dev.forward(toks[pos], pos)
        out["logits_sha256"].append(_sha(dev.state.logits))
    out["device_logits_sha256"] = _sha(dev.debug_read("logits", shape.vocab))
    out.update(_kv(dev, shape, PROMPT + steps))
    out["forward_served"] = _served(dev)
    dev = ctx.load(shape, wtype, **kw)
    dev.prefill(toks[:PROMPT], want_logits=False)
    out["ids"] = [dev.forward_argmax(toks[pos], pos) for pos in range(PROMPT, PROMPT + steps)]
    out["argmax_kv"] = _kv(dev, shape, PROMPT + steps)
    out["argmax_served"] = _served(dev)
    return out


def _force_tp_plan(ctx, shape, wtype, steps=6):
    """NL_FORCE_TP_PLAN=1: the all-reduce seams with one rank (a communicator of one), the non-direct logits branch"""
    toks = _tokens(shape, PROMPT + steps)
    g = gguf.load_gguf(ctx.gguf(shape, wtype))
    out = {"logits_sha256": [], "ids": []}
    for which in ("forward", "argmax"):
        dev = ctx.model.load_llama_model(g, comm_id=ctx.model.comm_unique_id())
        ctx.devs.append(dev)
        dev.prefill(toks[:PROMPT], want_logits=False)
        for pos in range(PROMPT, PROMPT + steps):
            if which == "forward":
                dev.forward(toks[pos], pos)
                out["logits_sha256"].append(_sha(dev.state.logits))
            else:
                out["ids"].append(dev.forward_argmax(toks[pos], pos))
        out[which + "_kv"] = _kv(dev, shape, PROMPT + steps)
        out[which + "_served"] = _served(dev)
    return out


def _session_interrupted(ctx, shape, wtype):
    """a resident session ended by a stream switch and by forward / forward_argmax alternations (a session started without
    logits cannot serve a call that wants them)"""
    toks = [_tokens(shape, PROMPT + 8, seed=29 + s) for s in range(2)]
    dev = ctx.load(shape, wtype, max_streams=2)
    for s in range(2):
        dev.prefill(toks[s][:PROMPT], stream=s, want_logits=False)
    out = {"steps": []}
    nxt = [PROMPT, PROMPT]
    for call, s in (("f", 0), ("f", 0), ("f", 1), ("a", 0), ("a", 0), ("f", 0), ("a", 1), ("a", 1), ("f", 1), ("a", 0), ("f", 1)):
        pos = nxt[s]
        nxt[s] += 1
        if call == "f":
            dev.forward(toks[s][pos], pos, stream=s)
            out["steps"].append(_sha(dev.state.logits))
        else:
            out["steps"].append(dev.forward_argmax(toks[s][pos], pos, stream=s))
    for s in range(2):
        out[f"stream{s}"] = _kv(dev, shape, nxt[s], stream=s)
    out["served"] = _served(dev)
    return out


def _above_high_water(ctx, shape, wtype):
    """a step at a position above the stream's high-water mark: 20 positions written, reset, a 9-token prompt, then position 14 --
    rows 9..13 hold the earlier text and are cleared before the step (note_positions)"""
    toks = _tokens(shape, 24)
    out = {}
    for which in ("forward", "argmax"):
        dev = ctx.load(shape, wtype)
        dev.prefill(toks[:20], want_logits=False)
        dev.reset()
        dev.prefill(toks[:PROMPT], want_logits=False)
        if which == "forward":
            dev.forward(toks[14], 14)
            out["logits_sha256"] = _sha(dev.state.logits)
        else:
            out["id"] = dev.forward_argmax(toks[14], 14)
        out[which + "_kv"] = _kv(dev, shape, 15)
        out[which + "_served"] = _served(dev)
    return out


# ---- nl_decode_greedy ---------------------------------------------------------------------------------------------------------
def _greedy(ctx, shape, wtype, steps=40, prompt=PROMPT, **kw):
    toks = _tokens(shape, prompt + 1)
    dev = ctx.load(shape, wtype, **kw)
    out = {"plan_at_start": _served(dev)["plan"]}
    dev.prefill(toks[:prompt], want_logits=False)
    out["ids"] = dev.decode_greedy(toks[prompt], prompt, steps)
    end = prompt + len(out["ids"])
    out["device_logits_sha256"] = _sha(dev.debug_read("logits", shape.vocab))
    out.update(_kv(dev, shape, end))
    out["served"] = _served(dev)
    if end < shape.seq_len:                    # the chain left the single-token state coherent: the next step's logits
        dev.forward(out["ids"][-1], end)
        out["next_logits_sha256"] = _sha(dev.state.logits)
    return out


# ---- nl_sample_decode ---------------------------------------------------------------------------------------------------------
def _window(rng, vocab, setting, filled):
    return [int(t) for t in rng.integers(0, vocab, size=setting["rep_window"] // 2)] if filled else []


def _sample(ctx, shape, wtype, order=(0, 1, 2), steps=40, one_handle=False, **kw):
    """40 sampled steps per setting behind a 9-token prompt's logits (greedy from an empty window, top-p and top-k from half-filled
    ones); one_handle: every call on the same handle, each continuing where the one before stopped (the 16-step graph is captured
    again when the settings change)"""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(37))
    toks = _tokens(shape, PROMPT)
    out = {"ids": [], "windows": [], "n_recent": [], "served": []}
    dev, pos = None, PROMPT
    for k in order:
        if dev is None or not one_handle:
            dev, pos = ctx.load(shape, wtype, **kw), PROMPT
            dev.prefill(toks)
        us = rng.random(steps, dtype=np.float32)
        ids, rec = dev.sample_decode(pos, steps, uniforms=us, recent=_window(rng, shape.vocab, SETTINGS[k], k != 0), **SETTINGS[k])
        pos += len(ids)
        out["ids"].append(ids)
        out["windows"].append(rec)
        out["n_recent"].append(len(rec))
        out["served"].append(_served(dev))
    out["device_logits_sha256"] = _sha(dev.debug_read("logits", shape.vocab))
    out.update(_kv(dev, shape, pos))
    return out


# ---- nl_profile_forward -------------------------------------------------------------------------------------------------------
def _profile(ctx, shape, wtype, **kw):
    toks = _tokens(shape, PROMPT + 2)
    dev = ctx.load(shape, wtype, **kw)
    out = {"plan_at_start": _served(dev)["plan"]}
    dev.prefill(toks[:PROMPT], want_logits=False)
    prof = dev.profile_forward(toks[PROMPT], PROMPT, iters=3)
    out["calls"] = [[kind, calls] for kind, (_, calls) in prof.items()]
    dev.prefill(toks[:PROMPT + 1], want_logits=False)          # (the replays left position 9 unwritten: the prompt again, through it)
    dev.forward(toks[PROMPT + 1], PROMPT + 1)
    out["logits_sha256"] = _sha(dev.state.logits)
    out.update(_kv(dev, shape, PROMPT + 2))
    out["served"] = _served(dev)
    return out


# ---- nl_group_forward (LocalTPGroup) ----------------------------------------------------------------------------------------
def _local_group(ctx, fused, n=2, steps=6):
    g = gguf.load_gguf(ctx.gguf(SE_TP, "q4_0", mode="qrand"))
    grp = ctx.model.LocalTPGroup(g, n, fused=fused)
    ctx.devs.extend(grp.shards)
    out = {"plan_at_start": [_served(s)["plan"] for s in grp.shards], "logits_sha256": []}
    for pos, t in enumerate(_tokens(SE_TP, steps)):
        out["logits_sha256"].append(_sha(grp.forward(t, pos)))
    out["served"] = [_served(s) for s in grp.shards]
    return out


# ---- a group handle (nl_create_group): a child process with a hardware queue per rank -------------------------------------------
def _group_worker(path):
    import numpy as np
    from nanollama_amd import model
    grp = model.load_llama_model(gguf.load_gguf(path), devices=[0, 0])
    toks = _tokens(SE_GRP, PROMPT + 1)
    grp.prefill(toks[:PROMPT])
    out = {"prefill_logits_sha256": _sha(grp.state.logits), "plan": _served(grp)["plan"]}
    out["argmax"] = grp.forward_argmax(toks[PROMPT], PROMPT)
    out["greedy_ids"] = grp.decode_greedy(toks[PROMPT], PROMPT, 24)
    grp.reset()
    grp.prefill(toks[:PROMPT])
    rng = np.random.Generator(np.random.PCG64(41))
    us = rng.random(24, dtype=np.float32)
    ids, rec = grp.sample_decode(PROMPT, 24, uniforms=us, recent=_window(rng, SE_GRP.vocab, SETTINGS[1], True), **SETTINGS[1])
    out.update(sampled_ids=ids, window=rec, n_recent=len(rec), last_error=grp.last_error())
    grp.close()
    print("RECORD " + json.dumps(out))


def _group_handle(ctx):
    path = ctx.gguf(SE_GRP, "q4_0", mode="qrand")
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8", NL_P2P_TIMEOUT_MS="5000")        # as tests/test_gpu_group.py
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--group-worker", path], env=env, capture_output=True, text=True, timeout=300)
    rec = [ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
    if r.returncode != 0 or not rec:
        raise RuntimeError(f"group worker failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    out = json.loads(rec[-1][7:])
    err = out.pop("last_error")
    if err:
        raise Unforced(err) if FUSED_NOTE in err else RuntimeError(err)
    return out


# ---- op-level entry points ------------------------------------------------------------------------------------------------
def _op_data():
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(43))
    logits = (rng.standard_normal((5, 512), dtype=np.float32) * np.float32(3.0))
    return rng, logits


def _ops(ctx):
    import numpy as np
    from nanollama_amd import quant
    m = ctx.model
    rng, logits = _op_data()
    out = {}
    rows, cols = 64, 256
    w = (rng.random((rows, cols), dtype=np.float32) * 2 - 1) * np.float32(0.05)
    x = rng.standard_normal((5, cols), dtype=np.float32)
    for wtype in ("q4_0", "q8_0", "q4_k", "f16"):
        # (Q4_K has no quantiser here: raw random blocks, as the models of synth's qrand mode hold them)
        raw = (synth._draw_qrand(synth.ModelShape("x", 1, cols, 1, 1, 32), 47, "t", (rows, cols), "matrix", synth.WTYPES[wtype])
               if wtype == "q4_k" else quant.encode(w, synth.WTYPES[wtype]))
        out[f"matmul_{wtype}_sha256"] = _sha(m.op_matmul(raw, synth.WTYPES[wtype], x[0], rows, cols))
    out["matmul_batch_q4_0_sha256"] = _sha(m.op_matmul_batch(quant.encode(w, synth.WTYPES["q4_0"]), synth.WTYPES["q4_0"], x, rows, cols))
    out["rmsnorm_sha256"] = _sha(m.op_rmsnorm(x[1], rng.standard_normal(cols, dtype=np.float32), 1e-5))
    out["exp_sha256"] = _sha(m.op_exp(rng.standard_normal(1000, dtype=np.float32) * np.float32(4.0)))
    out["sample"] = []
    for k, s in enumerate(SETTINGS):
        picked, lg, rec = m.op_sample(logits[k], uniform=float(rng.random(dtype=np.float32)), recent=_window(rng, 512, s, True), **s)
        out["sample"].append({"id": picked, "logits_sha256": _sha(lg), "window": rec, "n_recent": len(rec)})
    ids, lg, recs = m.op_sample_rows(logits[:3], SETTINGS, rng.random(3, dtype=np.float32), [_window(rng, 512, s, True) for s in SETTINGS])
    out["sample_rows"] = {"ids": ids, "logits_sha256": _sha(lg), "windows": recs, "n_recent": [len(r) for r in recs]}
    targets = [int(t) for t in rng.integers(0, 512, size=5)]
    targets[2] = -1
    lp, lse, am = m.op_score_rows(logits, targets)
    out["score_rows"] = {"logprob_sha256": _sha(lp), "lse_sha256": _sha(lse), "argmax": [int(v) for v in am]}
    return out


def _op_argument_errors(ctx):
    """one argument error per op-level function: the return code (the checks stand before the first allocation of each function)"""
    import ctypes as C
    import numpy as np
    from nanollama_amd import _lib
    L = _lib.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    f = np.zeros(1024, dtype=np.float32)
    i = np.zeros(64, dtype=np.int32)
    raw = np.zeros(64 * 256 // 32 * 18, dtype=np.uint8)
    F, I = f.ctypes.data_as(fp), i.ctypes.data_as(ip)
    p = _lib.NlSampleParams(0.8, 0.0, 50, 1.15, 8)                 # top_p must be > 0
    ok = _lib.NlSampleParams(0.8, 0.9, 50, 1.15, 8)
    n1 = C.c_int(9)                                                # n_recent above rep_window
    calls = {
        "op_matmul": lambda: L.nl_op_matmul(0, synth.WTYPES["q4_0"], raw.ctypes.data, raw.nbytes, F, F, 64, 250),          # cols % 32
        "op_matmul_batch": lambda: L.nl_op_matmul_batch(0, synth.WTYPES["q4_0"], raw.ctypes.data, raw.nbytes, F, F, 64, 256, 0),
        "op_rmsnorm": lambda: L.nl_op_rmsnorm(0, F, None, C.c_float(1e-5), F, 256),
        "op_exp": lambda: L.nl_op_exp(0, F, F, 0),
        "op_sample": lambda: L.nl_op_sample(0, F, 512, C.byref(p), C.c_float(0.5), I, C.byref(C.c_int(0)), I),
        "op_sample_n_recent": lambda: L.nl_op_sample(0, F, 512, C.byref(ok), C.c_float(0.5), I, C.byref(n1), I),
        "op_sample_rows": lambda: L.nl_op_sample_rows(0, F, 512, 1, C.byref(p), F, I, 8, I, I),
        "op_score_rows": lambda: L.nl_op_score_rows(0, F, 512, 1, I, None, F, I),
    }
    return {name: int(call()) for name, call in calls.items()}


PD0 = {"NL_PERSIST": "0"}
IDLE = {"NL_PERSIST_IDLE_US": "2000000"}          # a resident session outlives the host's pauses between calls: launches are exact
QUIET = {"NL_QUIET": "1"}
FUSED_REDO = {**PD0, **QUIET, "NL_FUSED_SPIN_LIMIT": "0"}
FUSED_MODEL = ((SE_FUSED, "q4_0"),)

# name: (environment of the case, the note its knobs force on a handle (or None), function of a _Ctx -> record)
CASES = {
    "per_call_session": (IDLE, None, _each_model(_per_call)),
    "per_call_persistent_step": ({"NL_PERSIST_SESSION": "0"}, None, _each_model(_per_call)),
    "per_call_call_box": (PD0, None, _each_model(_per_call)),
    "per_call_no_call_box": ({**PD0, "NL_NO_CALL_BOX": "1"}, None, _each_model(_per_call)),
    "per_call_dma_logits": ({**PD0, "NL_NO_CALL_BOX": "1", "NL_NO_HOST_LOGITS": "1"}, None, _each_model(_per_call)),
    "per_call_no_graph": ({**PD0, "NL_NO_GRAPH": "1"}, None, _each_model(_per_call)),
    "per_call_force_tp_plan": ({**PD0, "NL_FORCE_TP_PLAN": "1"}, None, _each_model(_force_tp_plan)),
    "per_call_persist_give_up": ({**QUIET, "NL_PERSIST_SPIN_LIMIT": "0"}, PD_NOTE, _each_model(_per_call)),
    "per_call_persistent_step_give_up": ({**QUIET, "NL_PERSIST_SESSION": "0", "NL_PERSIST_SPIN_LIMIT": "0"}, PD_NOTE, _each_model(_per_call)),
    "per_call_fused_plan": (PD0, None, _each_model(_per_call, FUSED_MODEL)),
    "per_call_fused_redo": (FUSED_REDO, FUSED_NOTE, _each_model(_per_call, FUSED_MODEL)),
    "per_call_fused_redo_no_call_box": ({**FUSED_REDO, "NL_NO_CALL_BOX": "1"}, FUSED_NOTE, _each_model(_per_call, FUSED_MODEL)),
    "session_interrupted": (IDLE, None, _each_model(_session_interrupted)),
    "above_high_water_session": (IDLE, None, _each_model(_above_high_water)),
    "above_high_water_launch_plans": (PD0, None, _each_model(_above_high_water)),
    "greedy_launch_plans": (PD0, None, _each_model(_greedy)),                                  # two 16-step graphs + 8 single steps
    "greedy_persistent": ({}, None, _each_model(_greedy)),                                     # one persistent launch
    "greedy_hand_over": ({"NL_PERSIST_MAX_POS": "20"}, None, _each_model(_greedy)),            # 11 persistent steps, then the plans
    "greedy_no_graph": ({"NL_NO_GRAPH": "1"}, None, _each_model(_greedy)),
    "greedy_no_graph_launch_plans": ({**PD0, "NL_NO_GRAPH": "1"}, None, _each_model(_greedy)),
    "greedy_clipped_at_seq_len": ({}, None, _each_model(lambda c, s, w: _greedy(c, s, w, prompt=s.seq_len - 12))),
    "greedy_clipped_at_seq_len_launch_plans": (PD0, None, _each_model(lambda c, s, w: _greedy(c, s, w, prompt=s.seq_len - 12))),
    "greedy_persist_give_up": ({**QUIET, "NL_PERSIST_SPIN_LIMIT": "0"}, PD_NOTE, _each_model(_greedy)),
    "greedy_fused_plan": (PD0, None, _each_model(_greedy, FUSED_MODEL)),
    "greedy_fused_redo": (FUSED_REDO, FUSED_NOTE, _each_model(_greedy, FUSED_MODEL)),
    "sample_decode": ({}, None, _each_model(_sample)),
    "sample_decode_recapture": ({}, None, _each_model(lambda c, s, w: _sample(c, s, w, order=(1, 2, 0, 1), one_handle=True))),
    "sample_decode_no_graph": ({"NL_NO_GRAPH": "1"}, None, _each_model(_sample)),
    "sample_decode_no_sample_embed": ({"NL_NO_SAMPLE_EMBED": "1"}, None, _each_model(_sample)),
    "sample_decode_fused_plan": (PD0, None, _each_model(_sample, FUSED_MODEL)),
    "sample_decode_fused_redo": (FUSED_REDO, FUSED_NOTE, _each_model(_sample, FUSED_MODEL)),   # the samp_keep restore
    "profile_forward": ({}, None, _each_model(_profile)),
    "profile_forward_fused_plan": (PD0, None, _each_model(_profile, FUSED_MODEL)),
    "profile_forward_fused_redo": (FUSED_REDO, FUSED_NOTE, _each_model(_profile, FUSED_MODEL)),
    "local_group_2": ({}, None, lambda c: _local_group(c, False)),
    "local_group_2_fused": ({}, None, lambda c: _local_group(c, True)),
    "local_group_2_fused_redo": ({**QUIET, "NL_FUSED_SPIN_LIMIT": "0"}, FUSED_NOTE, lambda c: _local_group(c, True)),
    "group_handle_2": ({}, None, _group_handle),
    "ops": ({}, None, _ops),
    "op_argument_errors": ({}, None, _op_argument_errors),
}


def run_case(model, name, workdir):
    """-> the record of CASES[name]; Unforced when a handle of the case gave up a rung that the case's knobs did not force"""
    env, note, fn = CASES[name]
    with _env(env):
        ctx = _Ctx(model, workdir, note)
        try:
            out = fn(ctx)
        except Exception:
            ctx.close()
            raise
        ctx.finish()
    return out


def main():
    if sys.argv[1] == "--group-worker":
        return _group_worker(sys.argv[2])
    from nanollama_amd import _lib, model
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in CASES:
            t0 = time.perf_counter()
            try:
                out[name] = run_case(model, name, tmp)
            except Unforced as exc:
                print(f"[retry] {name}: {exc}")
                out[name] = run_case(model, name, tmp)
            print(f"{name} ({time.perf_counter() - t0:.1f} s)", json.dumps(out[name])[:120], flush=True)
    out["_build"] = _lib.build_info()
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
