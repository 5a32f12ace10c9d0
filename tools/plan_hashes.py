"""Bit-level record of the per-token launch plans (build_plan / build_plan_blocks and the op makers of
nanollama_amd/csrc/nl_engine.hip): one case per plan variant -- the five-launch plan (eager, under the forced tensor-parallel
seams), fused modes 1, 2, 4 (matrix and vector pipe, every NL_PREFETCH branch, with and without helper blocks) on one handle, mode 3
on the shards of an in-process group, the push seams between two rank processes and in loopback, and the designed give-ups.  Each
case steps a two-layer synthetic model token by token through forward (a 9-token prompt teacher-forced, then 12 further steps), then
one decode_greedy chain of 24 (the multi-step graph with the fused argmax + embed), and records per step the sha256 of the logits and
the argmax id, the chain's ids, plan_info(), persist_info() and -- where nl_profile_forward applies (one handle: not the shards of a
group, not the ranks of a push group) -- the launches per kind of a position served by each plan of the handle.  Every case runs
with NL_PERSIST=0, so the launch plans serve every step, and asserts that the variant it names did serve (fused mode, kinds, no note
on the handle but the one its knobs force).  Run at a commit whose results are to be kept, the output is the fixture the next commit
is held to (tests/golden/plan_parent_hashes.json; tests/test_gpu_plan_bits.py imports CASES and run_case from here).
usage: python tools/plan_hashes.py OUT.json        (python tools/plan_hashes.py --rank-worker GGUF MODE: a rank of the push cases)"""
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time
from dataclasses import replace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from nanollama_amd import gguf, synth
import attn_cases

seh = sys.modules.get("single_entry_hashes")       # (one copy per process: whoever catches seh.Unforced must see this module's class)
if seh is None:
    _spec = importlib.util.spec_from_file_location("single_entry_hashes", os.path.join(ROOT, "tools", "single_entry_hashes.py"))
    seh = sys.modules["single_entry_hashes"] = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(seh)
_env, _sha, _served, _tokens, Unforced, FUSED_NOTE = seh._env, seh._sha, seh._served, seh._tokens, seh.Unforced, seh.FUSED_NOTE

SHAPES = attn_cases.SHAPES
QKNORM = replace(SHAPES["gqa"], name="pl_qknorm", qk_norm=True)
HELPERS = synth.ModelShape("big_geo_h", 2, 4096, 64, 16, 1024, seq_len=2048, interm=2048)    # tests/test_gpu_tp_fused.py
PL_TP = synth.ModelShape("pl_tp", 2, 1024, 16, 4, 4096, seq_len=64, interm=2048)             # a shard takes tp_ffn_kernel
PL_TP_WIDE = synth.ModelShape("pl_tp_wide", 2, 1024, 16, 4, 4096, seq_len=64, interm=8192)   # ... wide_ffn_kernel (NL_WIDE_FFN=2)
PROMPT, STEPS, CHAIN = 9, 12, 24
LONE_RUNNER_CAP = 1024      # TP_NCH_MAX x TP_PASS of nl_tp.h: positions a head's runner covers without helper blocks
GENERAL_MODELS = (("gqa", "q8_0"), ("gqa", "q4_0"), ("gqa", "f16"), ("gqa_bias", "q8_0"), ("gqa_conj", "q8_0"), ("hd32_g3", "q8_0"),
                  (QKNORM, "q8_0"))


def _shape(key):
    return SHAPES[key] if isinstance(key, str) else key


def _plan_index(pl, pos, helpers):
    """nl_engine.hip plan_index: 0 general, 1 fused, 2 fused with helper blocks (from the second 256-position pass on)"""
    if not (pl["fused_mode"] and pos < pl["fused_max_pos"]):
        return 0
    return 2 if helpers and pos >= 256 else 1


def _steps(step, toks, pos0):
    """toks teacher-forced from pos0 on: per step the sha256 of the logits and the argmax id"""
    import numpy as np
    out = {"logits_sha256": [], "argmax": []}
    for k, t in enumerate(toks):
        lg = step(t, pos0 + k)
        out["logits_sha256"].append(_sha(lg))
        out["argmax"].append(int(np.argmax(lg)))
    return out


def _single(ctx, shape, wtype, mode, kinds=None, mode_after=None, prefill=0, n_steps=PROMPT + STEPS, helpers=None, loader=None, gen=None):
    """the record of one handle.  mode: the fused mode the handle must report after loading (mode_after: and at the end, where the
    case retires the plan); kinds: launches per kind of a step on the handle's first plan; helpers: True / False for the case
    that is about the helper blocks (the handle's position limit above / at the lone runner's cap)"""
    shape = _shape(shape)
    toks = _tokens(shape, prefill + n_steps)
    dev = loader(ctx, shape, wtype) if loader else ctx.load(shape, wtype, **(gen or {}))
    start = dev.plan_info()
    assert start["fused_mode"] == mode, (shape.name, wtype, start)
    if helpers is not None:
        assert (start["fused_max_pos"] > LONE_RUNNER_CAP) == helpers, start
    out = {"plan_at_start": _served(dev)["plan"]}
    if prefill:
        dev.prefill(toks[:prefill], want_logits=False)

    def step(t, pos):
        dev.forward(t, pos)
        return dev.state.logits
    out.update(_steps(step, toks[prefill:], prefill))
    pos = prefill + n_steps
    out["ids"] = dev.decode_greedy(out["argmax"][-1], pos, CHAIN)
    end = pos + len(out["ids"])
    out["served"] = _served(dev)
    now = dev.plan_info()
    assert now["fused_mode"] == (mode if mode_after is None else mode_after), (shape.name, wtype, now, dev.last_error())
    # launches per kind at one position of every plan that serves a position of this handle (the replays leave the stream unwritten
    # from that position on: last)
    at = {}
    for p in (end, 100, 300, now["fused_max_pos"]):
        if 0 <= p < shape.seq_len:
            at.setdefault(_plan_index(now, p, bool(helpers)), p)
    out["kinds"] = {}
    for k, p in sorted(at.items()):
        prof = dev.profile_forward(out["ids"][-1], p, iters=2)
        out["kinds"][f"plan{k}"] = [[kind, calls] for kind, (_, calls) in prof.items() if calls]
    if kinds is not None:
        got = dict(out["kinds"][f"plan{_plan_index(now, end, bool(helpers))}"])      # the plan that served the chain's last step
        assert all(got.get(k, 0) == v for k, v in kinds.items()), (shape.name, wtype, kinds, got)
    return out


def _each(models, mode, kinds=None, **kw):
    def run(ctx):
        out = {}
        for shape, wtype in models:
            k = dict(kinds) if kinds else None
            if k and _shape(shape).qk_norm and "qkv_rope" in k:
                k["qkv_rope"] *= 2                                    # (the qk-norm launch counts as a projection launch)
            out[f"{_shape(shape).name}_{wtype}"] = _single(ctx, shape, wtype, mode, k, **kw)
        return out
    return run


def _with_comm(ctx, shape, wtype):
    """NL_FORCE_TP_PLAN=1: the all-reduce / all-gather seams with one rank (a communicator of one), as seh._force_tp_plan"""
    dev = ctx.model.load_llama_model(gguf.load_gguf(ctx.gguf(shape, wtype)), comm_id=ctx.model.comm_unique_id())
    ctx.devs.append(dev)
    return dev


def _loopback(ctx, shape, wtype):
    """rank 0 of 2 alone, every peer slot its own (nl_p2p_loopback), as bench.py --shard-of sets it up"""
    dev = ctx.model.load_llama_model(gguf.load_gguf(ctx.gguf(shape, wtype, mode="qrand")), tp_rank=0, tp_size=2, p2p_loopback=True)
    ctx.devs.append(dev)
    return dev


# ---- mode 3 on the shards of an in-process group (nl_group_forward: no chained decode -- the chain is 24 per-call steps) ----------
def _group(shape, wtype, fused, mode, n=2):
    def run(ctx):
        import numpy as np
        grp = ctx.model.LocalTPGroup(gguf.load_gguf(ctx.gguf(shape, wtype, mode="qrand")), n, fused=fused)
        ctx.devs.extend(grp.shards)
        out = {"plan_at_start": [_served(s)["plan"] for s in grp.shards]}
        assert all(s.plan_info()["fused_mode"] == mode for s in grp.shards), out
        out.update(_steps(lambda t, pos: grp.forward(t, pos), _tokens(shape, PROMPT + STEPS), 0))
        tok, out["ids"] = out["argmax"][-1], []
        for pos in range(PROMPT + STEPS, PROMPT + STEPS + CHAIN):
            tok = int(np.argmax(grp.forward(tok, pos)))
            out["ids"].append(tok)
        out["final_logits_sha256"] = _sha(grp.logits)
        out["served"] = [_served(s) for s in grp.shards]
        assert all(s.plan_info()["fused_mode"] == mode for s in grp.shards), out["served"]
        return out
    return run


# ---- push seams: two rank processes over the push all-reduce, as tests/test_gpu_p2p.py::run_ranks starts them ----------------------
def _rank_worker(path, mode):
    from nanollama_amd import model
    from nanollama_amd.dist import Rendezvous
    rdv = Rendezvous(timeout_s=60.0)
    dev = model.load_llama_model(gguf.load_gguf(path), device=rdv.local_rank, tp_rank=rdv.rank, tp_size=rdv.world, p2p_allgather=rdv.allgather_bytes)
    out = {"plan_at_start": _served(dev)["plan"]}
    assert dev.plan_info()["fused_mode"] == int(mode), dev.plan_info()
    rdv.barrier()

    def step(t, pos):
        dev.forward(t, pos)
        return dev.state.logits
    out.update(_steps(step, _tokens(PL_TP, PROMPT + STEPS), 0))
    out["ids"] = dev.decode_greedy(out["argmax"][-1], PROMPT + STEPS, CHAIN)
    rdv.barrier()
    out["served"] = _served(dev)
    out["last_error"] = dev.last_error()
    dev.close()
    rdv.close()
    print("RECORD " + json.dumps(out), flush=True)


def _ranks(mode, n=2):
    def run(ctx):
        path = ctx.gguf(PL_TP, "q4_0", mode="qrand")
        port = 29000 + (os.getpid() * 11 + n * 37) % 2000
        procs = []
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                       NL_P2P_TIMEOUT_MS="5000", GPU_MAX_HW_QUEUES="8", NL_BENCH_ONE_DEVICE="1")
            procs.append(subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "--rank-worker", path, str(mode)],
                                          env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
        done = [p.communicate() + (p.returncode,) for p in procs]       # (each child ends by itself or at its own time limit)
        out = {}
        for r, (so, se, rc) in enumerate(done):
            rec = [ln for ln in so.splitlines() if ln.startswith("RECORD ")]
            if rc != 0 or not rec:
                raise RuntimeError(f"rank {r} failed ({rc}):\n{so[-2000:]}\n{se[-4000:]}")
            out[f"rank{r}"] = json.loads(rec[-1][7:])
            err = out[f"rank{r}"].pop("last_error")
            if err:
                raise Unforced(err) if FUSED_NOTE in err else RuntimeError(err)
        assert all(out[f"rank{r}"]["logits_sha256"] == out["rank0"]["logits_sha256"] and out[f"rank{r}"]["ids"] == out["rank0"]["ids"]
                   for r in range(n)), "the ranks disagree on the gathered logits / greedy ids"
        return out
    return run


PD0 = {"NL_PERSIST": "0"}
GENERAL = {**PD0, "NL_FUSED_ATTN": "0"}
M4 = {**PD0, "NL_WIDE_FFN": "2"}               # (`wide`'s 64-workgroup feed-forward grid does not fill the chip: 2 takes it anyway)
GIVE_UP = {**PD0, "NL_QUIET": "1", "NL_FUSED_SPIN_LIMIT": "0"}
K_GENERAL = {"qkv_rope": 2, "attention": 2, "wo_resid": 2, "gate_up_swiglu": 2, "down_resid": 2, "attn_block": 0, "ffn_block": 0}
K_M1_FFN = {"attn_block": 2, "ffn_block": 1, "gate_up_swiglu": 1, "down_resid": 1, "qkv_rope": 0, "wo_resid": 0}
K_M1 = {"attn_block": 2, "ffn_block": 0, "gate_up_swiglu": 2, "down_resid": 2, "qkv_rope": 0, "wo_resid": 0}
K_M2 = {"attn_block": 2, "wo_resid": 2, "gate_up_swiglu": 2, "down_resid": 2, "qkv_rope": 0, "attention": 0, "ffn_block": 0}
K_M4_WIDE = {"attn_block": 2, "ffn_block": 2, "wo_resid": 0, "gate_up_swiglu": 0, "down_resid": 0}
K_M4 = {"attn_block": 2, "ffn_block": 0, "wo_resid": 0, "gate_up_swiglu": 2, "down_resid": 2}
M1_MODELS = (("gqa", "q8_0"), ("gqa", "q4_0"))
WIDE_Q4 = (("wide", "q4_0"),)
HELPER_MODEL = ((HELPERS, "q4_0"),)
HELPER_RUN = dict(prefill=250, n_steps=13, gen={"mode": "qrand"})      # positions 250 .. 262: both sides of the second pass's first position


def _m4(env, kinds=K_M4_WIDE, models=WIDE_Q4, **kw):
    return ({**M4, **env}, None, _each(models, 4, kinds, **kw))


# name: (environment of the case, the note its knobs force on a handle (or None), function of a seh._Ctx -> record)
CASES = {
    "general": (GENERAL, None, _each(GENERAL_MODELS, 0, K_GENERAL)),
    "general_no_graph": ({**GENERAL, "NL_NO_GRAPH": "1"}, None, _each(GENERAL_MODELS, 0, K_GENERAL)),
    "general_force_tp_plan": ({**GENERAL, "NL_FORCE_TP_PLAN": "1"}, None, _each(GENERAL_MODELS, 0, K_GENERAL, loader=_with_comm)),
    "mode1_ffn_block": ({**PD0, "NL_FUSED_FFN": "1"}, None, _each(M1_MODELS, 1, K_M1_FFN)),
    "mode1_gemv_ffn": ({**PD0, "NL_FUSED_FFN": "0"}, None, _each(M1_MODELS, 1, K_M1)),
    "mode2": ({**PD0, "NL_ATTN_WO": "0"}, None, _each(WIDE_Q4, 2, K_M2)),
    "mode4_matrix_pipe": _m4({}),
    "mode4_vector_pipe": _m4({"NL_MFMA_DOT": "0"}),
    "mode4_gemv_ffn": ({**PD0, "NL_WIDE_FFN": "0"}, None, _each(WIDE_Q4, 4, K_M4)),
    "mode4_prefetch_0": _m4({"NL_PREFETCH": "0"}),
    "mode4_prefetch_1": _m4({"NL_PREFETCH": "1"}),
    "mode4_prefetch_1_2": _m4({"NL_PREFETCH": "3"}),
    "mode4_prefetch_1_4": _m4({"NL_PREFETCH": "5"}),
    "mode4_prefetch_1_8": _m4({"NL_PREFETCH": "9"}),
    "mode4_prefetch_1_16": _m4({"NL_PREFETCH": "17"}),
    "mode4_q8_0": _m4({}, models=(("wide", "q8_0"),)),
    "mode4_helpers": (PD0, None, _each(HELPER_MODEL, 4, K_M4_WIDE, helpers=True, **HELPER_RUN)),
    "mode4_no_helpers": ({**PD0, "NL_ATTN_HELPERS": "0"}, None, _each(HELPER_MODEL, 4, K_M4_WIDE, helpers=False, **HELPER_RUN)),
    "mode3_group_q4_0": (PD0, None, _group(PL_TP, "q4_0", True, 3)),
    "mode3_group_q8_0": (PD0, None, _group(PL_TP, "q8_0", True, 3)),
    "mode3_group_wide_ffn": ({**PD0, "NL_WIDE_FFN": "2"}, None, _group(PL_TP_WIDE, "q4_0", True, 3)),
    "plain_group": (PD0, None, _group(PL_TP, "q4_0", False, 0)),
    "push_ranks_five_launch": ({**PD0, "NL_FUSED_ATTN": "0"}, None, _ranks(0)),
    "push_ranks_two_launch": ({**PD0, "NL_QUIET": "1"}, None, _ranks(3)),
    "push_loopback": (PD0, None, _each(((PL_TP, "q4_0"),), 3, {"attn_block": 2, "ffn_block": 2}, loader=_loopback)),
    "give_up_mode1": (GIVE_UP, FUSED_NOTE, _each(M1_MODELS, 1, K_GENERAL, mode_after=0)),
    "give_up_mode4": ({**GIVE_UP, "NL_WIDE_FFN": "2"}, FUSED_NOTE, _each(WIDE_Q4, 4, K_GENERAL, mode_after=0)),
}


def run_case(model, name, workdir):
    """-> the record of CASES[name]; Unforced when a handle of the case gave up a rung that the case's knobs did not force"""
    env, note, fn = CASES[name]
    with _env(env):
        ctx = seh._Ctx(model, workdir, note)
        try:
            out = fn(ctx)
        except Exception:
            ctx.close()
            raise
        ctx.finish()
    return out


def _dumps(rec, depth=0):
    """JSON with one line per list (a record is dicts of dicts; its leaves are lists, strings and numbers)"""
    if not isinstance(rec, dict):
        return json.dumps(rec)
    pad = " " * (depth + 1)
    return "{\n" + ",\n".join(f"{pad}{json.dumps(k)}: {_dumps(v, depth + 1)}" for k, v in rec.items()) + "\n" + " " * depth + "}"


def main():
    if sys.argv[1] == "--rank-worker":
        return _rank_worker(sys.argv[2], sys.argv[3])
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
    info = _lib.build_info()
    out["_build"] = {k: info[k] for k in ("lib_src_sha16", "lib_git_head_at_build")}
    with open(sys.argv[1], "w") as fh:
        fh.write(_dumps(out) + "\n")


if __name__ == "__main__":
    main()
