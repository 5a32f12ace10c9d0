"""Attention inputs in which one key dominates the softmax, and a float64 forward to hold every attention path to.

Random synth models keep attention scores within about +-5.5 with the largest some 3 nats above the median: no accumulator
is ever rescaled by alpha -> 0, no split's merge weight underflows, the newest key never wins by a margin.  The cases here
override `blk.*.attn_q.weight` (and, for `shift`, `blk.*.attn_k.bias`) of a two-layer synth model so that they do:

  sharp      attn_q = SIGMA x the drawn attn_q: scores +-45, the maximum ~25 nats above the median, at a random position
  self       the rows of query head h = +SIGMA x the rows of attn_k of kv head h // group: the newest key always wins, by 50 to
             110 nats; every earlier split's weight is ~e^-60, every step rescales.  Well-conditioned.
  anti       the same with -SIGMA: the newest key is always the lowest score, the maximum is elsewhere
  shift_pos  sharp on an attn_bias shape whose attn_k.bias is +16 on the lowest-frequency rotary dimension of every kv head
  shift_neg  (index hd/2 - 1) and 0 elsewhere: a near-constant offset of tens of nats on every score of a row; -16 likewise

The reference is forward_f64: the architecture as oracle/nl_oracle.c states it (go/model.go:490-620) in plain numpy float64 --
embedding, RMSNorm, Q/K/V + optional biases, RoPE (standard and conjugate, pairing (i, i + hd/2)), GQA attention with an exact
softmax, WO + residual, SwiGLU, final norm, LM head -- over the DEQUANTISED tensors of the encoded file (oracle.dequant), so
quantisation is part of the model and not of the error.  The two float32 constants the engine and the oracle share are part of
the model in the same way: the cos/sin tables ((float)cos(angle), go/model.go:346-358) and the score scale (float)(1/sqrt(hd)).

tests/test_attn_cases_cpu.py pins the generator (the oracle stays within REF_CAP of forward_f64 on every case, and the cases
do contain the rows they exist for); tests/test_gpu_attention_sharp.py holds every attention kernel to forward_f64, and
tests/test_gpu_attention_geometry.py every (head_dim, GQA group) instantiation of them (GEO below).  What the two GPU files share
-- the bound, the witnesses, the batch layouts, the mixed steps -- stands at the end of this module.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import numpy as np

from nanollama_amd import gguf, synth

SIGMA = 8.0
SPLIT = 128            # keys per attention split / pass of every decode kernel
REF_CAP = 5e-5         # max|oracle - f64| / max(1, std): half the project's logits tolerance -- a condition on the inputs
GPU_TOL = 1e-4         # DESIGN section 5's standing bound, here against float64

N_TOKENS = 300         # three 128-key splits, and past the 256-token threshold of the K/V fp16 images
N_TOKENS_WIDE = 160

_A = synth.ModelShape("sh_gqa", 2, 256, 4, 2, 512, seq_len=320, interm=512)
SHAPES: Dict[str, synth.ModelShape] = {
    "gqa": _A,                                                       # the fb_gqa geometry, two layers
    "gqa_bias": replace(_A, name="sh_gqa_bias", attn_bias=True),
    "gqa_conj": replace(_A, name="sh_gqa_conj", rope_conjugate=True),
    "mha4": synth.ModelShape("sh_mha4", 2, 256, 4, 4, 512, seq_len=320, interm=512),      # the persistent decode's D 256, 4/4
    "mha3": synth.ModelShape("sh_mha3", 2, 192, 3, 3, 1024, seq_len=320),                # the fb_mha geometry, two layers
    "hd32_g3": synth.ModelShape("sh_hd32", 2, 192, 6, 2, 512, seq_len=320, interm=384),  # head_dim 32, three query heads per kv head
    "wide": synth.ModelShape("sh_wide", 2, 1024, 16, 4, 512, seq_len=192, interm=1024),  # the projection + attention launch's tier
}

# One shape per attention geometry nl_create admits -- head_dim 32 / 64 x 1, 2, 3, 4, 6, 8 query heads per kv head; every attention
# kernel is a template over that pair.  The smallest models that still have two kv heads (a wrong kv-head index shows):
# D = hd * 2G, H = 2G.  (64, 2) is "gqa" and (32, 3) is "hd32_g3" above; the other ten are geo_{hd}_{g}.
GEOMETRIES: List[Tuple[int, int]] = [(hd, g) for hd in (32, 64) for g in (1, 2, 3, 4, 6, 8)]
GEO: Dict[Tuple[int, int], str] = {}
for _hd, _g in GEOMETRIES:
    _have = [k for k, s in SHAPES.items() if (s.dim, s.n_head, s.n_kv_head, s.seq_len) == (_hd * 2 * _g, 2 * _g, 2, 320)
             and not s.attn_bias and not s.rope_conjugate]
    GEO[_hd, _g] = _have[0] if _have else f"geo_{_hd}_{_g}"
    if not _have:
        SHAPES[GEO[_hd, _g]] = synth.ModelShape(f"geo_{_hd}_{_g}", 2, _hd * 2 * _g, 2 * _g, 2, 512, seq_len=320, interm=256)
# q4_0 where D is a whole number of 256-column groups: those steps go through dgemm_kernel's RoPE epilogue
GEO_Q4 = [(hd, g) for hd, g in GEOMETRIES if (hd * 2 * g) % 256 == 0]

# (shape, weight type, case): exactly the models the GPU files use; test_attn_cases_cpu.py runs every one of them
CASES: List[Tuple[str, str, str]] = (
    [("gqa", "q8_0", c) for c in ("sharp", "self", "anti")] + [("gqa", "q4_0", "sharp")]
    + [("gqa", "f16", c) for c in ("sharp", "self", "anti")]
    + [("gqa_bias", "q8_0", c) for c in ("shift_pos", "shift_neg")]
    + [("gqa_conj", "q4_0", "sharp"), ("gqa_conj", "q8_0", "sharp")]
    + [("mha4", "q8_0", c) for c in ("sharp", "self", "anti")]
    + [("mha3", "q8_0", c) for c in ("sharp", "self", "anti")]
    + [("hd32_g3", "q8_0", "sharp")]
    + [("wide", "q4_0", c) for c in ("sharp", "self", "anti")])
# the geometry grid (tests/test_gpu_attention_geometry.py): sharp and anti -- the case in which a split's merge weight underflows --
# at q8_0 for all twelve, sharp at q4_0 for GEO_Q4.  (The (64, 2) and (32, 3) ones partly stand above already.)
for _c in ([(GEO[k], "q8_0", c) for k in GEOMETRIES for c in ("sharp", "anti")] + [(GEO[k], "q4_0", "sharp") for k in GEO_Q4]):
    if _c not in CASES:
        CASES.append(_c)

SEED = 8101

# sigma per case: SIGMA unless the CPU oracle breaks REF_CAP there (measured by test_attn_cases_cpu.py; DESIGN section 5 lists them)
SIGMA_OF: Dict[Tuple[str, str, str], float] = {
    ("gqa_bias", "q8_0", "shift_pos"): 4.0,        # sigma 8: max|oracle - f64| = 5.7e-5 at step 296
}

# the chained greedy run of the persistent decode: a teacher-forced prompt, then steps whose tokens the decoder picks -- positions
# PERSIST_PROMPT .. PERSIST_PROMPT + PERSIST_STEPS - 1 cross 128
PERSIST_PROMPT, PERSIST_STEPS = 100, 60


def sigma_of(key: Tuple[str, str, str]) -> float:
    return SIGMA_OF.get(tuple(key), SIGMA)


def n_tokens(shape_key: str) -> int:
    return N_TOKENS_WIDE if shape_key == "wide" else N_TOKENS


def tokens(shape_key: str) -> List[int]:
    """the fixed token sequence every teacher-forced test of a shape feeds"""
    return synth.prompt_ids(n_tokens(shape_key), SHAPES[shape_key].vocab, seed=29)


def case_overrides(shape: synth.ModelShape, floats: Dict[str, np.ndarray], case: str, sigma: float = SIGMA) -> Dict[str, np.ndarray]:
    """the tensors a case replaces, from the float weights drawn once for the shape"""
    hd, group = shape.head_dim, shape.n_head // shape.n_kv_head
    out: Dict[str, np.ndarray] = {}
    s = np.float32(sigma)
    for l in range(shape.n_layer):
        wq, wk = floats[f"blk.{l}.attn_q.weight"], floats[f"blk.{l}.attn_k.weight"]
        if case in ("sharp", "shift_pos", "shift_neg"):
            out[f"blk.{l}.attn_q.weight"] = (wq * s).astype(np.float32)
        elif case in ("self", "anti"):
            sign = s if case == "self" else -s
            rows = [wk[(h // group) * hd:(h // group + 1) * hd] * sign for h in range(shape.n_head)]
            out[f"blk.{l}.attn_q.weight"] = np.concatenate(rows, axis=0).astype(np.float32)
        else:
            raise ValueError(f"unknown case {case}")
        if case in ("shift_pos", "shift_neg"):
            if not shape.attn_bias:
                raise ValueError("shift needs an attn_bias shape")
            b = np.zeros(shape.kv_dim, dtype=np.float32)
            b[np.arange(shape.n_kv_head) * hd + hd // 2 - 1] = 16.0 if case == "shift_pos" else -16.0
            out[f"blk.{l}.attn_k.bias"] = b
    return out


def build_case(path: str, shape_key: str, wtype: str, case: str, sigma: Optional[float] = None) -> gguf.GGUFFile:
    """write the case's GGUF to `path` and load it"""
    shape = SHAPES[shape_key]
    if sigma is None:
        sigma = sigma_of((shape_key, wtype, case))
    scratch = path + ".f32"
    floats = synth.generate_gguf(scratch, shape, "f32", SEED, keep_float=True)      # the drawn weights, once
    os.remove(scratch)
    synth.generate_gguf(path, shape, wtype, SEED, overrides=case_overrides(shape, floats, case, sigma))
    return gguf.load_gguf(path)


# ---------------------------------------------------------------------------------------------- float64 forward ---

def _dequant(g: gguf.GGUFFile, name: str) -> Optional[np.ndarray]:
    from oracle import oracle
    if name not in g.tensor_order:
        return None
    data, info = g.get_tensor(name)
    w = oracle.dequant(data, info.type, info.nel).astype(np.float64)
    return w.reshape(info.dims[1], info.dims[0]) if info.ndims == 2 else w


@dataclass
class F64Run:
    logits: np.ndarray      # [T, vocab]
    k: np.ndarray           # [layer, kv head, T, hd]: the rotated K rows, the device cache's layout
    v: np.ndarray           # [layer, kv head, T, hd]
    argmax: np.ndarray      # [T, layer, head]: index of the score row's maximum
    max_score: np.ndarray   # [T, layer, head]
    top2_gap: np.ndarray    # [T, layer, head]: best minus second best score (inf at position 0)
    over_median: np.ndarray # [T, layer, head]: best minus the median score of the row
    split_gap: np.ndarray   # [T, layer, head, splits]: m_c - M per SPLIT-key split, nan where the split holds no key yet
    norm_ms: Optional[np.ndarray] = None   # [T, 2 layers + 1]: mean(x^2) of every RMSNorm's input (attention, feed-forward, ..., final)
    gate: Optional[np.ndarray] = None      # [T, layer, I]: the SiLU's pre-activations
    chan_ms: Optional[np.ndarray] = None   # [2 layers + 1, D]: mean over the steps of x^2 per channel of every RMSNorm's input


class F64Model:
    """forward_f64's weights, read once from a loaded GGUF"""

    def __init__(self, g: gguf.GGUFFile):
        m = g.meta
        self.L, self.D, self.H, self.KV = m.num_layers, m.embed_dim, m.num_heads, m.num_kv_heads
        self.hd = m.head_dim or self.D // self.H
        self.seq_len = min(m.seq_len, 2048)
        self.eps = float(np.float32(m.rms_norm_eps))
        self.conj = bool(m.rope_conjugate)
        if m.qk_norm:
            raise ValueError("qk_norm shapes are out of scope: the norm removes the scale the cases put on attn_q")
        self.embd = _dequant(g, "token_embd.weight")
        out = _dequant(g, "output.weight")
        self.out = self.embd if out is None else out
        self.out_norm = _dequant(g, "output_norm.weight")
        self.layers = []
        for l in range(self.L):
            t = lambda s: _dequant(g, f"blk.{l}.{s}")
            self.layers.append({k: t(n) for k, n in (
                ("attn_norm", "attn_norm.weight"), ("ffn_norm", "ffn_norm.weight"), ("wq", "attn_q.weight"), ("wk", "attn_k.weight"),
                ("wv", "attn_v.weight"), ("wo", "attn_output.weight"), ("gate", "ffn_gate.weight"), ("up", "ffn_up.weight"),
                ("down", "ffn_down.weight"), ("bq", "attn_q.bias"), ("bk", "attn_k.bias"), ("bv", "attn_v.bias"),
                ("bo", "attn_output.bias"))})
        half = self.hd // 2
        theta = float(np.float32(m.rope_theta))
        freq = 1.0 / np.power(theta, (2.0 * np.arange(half)) / float(self.hd))
        angle = np.arange(self.seq_len, dtype=np.float64)[:, None] * freq[None, :]
        self.cos = np.cos(angle).astype(np.float32).astype(np.float64)        # float32 tables, as the engine and the oracle hold them
        self.sin = np.sin(angle).astype(np.float32).astype(np.float64)
        self.scale = float(np.float32(1.0 / np.sqrt(float(self.hd))))

    def _rms(self, x, w):
        return x * (1.0 / np.sqrt((x * x).mean(axis=-1, keepdims=True) + self.eps)) * w

    def _rope(self, x, pos):
        """x [T, heads, hd]; applyRoPE go/model.go:449-461 / applyRoPEConjugate :465-477"""
        half = self.hd // 2
        c, s = self.cos[pos][:, None, :], self.sin[pos][:, None, :]
        if self.conj:
            s = -s
        x0, x1 = x[..., :half], x[..., half:]
        return np.concatenate([x0 * c - x1 * s, x0 * s + x1 * c], axis=-1)

    def forward(self, toks) -> F64Run:
        """teacher-forced over `toks` from position 0: every step at once (causal mask)"""
        toks = np.asarray(toks, dtype=np.int64)
        T, H, KV, hd, L = len(toks), self.H, self.KV, self.hd, self.L
        group = H // KV
        pos = np.arange(T)
        nsplit = (T + SPLIT - 1) // SPLIT
        x = self.embd[toks].copy()
        ks, vs = np.zeros((L, KV, T, hd)), np.zeros((L, KV, T, hd))
        amax, mx = np.zeros((T, L, H), dtype=np.int64), np.zeros((T, L, H))
        top2, sgap = np.full((T, L, H), np.inf), np.full((T, L, H, nsplit), np.nan)
        overmed = np.zeros((T, L, H))
        causal = pos[None, :] <= pos[:, None]
        norm_ms, chan_ms, gates = [], [], []

        def norm_in(x):                   # the input of an RMSNorm
            norm_ms.append((x * x).mean(axis=-1))
            chan_ms.append((x * x).mean(axis=0))

        for l, W in enumerate(self.layers):
            norm_in(x)
            xb = self._rms(x, W["attn_norm"])
            q, k, v = xb @ W["wq"].T, xb @ W["wk"].T, xb @ W["wv"].T
            if W["bq"] is not None: q = q + W["bq"]
            if W["bk"] is not None: k = k + W["bk"]
            if W["bv"] is not None: v = v + W["bv"]
            q = self._rope(q.reshape(T, H, hd), pos)
            k = self._rope(k.reshape(T, KV, hd), pos)
            v = v.reshape(T, KV, hd)
            ks[l], vs[l] = k.transpose(1, 0, 2), v.transpose(1, 0, 2)
            att = np.zeros((T, H, hd))
            for h in range(H):
                kh, vh = k[:, h // group], v[:, h // group]
                sc = np.where(causal, (q[:, h] @ kh.T) * self.scale, -np.inf)
                m = sc.max(axis=1)
                amax[:, l, h], mx[:, l, h] = sc.argmax(axis=1), m
                overmed[:, l, h] = m - np.nanmedian(np.where(causal, sc, np.nan), axis=1)
                if T > 1:
                    top2[1:, l, h] = m[1:] - np.partition(sc[1:], -2, axis=1)[:, -2]
                for c in range(nsplit):
                    seen = pos >= c * SPLIT
                    sgap[seen, l, h, c] = sc[seen, c * SPLIT:(c + 1) * SPLIT].max(axis=1) - m[seen]
                p = np.exp(sc - m[:, None])
                att[:, h] = (p / p.sum(axis=1, keepdims=True)) @ vh
            o = att.reshape(T, H * hd) @ W["wo"].T
            if W["bo"] is not None: o = o + W["bo"]
            x = x + o
            norm_in(x)
            xb = self._rms(x, W["ffn_norm"])
            g_, u = xb @ W["gate"].T, xb @ W["up"].T
            gates.append(g_)
            with np.errstate(over="ignore"):       # exp(-g) = inf for g < -709: g / inf = -0, the limit
                x = x + ((g_ / (1.0 + np.exp(-g_))) * u) @ W["down"].T
        norm_in(x)
        logits = self._rms(x, self.out_norm) @ self.out.T
        return F64Run(logits, ks, vs, amax, mx, top2, overmed, sgap,
                      np.stack(norm_ms, axis=1), np.stack(gates, axis=1), np.stack(chan_ms, axis=0))


def forward_f64(g: gguf.GGUFFile, toks) -> F64Run:
    return F64Model(g).forward(toks)


def oracle_errs(g: gguf.GGUFFile, seq, run: F64Run) -> Tuple[List[float], List[int]]:
    """the CPU oracle teacher-forced over `seq`: max|oracle - f64| / max(1, std) of every step (the inputs' condition) and the
    oracle's greedy id of every step"""
    from oracle import oracle
    ref = oracle.OracleModel(g)
    errs, ids = [], []
    for pos, t in enumerate(seq):
        lg = ref.forward(int(t), pos)
        errs.append(rel_err(lg, run.logits[pos]))
        ids.append(int(oracle.argmax(lg)))
    ref.close()
    return errs, ids


def rel_err(got: np.ndarray, want64: np.ndarray) -> float:
    """max|got - f64| / max(1, std(f64 logits)) of one step"""
    return float(np.abs(np.asarray(got, dtype=np.float64) - want64).max()) / max(1.0, float(want64.std()))


def coverage(run: F64Run, steps=None) -> Dict[str, int]:
    """how many (step, layer, head) score rows of `steps` (default: all) are of each kind the cases exist for"""
    T = run.argmax.shape[0]
    sel = np.arange(T) if steps is None else np.asarray(sorted(set(int(s) for s in steps)), dtype=np.int64)
    pos = sel[:, None, None]
    am, gap = run.argmax[sel], run.split_gap[sel]
    late = pos >= 2 * SPLIT
    return {"rows": int(am.size),
            "rows_at_pos_ge_256": int(np.broadcast_to(late, am.shape).sum()),
            "max_in_split0_at_pos_ge_256": int((late & (am < SPLIT)).sum()),
            "max_in_last_split_at_pos_ge_256": int((late & (am // SPLIT == pos // SPLIT)).sum()),
            "max_is_newest_key": int((am == pos).sum()),
            "split_weight_underflows": int((np.nan_to_num(gap, nan=0.0).min(axis=-1) < -88.0).sum())}


# ------------------------------------------------------------------- what the GPU files share: bounds, witnesses, layouts ---
# (tests/test_gpu_attention_sharp.py, tests/test_gpu_attention_geometry.py and the latter's child, tests/attn_geometry_worker.py.
#  `model` below is nanollama_amd.model: this module itself never loads the HIP library.)

KV_TOL = 2e-5          # single ops, DESIGN section 5: |d| <= 2e-5 * (1 + |v|)

_cases: Dict[Tuple[str, str, str], tuple] = {}


def cached_case(mkdir, key: Tuple[str, str, str]):
    """(loaded GGUF, token sequence, F64Model, float64 run over the sequence) of a (shape, weight type, case), built once per
    process; mkdir() returns a fresh directory for the file"""
    key = tuple(key)
    assert key in CASES, f"{key} is not pinned by test_attn_cases_cpu.py"
    if key not in _cases:
        g = build_case(os.path.join(str(mkdir()), "m.gguf"), *key)
        toks = tokens(key[0])
        _cases[key] = (g, toks, F64Model(g), forward_f64(g, toks))
    return _cases[key]


class Worst:
    """the largest max|gpu - f64| / max(1, std) of a test, and where"""

    def __init__(self, what):
        self.what, self.err, self.at = what, 0.0, None

    def see(self, got, want64, at):
        e = rel_err(got, want64)
        if e > self.err:
            self.err, self.at = e, at
        return e

    def line(self, run=None):
        note = ""
        if run is not None and isinstance(self.at, int):
            note = f", smallest top-two margin of that step {float(run.top2_gap[self.at].min()):.2f} nats"
        return f"{self.what}: max|gpu-f64|/max(1,std) = {self.err:.2e} (at {self.at}{note})"

    def close(self, run=None):
        print("\n" + self.line(run))
        assert self.err <= GPU_TOL, (self.what, self.err, self.at)


def kinds(dev, pos):
    """the launch kinds of the single-token step at `pos` and how many of each"""
    return {k: c for k, (ms, c) in dev.profile_forward(5, pos, iters=1).items() if c}


def teacher_forced(dev, toks, run, w):
    for pos, t in enumerate(toks):
        dev.forward(t, pos)
        w.see(dev.state.logits, run.logits[pos], pos)


# Decode batches: five streams at ragged positions, five steps each.  A step's attention grid has as many 128-key splits as its
# deepest row needs (batched_step, nl_engine.hip), and the engine rotates q / k inside the attention launch (attn_rope_prologue,
# which also adds the biases and stores the K / V rows) only while that is at most two and the Q|K|V GEMM is the plain one (Q8_0 /
# F16 files; a Q4_0 file's short steps go to dgemm_kernel, which rotates in its own epilogue):
#   one_split     every position below 128: attn_kernel<FIN> writes the WO fragments itself, no merge launch;  NL_ROPE_IN_ATTN acts
#   two_splits    positions 3 .. 204, two streams cross 128: items + battn_merge_kernel over two partials;      NL_ROPE_IN_ATTN acts
#   three_splits  positions 3 .. 294, straddling 128 and 256: items + battn_merge_kernel over three partials; the knob is inert (the
#                 brope_kv launch rotates whatever it says), both values run because the step graph is keyed on it
BATCH_STARTS = {"one_split": [0, 3, 60, 100, 122], "two_splits": [3, 100, 124, 126, 200], "three_splits": [3, 125, 127, 254, 290]}
BATCH_STEPS = 5
BATCH_BELOW = {"one_split": 128, "two_splits": 256, "three_splits": 300}


def batch_run(dev, toks, start) -> np.ndarray:
    """BATCH_STEPS decode steps of len(start) streams that stand at `start` (prefilled here): logits [step, stream, vocab]"""
    ns = len(start)
    for s in range(ns):
        if start[s]:
            dev.prefill(toks[:start[s]], stream=s, want_logits=False)
    out = []
    for k in range(BATCH_STEPS):
        pos = [start[s] + k for s in range(ns)]
        ids, lg = dev.forward_batch(list(range(ns)), [toks[p] for p in pos], pos, want_logits=True)
        out.append(lg.copy())
    return np.stack(out)


def batch_see(w: Worst, out: np.ndarray, run: F64Run, start) -> None:
    for k in range(BATCH_STEPS):
        for s in range(len(start)):
            w.see(out[k, s], run.logits[start[s] + k], start[s] + k)


PROMPT_PREFIXES = (130, 257, 300)      # a prompt's logits are its last row's: three prefixes


def prompt_run(dev, g: gguf.GGUFFile, toks, run: F64Run, w: Worst, what: str):
    """prefill every prefix of PROMPT_PREFIXES on `dev` (logits of the last row into `w`), then read the K / V rows of all 300
    positions: ({prefix: logits}, {"k_cache" | "v_cache": rows}, the worst |gpu - f64| / (1 + |v|) of the rows)"""
    m = g.meta
    hd, S = m.head_dim, m.seq_len
    nkv = m.num_layers * m.num_kv_heads * S * hd
    last, cache, kv_worst = {}, {}, 0.0
    for n in PROMPT_PREFIXES:
        dev.reset()
        dev.prefill(toks[:n])
        last[n] = dev.state.logits.copy()
        w.see(last[n], run.logits[n - 1], n - 1)
    for which, want in (("k_cache", run.k), ("v_cache", run.v)):
        got = dev.debug_read(which, nkv).reshape(m.num_layers, m.num_kv_heads, S, hd)[:, :, :PROMPT_PREFIXES[-1]]
        cache[which] = got
        d = float((np.abs(got.astype(np.float64) - want) / (1.0 + np.abs(want))).max())
        print(f"\n{which} {what}: max|gpu-f64|/(1+|v|) = {d:.2e}")
        kv_worst = max(kv_worst, d)
    return last, cache, kv_worst


def mixed_steps(toks, chunk):
    """a 200-token prompt (stream 2) beside two decode rows that stand at 130 and 260.  chunk 199: ONE step carries the whole
    prompt -- a single segment of 199 rows (seven query tiles of 32, tiles that straddle key 128) and its final token as an output
    row; chunk 64: the same prompt admitted as 64 / 64 / 64 / 7 rows (segments that start at a position > 0, a short last one)."""
    steps, a, b = [], 130, 260
    bounds = [(p0, min(p0 + chunk, 199)) for p0 in range(0, 199, chunk)]
    for k, (p0, p1) in enumerate(bounds):
        out = [(0, a + k), (1, b + k)] + ([(2, 199)] if p1 == 199 else [])      # the final prompt token joins as an output row
        rows = out + [(2, p) for p in range(p0, p1)]
        steps.append(([s for s, _ in rows], [toks[p] for _, p in rows], [p for _, p in rows], len(out)))
    k = len(bounds)
    steps.append(([0, 1, 2], [toks[a + k], toks[b + k], toks[200]], [a + k, b + k, 200], 3))   # a decode step over the chunk's K / V
    return steps


def mixed_run(model, g, toks, chunk, knob, monkeypatch):
    """the steps of mixed_steps on a fresh handle: (logits of the output rows per step, their positions)"""
    monkeypatch.setenv("NL_MIXED_ATTN", knob)
    dev = model.load_llama_model(g, max_streams=3)
    dev.prefill(toks[:130], stream=0, want_logits=False)
    dev.prefill(toks[:260], stream=1, want_logits=False)
    got = []
    for streams, tk, pos, n_out in mixed_steps(toks, chunk):
        ids, lg = dev.forward_mixed(streams, tk, pos, n_out, want_logits=True)
        got.append((lg.copy(), pos[:n_out]))
    dev.close()
    return got


class PlacementMiss(Exception):
    pass


def no_warning(dev):
    err = dev.last_error()
    if "not placed 32 per XCD" in err:       # a property of the moment on the device (nl_persist.h): the chunk was redone on the
        raise PlacementMiss(err)             # launch plans, so the run did not test the persistent path
    return err == ""


def persistent_run(model, g, toks, f64, run, what):
    """the persistent decode (pd_decode_kernel) over the case: the resident session teacher-forced, then a chained greedy run"""
    dev = model.load_llama_model(g)
    try:
        info = dev.persist_info()
        assert info["ready"] and info["max_pos"] == 320, info
        # (a) the resident session: per-call Forward over the whole sequence, passes of 128 keys from position 128 and 256 on
        w = Worst(f"persistent decode, resident session {what}")
        teacher_forced(dev, toks, run, w)
        info = dev.persist_info()          # (one resident launch unless the host paused longer than the idle limit)
        assert no_warning(dev) and info["tokens"] == len(toks) and 1 <= info["launches"] <= 4, info
        # (b) chained greedy steps at positions 100 .. 159: below 128 a head's single record, above it the merge of the records
        # in LDS.  The device picks its own tokens; the float64 forward is fed the ids it produced.
        dev.reset()
        n0, steps = PERSIST_PROMPT, PERSIST_STEPS
        dev.prefill(toks[:n0])
        tok = int(np.argmax(dev.state.logits))
        fed, rows = [], []
        for i in range(steps):
            fed.append(tok)
            (tok,) = dev.decode_greedy(tok, n0 + i, 1)
            rows.append(dev.debug_read("logits", g.meta.vocab_size))
        info2 = dev.persist_info()
        assert no_warning(dev) and info2["tokens"] - info["tokens"] == steps, (info, info2)
    finally:
        dev.close()
    seq = list(toks[:n0]) + fed
    want = f64.forward(seq)
    # the inputs' condition on the sequence the device chose (test_attn_cases_cpu.py pins it on the oracle's own chain): the CPU
    # oracle, teacher-forced with the device's ids, stays within REF_CAP of float64 there too
    errs, oracle_ids = oracle_errs(g, seq, want)
    picked = fed[1:] + [tok]                                         # the id the device chose at positions n0 .. n0 + steps - 1
    same = sum(picked[i] == oracle_ids[n0 + i] for i in range(steps))
    print(f"\npersistent decode, greedy chain {what}: max|oracle-f64| on the device's ids = {max(errs):.2e}; "
          f"{same} of {steps} device ids are the oracle's (all: the device followed the oracle's own chain)")
    assert max(errs) <= REF_CAP, max(errs)
    wg = Worst(f"persistent decode, greedy chain {what}")
    for i in range(steps):
        wg.see(rows[i], want.logits[n0 + i], n0 + i)
    if what.endswith("/self"):             # on the ids the device chose the newest key still wins every row
        cov = coverage(want, range(n0, n0 + steps))
        assert cov["max_is_newest_key"] == cov["rows"], cov
    w.close(run)
    wg.close(want)
