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
do contain the rows they exist for); tests/test_gpu_attention_sharp.py holds every attention kernel to forward_f64.
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

# (shape, weight type, case): exactly the models the GPU file uses; test_attn_cases_cpu.py runs every one of them
CASES: List[Tuple[str, str, str]] = (
    [("gqa", "q8_0", c) for c in ("sharp", "self", "anti")] + [("gqa", "q4_0", "sharp")]
    + [("gqa", "f16", c) for c in ("sharp", "self", "anti")]
    + [("gqa_bias", "q8_0", c) for c in ("shift_pos", "shift_neg")]
    + [("gqa_conj", "q4_0", "sharp"), ("gqa_conj", "q8_0", "sharp")]
    + [("mha4", "q8_0", c) for c in ("sharp", "self", "anti")]
    + [("mha3", "q8_0", c) for c in ("sharp", "self", "anti")]
    + [("hd32_g3", "q8_0", "sharp")]
    + [("wide", "q4_0", c) for c in ("sharp", "self", "anti")])

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
