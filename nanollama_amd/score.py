"""Scoring a token sequence: log-probabilities, perplexity, bits per byte.

Host logic over `model.score(tokens, targets, pos0, stream)` (nl_score: the prompt path with an LM head over every row and
a device reduction of each logits row, so no logits reach the host) and `model.reset(stream)`; nothing here imports the GPU
library, so a fake model serves in tests.  The reference judges a checkpoint by bits per byte (nanollama/core_eval.py:15-54:
one forward over the text, mean cross entropy x tokens / bytes / ln 2); score_text is that quantity for a GGUF.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np


@dataclass
class ScoreResult:
    n_tokens: int                        # ids scored
    logprob: float                       # float64 sum of their float32 natural-log probabilities
    nll: float                           # -logprob / n_tokens (inf when nothing was scored)
    ppl: float                           # exp(nll)
    token_logprobs: List[float] = field(default_factory=list)
    greedy_matches: int = 0              # scored rows whose greedy id is the target
    n_bytes: Optional[int] = None        # score_text / score_continuation: UTF-8 bytes of the scored text ...
    bpb: Optional[float] = None          # ... and -logprob / n_bytes / ln 2


def _exp(x: float) -> float:
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def windows(n_ids: int, seq_len: int, n_context: int = 1):
    """The calls that score ids[n_context:] of an n_ids-long list on a context of seq_len positions: (first input, number of
    inputs, per input the index of its target id or -1).  Window k feeds ids[k S : (k + 1) S] at positions 0 .. and asks each
    input for the id behind it -- the last input of a full window for the first id of the next one, so every id from
    n_context on is scored exactly once; the very last id has nothing behind it, and ids below n_context are context only.
    Windows with nothing to score are left out."""
    S = int(seq_len)
    if S < 1:
        raise ValueError("seq_len must be >= 1")
    n_context = max(int(n_context), 1)
    out = []
    for lo in range(0, n_ids, S):
        hi = min(lo + S, n_ids)
        tgt = [j + 1 if j + 1 < n_ids and j + 1 >= n_context else -1 for j in range(lo, hi)]
        if any(t >= 0 for t in tgt):
            out.append((lo, hi - lo, tgt))
    return out


def score_ids(model, ids: Sequence[int], stream: int = 0, n_context: int = 1) -> ScoreResult:
    """log P(ids[n_context:] | what precedes them).  A list longer than the model's seq_len runs in windows of seq_len ids,
    each from position 0 after a reset (a window's first ids see a short context, as in any strided perplexity run)."""
    ids = [int(t) for t in ids]
    lps: List[float] = []
    matches = 0
    for lo, n, tgt_idx in windows(len(ids), model.config.seq_len, n_context):
        targets = [ids[j] if j >= 0 else -1 for j in tgt_idx]
        model.reset(stream)
        lp, am = model.score(ids[lo:lo + n], targets, 0, stream)
        for i, t in enumerate(targets):
            if t >= 0:
                lps.append(float(lp[i]))
                matches += int(int(am[i]) == t)
    total = float(np.sum(np.asarray(lps, dtype=np.float64))) if lps else 0.0
    nll = -total / len(lps) if lps else math.inf
    return ScoreResult(len(lps), total, nll, _exp(nll), lps, matches)


def bits_per_byte(logprob: float, n_bytes: int) -> float:
    """nanollama/core_eval.py:47-52: mean loss x tokens / bytes / ln 2, with mean loss x tokens = -logprob."""
    return -logprob / n_bytes / math.log(2) if n_bytes > 0 else math.inf


def _with_bytes(r: ScoreResult, n_bytes: int) -> ScoreResult:
    r.n_bytes = n_bytes
    r.bpb = bits_per_byte(r.logprob, n_bytes) if r.n_tokens > 0 else math.inf
    return r


def score_text(model, tokenizer, text: str, stream: int = 0, score=score_ids) -> ScoreResult:
    """Bits per byte of a text as nanollama/core_eval.py:15-54 computes it: BOS in front (tokenizer.encode(text, True)), every
    id behind it scored; fewer than 2 ids give inf, as there."""
    return _with_bytes(score(model, tokenizer.encode(text, True), stream, 1), len(text.encode("utf-8")))


def continuation_ids(tokenizer, prompt: str, continuation: str):
    """(ids of prompt + continuation with BOS, n_context): the ids that the prompt alone also yields are context; a prompt
    whose last piece merges with the continuation's first contributes only the ids in front of the merged one."""
    full = tokenizer.encode(prompt + continuation, True)
    head = tokenizer.encode(prompt, True)
    n = 0
    while n < len(full) and n < len(head) and full[n] == head[n]:
        n += 1
    return full, max(n, 1)


def score_continuation(model, tokenizer, prompt: str, continuation: str, stream: int = 0, score=score_ids) -> ScoreResult:
    """log P(continuation | prompt); bpb is over the continuation's bytes."""
    full, n_context = continuation_ids(tokenizer, prompt, continuation)
    return _with_bytes(score(model, full, stream, n_context), len(continuation.encode("utf-8")))
