"""Continuous batching behind POST /chat: concurrent requests decode as one sampled batch (nl_forward_batch_sample).

The reference serves one request at a time (go/serve.go:56,106-108: one CPU engine behind a mutex).  Here one worker
thread owns the model handle (single-caller) and runs a loop of steps; every step

  1. admits waiting requests while a stream is free: reset(stream), prefill of the first n_prompt - 1 prompt tokens
     (n_prompt = min(len, seq_len - 1), as Engine.generate_ids); the request joins with its last prompt token at
     position n_prompt - 1;
  2. steps every active request with one forward_batch_sample call -- Forward, penalty, sampling and the recent window of
     every row on the device -- and applies the stop rules of Engine.generate_ids per row: EOS ends the request and is
     not emitted (go/main.go:203); otherwise the id is emitted, and the output cap, max_tokens and the end of the context
     each end the request.

A finished request gets its text and frees its stream; a request that arrives meanwhile joins at the next step.
POST /score jobs (score(ids, n_context)) wait in the same queue: the worker gives one a free stream, scores on it
(score.score_ids: reset and nl_score per window) and frees the stream again -- it occupies the worker as a whole-prompt
prefill at admission does.
With prefill_chunk = N > 0 (--prefill-chunk) admission no longer runs the prompt: it only resets the stream and seeds the
request's generator, and every step is ONE forward_mixed_sample call (nl_forward_mixed_sample) -- the decoding requests as
output rows, then up to N prompt tokens of the admitted requests in admission order.  A prompt may span several steps and
several short prompts may share one step's budget; in the step that feeds the last of a request's tokens 0 .. n_prompt - 2
its final prompt token joins as an output row (it does not count against N) and the request decodes from then on.  The
requests that are already decoding get a token in every step instead of waiting for whole prompts.

Settings per request follow go/serve.go:94-103 (temperature, max_tokens and top_k come from the request when > 0); top_p,
rep_penalty and rep_window are the server's.  A request may name one of the model's voices (nl_set_voice): the worker binds
the stream it gives the request -- or the score job -- to that voice (nl_stream_voice; none named: voice 0) before the first
step that carries the stream's rows, so the rows of one step each take their own voice's gamma.  Each request samples from its own generator, seeded from the scheduler's
(seeded by --seed) in admission order, and draws a uniform only while its temperature is > 0, as Engine does.

Several samples of one prompt (generate_samples, "n" in POST /chat; Engine.generate(tokens, num_samples=N) and
KVCache.prefill, nanollama/engine.py:222-299 and :139-153): the request waits at the head of the queue until n streams are
free, its first stream -- the leader -- is reset, bound and prefilled exactly as a single request's, then ONE
kv_fork(leader, siblings, n_prompt - 1) (nl_kv_fork) copies the prompt's K / V rows into the other n - 1 streams and all n rows
feed the final prompt token at position n_prompt - 1, each with its own generator (the leader's drawn first, so it is the one
an n = 1 request would have had), repetition window and text.  With prefill_chunk > 0 the leader is chunked as any request
and the fork follows the step that fed its last chunk; the siblings join the next step.  Rows finish independently, a
finished row's stream is free at once, and the request returns when its last row has finished.  n = 1 makes the engine calls
a request made before there was an n.
"""
from __future__ import annotations

import collections
import threading
import time
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from .engine import GenParams
from .engine_text import TextOutput
from .score import ScoreResult, score_ids

MAX_PARALLEL = 64            # rows of one nl_forward_batch_sample call (the LM head's batch)
MAX_VOCAB = 131072           # the device sampler's vocabularies
MAX_TOP_K = 1024             # the device sampler's top-k list


class RequestError(Exception):
    """A request the scheduler could not serve: status 400 (settings the device sampler does not take) or 500 (engine)."""

    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = status


@dataclass
class _Request:
    tokens: List[int]
    params: GenParams
    voice: int = 0
    done: threading.Event = field(default_factory=threading.Event)
    text: str = ""
    error: Optional[RequestError] = None
    n: int = 1                                       # samples: rows of the batch that share this prompt
    texts: List[str] = field(default_factory=list)   # one per sample, in sample order
    left: int = 0                                    # rows that have not finished yet


@dataclass
class _ScoreJob:
    ids: List[int]
    n_context: int
    voice: int = 0
    done: threading.Event = field(default_factory=threading.Event)
    result: Optional[ScoreResult] = None
    error: Optional[RequestError] = None


@dataclass
class _Row:
    req: _Request
    stream: int
    token: int               # fed at `pos` by the next step
    pos: int
    rng: np.random.Generator
    out: TextOutput
    recent: List[int] = field(default_factory=list)
    n_out: int = 0           # ids sampled so far (EOS included)
    pre: int = 0             # prefill_chunk > 0: prompt tokens (0 .. n_prompt - 2) to feed before the row decodes ...
    fed: int = 0             # ... and how many of them have been fed
    sample: int = 0          # which of the request's n samples this row is (0: the leader, which runs the prompt)
    siblings: List["_Row"] = field(default_factory=list)   # the leader, prefill_chunk > 0: rows that join once it forks


class BatchScheduler:
    def __init__(self, model, tokenizer, parallel: int, rep_penalty: float = 1.15, rep_window: int = 64,
                 seed: Optional[int] = None, prefill_chunk: int = 0):
        if not 1 <= parallel <= min(MAX_PARALLEL, model.max_streams):
            raise ValueError(f"parallel must be in [1, {min(MAX_PARALLEL, model.max_streams)}] (the handle's max_streams)")
        if model.config.vocab_size > MAX_VOCAB:
            raise ValueError(f"batched sampling covers vocabularies up to {MAX_VOCAB}, not {model.config.vocab_size}")
        if not 0 <= rep_window <= 1024:
            raise ValueError("rep_window must be in [0, 1024] for batched sampling")
        if prefill_chunk < 0:
            raise ValueError("prefill_chunk must be >= 0")
        if prefill_chunk > 0:
            max_rows = model.mixed_capacity[0]
            if parallel + prefill_chunk > max_rows:
                raise ValueError(f"parallel + prefill_chunk = {parallel + prefill_chunk} exceeds the {max_rows} rows of one "
                                 f"mixed step (prefill_chunk <= {max_rows - parallel} with parallel {parallel})")
        self.prefill_chunk = int(prefill_chunk)
        self.max_step_gap_ms = 0.0                      # longest interval between two consecutive steps that both carried a decoding row
        self._last_decode_step = None
        self.model, self.tokenizer = model, tokenizer
        self.parallel = parallel
        self.eos_id = tokenizer.eos_id
        self.rep_penalty = float(np.float32(rep_penalty))
        self.rep_window = int(rep_window)
        self.rng = np.random.default_rng(seed)
        self.steps = 0                                  # forward_batch_sample / forward_mixed_sample calls so far
        self._cv = threading.Condition()
        self._queue: collections.deque = collections.deque()
        self._closed = False
        self._worker = threading.Thread(target=self._run, name="batch-scheduler", daemon=True)
        self._worker.start()

    # ---- callers (any thread) ----
    def _check_voice(self, voice: int) -> int:
        if voice and int(voice) not in (getattr(self.model, "voices", None) or {}).values():
            raise RequestError(400, f"unknown voice id {voice}")
        return int(voice)

    def _bind(self, stream: int, voice: int) -> None:
        """The worker, before the first step with rows of `stream`: the stream speaks as `voice`.  A model without named
        voices has every stream on voice 0 for good."""
        if getattr(self.model, "voices", None):
            self.model.stream_voice(stream, voice)

    def generate_quiet(self, prompt: str, params: GenParams, voice: int = 0) -> str:
        """GenerateQuiet (go/main.go:233-291) as one row of the shared batch, in the voice with id `voice` (model.voices; 0: the
        default); blocks until the request is done.  Raises RequestError (status 400 / 500)."""
        return self.generate_samples(prompt, params, 1, voice=voice)[0]

    def generate_samples(self, prompt: str, params: GenParams, n, voice: int = 0) -> List[str]:
        """n completions of one prompt (Engine.generate_batch, nanollama/engine.py:354) as n rows of the shared batch that
        share one prefill; 1 <= n <= parallel.  Blocks until the last row is done; the texts come in sample order."""
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= self.parallel:
            raise RequestError(400, f"n must be an integer in [1, {self.parallel}] (the server's --parallel), got {n!r}")
        if not params.top_p > 0:
            raise RequestError(400, f"top_p must be > 0, got {params.top_p}")
        if params.temperature > 0 and params.top_p >= 1.0 and not 1 <= params.top_k <= MAX_TOP_K:
            raise RequestError(400, f"top_k must be in [1, {MAX_TOP_K}] for batched sampling, got {params.top_k}")
        req = _Request(self.tokenizer.encode(prompt, True), params, self._check_voice(voice), n=n, texts=[""] * n, left=n)
        with self._cv:
            if self._closed:
                raise RequestError(500, "scheduler closed")
            self._queue.append(req)
            self._cv.notify()
        req.done.wait()
        if req.error is not None:
            raise req.error
        return list(req.texts)

    def score(self, ids: List[int], n_context: int = 1, voice: int = 0) -> ScoreResult:
        """score.score_ids(model, ids, a free stream, n_context) on the worker, in voice `voice`; blocks until done.
        Raises RequestError (400: unknown voice id; 500)."""
        job = _ScoreJob([int(t) for t in ids], int(n_context), self._check_voice(voice))
        with self._cv:
            if self._closed:
                raise RequestError(500, "scheduler closed")
            self._queue.append(job)
            self._cv.notify()
        job.done.wait()
        if job.error is not None:
            raise job.error
        return job.result

    def close(self) -> None:
        with self._cv:
            self._closed = True
            self._cv.notify()
        self._worker.join()

    # ---- the worker ----
    def _finish(self, row: _Row, free: List[int]) -> None:
        req = row.req
        req.texts[row.sample] = row.out.text()
        free.append(row.stream)
        req.left -= 1
        if req.left == 0:                               # the request completes with its last row
            req.text = req.texts[0]
            req.done.set()

    def _fail(self, req, status: int, exc: BaseException) -> None:
        req.error = RequestError(status, f"{type(exc).__name__}: {exc}")
        req.done.set()

    def _score(self, job: _ScoreJob, stream: int, free: List[int]) -> None:
        try:
            self.model.reset(stream)
            self._bind(stream, job.voice)
            job.result = score_ids(self.model, job.ids, stream, job.n_context)
        except Exception as exc:                        # engine error: this job fails, the scheduler goes on
            free.append(stream)
            self._fail(job, 500, exc)
            return
        free.append(stream)
        job.done.set()

    def _fork(self, row: _Row, n_pos: int) -> None:
        """The leader's rows [0, n_pos) into every sibling's stream, in one call; the siblings speak in the request's voice."""
        self.model.kv_fork(row.stream, [s.stream for s in row.siblings], n_pos)
        for s in row.siblings:
            self._bind(s.stream, row.req.voice)

    def _admit(self, req: _Request, streams: List[int], active: List[_Row], free: List[int]) -> None:
        """streams: one per sample; the first is the leader's, which runs the prompt."""
        stream = streams[0]
        if isinstance(req, _ScoreJob):
            self._score(req, stream, free)
            return
        cfg = self.model.config
        p = req.params
        n_prompt = min(len(req.tokens), max(cfg.seq_len - 1, 0))
        # one generator per sample, the leader's first: with one --seed it is the generator an n = 1 request would have had
        rows = [_Row(req, s, req.tokens[n_prompt - 1] if n_prompt else 0, n_prompt - 1,
                     np.random.default_rng(int(self.rng.integers(0, 2 ** 63 - 1))), TextOutput(self.tokenizer), sample=i)
                for i, s in enumerate(streams)]
        row = rows[0]
        row.siblings = rows[1:]
        if p.max_tokens <= 0 or n_prompt <= 0:       # nothing to sample
            for r in rows:
                self._finish(r, free)
            return
        fork_now = bool(row.siblings) and (not self.prefill_chunk or n_prompt == 1)
        try:
            self.model.reset(stream)
            self._bind(stream, req.voice)
            if n_prompt > 1 and not self.prefill_chunk:
                self.model.prefill(req.tokens[:n_prompt - 1], pos0=0, stream=stream, want_logits=False)
            if fork_now:
                self._fork(row, n_prompt - 1)
        except Exception as exc:                        # engine error: this request fails, the scheduler goes on
            free.extend(streams)
            self._fail(req, 500, exc)
            return
        if self.prefill_chunk:
            row.pre = n_prompt - 1
        active.append(row)
        if fork_now:                                    # (chunked prompts: the siblings join behind the leader's last chunk)
            active.extend(row.siblings)
            row.siblings = []

    def _note_step(self, decoding: bool) -> None:
        """max_step_gap_ms: called when a step returns; `decoding`: it carried a row of a request that was already decoding."""
        now = time.perf_counter()
        if decoding and self._last_decode_step is not None:
            self.max_step_gap_ms = max(self.max_step_gap_ms, (now - self._last_decode_step) * 1e3)
        self._last_decode_step = now if decoding else None

    def _apply(self, rows: List[_Row], ids, recents, free: List[int]) -> List[_Row]:
        """The stop rules of Engine.generate_ids on the sampled rows; returns the ones that go on."""
        seq_len = self.model.config.seq_len
        keep = []
        for r, t, rec in zip(rows, ids, recents):
            r.recent, r.n_out = rec, r.n_out + 1
            if t == self.eos_id:                        # go/main.go:203: not emitted
                self._finish(r, free)
                continue
            capped = r.out.add(t)
            r.token, r.pos = t, r.pos + 1
            # Engine.generate_ids forwards the id at r.pos and stops when that leaves no position to sample from
            # (pos + 1 >= seq_len after its increment), after max_tokens ids, or at the output cap
            if capped or r.n_out >= r.req.params.max_tokens or r.pos + 1 >= seq_len:
                self._finish(r, free)
            else:
                keep.append(r)
        return keep

    def _settings(self, rows: List[_Row]):
        params = [dict(temperature=r.req.params.temperature, top_p=r.req.params.top_p, top_k=max(r.req.params.top_k, 1),
                       rep_penalty=self.rep_penalty, rep_window=self.rep_window) for r in rows]
        uniforms = [r.rng.random(dtype=np.float32) if r.req.params.temperature > 0 else np.float32(0) for r in rows]
        return params, uniforms

    def _step_mixed(self, active: List[_Row], free: List[int]) -> None:
        """prefill_chunk > 0: one forward_mixed_sample call.  A row of `active` with fed < pre is still being admitted."""
        decoding = [r for r in active if r.fed >= r.pre]
        out_rows, chunks, touched, budget = list(decoding), [], [], self.prefill_chunk
        for r in active:                                # admission order
            if r.fed >= r.pre or budget == 0:
                continue
            take = min(r.pre - r.fed, budget)
            chunks.append((r, r.fed, take))
            touched.append(r)
            budget -= take
            if r.fed + take == r.pre:                   # its last chunk: the final prompt token samples in this step
                out_rows.append(r)
        streams = [r.stream for r in out_rows] + [r.stream for r, p0, k in chunks for _ in range(k)]
        tokens = [r.token for r in out_rows] + [r.req.tokens[p] for r, p0, k in chunks for p in range(p0, p0 + k)]
        pos = [r.pos for r in out_rows] + [p for r, p0, k in chunks for p in range(p0, p0 + k)]
        params, uniforms = self._settings(out_rows)
        try:
            ids, recents = self.model.forward_mixed_sample(streams, tokens, pos, len(out_rows), params, uniforms,
                                                           [r.recent for r in out_rows])
        except Exception as exc:                        # engine error: the requests of this call fail, the scheduler goes on
            failed = {id(r) for r in out_rows + touched}
            for r in active:
                if id(r) in failed:
                    free.extend([r.stream] + [s.stream for s in r.siblings])
                    self._fail(r.req, 500, exc)
            active[:] = [r for r in active if id(r) not in failed]
            self._last_decode_step = None
            return
        self.steps += 1
        self._note_step(bool(decoding))
        for r, p0, k in chunks:
            r.fed = p0 + k
        joined, lost = [], set()
        for r in out_rows:                              # a leader whose last chunk this step fed: its rows [0, pre) exist now
            if r.siblings:
                try:
                    self._fork(r, r.pre)
                    joined.extend(r.siblings)
                except Exception as exc:                # engine error: the request fails with all its streams, as a prefill's
                    free.extend([r.stream] + [s.stream for s in r.siblings])
                    self._fail(r.req, 500, exc)
                    lost.add(id(r))
                r.siblings = []
        going = [(r, t, rec) for r, t, rec in zip(out_rows, ids, recents) if id(r) not in lost]
        kept = {id(r) for r in self._apply([g[0] for g in going], [g[1] for g in going], [g[2] for g in going], free)}
        sampled = {id(r) for r in out_rows}
        active[:] = [r for r in active if id(r) in kept or id(r) not in sampled] + joined

    def _step(self, active: List[_Row], free: List[int]) -> None:
        params, uniforms = self._settings(active)
        try:
            ids, recents = self.model.forward_batch_sample([r.stream for r in active], [r.token for r in active],
                                                           [r.pos for r in active], params, uniforms,
                                                           [r.recent for r in active])
        except Exception as exc:                        # engine error: the requests of this call fail, the scheduler goes on
            for r in active:
                free.append(r.stream)
                self._fail(r.req, 500, exc)
            active.clear()
            self._last_decode_step = None
            return
        self.steps += 1
        self._note_step(True)
        active[:] = self._apply(active, ids, recents, free)

    def _run(self) -> None:
        free = list(range(self.parallel))
        active: List[_Row] = []
        while True:
            with self._cv:
                while not self._closed and not self._queue and not active:
                    self._cv.wait()
                if self._closed:
                    pending = list(self._queue) + [r.req for r in active]
                    self._queue.clear()
                    break
                admit = []                              # first in, first out: the head waits for all its streams, nothing overtakes it
                while self._queue and len(free) >= getattr(self._queue[0], "n", 1):
                    req = self._queue.popleft()
                    admit.append((req, [free.pop(0) for _ in range(getattr(req, "n", 1))]))
            for req, streams in admit:
                self._admit(req, streams, active, free)
            if active and self.prefill_chunk:
                self._step_mixed(active, free)
            elif active:
                self._step(active, free)
            if not active:
                self._last_decode_step = None           # (idle until the next request: not a gap between steps)
        for req in pending:
            self._fail(req, 500, RuntimeError("scheduler closed"))
