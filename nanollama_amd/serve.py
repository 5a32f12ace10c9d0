"""HTTP chat server -- the endpoints and JSON shapes of go/serve.go.

    GET  /        chat UI (a minimal page of our own; the reference embeds go/ui.html)
    POST /chat    {"messages":[{"role","content"}], "temperature", "max_tokens", "top_k"} -> {"response"}
                  (+ "n": 2 .. --parallel, with --parallel N: that many samples of the prompt from one prefill ->
                  {"response": sample 0, "responses": [all n]}; absent or 1: the reply above; anything else 400 {"error"})
    POST /score   {"text"} or {"prompt","continuation"} (+ "details": true) -> {"tokens","logprob","nll","ppl","bpb"}
                  (+ "token_logprobs"); no counterpart in go/serve.go -- the quantity is nanollama/core_eval.py's bits per byte
                  Both bodies take an optional "voice": NAME (one of the server's --voice names; absent: the default voice,
                  --gamma or none); an unknown name is 400 {"error"}
    GET  /health  {"status","params_millions","layers","dim","heads","kv_heads","vocab_size","gamma_loaded"}
                  (+ "voices": [names] when the server has --voice entries)
                  (+ "steps","prefill_chunk","max_step_gap_ms","max_samples" with --parallel N)

One generation at a time (the model handle is single-caller): a lock around GenerateQuiet, as go/serve.go:56,106-108.
With --parallel N the engine is a BatchScheduler (batch_serve.py): concurrent requests decode as one batch, no lock.
"""
from __future__ import annotations

import contextlib
import json
import math
import threading
from dataclasses import replace
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer

from .batch_serve import BatchScheduler, RequestError
from .engine import GenParams
from .score import score_continuation, score_text

UI_HTML = b"""<!doctype html><html><head><meta charset="utf-8"><title>nanollama</title>
<style>body{font-family:sans-serif;max-width:46em;margin:2em auto}#log{white-space:pre-wrap;border:1px solid #ccc;
padding:1em;min-height:12em}input{width:80%}</style></head><body><h3>nanollama on MI355X</h3><div id="log"></div>
<p><input id="msg" placeholder="Say something"><button onclick="send()">Send</button></p><script>
async function send(){const m=document.getElementById('msg');const log=document.getElementById('log');
const text=m.value;if(!text)return;log.textContent+='> '+text+'\\n';m.value='';
const r=await fetch('/chat',{method:'POST',headers:{'Content-Type':'application/json'},
body:JSON.stringify({messages:[{role:'user',content:text}]})});const j=await r.json();
log.textContent+=j.response+'\\n\\n';}
document.getElementById('msg').addEventListener('keydown',e=>{if(e.key==='Enter')send();});
</script></body></html>"""


def _voices(engine) -> dict:
    return getattr(getattr(engine, "model", None), "voices", None) or {}


def request_voice(engine, req: dict) -> int:
    """The voice id a request body asks for: "voice": NAME among the model's voices; absent: 0, the default voice.
    Raises RequestError (400, JSON) for anything else."""
    name = req.get("voice")
    if name is None:
        return 0
    voices = _voices(engine)
    if not isinstance(name, str) or name not in voices:
        raise RequestError(400, f"unknown voice {name!r}: this server has {sorted(voices) if voices else 'no named voices'}")
    return voices[name]


def bind_voice(engine, voice: int) -> None:
    """One-caller engine: stream 0 speaks as `voice` from here on (called under the request lock).  A model without named
    voices has every stream on voice 0 for good."""
    if _voices(engine):
        engine.model.stream_voice(0, voice)


def request_samples(engine, req: dict) -> int:
    """The number of samples a /chat body asks for: "n", an integer in [1, parallel]; absent: 1.  Raises RequestError (400,
    JSON) for anything else; the serial server serves n = 1 only."""
    n = req.get("n")
    if n is None:
        return 1
    most = engine.parallel if isinstance(engine, BatchScheduler) else 1
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise RequestError(400, f'"n" must be an integer >= 1, got {n!r}')
    if n > most:
        raise RequestError(400, f'"n" = {n} exceeds the {most} samples this server draws at once: start it with --parallel {n} or more')
    return n


def handle_chat(engine, defaults: GenParams, lock: threading.Lock, body: bytes):
    """POST /chat (go/serve.go:69-111).  Returns (status, payload)."""
    try:
        req = json.loads(body.decode("utf-8") or "{}")
        if not isinstance(req, dict):
            raise ValueError("request must be a JSON object")
    except (ValueError, UnicodeDecodeError) as exc:
        return 400, "bad request: " + str(exc)
    try:
        voice = request_voice(engine, req)
        n = request_samples(engine, req)
    except RequestError as exc:
        return exc.status, {"error": str(exc)}
    messages = req.get("messages") or []
    if len(messages) == 0:
        return 200, {"response": "Send a message."}
    last = messages[-1] if isinstance(messages[-1], dict) else {}
    prompt = last.get("content") or ""
    if prompt == "":
        return 200, {"response": "Empty message."}
    params = defaults                       # request values override defaults only when > 0 (:94-103)
    if isinstance(req.get("max_tokens"), (int, float)) and req["max_tokens"] > 0:
        params = replace(params, max_tokens=int(req["max_tokens"]))
    if isinstance(req.get("temperature"), (int, float)) and req["temperature"] > 0:
        params = replace(params, temperature=float(req["temperature"]))
    if isinstance(req.get("top_k"), (int, float)) and req["top_k"] > 0:
        params = replace(params, top_k=int(req["top_k"]))
    try:
        with lock:
            if isinstance(engine, BatchScheduler) and n > 1:
                results = engine.generate_samples(prompt, params, n, voice=voice)
                return 200, {"response": results[0], "responses": results}
            if isinstance(engine, BatchScheduler):
                result = engine.generate_quiet(prompt, params, voice=voice)
            else:
                bind_voice(engine, voice)
                result = engine.generate_quiet(prompt, params)
    except RequestError as exc:             # (batch scheduler: settings it cannot serve, or an engine error)
        return exc.status, str(exc)
    return 200, {"response": result}


def handle_score(engine, lock, body: bytes):
    """POST /score.  {"text"}: the whole text behind BOS, bpb over its bytes; {"prompt", "continuation"}: the continuation given
    the prompt, bpb over the continuation's bytes.  Returns (status, payload)."""
    try:
        req = json.loads(body.decode("utf-8") or "{}")
        if not isinstance(req, dict):
            raise ValueError("request must be a JSON object")
        text, prompt, cont = req.get("text"), req.get("prompt"), req.get("continuation")
        if text is not None and (prompt is not None or cont is not None):
            raise ValueError('either "text" or "prompt" and "continuation"')
        if text is None and (prompt is None or cont is None):
            raise ValueError('"text", or "prompt" and "continuation", required')
        if not all(isinstance(v, str) for v in (text, prompt, cont) if v is not None):
            raise ValueError("text fields must be strings")
        if (text if text is not None else cont) == "":
            raise ValueError("nothing to score: empty " + ("text" if text is not None else "continuation"))
    except (ValueError, UnicodeDecodeError) as exc:
        return 400, "bad request: " + str(exc)
    try:
        voice = request_voice(engine, req)
    except RequestError as exc:
        return exc.status, {"error": str(exc)}
    # a BatchScheduler scores on a stream of its own worker (its score(ids, n_context)); a TextEngine's handle is single-caller
    if isinstance(engine, BatchScheduler):
        run = lambda model, ids, stream, n_context: engine.score(ids, n_context, voice=voice)
    else:
        from .score import score_ids as run
    try:
        with lock:
            if not isinstance(engine, BatchScheduler):
                bind_voice(engine, voice)
            if text is not None:
                r = score_text(engine.model, engine.tokenizer, text, score=run)
            else:
                r = score_continuation(engine.model, engine.tokenizer, prompt, cont, score=run)
    except RequestError as exc:
        return exc.status, str(exc)
    if r.n_tokens == 0:
        return 400, "bad request: nothing to score (the continuation adds no token to the prompt)"
    num = lambda v: v if math.isfinite(v) else None          # (a target whose logit is -inf: JSON has no infinity)
    out = {"tokens": r.n_tokens, "logprob": num(r.logprob), "nll": num(r.nll), "ppl": num(r.ppl), "bpb": num(r.bpb)}
    if req.get("details") is True:
        out["token_logprobs"] = [num(v) for v in r.token_logprobs]
    return 200, out


def handle_health(engine):
    """GET /health (go/serve.go:114-126)."""
    from .cli import estimate_params
    c = engine.model.config
    out = {"status": "ok", "params_millions": estimate_params(c) // 1_000_000, "layers": c.num_layers,
           "dim": c.embed_dim, "heads": c.num_heads, "kv_heads": c.num_kv_heads, "vocab_size": c.vocab_size,
           "gamma_loaded": engine.model.gamma is not None}
    if _voices(engine):                          # a server with --voice entries: their names (none: the reference's keys, no more)
        out["voices"] = list(_voices(engine))
    if isinstance(engine, BatchScheduler):       # --parallel N: the scheduler's counters (tools/bench_serve_parallel.py)
        out.update(steps=engine.steps, prefill_chunk=engine.prefill_chunk, max_step_gap_ms=round(engine.max_step_gap_ms, 3),
                   max_samples=engine.parallel)
    return out


def make_handler(engine, defaults: GenParams):
    # a BatchScheduler takes concurrent requests itself (its worker owns the handle); a TextEngine is single-caller
    lock = contextlib.nullcontext() if isinstance(engine, BatchScheduler) else threading.Lock()

    class Handler(BaseHTTPRequestHandler):
        def log_message(self, fmt, *args):  # quiet
            pass

        def _json(self, status, payload):
            data = (json.dumps(payload) + "\n").encode("utf-8")
            self.send_response(status)
            self.send_header("Content-Type", "application/json")
            self.send_header("Content-Length", str(len(data)))
            self.end_headers()
            self.wfile.write(data)

        def _text(self, status, text):
            data = (text + "\n").encode("utf-8")
            self.send_response(status)
            self.send_header("Content-Type", "text/plain; charset=utf-8")
            self.send_header("Content-Length", str(len(data)))
            self.end_headers()
            self.wfile.write(data)

        def do_GET(self):
            if self.path == "/":
                self.send_response(200)
                self.send_header("Content-Type", "text/html; charset=utf-8")
                self.send_header("Content-Length", str(len(UI_HTML)))
                self.end_headers()
                self.wfile.write(UI_HTML)
            elif self.path == "/health":
                self._json(200, handle_health(engine))
            elif self.path in ("/chat", "/score"):
                self._text(405, "POST only")
            else:
                self._text(404, "404 page not found")

        def do_POST(self):
            if self.path not in ("/chat", "/score"):
                self._text(404, "404 page not found")
                return
            n = int(self.headers.get("Content-Length") or 0)
            if self.path == "/score":
                status, payload = handle_score(engine, lock, self.rfile.read(n))
            else:
                status, payload = handle_chat(engine, defaults, lock, self.rfile.read(n))
            if isinstance(payload, str):
                self._text(status, payload)
            else:
                self._json(status, payload)

    return Handler


class _BatchHTTPServer(ThreadingHTTPServer):
    request_queue_size = 128     # a batching server's clients connect at once (the default backlog of 5 resets some)


def run_server(engine, defaults: GenParams, port: int) -> None:
    """runServer go/serve.go:54-131"""
    srv_cls = _BatchHTTPServer if isinstance(engine, BatchScheduler) else ThreadingHTTPServer
    srv = srv_cls(("", port), make_handler(engine, defaults))
    print(f"[nanollama] web UI at http://localhost:{port}")
    try:
        srv.serve_forever()
    finally:
        srv.server_close()
