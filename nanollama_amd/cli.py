"""Command-line host -- the flags and modes of go/main.go:25-132 over the HIP engine.

    python -m nanollama_amd --model m.gguf --prompt "Hello"            (one shot)
    python -m nanollama_amd --model m.gguf --interactive               (REPL, /quit /exit /info)
    python -m nanollama_amd --model m.gguf --serve --port 8080         (HTTP: GET /, POST /chat, POST /score, GET /health)
    python -m nanollama_amd --model m.gguf --score text.txt            (log-probability, perplexity, bits per byte of a text)
    python -m nanollama_amd --model m.gguf --serve --parallel 16 --prefill-chunk 64   (batched server, chunked admission)
    python -m nanollama_amd --model m.gguf --voice leo=leo.npz --voice yent=yent.npz --serve --parallel 16
                                                                        (one base, several gamma essences: "voice" per request)
    python -m nanollama_amd --model m.gguf --voice leo=leo.npz --use-voice leo --prompt "Hello"
    python -m nanollama_amd --model m.gguf --prompt "Hello" --samples 4 --seed 1    (four completions from one prefill)
"""
from __future__ import annotations

import argparse
import os
import sys

from .engine import GenParams
from .engine_text import TextEngine
from .gguf import GGUFError, load_gguf
from .model import load_llama_model
from .tokenizer import Tokenizer


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="nanollama", description="nanollama inference on MI355X (GGUF in, text out)")
    ap.add_argument("--model", default="", help="Path to GGUF model file (required)")
    ap.add_argument("--gamma", default="", help="Path to gamma NPZ file (optional, personality)")
    ap.add_argument("--voice", action="append", default=[], metavar="NAME=PATH",
                    help="a named gamma NPZ next to --gamma (repeatable, at most 63): /chat and /score requests pick one with "
                         '"voice": NAME, other runs with --use-voice NAME; --gamma stays the default voice')
    ap.add_argument("--use-voice", default="", metavar="NAME",
                    help="with --prompt, --interactive, --score or stdin: generate / score as the --voice of this name")
    ap.add_argument("--prompt", default="", help="Prompt text (if empty, reads from stdin)")
    ap.add_argument("--max-tokens", type=int, default=256, help="Maximum tokens to generate")
    ap.add_argument("--temp", type=float, default=0.8, help="Sampling temperature (0 = greedy)")
    ap.add_argument("--top-p", type=float, default=0.9, help="Top-p (nucleus) sampling threshold")
    ap.add_argument("--top-k", type=int, default=50, help="Top-k sampling (used when top-p >= 1.0)")
    ap.add_argument("--rep-penalty", type=float, default=1.15, help="Repetition penalty (1.0 = disabled)")
    ap.add_argument("--rep-window", type=int, default=64, help="Repetition penalty lookback window")
    ap.add_argument("--interactive", action="store_true", help="Interactive REPL mode")
    ap.add_argument("--serve", action="store_true", help="Start HTTP chat server")
    ap.add_argument("--port", type=int, default=8080, help="HTTP server port (used with --serve)")
    ap.add_argument("--list-tensors", action="store_true", help="List all tensors and exit")
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    ap.add_argument("--gpus", type=int, default=1,
                    help="shard the model tensor-parallel over this many GPUs of the node (2, 4 or 8: devices --device .. --device + N - 1; "
                         "the 7.9B tier's configuration).  One process, one engine: --serve and --interactive work unchanged")
    ap.add_argument("--seed", type=int, default=None, help="sampling seed (default: entropy, like the reference)")
    ap.add_argument("--parallel", type=int, default=1,
                    help="with --serve: decode up to N concurrent /chat requests as one sampled batch (N <= 64; "
                         "1 = one request at a time, as the reference)")
    ap.add_argument("--prefill-chunk", type=int, default=0,
                    help="with --serve --parallel N: admit prompts in chunks of up to this many tokens that share a step with "
                         "the decoding requests (mixed steps) instead of running each prompt whole while the others wait; "
                         "0 = whole prompts at admission")
    ap.add_argument("--score", default="", metavar="PATH",
                    help="score the text in PATH ('-': stdin) instead of generating: prints tokens, nll, ppl, bits per byte "
                         "and tokens/s; not with --serve, --interactive or --prompt")
    ap.add_argument("--samples", type=int, default=1, metavar="N",
                    help="with --prompt: N completions of the prompt from ONE prefill (the prompt's K/V rows are copied into "
                         "N - 1 further streams and the N rows decode as one batch; N <= 64), each printed under a line "
                         "'--- sample i ---'; 1 = one completion, streamed as it is generated")
    return ap


def check_samples(args) -> None:
    """--samples N: N > 1 is a mode of --prompt on one GPU (the rows decode through the batched sampler)."""
    if not 1 <= args.samples <= 64:
        raise RuntimeError("--samples must be in [1, 64]")
    if args.samples == 1:
        return
    for flag, on in (("--interactive", args.interactive), ("--score", bool(args.score)), ("--serve", args.serve)):
        if on:
            raise RuntimeError(f"--samples cannot be combined with {flag}" + (': a request asks with "n"' if flag == "--serve" else ""))
    if not args.prompt:
        raise RuntimeError("--samples needs --prompt")
    if args.gpus > 1:
        raise RuntimeError("--samples > 1 needs --gpus 1")
    if not 0 <= args.rep_window <= 1024:
        raise RuntimeError("--samples > 1 needs --rep-window <= 1024")


def run_samples(eng, prompt: str, params: GenParams, args, out=None) -> None:
    """--samples N: the prompt as one n = N request of a BatchScheduler of N rows; the completions in sample order."""
    from .batch_serve import BatchScheduler, RequestError
    out = out or sys.stdout
    sched = BatchScheduler(eng.model, eng.tokenizer, args.samples, rep_penalty=args.rep_penalty, rep_window=args.rep_window,
                           seed=args.seed)
    try:
        texts = sched.generate_samples(prompt, params, args.samples, voice=eng.model.voices[args.use_voice] if args.use_voice else 0)
    except RequestError as exc:
        raise RuntimeError(str(exc)) from exc
    finally:
        sched.close()
    for i, text in enumerate(texts):
        print(f"--- sample {i} ---", file=out)
        print(text, file=out)


def check_score(args) -> None:
    """--score: a mode of its own, on one GPU (a device group has no scoring entry point)."""
    if not args.score:
        return
    for flag, on in (("--serve", args.serve), ("--interactive", args.interactive), ("--prompt", bool(args.prompt))):
        if on:
            raise RuntimeError(f"--score cannot be combined with {flag}")
    if args.gpus > 1:
        raise RuntimeError("--score needs --gpus 1 (scoring is not available on a device group)")


def run_score(eng, path: str, out=None) -> None:
    import time
    from .score import score_text
    out = out or sys.stdout
    text = sys.stdin.read() if path == "-" else open(path, encoding="utf-8").read()
    t0 = time.perf_counter()
    r = score_text(eng.model, eng.tokenizer, text)
    dt = time.perf_counter() - t0
    print(f"tokens {r.n_tokens}  nll {r.nll:.6f}  ppl {r.ppl:.4f}  bpb {r.bpb:.6f}  {r.n_tokens / dt if dt > 0 else 0.0:.1f} tokens/s", file=out)


MAX_NAMED_VOICES = 63        # voices 1 .. NL_MAX_VOICES - 1 (voice 0 is --gamma)


def parse_voices(specs) -> list:
    """--voice NAME=PATH ...: [(name, path)], names unique and non-empty."""
    out = []
    for spec in specs:
        name, sep, path = spec.partition("=")
        name = name.strip()
        if not sep or not name or not path:
            raise RuntimeError(f"--voice takes NAME=PATH, got {spec!r}")
        if name in [n for n, _ in out]:
            raise RuntimeError(f"--voice {name!r} is given twice")
        out.append((name, path))
    if len(out) > MAX_NAMED_VOICES:
        raise RuntimeError(f"at most {MAX_NAMED_VOICES} --voice entries, got {len(out)}")
    return out


def check_voices(args) -> None:
    """--voice / --use-voice: the specs parse, and --use-voice names one of them (a server's requests name their own)."""
    names = [n for n, _ in parse_voices(args.voice)]
    if args.use_voice and args.serve:
        raise RuntimeError('--use-voice is not for --serve: a request names its voice ("voice": NAME)')
    if args.use_voice and args.use_voice not in names:
        raise RuntimeError(f"--use-voice {args.use_voice!r} is not among the --voice names ({', '.join(names) or 'none given'})")


def load_voices(model, specs) -> None:
    """Define voices 1, 2, ... from the --voice files (gamma.load_gamma) and record their names in model.voices."""
    from .gamma import load_gamma
    for vid, (name, path) in enumerate(parse_voices(specs), start=1):
        try:
            ge = load_gamma(path)
        except ValueError as exc:
            raise RuntimeError(f"--voice {name}: {exc}") from exc
        if ge.embed_dim != model.config.embed_dim:
            raise RuntimeError(f"--voice {name}: gamma embed_dim {ge.embed_dim} != model dim {model.config.embed_dim}")
        if ge.num_tokens == 0:
            raise RuntimeError(f"--voice {name}: the file lists no tokens")
        try:
            model.set_voice(vid, ge.indices, ge.values)
        except ValueError as exc:
            raise RuntimeError(f"--voice {name}: {exc}") from exc
        model.voices[name] = vid
        print(f"[nanollama] voice {name!r} loaded: {ge.num_tokens} tokens modified")


MAX_MIXED_ROWS = 512         # rows of one mixed step (nl_mixed_capacity reports the handle's own limit, at most this)


def check_prefill_chunk(args, max_rows: int = MAX_MIXED_ROWS) -> None:
    """--prefill-chunk: needs the batched server, and parallel + chunk rows must fit one mixed step of the handle."""
    if args.prefill_chunk < 0:
        raise RuntimeError("--prefill-chunk must be >= 0")
    if args.prefill_chunk > 0 and not batched(args):
        raise RuntimeError("--prefill-chunk needs --serve --parallel N with N > 1")
    if args.prefill_chunk > 0 and args.parallel + args.prefill_chunk > max_rows:
        raise RuntimeError(f"--parallel {args.parallel} + --prefill-chunk {args.prefill_chunk} exceeds the {max_rows} rows of one "
                           f"mixed step: --prefill-chunk <= {max_rows - args.parallel}")


def check_parallel(args) -> None:
    """--parallel: 1 is the serial server; N > 1 needs one GPU (a device group has no batched sampler)."""
    if not 1 <= args.parallel <= 64:
        raise RuntimeError("--parallel must be in [1, 64]")
    if args.parallel > 1 and args.gpus > 1:
        raise RuntimeError("--parallel > 1 needs --gpus 1")
    if args.parallel > 1 and not 0 <= args.rep_window <= 1024:
        raise RuntimeError("--parallel > 1 needs --rep-window <= 1024")


def batched(args) -> bool:
    return bool(args.serve) and args.parallel > 1


def estimate_params(cfg) -> int:
    """estimateParams go/main.go:411-425"""
    embed = cfg.vocab_size * cfg.embed_dim
    attn = cfg.embed_dim * (cfg.num_heads * cfg.head_dim) + 2 * cfg.embed_dim * (cfg.num_kv_heads * cfg.head_dim) + \
        cfg.embed_dim * cfg.embed_dim
    mlp = 3 * cfg.embed_dim * cfg.interm_size
    return 2 * embed + cfg.num_layers * (attn + mlp + 2 * cfg.embed_dim) + cfg.embed_dim


def list_tensors(g) -> None:
    for name, info in g.tensors.items():
        dims = ", ".join(str(d) for d in info.dims[:info.ndims])
        print("  %-50s  type=%d  dims=[%s]  %.2f MB" % (name, info.type, dims, info.nbytes() / 1024 / 1024))


def load_engine(args) -> TextEngine:
    print(f"[nanollama] loading {args.model}")
    g = load_gguf(args.model, verbose=True)
    if args.gpus > 1:
        if args.gpus not in (2, 4, 8):
            raise RuntimeError("--gpus must be 1, 2, 4 or 8")
        devs = list(range(args.device, args.device + args.gpus))
        if os.environ.get("NL_GROUP_ONE_DEVICE"):      # test pool: every rank on --device (what a one-GPU box can run)
            devs = [args.device] * args.gpus
        print(f"[nanollama] tensor-parallel over devices {devs} (push all-reduce between the ranks of this process)")
        model = load_llama_model(g, devices=devs, verbose=True)
    else:
        model = load_llama_model(g, device=args.device, max_streams=args.parallel if batched(args) else max(getattr(args, "samples", 1), 1),
                                 verbose=True)
    if batched(args) and model.config.vocab_size > 131072:
        raise RuntimeError(f"--parallel > 1 covers vocabularies up to 131072, not {model.config.vocab_size}")
    if getattr(args, "samples", 1) > 1 and model.config.vocab_size > 131072:
        raise RuntimeError(f"--samples > 1 covers vocabularies up to 131072, not {model.config.vocab_size}")
    if args.gamma:
        from .gamma import load_gamma
        try:
            ge = load_gamma(args.gamma)
            if ge.embed_dim != model.config.embed_dim:
                print(f"warning: gamma embed_dim {ge.embed_dim} != model dim {model.config.embed_dim}, skipping", file=sys.stderr)
            else:
                model.set_gamma(ge.indices, ge.values)
                print(f"[nanollama] personality loaded: {ge.num_tokens} tokens modified")
        except ValueError as exc:
            print(f"warning: failed to load gamma: {exc}", file=sys.stderr)
    load_voices(model, args.voice)
    if args.use_voice:
        model.stream_voice(0, model.voices[args.use_voice])
    tok = Tokenizer(g.meta, verbose=True)
    eng = TextEngine(model, tok, rep_penalty=args.rep_penalty, rep_window=args.rep_window, seed=args.seed)
    print("[nanollama] ready — %dM params, %d layers, %d dim" % (estimate_params(model.config) // 1_000_000,
                                                                 model.config.num_layers, model.config.embed_dim))
    return eng


def run_repl(eng: TextEngine, params: GenParams) -> None:
    """runREPL go/main.go:428-459"""
    print("nanollama interactive mode. Type /quit to exit.\n")
    while True:
        try:
            text = input("> ").strip()
        except EOFError:
            return
        if not text:
            continue
        if text in ("/quit", "/exit"):
            return
        if text == "/info":
            c = eng.model.config
            print(f"Model: {c.num_layers} layers, {c.embed_dim} dim, {c.num_heads} heads, {c.num_kv_heads} kv_heads, {c.vocab_size} vocab")
            print("Params: ~%dM" % (estimate_params(c) // 1_000_000))
            print(f"Gamma: {eng.model.gamma is not None}")
            if getattr(eng.model, "voices", None):
                print(f"Voices: {', '.join(eng.model.voices)}")
            print(f"Flags: qk_norm={c.qk_norm} rope_conjugate={c.rope_conjugate}")
            continue
        eng.generate(text, params, stream=sys.stdout)
        print()


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if not args.model:
        print("Usage: nanollama --model <path.gguf> [--gamma <path.npz>] [--prompt <text>]", file=sys.stderr)
        build_parser().print_help(sys.stderr)
        return 1
    try:
        if args.list_tensors:
            list_tensors(load_gguf(args.model, verbose=True))
            return 0
        check_parallel(args)
        check_prefill_chunk(args)
        check_score(args)
        check_samples(args)
        check_voices(args)
        eng = load_engine(args)
        if args.prefill_chunk > 0:
            check_prefill_chunk(args, eng.model.mixed_capacity[0])
    except (GGUFError, OSError, RuntimeError, ImportError) as exc:
        print(f"error: {exc}", file=sys.stderr)
        return 1
    params = GenParams(max_tokens=args.max_tokens, temperature=args.temp, top_p=args.top_p, top_k=args.top_k)
    if args.score:
        try:
            run_score(eng, args.score)
        except (OSError, UnicodeDecodeError, RuntimeError) as exc:
            print(f"error: {exc}", file=sys.stderr)
            return 1
        return 0
    if args.serve:
        from .serve import run_server
        if batched(args):
            from .batch_serve import BatchScheduler
            sched = BatchScheduler(eng.model, eng.tokenizer, args.parallel, rep_penalty=args.rep_penalty,
                                   rep_window=args.rep_window, seed=args.seed, prefill_chunk=args.prefill_chunk)
            print(f"[nanollama] continuous batching: up to {args.parallel} requests per decode step" +
                  (f", prompts admitted in chunks of {args.prefill_chunk} tokens" if args.prefill_chunk else ""))
            try:
                run_server(sched, params, args.port)
            finally:
                sched.close()
            return 0
        run_server(eng, params, args.port)
    elif args.interactive:
        run_repl(eng, params)
    elif args.prompt and args.samples > 1:
        try:
            run_samples(eng, args.prompt, params, args)
        except RuntimeError as exc:
            print(f"error: {exc}", file=sys.stderr)
            return 1
    elif args.prompt:
        print(eng.generate(args.prompt, params, stream=sys.stdout))
    else:
        print("> ", end="", flush=True)
        for line in sys.stdin:
            text = line.strip()
            if text in ("/quit", "/exit"):
                break
            if text:
                print(eng.generate(text, params, stream=sys.stdout))
                print()
            print("> ", end="", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
