"""Host side of voices (--voice / --use-voice, "voice" in POST /chat and POST /score, /health, BatchScheduler) with stand-in
models that record every call: which stream was bound to which voice, and that the bind came before the first step that
carried the stream's rows.  No GPU."""
import contextlib
import threading
from types import SimpleNamespace

import numpy as np
import pytest

from nanollama_amd import _lib, cli, serve
from nanollama_amd.batch_serve import BatchScheduler, RequestError
from nanollama_amd.engine import GenParams

NOLOCK = contextlib.nullcontext()
EOS = 2


class FakeTokenizer:
    eos_id = EOS

    def encode(self, text, add_bos=True):
        return ([1] if add_bos else []) + [3 + (ord(c) % 40) for c in text]

    def decode_token_bytes(self, t):
        return bytes([97 + t % 26])


class FakeModel:
    """Records every call in order.  Steps check that each row's stream carries the voice its request asked for:
    `expect` maps a prompt's first content token to the voice id its rows must run under."""

    def __init__(self, voices=None, max_streams=4, seq_len=64):
        self.max_streams = max_streams
        self.config = SimpleNamespace(seq_len=seq_len, vocab_size=512, num_layers=1, embed_dim=8, num_heads=1, num_kv_heads=1,
                                      head_dim=8, interm_size=8, qk_norm=False, rope_conjugate=False)
        self.gamma = None
        self.voices = dict(voices or {})
        self.bound = {}           # stream -> voice
        self.calls = []
        self.rows = []            # (stream, voice at the time) of every row of every step / prefill / score
        self.gate = None
        self.mu = threading.Lock()

    @property
    def mixed_capacity(self):
        return 512, 64

    def reset(self, stream):
        self.calls.append(("reset", stream))

    def stream_voice(self, stream, voice):
        assert 0 <= stream < self.max_streams and (voice == 0 or voice in self.voices.values())
        self.calls.append(("bind", stream, voice))
        self.bound[stream] = voice

    def _note(self, streams):
        for s in streams:
            self.rows.append((s, self.bound.get(s, 0)))

    def prefill(self, tokens, pos0=0, stream=0, want_logits=True):
        self.calls.append(("prefill", stream))
        self._note([stream])

    def score(self, tokens, targets, pos0=0, stream=0):
        self.calls.append(("score", stream))
        self._note([stream])
        return np.full(len(tokens), -1.0, np.float32), np.zeros(len(tokens), np.int32)

    def _step(self, streams, tokens, params, recents, n_out):
        if self.gate is not None:
            self.gate.wait(5)
        self.calls.append(("step", list(streams)))
        self._note(streams)
        ids = [3 + (t + 1) % 40 for t in tokens[:n_out]]
        return ids, [list(r) + [i] for r, i in zip(recents, ids)]

    def forward_batch_sample(self, streams, tokens, pos, params, uniforms, recents):
        return self._step(streams, tokens, params, recents, len(streams))

    def forward_mixed_sample(self, streams, tokens, pos, n_out, params, uniforms, recents):
        return self._step(streams, tokens, params, recents, n_out)


class FakeEngine:
    """the one-caller engine of the serial server (TextEngine's surface)"""

    def __init__(self, voices=None):
        self.model = FakeModel(voices, max_streams=1)
        self.tokenizer = FakeTokenizer()

    def generate_quiet(self, prompt, params):
        self.model.calls.append(("generate", prompt, self.model.bound.get(0, 0)))
        return "echo:" + prompt


VOICES = {"leo": 1, "yent": 2}


def test_voice_flag_parsing_and_errors(capsys):
    a = cli.build_parser().parse_args(["--model", "m.gguf"])
    assert a.voice == [] and a.use_voice == "" and cli.parse_voices(a.voice) == []
    a = cli.build_parser().parse_args(["--model", "m.gguf", "--voice", "leo=/tmp/leo.npz", "--voice", "yent=a=b.npz", "--use-voice", "yent"])
    assert cli.parse_voices(a.voice) == [("leo", "/tmp/leo.npz"), ("yent", "a=b.npz")]       # (the first '=' separates)
    cli.check_voices(a)
    for bad in (["leo"], ["=x.npz"], ["leo="], [" =x.npz"], ["leo=a.npz", "leo=b.npz"]):
        with pytest.raises(RuntimeError):
            cli.parse_voices(bad)
    cli.parse_voices([f"v{i}=f.npz" for i in range(63)])
    with pytest.raises(RuntimeError):
        cli.parse_voices([f"v{i}=f.npz" for i in range(64)])                                  # voices 1 .. 63
    with pytest.raises(RuntimeError):
        cli.check_voices(cli.build_parser().parse_args(["--model", "m", "--voice", "leo=l.npz", "--use-voice", "nobody"]))
    with pytest.raises(RuntimeError):
        cli.check_voices(cli.build_parser().parse_args(["--model", "m", "--voice", "leo=l.npz", "--use-voice", "leo", "--serve"]))
    # a bad spec ends the run before anything is loaded: exit 1 and an "error:" line, as the other flag errors
    assert cli.main(["--model", "/nonexistent.gguf", "--voice", "noequals"]) == 1
    assert "error: --voice takes NAME=PATH" in capsys.readouterr().err
    assert cli.main(["--model", "/nonexistent.gguf", "--voice", "a=x.npz", "--use-voice", "b"]) == 1
    assert "--use-voice 'b' is not among" in capsys.readouterr().err


def test_load_voices_defines_ids_in_order_and_refuses_bad_files(tmp_path):
    calls = []
    model = SimpleNamespace(config=SimpleNamespace(embed_dim=8), voices={},
                            set_voice=lambda v, i, x: calls.append((v, list(i), x.shape, x.dtype)))
    for name, dt in (("a", np.float32), ("b", np.float16)):
        np.savez(tmp_path / f"{name}.npz", indices=np.array([3, 5], np.int32), values=np.ones((2, 8), dt),
                 vocab_size=np.array(512), embed_dim=np.array(8))
    cli.load_voices(model, [f"leo={tmp_path / 'a.npz'}", f"yent={tmp_path / 'b.npz'}"])
    assert model.voices == {"leo": 1, "yent": 2}
    assert calls == [(1, [3, 5], (2, 8), np.float32), (2, [3, 5], (2, 8), np.float16)]
    np.savez(tmp_path / "wide.npz", indices=np.array([3], np.int32), values=np.ones((1, 16), np.float32),
             vocab_size=np.array(512), embed_dim=np.array(16))
    for bad in (f"x={tmp_path / 'missing.npz'}", f"x={tmp_path / 'wide.npz'}"):
        with pytest.raises(RuntimeError):
            cli.load_voices(SimpleNamespace(config=SimpleNamespace(embed_dim=8), voices={}, set_voice=lambda *a: None), [bad])


def test_handle_chat_and_score_bind_stream_0_before_generation():
    eng, lock, d = FakeEngine(VOICES), threading.Lock(), GenParams()
    st, out = serve.handle_chat(eng, d, lock, b'{"messages":[{"content":"hi"}],"voice":"yent"}')
    assert (st, out) == (200, {"response": "echo:hi"})
    assert eng.model.calls == [("bind", 0, 2), ("generate", "hi", 2)]
    st, out = serve.handle_chat(eng, d, lock, b'{"messages":[{"content":"yo"}]}')          # absent: the default voice again
    assert st == 200 and eng.model.calls[-2:] == [("bind", 0, 0), ("generate", "yo", 0)]
    for body in (b'{"messages":[{"content":"hi"}],"voice":"nobody"}', b'{"messages":[{"content":"hi"}],"voice":7}',
                 b'{"messages":[],"voice":"nobody"}'):
        n = len(eng.model.calls)
        st, out = serve.handle_chat(eng, d, lock, body)
        assert st == 400 and isinstance(out, dict) and "unknown voice" in out["error"] and len(eng.model.calls) == n
    st, out = serve.handle_score(eng, lock, b'{"text":"abc","voice":"leo"}')
    assert st == 200 and out["tokens"] == 3
    i = eng.model.calls.index(("bind", 0, 1))
    assert ("score", 0) in eng.model.calls[i:] and ("score", 0) not in eng.model.calls[:i]
    assert eng.model.rows[-1] == (0, 1)
    st, out = serve.handle_score(eng, lock, b'{"text":"abc","voice":"nobody"}')
    assert st == 400 and "unknown voice" in out["error"]
    # a server without named voices: no bind is ever sent, a named voice is unknown
    bare = FakeEngine()
    assert serve.handle_chat(bare, d, lock, b'{"messages":[{"content":"hi"}]}')[0] == 200
    assert bare.model.calls == [("generate", "hi", 0)]
    assert serve.handle_chat(bare, d, lock, b'{"messages":[{"content":"hi"}],"voice":"leo"}')[0] == 400


def test_health_lists_the_voices_and_keeps_the_old_keys():
    old = {"status", "params_millions", "layers", "dim", "heads", "kv_heads", "vocab_size", "gamma_loaded"}
    h = serve.handle_health(FakeEngine(VOICES))
    assert old <= set(h) and h["voices"] == ["leo", "yent"] and h["gamma_loaded"] is False
    assert set(serve.handle_health(FakeEngine())) == old           # no named voices: the reference's keys, nothing else
    sched = BatchScheduler(FakeModel(VOICES), FakeTokenizer(), 2)
    try:
        h = serve.handle_health(sched)
        assert old | {"steps", "prefill_chunk", "max_step_gap_ms"} <= set(h) and h["voices"] == ["leo", "yent"]
    finally:
        sched.close()


def _first_use(model, stream, start):
    """index of the first call from `start` on that carried rows of `stream`"""
    for i in range(start, len(model.calls)):
        c = model.calls[i]
        if (c[0] in ("prefill", "score") and c[1] == stream) or (c[0] == "step" and stream in c[1]):
            return i
    return None


@pytest.mark.parametrize("prefill_chunk", [0, 4])
def test_scheduler_binds_each_request_to_its_stream_before_its_first_rows(prefill_chunk):
    m = FakeModel(VOICES, max_streams=2)
    s = BatchScheduler(m, FakeTokenizer(), 2, seed=1, prefill_chunk=prefill_chunk)
    want = [("hello there", 1), ("abc", 2), ("more text here", 0), ("x", 2), ("yy", 1)]      # 5 requests over 2 streams: reuse
    out = [None] * len(want)
    try:
        def go(i):
            out[i] = s.generate_quiet(want[i][0], GenParams(max_tokens=4, temperature=0.0), voice=want[i][1])
        ths = [threading.Thread(target=go, args=(i,)) for i in range(len(want))]
        for t in ths:
            t.start()
        for t in ths:
            t.join(10)
        sc = s.score(FakeTokenizer().encode("scored"), 1, voice=2)
        assert sc.n_tokens == 6
        with pytest.raises(RequestError) as exc:
            s.generate_quiet("hi", GenParams(max_tokens=2, temperature=0.0), voice=9)
        assert exc.value.status == 400
        with pytest.raises(RequestError):
            s.score([1, 5, 6], 1, voice=9)
    finally:
        s.close()
    assert all(o is not None and len(o) == 4 for o in out)
    binds = [(i, c) for i, c in enumerate(m.calls) if c[0] == "bind"]
    assert len(binds) == len(want) + 1 and sorted(c[2] for _, c in binds) == sorted([v for _, v in want] + [2])
    for i, (_, stream, voice) in binds:
        assert m.calls[i - 1] == ("reset", stream)                 # admission: reset, bind, then the stream's rows
        nxt = _first_use(m, stream, i + 1)
        assert nxt is not None
        # no row of the stream between its reset and the bind, and every row up to the stream's next reset runs under this voice
    cur = {}
    rows = iter(m.rows)
    for c in m.calls:
        if c[0] == "bind":
            cur[c[1]] = c[2]
        elif c[0] in ("prefill", "score"):
            assert next(rows) == (c[1], cur[c[1]])
        elif c[0] == "step":
            for st in c[1]:
                assert next(rows) == (st, cur[st])


def test_two_concurrent_requests_with_different_voices_bind_two_streams():
    m = FakeModel(VOICES, max_streams=2)
    m.gate = threading.Event()
    s = BatchScheduler(m, FakeTokenizer(), 2, seed=1)
    out = {}
    try:
        ths = [threading.Thread(target=lambda n=n, v=v: out.__setitem__(n, s.generate_quiet("hello " + n, GenParams(max_tokens=6, temperature=0.0), voice=v)))
               for n, v in VOICES.items()]
        for t in ths:
            t.start()
        m.gate.set()
        for t in ths:
            t.join(10)
    finally:
        s.close()
    assert set(out) == set(VOICES)
    binds = [c for c in m.calls if c[0] == "bind"]
    assert sorted(c[2] for c in binds) == [1, 2] and len({c[1] for c in binds}) == 2          # two voices, two streams
    both = [c for c in m.calls if c[0] == "step" and len(c[1]) == 2]
    assert both                                                                                # ... that shared steps
    assert {(st, v) for st, v in m.rows if v} == {(c[1], c[2]) for c in binds}


def test_a_scheduler_without_named_voices_sends_no_bind():
    m = FakeModel(max_streams=2)
    s = BatchScheduler(m, FakeTokenizer(), 2, seed=1)
    try:
        assert len(s.generate_quiet("abc", GenParams(max_tokens=3, temperature=0.0))) == 3
    finally:
        s.close()
    assert not [c for c in m.calls if c[0] == "bind"]


def test_abi_names_are_exported():
    for name in ("nl_set_voice", "nl_stream_voice", "nl_voice_info"):
        assert name in _lib.EXPORTS
    assert _lib.NL_MAX_VOICES == 64
