"""GPU tests of nl_kv_fork (include/nanollama_hip.h; KVCache.prefill, nanollama/engine.py:139-153): the K / V rows [0, n_pos) of
one stream copied into others in one launch.  The copy is held bitwise (nl_debug_read), the destinations' high-water marks
through the zeros a later jump must read, and every entry point must go on from a forked stream exactly as from a stream that
prefilled the prompt itself: equal rows, equal shapes and equal cache bits give bitwise-equal logits and ids, so
any difference is a fork defect.  One forked stream is also held to the oracle within the whole-forward bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nanollama_amd import gguf, synth
from nanollama_amd.engine import GenParams

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOGIT_TOL = 1e-4          # whole-forward logits against the oracle: <= LOGIT_TOL * max(1, std(logits)) (tests/test_gpu_parity.py)
NL_ERR_INVALID, NL_ERR_STATE = -1, -4


@pytest.fixture(scope="module")
def hip():
    from nanollama_amd import _lib, model
    if _lib.lib().nl_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return model


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ggufs(tmp_path_factory):
    """tiny q8_0: 2 layers, 2 kv heads, head_dim 32, seq_len 64; small_test q4_0: 3 layers, 3 kv heads, head_dim 64, seq_len 256"""
    p = str(tmp_path_factory.mktemp("fork") / "small_test_q4_0.gguf")
    synth.generate_gguf(p, synth.TIERS["small_test"], "q4_0", 211)
    return {"tiny": gguf.load_gguf(os.path.join(GOLDEN, "tiny_q8_0.gguf")), "small_test": gguf.load_gguf(p)}


@pytest.fixture(scope="module")
def handles(hip, ggufs):
    """one handle per (model, max_streams), shared by the tests that leave no state behind but K / V rows and marks"""
    made = {}

    def get(name, max_streams=4):
        if (name, max_streams) not in made:
            made[name, max_streams] = hip.load_llama_model(ggufs[name], max_streams=max_streams)
        return made[name, max_streams]
    yield get
    for h in made.values():
        h.close()


def _kv(dev, stream):
    """(K, V) of one stream as [layer][kv head][pos][head_dim]"""
    c = dev.config
    n = c.num_layers * c.num_kv_heads * c.seq_len * c.head_dim
    shape = (c.num_layers, c.num_kv_heads, c.seq_len, c.head_dim)
    return dev.debug_read("k_cache", n, stream).reshape(shape).copy(), dev.debug_read("v_cache", n, stream).reshape(shape).copy()


def _same(a, b):
    return a.tobytes() == b.tobytes()


# ---- the bits of the copy ---------------------------------------------------------------------------------------------------
# P: the shortest run (one position: 128 B at head_dim 32, 256 B at 64), runs that are no multiple of a workgroup's 16 KiB piece,
# the edges of the 128-key attention chunks, and the whole context
@pytest.mark.parametrize("name,P", [("small_test", 1), ("small_test", 2), ("small_test", 127), ("small_test", 128), ("small_test", 129),
                                    ("small_test", 255), ("small_test", 256), ("tiny", 1), ("tiny", 63)])
def test_rows_are_copied_bitwise_and_nothing_else_moves(handles, name, P):
    dev = handles(name, 5)
    vocab = dev.config.vocab_size
    for s in range(5):
        dev.reset(s)
    dev.prefill(synth.prompt_ids(7, vocab, seed=40 + P), stream=4, want_logits=False)       # a bystander with rows of its own
    for s, n in ((0, 3), (1, 5)):                                                              # destinations that held other rows
        dev.prefill(synth.prompt_ids(n, vocab, seed=s), stream=s, want_logits=False)
    dev.prefill(synth.prompt_ids(P, vocab, seed=P), stream=3, want_logits=False)
    before = {s: _kv(dev, s) for s in range(5)}
    assert before[3][0][:, :, :P].any() and before[3][1][:, :, :P].any()                       # the source holds real rows
    dev.kv_fork(3, [1, 0, 2], P)                                                               # the list is unordered
    after = {s: _kv(dev, s) for s in range(5)}
    for d in (0, 1, 2):
        for c in (0, 1):
            assert _same(after[d][c][:, :, :P], before[3][c][:, :, :P]), (name, P, d, "kv"[c])
            assert _same(after[d][c][:, :, P:], before[d][c][:, :, P:]), (name, P, d, "rows past n_pos were written")
    for s in (3, 4):
        assert _same(after[s][0], before[s][0]) and _same(after[s][1], before[s][1]), (name, P, s)


def test_the_highest_stream_of_four_forks_into_the_three_below(handles):
    dev = handles("small_test", 4)
    P = 129
    for s in range(4):
        dev.reset(s)
    dev.prefill(synth.prompt_ids(P, dev.config.vocab_size, seed=5), stream=3, want_logits=False)
    src = _kv(dev, 3)
    dev.kv_fork(3, [1, 0, 2], P)
    for d in (0, 1, 2):
        got = _kv(dev, d)
        assert _same(got[0][:, :, :P], src[0][:, :, :P]) and _same(got[1][:, :, :P], src[1][:, :, :P]), d
    again = _kv(dev, 3)
    assert _same(again[0], src[0]) and _same(again[1], src[1])


# ---- the mark ----------------------------------------------------------------------------------------------------------------
def test_a_destination_stands_at_n_pos_whatever_it_held(hip, ggufs):
    g = ggufs["tiny"]
    vocab = g.meta.vocab_size
    dev, fresh = hip.load_llama_model(g, max_streams=4), hip.load_llama_model(g, max_streams=4)
    try:
        eight, other = synth.prompt_ids(8, vocab, seed=3), synth.prompt_ids(40, vocab, seed=4)
        dev.prefill(other, stream=1, want_logits=False)                  # the destination ran to position 40
        dev.prefill(eight, stream=0, want_logits=False)
        dev.kv_fork(0, [1], 8)
        dev.forward(17, 11, stream=1)                                    # a legal jump: rows 8 .. 10 must read as zeros
        fresh.prefill(eight, stream=1, want_logits=False)
        fresh.forward(17, 11, stream=1)
        assert _same(dev.state.logits, fresh.state.logits)
        k = _kv(dev, 1)[0]
        assert not k[:, :, 8:11].any() and k[:, :, 11].any()
        # n_pos == 0 is nl_reset of the destination
        dev.kv_fork(0, [1], 0)
        dev.forward(23, 3, stream=1)
        fresh.reset(1)
        fresh.forward(23, 3, stream=1)
        assert _same(dev.state.logits, fresh.state.logits)
    finally:
        dev.close()
        fresh.close()


# ---- every entry point goes on from a fork as from its own prefill ----------------------------------------------------------------
def _prepare(dev, prompt, forked):
    for s in range(4):
        dev.reset(s)
    if forked:
        dev.prefill(prompt, stream=0, want_logits=False)
        dev.kv_fork(0, [1, 2, 3], len(prompt))
    else:
        for s in range(4):
            dev.prefill(prompt, stream=s, want_logits=False)


def _entry_points(dev, prompt, forked):
    """the same calls on either handle; everything they return, as bytes-comparable values"""
    P, vocab = len(prompt), dev.config.vocab_size
    toks = synth.prompt_ids(64, vocab, seed=77)
    out = {}
    _prepare(dev, prompt, forked)
    dev.forward(toks[0], P, stream=1)
    out["forward"] = dev.state.logits.copy()
    out["forward_argmax"] = dev.forward_argmax(toks[1], P + 1, stream=1)
    out["decode_greedy"] = dev.decode_greedy(toks[2], P, 12, stream=2)
    dev.forward(toks[3], P, stream=3)
    us = np.random.default_rng(11).random(6, dtype=np.float32)
    out["sample_decode"] = dev.sample_decode(P + 1, 6, 0.8, 0.9, 50, 1.15, 16, us, [], stream=3)
    _prepare(dev, prompt, forked)
    for i in range(6):
        ids, lg = dev.forward_batch([0, 1, 2, 3], toks[4 * i:4 * i + 4], [P + i] * 4, want_logits=True)
        out[f"forward_batch {i}"] = (ids, lg.copy())
    _prepare(dev, prompt, forked)
    params = [dict(temperature=t, top_p=p, top_k=20, rep_penalty=1.15, rep_window=8) for t, p in ((0.8, 0.9), (0.0, 1.0), (1.1, 1.0), (0.6, 0.95))]
    recents, feed = [[] for _ in range(4)], toks[:4]
    rng = np.random.default_rng(12)
    for i in range(6):
        ids, recents = dev.forward_batch_sample([0, 1, 2, 3], feed, [P + i] * 4, params, rng.random(4, dtype=np.float32), recents)
        out[f"forward_batch_sample {i}"] = (ids, [list(r) for r in recents])
        feed = ids
    _prepare(dev, prompt, forked)
    ids, lg = dev.forward_mixed([1, 2] + [3] * 5, [toks[0], toks[1]] + toks[10:15], [P, P] + list(range(P, P + 5)), 2, want_logits=True)
    out["forward_mixed"] = (ids, lg.copy(), _kv(dev, 3)[0][:, :, :P + 5].copy())
    _prepare(dev, prompt, forked)
    lp, am = dev.score(toks[20:26], toks[21:27], pos0=P, stream=1)
    out["score"] = (lp.copy(), am.copy())
    return out


def _flat(v):
    if isinstance(v, np.ndarray):
        return v.tobytes()
    if isinstance(v, (tuple, list)):
        return tuple(_flat(x) for x in v)
    return v


@pytest.mark.parametrize("name,P", [("tiny", 9), ("small_test", 130)])
def test_every_entry_point_continues_a_fork_as_its_own_prefill(hip, ggufs, name, P):
    prompt = synth.prompt_ids(P, ggufs[name].meta.vocab_size, seed=21)
    a, b = hip.load_llama_model(ggufs[name], max_streams=4), hip.load_llama_model(ggufs[name], max_streams=4)
    try:
        want, got = _entry_points(a, prompt, False), _entry_points(b, prompt, True)
    finally:
        a.close()
        b.close()
    assert list(want) == list(got)
    for key in want:
        assert _flat(want[key]) == _flat(got[key]), f"{name}: {key} differs between a forked stream and one that prefilled itself"


# ---- against the oracle ------------------------------------------------------------------------------------------------------------
def test_a_forked_stream_matches_the_oracle(handles, ggufs, orc):
    g = ggufs["tiny"]
    dev = handles("tiny", 4)
    seq = synth.prompt_ids(19, g.meta.vocab_size, seed=31)
    for s in range(4):
        dev.reset(s)
    dev.prefill(seq[:9], stream=0, want_logits=False)
    dev.kv_fork(0, [2], 9)
    ref = orc.OracleModel(g)
    for pos, t in enumerate(seq[:9]):
        ref.forward(t, pos)
    worst = 0.0
    for pos in range(9, 19):
        want = ref.forward(seq[pos], pos)
        dev.forward(seq[pos], pos, stream=2)
        worst = max(worst, float(np.abs(dev.state.logits - want).max()) / max(1.0, float(want.std())))
    ref.close()
    print(f"\nforked stream, 10 forced tokens: max|gpu-oracle| / max(1, std) = {worst:.2e} of {LOGIT_TOL}")
    assert worst <= LOGIT_TOL


# ---- cached graphs -----------------------------------------------------------------------------------------------------------------
def test_the_fork_is_data_to_a_cached_step_graph(hip, ggufs):
    g = ggufs["tiny"]
    vocab = g.meta.vocab_size
    first, prompt, feed = synth.prompt_ids(4, vocab, seed=1), synth.prompt_ids(9, vocab, seed=2), synth.prompt_ids(4, vocab, seed=3)
    a, b = hip.load_llama_model(g, max_streams=4), hip.load_llama_model(g, max_streams=4)
    try:
        for dev in (a, b):                               # the 4-row step twice: its graph is cached
            dev.forward_batch([0, 1, 2, 3], first, [0] * 4)
            dev.forward_batch([0, 1, 2, 3], first, [1] * 4)
        _prepare(a, prompt, False)
        _prepare(b, prompt, True)
        want, got = a.forward_batch([0, 1, 2, 3], feed, [9] * 4, want_logits=True), b.forward_batch([0, 1, 2, 3], feed, [9] * 4, want_logits=True)
    finally:
        a.close()
        b.close()
    assert want[0] == got[0] and _same(want[1], got[1])


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_errors_come_before_any_work_and_change_nothing(hip, ggufs):
    import ctypes as C
    from nanollama_amd import _lib
    g = ggufs["tiny"]
    vocab = g.meta.vocab_size
    dev, twin = hip.load_llama_model(g, max_streams=4), hip.load_llama_model(g, max_streams=4)
    try:
        for d in (dev, twin):
            d.prefill(synth.prompt_ids(9, vocab, seed=5), stream=0, want_logits=False)
            d.prefill(synth.prompt_ids(40, vocab, seed=6), stream=1, want_logits=False)
        before = [_kv(dev, s) for s in range(4)]
        cases = [(-1, [1], 4, "-1"), (4, [1], 4, "4"), (0, [1, 4], 4, "4"), (0, [-2], 4, "-2"), (0, [1, 0], 4, "0"), (0, [1, 2, 1], 4, "1"),
                 (0, [], 0, "0"), (0, [1, 2, 3, 1], 4, "4"), (0, [1], -1, "-1"), (0, [1], 65, "65"), (0, [1], 10, "10"), (2, [1], 1, "1")]
        for src, dst, n_pos, names in cases:
            with pytest.raises(_lib.NlError) as ei:
                dev.kv_fork(src, dst, n_pos)
            assert ei.value.code == NL_ERR_INVALID and names in dev.last_error() and "nl_kv_fork" in dev.last_error(), (src, dst, n_pos, dev.last_error())
            for s in range(4):
                now = _kv(dev, s)
                assert _same(now[0], before[s][0]) and _same(now[1], before[s][1]), (src, dst, n_pos, s)
        assert _lib.lib().nl_kv_fork(dev._h, 0, None, 1, 4) == NL_ERR_INVALID and "null" in dev.last_error()
        # the marks too: stream 1 still stands at 40 (a step there attends over its own 40 rows), stream 0 at 9
        for s, pos in ((1, 40), (0, 9)):
            dev.forward(33, pos, stream=s)
            twin.forward(33, pos, stream=s)
            assert _same(dev.state.logits, twin.state.logits), s
    finally:
        dev.close()
        twin.close()
    # before nl_finalize
    L = _lib.lib()
    cfg = _lib.NlConfig(2, 128, 4, 2, 32, 512, 512, 64, 1e-5, 10000.0, 0, 0, 4, 0, 0, 1, 0)
    h = C.c_void_p()
    assert L.nl_create(C.byref(cfg), C.byref(h)) == 0
    try:
        assert L.nl_kv_fork(h, 0, (C.c_int * 1)(1), 1, 0) == NL_ERR_STATE
        assert b"nl_finalize" in L.nl_last_error(h)
    finally:
        L.nl_destroy(h)


# ---- voices ------------------------------------------------------------------------------------------------------------------------
def test_voice_bindings_are_not_touched(hip, ggufs):
    g = ggufs["tiny"]
    dev = hip.load_llama_model(g, max_streams=4)
    try:
        rng = np.random.default_rng(8)
        idx = np.array([5, 9, 70], dtype=np.int32)
        for v in (1, 2):
            dev.set_voice(v, idx, (rng.standard_normal((3, g.meta.embed_dim)) * 0.3).astype(np.float32))
        dev.stream_voice(2, 1)
        dev.stream_voice(0, 2)
        dev.prefill([1, 5, 9, 70, 3], stream=0, want_logits=False)
        dev.kv_fork(0, [2, 3], 5)
        assert [dev.voice_info(s)["voice"] for s in range(4)] == [2, 0, 1, 0]
    finally:
        dev.close()


# ---- persistent decode -------------------------------------------------------------------------------------------------------------
def test_a_fork_ends_a_resident_session_and_both_streams_go_on(hip, tmp_path):
    shape = synth.ModelShape("pd_fork", 5, 256, 4, 4, 2048, seq_len=256, interm=512)       # tests/test_gpu_persist.py's small shape
    p = str(tmp_path / "m.gguf")
    synth.generate_gguf(p, shape, "q8_0", 131)
    g = gguf.load_gguf(p)
    dev, own = hip.load_llama_model(g, max_streams=2), hip.load_llama_model(g, max_streams=2)
    try:
        if not dev.persist_info()["ready"]:
            pytest.skip("persist_info: the persistent decode is not ready on this device")
        toks = synth.prompt_ids(20, shape.vocab, seed=3)
        for pos, t in enumerate(toks):
            last = dev.forward_argmax(t, pos, stream=0)                   # steps of one resident session
        launches = dev.persist_info()["launches"]
        dev.kv_fork(0, [1], 20)
        assert "retire" not in dev.last_error(), dev.last_error()
        got, t0 = [], last
        for i in range(8):                                                # stream 0 goes on from 20 ...
            t0 = dev.forward_argmax(t0, 20 + i, stream=0)
            got.append(t0)
        info = dev.persist_info()
        assert info["launches"] > launches, (launches, info)             # ... through a NEW session: the fork ended the one before
        ids = dev.decode_greedy(last, 20, 16, stream=1)
        assert "retire" not in dev.last_error(), dev.last_error()
        for s in (1, 0):                                                  # the witness: both streams fed the 20 tokens themselves
            for pos, t in enumerate(toks):
                want_last = own.forward_argmax(t, pos, stream=s)
        assert last == want_last
        want, t1 = [], last
        for i in range(8):
            t1 = own.forward_argmax(t1, 20 + i, stream=0)
            want.append(t1)
        assert got == want
        assert ids == own.decode_greedy(last, 20, 16, stream=1)
    finally:
        dev.close()
        own.close()


# ---- group -------------------------------------------------------------------------------------------------------------------------
GROUP_WORKER = r"""
import sys
import numpy as np
sys.path.insert(0, {root!r})
from nanollama_amd import gguf, model, synth
g = gguf.load_gguf(sys.argv[1])
vocab = g.meta.vocab_size
prompt, feed = synth.prompt_ids(6, vocab, seed=9), synth.prompt_ids(4, vocab, seed=10)
runs = []
for forked in (False, True):
    grp = model.load_llama_model(g, devices=[0, 0], max_streams=2)
    grp.prefill(prompt, stream=0, want_logits=False)
    if forked:
        grp.kv_fork(0, [1], len(prompt))
    else:
        grp.prefill(prompt, stream=1, want_logits=False)
    out = []
    for i, t in enumerate(feed):
        grp.forward(t, len(prompt) + i, stream=1)
        out.append(grp.state.logits.tobytes())
    assert grp.last_error() == "", grp.last_error()
    try:
        grp.kv_fork(0, [0], 1)
        raise SystemExit("a destination equal to the source was accepted")
    except model._lib.NlError as exc:
        assert exc.code == -1, exc
    grp.close()
    runs.append(out)
assert runs[0] == runs[1], "a forked stream of a group differs from one that prefilled itself"
print("group fork ok")
"""


def test_group_leader_forks_on_every_rank(tmp_path):
    # a fresh process with GPU_MAX_HW_QUEUES >= ranks, as tests/test_gpu_group.py: the ranks share ONE device here
    shape = synth.ModelShape("grp_fork", 3, 1024, 16, 4, 4096, seq_len=64, interm=2048)
    p = str(tmp_path / "m.gguf")
    synth.generate_gguf(p, shape, "q4_0", 61, mode="qrand")
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8", NL_P2P_TIMEOUT_MS="5000")
    r = subprocess.run([sys.executable, "-c", GROUP_WORKER.format(root=ROOT), p], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "group fork ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- the scheduler, end to end -----------------------------------------------------------------------------------------------------
class CharTokenizer:
    """The tiny model's pieces for decoding; a prompt becomes one id per character."""

    def __init__(self, tok, vocab):
        self.tok, self.vocab, self.eos_id = tok, vocab, tok.eos_id

    def encode(self, text, add_bos=True):
        return ([1] if add_bos else []) + [3 + ord(c) % (self.vocab - 3) for c in text]

    def decode_token_bytes(self, t):
        return self.tok.decode_token_bytes(t)


class Counting:
    """the model as the scheduler sees it, counting its calls"""

    def __init__(self, model):
        self._m, self.count = model, {}

    def __getattr__(self, name):
        attr = getattr(self._m, name)
        if not callable(attr):
            return attr

        def call(*a, **kw):
            self.count[name] = self.count.get(name, 0) + 1
            return attr(*a, **kw)
        return call


def test_scheduler_draws_three_samples_from_one_prefill(hip, ggufs):
    from nanollama_amd.batch_serve import BatchScheduler
    from nanollama_amd.tokenizer import Tokenizer
    g = ggufs["tiny"]
    tok = CharTokenizer(Tokenizer(g.meta), g.meta.vocab_size)
    dev = hip.load_llama_model(g, max_streams=4)
    m = Counting(dev)
    s = BatchScheduler(m, tok, 4, rep_penalty=1.15, rep_window=16, seed=7)
    s.eos_id = -1                                        # (no id ends a row early: every text has max_tokens pieces)
    try:
        prompt = "the quick brown fox"
        greedy = GenParams(max_tokens=12, temperature=0.0)
        one = s.generate_quiet(prompt, greedy)
        assert m.count.get("kv_fork", 0) == 0
        three = s.generate_samples(prompt, greedy, 3)
        assert three == [one] * 3                        # greedy rows of one prompt must agree
        m.count.clear()
        texts = s.generate_samples(prompt, GenParams(max_tokens=12, temperature=0.8, top_p=0.9, top_k=50), 3)
        assert len(texts) == 3 and all(isinstance(t, str) and t for t in texts)
        assert m.count["prefill"] == 1 and m.count["kv_fork"] == 1 and m.count["reset"] == 1
        assert m.count["forward_batch_sample"] == 12
    finally:
        s.close()
        dev.close()
