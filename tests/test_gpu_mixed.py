"""GPU tests of mixed steps (nl_forward_mixed / nl_forward_mixed_sample, nanollama_amd/csrc/nl_engine.hip; the segment-tile
attention kernel attn_seg_kernel, nl_batch.h): one step carries the decode rows of running requests AND chunks of the prompts
being admitted, a stream appearing once per row.  Reference: go/main.go:160-166 (a prompt goes through Forward token by token),
go/main.go:173-219 (decode), go/model.go:490-620 (Forward) -- per stream, the rows of a step must be what Forward gives in
ascending position order.  Every output row is held to the oracle; NL_MIXED_ATTN=0 (every row on the per-token attention
kernel), NL_DGEMM=0 and a Q8_0 file are further witnesses.

Tolerance (the project's): max|gpu - oracle| <= 1e-4 * max(1, std(oracle row)).  An id is compared with the oracle's argmax
where the oracle's top-2 gap exceeds 10 * 1e-4 * max(1, std); each test asserts that at most 2 % of the compared rows are left
out by that gate."""
import os
import sys

import numpy as np
import pytest

from nanollama_amd import gguf, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_mirror as sm  # noqa: E402

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
GATE_CAP = 0.02


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


@pytest.fixture(autouse=True)
def tile_kernel_for_every_segment(monkeypatch):
    # By default a step's prompt segments take the segment-tile kernel only from NL_MIXED_ATTN_MIN = 512 (row, visible chunk)
    # pairs on (below that the per-token kernel is faster); the small steps of these tests would never reach it.
    monkeypatch.setenv("NL_MIXED_ATTN_MIN", "0")


MX_A = synth.ModelShape("mx_a", 2, 256, 4, 2, 512, seq_len=320, interm=512)          # head_dim 64, GQA 2: query tile 32
SHAPES = {
    # as test_gpu_dgemm.SHAPES: head_dim 32 / GQA 8 (query tile 8) and MHA head_dim 64 (query tile 64), longer contexts here
    "hd32_gqa8": synth.ModelShape("mx_d", 1, 1024, 32, 4, 512, seq_len=192, interm=3072),
    "mha_hd64": synth.ModelShape("mx_b", 2, 512, 8, 8, 512, seq_len=192, interm=1024, rope_conjugate=True),
}
# token seeds of the shortened schedules: chosen on the CPU with the oracle alone so that the share of output rows under the argmax
# gate stays below the 2 % cap
TOKEN_SEEDS = {"hd32_gqa8": 11, "mha_hd64": 11, "gqa6": 11}
QUERY_TILE = {1: 64, 2: 32, 8: 8, 3: 16, 4: 16}      # rows of one segment a workgroup of attn_seg_kernel takes, by GQA factor


def _gguf(tmp_path, shape, wtype="q4_0", seed=307):
    p = tmp_path / f"{shape.name}_{wtype}.gguf"
    if not p.exists():
        synth.generate_gguf(str(p), shape, wtype, seed)
    return gguf.load_gguf(str(p))


class Schedule:
    """A teacher-forced serving run: `decode` streams stand at a position (their history goes through nl_forward), `prompts`
    (stream, n_prompt, arrival step) are admitted in list order with a per-step budget of non-output rows.  Every step:
    the decoding streams as output rows, then the budget's worth of prompt tokens in admission order; the final prompt token
    joins as an output row in the step that feeds the last of the tokens before it.  `tail` more steps after the last prompt
    is in."""

    def __init__(self, vocab, decode, prompts, budget=48, budgets=None, tail=8, token_seed=11, length=300):
        rng = np.random.Generator(np.random.PCG64(token_seed))
        self.streams = sorted(list(decode) + [s for s, _, _ in prompts])
        self.seqs = {s: [int(t) for t in rng.integers(3, vocab, size=length)] for s in range(max(self.streams) + 1)}
        self.decode = dict(decode)
        self.steps = []          # (streams, tokens, pos, n_out)
        self.segments = []       # (first position, rows) of the runs of non-output rows, over all steps
        pos = dict(decode)       # decoding streams -> next position
        fed = {s: 0 for s, _, _ in prompts}
        waiting = list(prompts)
        k, left = 0, None
        while True:
            b = (budgets or {}).get(k, budget)
            out, chunk = sorted(pos), []
            for s, n_prompt, arrival in waiting:
                if arrival > k or b == 0 or s in pos:
                    continue
                take = min(n_prompt - 1 - fed[s], b)
                if take:
                    chunk.append((s, fed[s], take))
                    self.segments.append((fed[s], take))
                fed[s] += take
                b -= take
                if fed[s] == n_prompt - 1:
                    out.append(s)
                    pos[s] = n_prompt - 1
            rows = [(s, pos[s]) for s in out] + [(s, p) for s, p0, t in chunk for p in range(p0, p0 + t)]
            self.steps.append(([s for s, _ in rows], [self.seqs[s][p] for s, p in rows], [p for _, p in rows], len(out)))
            for s in out:
                pos[s] += 1
            k += 1
            if all(s in pos for s, _, _ in waiting):
                left = tail if left is None else left - 1
                if left <= 0:
                    break
        self.end = dict(pos)     # positions written per stream


def _oracle_logits(orc, g, sched):
    orc.set_threads(min(16, os.cpu_count() or 1))
    refs = {}
    for s in sched.streams:
        ref = orc.OracleModel(g)
        refs[s] = [ref.forward(t, p).copy() for p, t in enumerate(sched.seqs[s][:sched.end[s]])]
        ref.close()
    orc.set_threads(1)
    return refs


def _history(dev, sched):
    for s, p0 in sched.decode.items():
        for p in range(p0):
            dev.forward(sched.seqs[s][p], p, stream=s)


def _run(dev, sched):
    """the schedule on a handle: per step (ids, logits of the output rows)"""
    out = []
    for streams, tokens, pos, n_out in sched.steps:
        ids, lg = dev.forward_mixed(streams, tokens, pos, n_out, want_logits=True)
        out.append((ids, lg.copy()))
    return out


def _check(sched, got, refs, what):
    """every output row of every step against the oracle; returns the worst relative difference"""
    worst, rows, gated = 0.0, 0, 0
    for k, ((streams, _, pos, n_out), (ids, lg)) in enumerate(zip(sched.steps, got)):
        for i in range(n_out):
            want = refs[streams[i]][pos[i]]
            scale = max(1.0, float(want.std()))
            worst = max(worst, float(np.abs(lg[i] - want).max()) / scale)
            top2 = np.partition(want, -2)[-2:]
            rows += 1
            if float(top2[1] - top2[0]) > 10 * LOGIT_TOL * scale:
                assert ids[i] == int(np.argmax(want)), (what, k, i, streams[i], pos[i])
            else:
                gated += 1
    print(f"\n{what}: {len(sched.steps)} steps, {rows} output rows, max|gpu-oracle| = {worst:.2e} (relative), "
          f"{gated} rows under the argmax gate")
    assert gated <= GATE_CAP * rows, (what, gated, rows)
    assert worst <= LOGIT_TOL, (what, worst)
    return worst


def _main_schedule(vocab):
    # streams 0-2 decode from 5, 126 (crosses 128) and 200; prompts of 40, 150 and 290 tokens in chunks of 48 (one step's budget
    # is 32: a segment equal to the query tile of this shape).  Step 0: decode rows only.  Step 1: the 39 rows of stream 3 (longer
    # than the tile) + its final token as an output row + the first 9 rows of stream 4 (shorter).  Step 4: the tail of stream 4
    # (positions 105..148, across 128) + its final token + the head of stream 5.  Stream 5's chunks cross 128 and 256.
    sched = Schedule(vocab, {0: 5, 1: 126, 2: 200}, [(3, 40, 1), (4, 150, 1), (5, 290, 4)], budget=48, budgets={6: 32})
    tile = QUERY_TILE[2]
    assert sched.steps[0][3] == len(sched.steps[0][0]) == 3                          # decode rows only
    lens = [n for _, n in sched.segments]
    assert any(n < tile for n in lens) and any(n == tile for n in lens) and any(n > tile for n in lens)
    for edge in (128, 256):                                                          # a chunk with rows on both sides
        assert any(p0 < edge < p0 + n for p0, n in sched.segments), edge
    assert any(n_out < len(st) and len(set(st[n_out:])) == 2 for st, _, _, n_out in sched.steps)   # a tail and the next head
    return sched


def test_ragged_schedule_matches_oracle_and_replays_bitwise(hip, orc, tmp_path):
    g = _gguf(tmp_path, MX_A)
    sched = _main_schedule(MX_A.vocab)
    refs = _oracle_logits(orc, g, sched)
    dev = hip.load_llama_model(g, max_streams=6)
    assert dev.mixed_capacity == (320, 64)
    _history(dev, sched)
    got = _run(dev, sched)
    _check(sched, got, refs, "ragged schedule, q4_0")
    # K / V rows written by non-output rows: against a handle fed token by token
    twin = hip.load_llama_model(g, max_streams=6)
    L, KV, hd, S = MX_A.n_layer, MX_A.n_kv_head, MX_A.head_dim, MX_A.seq_len
    for s in (3, 4, 5):
        for p in range(sched.end[s]):
            twin.forward(sched.seqs[s][p], p, stream=s)
        for which in ("k_cache", "v_cache"):
            a = dev.debug_read(which, L * KV * S * hd, stream=s).reshape(L, KV, S, hd)[:, :, :sched.end[s]]
            b = twin.debug_read(which, L * KV * S * hd, stream=s).reshape(L, KV, S, hd)[:, :, :sched.end[s]]
            d = float(np.abs(a - b).max()) / max(1.0, float(b.std()))
            print(f"{which} of stream {s}: max|mixed - token by token| = {d:.2e} (relative)")
            assert d <= LOGIT_TOL, (which, s, d)
    twin.close()
    # determinism: the schedule again from reset, on the same handle (the cached step graphs): bitwise
    for s in sched.streams:
        dev.reset(s)
    _history(dev, sched)
    again = _run(dev, sched)
    for k, ((ids, lg), (ids2, lg2)) in enumerate(zip(got, again)):
        assert ids == ids2 and lg.tobytes() == lg2.tobytes(), k
    dev.close()


def test_witnesses_per_token_attention_split_k_gemms_and_q8_0(hip, orc, tmp_path, monkeypatch):
    """Each variant is held to the oracle on its own; the largest differences between them are printed, not
    asserted."""
    sched = _main_schedule(MX_A.vocab)
    outs = {}
    TILE, PER_TOKEN, SPLIT_K, THRESHOLD = "tile kernel", "NL_MIXED_ATTN=0", "NL_DGEMM=0", "NL_MIXED_ATTN_MIN=512"
    for wtype, knob in (("q4_0", TILE), ("q4_0", PER_TOKEN), ("q4_0", SPLIT_K), ("q4_0", THRESHOLD), ("q8_0", TILE), ("q8_0", PER_TOKEN)):
        g = _gguf(tmp_path, MX_A, wtype)
        refs = _oracle_logits(orc, g, sched)
        with monkeypatch.context() as mp:
            if knob != TILE:
                mp.setenv(*knob.split("="))
            dev = hip.load_llama_model(g, max_streams=6)
            _history(dev, sched)
            got = _run(dev, sched)
            dev.close()
        _check(sched, got, refs, f"ragged schedule, {wtype}, {knob}")
        outs[(wtype, knob)] = np.concatenate([lg for _, lg in got])
    # (these steps are below the default threshold: every row on the per-token kernel, bit for bit)
    assert outs[("q4_0", THRESHOLD)].tobytes() == outs[("q4_0", PER_TOKEN)].tobytes()
    assert outs[("q4_0", TILE)].tobytes() != outs[("q4_0", PER_TOKEN)].tobytes()          # the tile kernel did run
    for a, b in ((("q4_0", TILE), ("q4_0", PER_TOKEN)), (("q4_0", TILE), ("q4_0", SPLIT_K)), (("q8_0", TILE), ("q8_0", PER_TOKEN))):
        print(f"{a} against {b}: max difference {float(np.abs(outs[a] - outs[b]).max()):.2e} (logit std {float(outs[a].std()):.2f})")


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("mixed_attn", ["1", "0"])
def test_shortened_schedule_on_other_head_shapes(hip, orc, tmp_path, monkeypatch, name, mixed_attn):
    shape = SHAPES[name]
    g = _gguf(tmp_path, shape)
    # prompts of 20, 70 and 150 tokens beside three decode streams; chunks cross position 128
    sched = Schedule(shape.vocab, {0: 3, 1: 125, 2: 60}, [(3, 20, 1), (4, 70, 1), (5, 150, 2)], budget=48, tail=4, token_seed=TOKEN_SEEDS[name],
                     length=170)
    refs = _oracle_logits(orc, g, sched)
    monkeypatch.setenv("NL_MIXED_ATTN", mixed_attn)
    dev = hip.load_llama_model(g, max_streams=6)
    _history(dev, sched)
    got = _run(dev, sched)
    dev.close()
    _check(sched, got, refs, f"{name}, NL_MIXED_ATTN={mixed_attn}")


def test_gqa_factor_outside_the_tile_kernel(hip, orc, tmp_path):
    """6 query heads over 1 kv head: a factor the tile kernels are not instantiated for (attn_tile_supported).  Such a model runs
    on the per-token attention kernel and the general launch plan throughout, and in a mixed step the per-token kernel serves
    the prompt segments too: the history (single-token steps), every output row and the decode tail against the oracle."""
    shape = synth.ModelShape("mx_g6", 1, 384, 6, 1, 512, seq_len=192, interm=512)
    g = _gguf(tmp_path, shape)
    sched = Schedule(shape.vocab, {0: 3, 1: 125, 2: 60}, [(3, 20, 1), (4, 70, 1), (5, 150, 2)], budget=48, tail=4, token_seed=TOKEN_SEEDS["gqa6"],
                     length=170)
    dev = hip.load_llama_model(g, max_streams=6)
    refs = _oracle_logits(orc, g, sched)
    _history(dev, sched)
    got = _run(dev, sched)
    dev.close()
    _check(sched, got, refs, "6 heads over 1 kv head")


def test_decode_batches_take_the_existing_path_bitwise(hip, tmp_path):
    g = _gguf(tmp_path, MX_A)
    n = 37
    rng = np.random.Generator(np.random.PCG64(21))
    start = [int(v) for v in rng.integers(0, 140, size=n)]
    toks = [[int(t) for t in rng.integers(3, MX_A.vocab, size=start[s] + 3)] for s in range(n)]
    settings = [dict(temperature=0.0, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=8),
                dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=64),
                dict(temperature=1.3, top_p=1.0, top_k=40, rep_penalty=1.3, rep_window=16)]
    params = [settings[i % 3] for i in range(n)]
    a, b = hip.load_llama_model(g, max_streams=n), hip.load_llama_model(g, max_streams=n)
    for dev in (a, b):
        for s in range(n):
            if start[s]:
                dev.prefill(toks[s][:start[s]], stream=s, want_logits=False)
    streams = list(range(n))
    for k in range(2):
        tk, ps = [toks[s][start[s] + k] for s in range(n)], [start[s] + k for s in range(n)]
        ids_a, lg_a = a.forward_mixed(streams, tk, ps, n, want_logits=True)
        ids_b, lg_b = b.forward_batch(streams, tk, ps, want_logits=True)
        assert ids_a == ids_b and lg_a.tobytes() == lg_b.tobytes(), k
    tk, ps = [toks[s][start[s] + 2] for s in range(n)], [start[s] + 2 for s in range(n)]
    us = rng.random(n, dtype=np.float32)
    recents = [[int(t) for t in rng.integers(0, MX_A.vocab, size=params[i]["rep_window"] // 2)] for i in range(n)]
    ids_a, rec_a = a.forward_mixed_sample(streams, tk, ps, n, params, us, recents)
    ids_b, rec_b = b.forward_batch_sample(streams, tk, ps, params, us, recents)
    assert ids_a == ids_b and rec_a == rec_b
    a.close()
    b.close()


def _host_pick(lg, p, recent, u, vocab):
    lg = sm.apply_penalty(lg, recent, p["rep_penalty"], vocab)
    if p["temperature"] <= 0:
        return int(np.argmax(lg))
    if p["top_p"] < 1.0:
        return sm.device_top_p(lg, p["temperature"], p["top_p"], u)[0]
    return sm.go_top_k(lg, p["temperature"], p["top_k"], u)


@pytest.mark.parametrize("wtype", ["q4_0", "q4_k"])
def test_sampler_of_a_mixed_step_picks_what_the_mirror_picks(hip, tmp_path, wtype):
    # the ids of nl_forward_mixed_sample = the host mirror's picks (penalty, then top-p / top-k / argmax) from the logits
    # nl_forward_mixed returns for the same call on a twin handle; q4_k: the single-token fallback with the per-row sampler
    shape = MX_A if wtype == "q4_0" else synth.ModelShape("mx_k", 1, 256, 4, 2, 512, seq_len=320, interm=512)
    g = _gguf(tmp_path, shape, wtype)
    sched = Schedule(shape.vocab, {0: 5, 1: 126, 2: 30, 3: 64}, [(4, 40, 0), (5, 100, 0)], budget=48, tail=2, token_seed=23)
    settings = [dict(temperature=0.0, top_p=0.9, top_k=50, rep_penalty=1.3, rep_window=8),
                dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=64),
                dict(temperature=1.3, top_p=1.0, top_k=40, rep_penalty=1.3, rep_window=16),
                dict(temperature=0.5, top_p=0.6, top_k=50, rep_penalty=1.0, rep_window=0),
                dict(temperature=0.7, top_p=1.0, top_k=1024, rep_penalty=1.2, rep_window=4)]
    rng = np.random.Generator(np.random.PCG64(29))
    dev, twin = hip.load_llama_model(g, max_streams=6), hip.load_llama_model(g, max_streams=6)
    _history(dev, sched)
    _history(twin, sched)
    windows = {s: [int(t) for t in rng.integers(0, shape.vocab, size=3)] for s in sched.streams}
    mixed = 0
    for k, (streams, tokens, pos, n_out) in enumerate(sched.steps):
        cur = [settings[(streams[i] + k) % len(settings)] for i in range(n_out)]
        recents = [windows[streams[i]][-cur[i]["rep_window"]:] if cur[i]["rep_window"] else [] for i in range(n_out)]
        us = rng.random(n_out, dtype=np.float32)
        ids, new_rec = dev.forward_mixed_sample(streams, tokens, pos, n_out, cur, us, recents)
        _, lg = twin.forward_mixed(streams, tokens, pos, n_out, want_logits=True)
        want = [_host_pick(lg[i], cur[i], recents[i], us[i], shape.vocab) for i in range(n_out)]
        assert ids == want, (k, ids, want)
        for i in range(n_out):
            assert new_rec[i] == (sm.push_recent(recents[i], want[i], cur[i]["rep_window"]) if cur[i]["rep_window"] else []), (k, i)
            windows[streams[i]] = windows[streams[i]] + [want[i]]
        mixed += len(streams) > n_out
    assert mixed >= 2
    dev.close()
    twin.close()


def test_arguments_are_checked_before_anything_is_queued(hip, orc, tmp_path):
    from nanollama_amd import _lib
    g = _gguf(tmp_path, MX_A)
    dev = hip.load_llama_model(g, max_streams=6)
    rng = np.random.Generator(np.random.PCG64(31))
    seq = [int(t) for t in rng.integers(3, MX_A.vocab, size=40)]
    max_rows, max_out = dev.mixed_capacity
    assert (max_rows, max_out) == (320, 64)
    for p in range(2):                                   # another request's K / V in the rows stream 1 will jump over below
        dev.forward(seq[30 + p], p, stream=1)
    dev.reset(1)
    bad = {
        "a repeated (stream, pos)": ([0, 1, 1], [5, 6, 7], [0, 3, 3], 1),
        "a repeated (stream, pos) across the output rows": ([1, 0, 1], [5, 6, 7], [3, 0, 3], 1),
        "a gap inside a stream's run": ([0, 1, 1, 1], [5, 6, 7, 8], [0, 0, 1, 3], 1),
        "descending order": ([0, 1, 1], [5, 6, 7], [0, 4, 3], 1),
        "n_out > n": ([0, 1], [5, 6], [0, 0], 3),
        "n_out > 64": ([0] * 70, [5] * 70, list(range(70)), 65),
        "n > max_rows": ([0] * (max_rows + 1), [5] * (max_rows + 1), [p % 320 for p in range(max_rows + 1)], 1),
        "a stream out of range": ([0, 6], [5, 6], [0, 0], 1),
    }
    for what, (streams, tokens, pos, n_out) in bad.items():
        with pytest.raises(_lib.NlError) as ei:
            dev.forward_mixed(streams, tokens, pos, n_out)
        assert ei.value.code == -1 and len(str(ei.value)) > len("NL_ERR_INVALID: "), what
        if "stream's run" in what or "repeated" in what or "descending" in what:
            assert "stream 1" in str(ei.value), (what, str(ei.value))
        with pytest.raises(_lib.NlError):
            dev.forward_mixed_sample(streams, tokens, pos, n_out, [dict(temperature=0.0, top_p=0.9, top_k=50, rep_penalty=1.0, rep_window=0)] * n_out,
                                     [0.0] * n_out, [[]] * n_out)
    # nothing was queued or marked: a valid call (stream 1 had rows in the refused calls) matches the oracle, and its run,
    # which starts at position 2 above the high-water mark 0, sees zero rows below, not the earlier request's (the oracle with
    # the same jump)
    orc.set_threads(1)
    ref = orc.OracleModel(g)
    want = [ref.forward(seq[p], p).copy() for p in range(2, 12)][-1]
    ref.close()
    ref0 = orc.OracleModel(g)
    want0 = ref0.forward(seq[0], 0).copy()
    ref0.close()
    ids, lg = dev.forward_mixed([1, 0] + [1] * 9, [seq[11], seq[0]] + seq[2:11], [11, 0] + list(range(2, 11)), 2, want_logits=True)
    for row, w in ((0, want), (1, want0)):
        assert float(np.abs(lg[row] - w).max()) <= LOGIT_TOL * max(1.0, float(w.std())), row
    dev.close()
    grp = hip.load_llama_model(gguf.load_gguf(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_q8_0.gguf")), devices=[0, 0])
    try:
        with pytest.raises(_lib.NlError) as ei:
            grp.forward_mixed([0, 0], [1, 2], [0, 1], 1)
        assert ei.value.code == -2
        with pytest.raises(_lib.NlError) as ei:
            grp.forward_mixed_sample([0, 0], [1, 2], [1, 0], 1, [dict(temperature=0.8, top_p=0.9, top_k=50, rep_penalty=1.15, rep_window=8)],
                                     [0.5], [[]])
        assert ei.value.code == -2
    finally:
        grp.close()


def test_formats_outside_the_multi_token_path_equal_single_steps_bitwise(hip, tmp_path):
    # Q4_K (whole 256-element super-blocks): the rows go through the single-token step in (stream, position) order
    shape = synth.ModelShape("mx_k", 1, 256, 4, 2, 512, seq_len=320, interm=512)
    g = _gguf(tmp_path, shape, "q4_k")
    rng = np.random.Generator(np.random.PCG64(37))
    t = [int(v) for v in rng.integers(3, shape.vocab, size=8)]
    dev, twin = hip.load_llama_model(g, max_streams=2), hip.load_llama_model(g, max_streams=2)
    for d in (dev, twin):
        d.forward(t[0], 0, stream=1)
    # rows: stream 0 once (output), stream 1 three times (its last row an output row, in front of the two below it)
    ids, lg = dev.forward_mixed([0, 1, 1, 1], [t[1], t[4], t[2], t[3]], [0, 3, 1, 2], 2, want_logits=True)
    twin.forward(t[1], 0, stream=0)
    want0 = twin.state.logits.copy()
    for p, tok in ((1, t[2]), (2, t[3]), (3, t[4])):
        twin.forward(tok, p, stream=1)
    want1 = twin.state.logits.copy()
    assert lg[0].tobytes() == want0.tobytes() and lg[1].tobytes() == want1.tobytes()
    assert ids == [int(np.argmax(want0)), int(np.argmax(want1))]
    dev.close()
    twin.close()


def test_goldie_full_shape_mixed_steps_match_oracle(hip, orc, tmp_path):
    # goldie Q4_0 (28 layers, D 1536, 24 heads / 6 kv heads, FFN 4096, vocabulary 48000): 48 decode rows at ragged positions
    # below 24, one walking 124..127, beside a 150-token prompt that arrives as chunks of 64 / 64 / 21 + its final token (the
    # second chunk crosses position 128) and a 16-token prompt that fits one step.  Against the oracle: two decode rows in every
    # step and the first three sampled positions of both admitted streams.
    shape = synth.TIERS["goldie"]
    p = os.path.join(os.environ.get("NL_BENCH_DIR", "/tmp"), "nl_bench_goldie_q4_0_qrand.gguf")   # bench.py's file when present
    if not os.path.exists(p):
        synth.generate_gguf(p + ".tmp", shape, "q4_0", mode="qrand")
        os.replace(p + ".tmp", p)
    g = gguf.load_gguf(p)
    assert (g.meta.num_layers, g.meta.embed_dim, g.meta.num_heads, g.meta.num_kv_heads, g.meta.interm_size,
            g.meta.vocab_size) == (28, 1536, 24, 6, 4096, 48000)
    rng = np.random.Generator(np.random.PCG64(64))
    nd = 48
    start = [int(v) for v in rng.integers(0, 24, size=nd)]
    start[5], start[47] = 9, 124
    seqs = [[int(t) for t in rng.integers(3, shape.vocab, size=160)] for _ in range(nd + 2)]
    A, B = nd, nd + 1                                      # the admitted streams: 150 and 16 tokens
    # steps: (non-output rows of A, of B, final tokens joining)
    plan = [((0, 64), (0, 15), [B]), ((64, 128), None, []), ((128, 149), None, [A]), (None, None, [])]
    orc.set_threads(min(32, os.cpu_count() or 1))
    wants = {}
    for s, upto in ((5, start[5] + 4), (47, start[47] + 4), (A, 152), (B, 18)):
        ref = orc.OracleModel(g)
        wants[s] = [ref.forward(t, pos).copy() for pos, t in enumerate(seqs[s][:upto])]
        ref.close()
    orc.set_threads(1)
    dev = hip.load_llama_model(g, max_streams=nd + 2)
    for s in range(nd):
        if start[s]:
            dev.prefill(seqs[s][:start[s]], stream=s, want_logits=False)
    pos = {s: start[s] for s in range(nd)}
    worst, rows, gated = 0.0, 0, 0
    for k, (ca, cb, joins) in enumerate(plan):
        for s in joins:
            pos[s] = 149 if s == A else 15
        out = sorted(pos)
        rowsk = [(s, pos[s]) for s in out]
        for s, c in ((A, ca), (B, cb)):
            if c:
                rowsk += [(s, q) for q in range(*c)]
        ids, lg = dev.forward_mixed([s for s, _ in rowsk], [seqs[s][q] for s, q in rowsk], [q for _, q in rowsk], len(out), want_logits=True)
        for i, s in enumerate(out):
            if s in wants and pos[s] < len(wants[s]):
                want = wants[s][pos[s]]
                scale = max(1.0, float(want.std()))
                worst = max(worst, float(np.abs(lg[i] - want).max()) / scale)
                rows += 1
                top2 = np.partition(want, -2)[-2:]
                if float(top2[1] - top2[0]) > 10 * LOGIT_TOL * scale:
                    assert ids[i] == int(orc.argmax(want)), (k, s)
                else:
                    gated += 1
        for s in out:
            pos[s] += 1
    # stream A's third sampled position: a decode batch over K / V the chunks wrote
    for k in range(1):
        out = sorted(pos)
        ids, lg = dev.forward_mixed(out, [seqs[s][pos[s]] for s in out], [pos[s] for s in out], len(out), want_logits=True)
        want = wants[A][pos[A]]
        worst = max(worst, float(np.abs(lg[out.index(A)] - want).max()) / max(1.0, float(want.std())))
        rows += 1
        for s in out:
            pos[s] += 1
    print(f"\ngoldie mixed steps: {rows} rows, max|gpu-oracle| = {worst:.2e} (relative), {gated} under the argmax gate")
    assert gated <= GATE_CAP * rows, (gated, rows)
    assert worst <= LOGIT_TOL
    dev.close()
