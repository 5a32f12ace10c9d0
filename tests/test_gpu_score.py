"""GPU tests of nl_score (nanollama_amd/csrc/nl_engine.hip; the row reduction is score_rows_kernel, nl_score.h): the prompt
path with an LM head over every row, each logits row reduced on the device to log P(target) and the greedy id.  Reference: the
oracle's Forward token by token (go/model.go:490-620) and a float64 log-softmax of its logits -- the cross entropy of
nanollama/core_eval.py:38-44 per token.

Tolerance, derived from the project's logit tolerance max|gpu - oracle| <= 1e-4 * max(1, std(oracle row)):
|d logprob| <= |d x_t| + |d lse| <= 2 max|d x|, so |gpu - oracle| <= 2 * 1e-4 * max(1, std(oracle row)) per row.  A greedy id
is compared where the oracle's top-2 gap exceeds 10 * 1e-4 * max(1, std); each test asserts that at most 2 % of its rows are
left out by that gate (the token seeds below were picked on the CPU with the oracle alone so that this holds)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nanollama_amd import gguf, score, synth

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
GATE_CAP = 0.02
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

MX_A = synth.ModelShape("mx_a", 2, 256, 4, 2, 512, seq_len=320, interm=512)          # head_dim 64, GQA 2
SHAPES = {
    "mx_a": MX_A,
    "mx_long": synth.ModelShape("mx_long", 2, 256, 4, 2, 512, seq_len=576, interm=512),      # MX_A with a context beyond one 512-row slab
    "hd32_gqa8": synth.ModelShape("mx_d", 1, 1024, 32, 4, 512, seq_len=192, interm=3072),
    "mha_hd64": synth.ModelShape("mx_b", 2, 512, 8, 8, 512, seq_len=192, interm=1024, rope_conjugate=True),
}
# (model, weight type) -> seed of its token sequence, chosen on the CPU with the oracle alone: the share of rows under the
# argmax gate stays below the 2 % cap for every prefix length the tests use
TOKEN_SEEDS = {("mx_a", "q4_0"): 11, ("mx_a", "q8_0"): 11, ("mx_a", "f16"): 11, ("mx_a", "q6_k"): 11, ("mx_a", "q5_0"): 11,
               ("hd32_gqa8", "q4_0"): 11, ("mha_hd64", "q4_0"): 11, ("tiny_qknorm_q8_0", ""): 11, ("tiny_tied_q8_0", ""): 11,
               ("tiny_q8_0", ""): 11, ("mx_long", "q4_0"): 11}
# 1, 2: below NL_BATCH_MIN, single-token steps; with NL_SCORE_SLAB=64: 64 | 65 the slab boundary, 130 a ragged third slab
LENGTHS = (1, 2, 3, 64, 65, 130)


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
def files(tmp_path_factory):
    """path of the GGUF of (model name, weight type), written once per module"""
    root = tmp_path_factory.mktemp("score")

    def get(name, wtype=""):
        if name not in SHAPES:
            return os.path.join(GOLDEN, name + ".gguf")
        p = root / f"{name}_{wtype}.gguf"
        if not p.exists():
            synth.generate_gguf(str(p), SHAPES[name], wtype, 307)
        return str(p)
    return get


def sequence(vocab, seq_len, seed):
    """seq_len + 1 ids: the inputs of a full context and the target of its last row"""
    return [int(t) for t in np.random.Generator(np.random.PCG64(seed)).integers(3, vocab, size=seq_len + 1)]


_REFS = {}


def reference(orc, path, ids, key=None):
    """the oracle's logits rows [len(ids)][vocab] for ids fed from position 0; computed once per key and left unchanged"""
    key = key or (path, len(ids))
    if key not in _REFS:
        orc.set_threads(min(16, os.cpu_count() or 1))
        ref = orc.OracleModel(gguf.load_gguf(path))
        rows = np.stack([ref.forward(t, p).copy() for p, t in enumerate(ids)])
        ref.close()
        orc.set_threads(1)
        rows.setflags(write=False)
        _REFS[key] = rows
    return _REFS[key]


def want_logprobs(rows, targets):
    x = rows.astype(np.float64)
    m = x.max(axis=1)
    lse = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
    t = np.asarray(targets)
    return np.where(t >= 0, x[np.arange(len(t)), np.maximum(t, 0)] - lse, 0.0)


def check(lp, am, rows, targets, what):
    """every row against the oracle; returns the worst |d logprob| relative to its bound"""
    want = want_logprobs(rows, targets)
    scale = np.maximum(1.0, rows.std(axis=1).astype(np.float64))
    rel = np.abs(lp.astype(np.float64) - want) / (2 * LOGIT_TOL * scale)
    top2 = np.partition(rows, -2, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 10 * LOGIT_TOL * scale
    print(f"{what}: {len(want)} rows, max|gpu - oracle| = {float(rel.max()):.3f} of the bound, {int((~clear).sum())} rows under the argmax gate")
    assert (rel <= 1.0).all(), (what, int(rel.argmax()), float(rel.max()))
    t = np.asarray(targets)
    assert (lp[t < 0] == 0.0).all(), what
    assert (am[clear] == rows.argmax(axis=1)[clear]).all(), (what, np.nonzero(am != rows.argmax(axis=1))[0][:8])
    assert (~clear).sum() <= GATE_CAP * len(want), (what, int((~clear).sum()))
    return float(rel.max())


def run_case(hip, orc, files, name, wtype, lengths, env=None):
    path = files(name, wtype)
    g = gguf.load_gguf(path)
    seq = sequence(g.meta.vocab_size, g.meta.seq_len, TOKEN_SEEDS[(name, wtype)])
    rows = reference(orc, path, seq[:-1])
    dev = hip.load_llama_model(g)
    try:
        for n in lengths:
            dev.reset(0)
            lp, am = dev.score(seq[:n], seq[1:n + 1])
            check(lp, am, rows[:n], seq[1:n + 1], f"{name} {wtype} n = {n}" + (f" {env}" if env else ""))
    finally:
        dev.close()


@pytest.mark.parametrize("slab", ["64", None])
def test_q4_0_every_length_matches_oracle(hip, orc, files, monkeypatch, slab):
    # the LM head runs over slabs of NL_SCORE_SLAB rows (512 unless set): 64 puts 1 .. 5 slabs, whole and ragged, under these lengths
    if slab:
        monkeypatch.setenv("NL_SCORE_SLAB", slab)
    run_case(hip, orc, files, "mx_a", "q4_0", LENGTHS + (MX_A.seq_len,), env=f"NL_SCORE_SLAB={slab}" if slab else None)


def test_a_context_beyond_one_default_slab(hip, orc, files):
    # 512 | 513: the boundary of the default slab; 576: a ragged second slab
    run_case(hip, orc, files, "mx_long", "q4_0", (512, 513, 576))


def test_slab_sizes_agree_bitwise_and_the_scratch_regrows(hip, files, monkeypatch):
    # a row's logits do not depend on the rows it shares a slab with only where the GEMM's split of K is the same; the results
    # of one slab size must replay bitwise, and a handle that has scored with a small slab must serve a larger one (the scratch grows)
    g = gguf.load_gguf(files("mx_a", "q4_0"))
    seq = sequence(MX_A.vocab, MX_A.seq_len, TOKEN_SEEDS[("mx_a", "q4_0")])
    dev = hip.load_llama_model(g)
    out = {}
    for slab in ("64", "128", "64", "512"):
        monkeypatch.setenv("NL_SCORE_SLAB", slab)
        dev.reset(0)
        lp, am = dev.score(seq[:320], seq[1:321])
        if slab in out:
            assert out[slab][0].tobytes() == lp.tobytes() and out[slab][1].tobytes() == am.tobytes(), slab
        out[slab] = (lp, am)
    dev.close()
    worst = max(float(np.abs(out[a][0] - out["64"][0]).max()) for a in ("128", "512"))
    print(f"slab 128 / 512 against 64: max|d logprob| = {worst:.2e}")
    assert worst <= 4 * LOGIT_TOL          # (each is within 2e-4 * max(1, std) of the oracle; std of these rows is 1.02)


def test_q4_0_long_run_gemm_above_100_tokens(hip, orc, files, monkeypatch):
    # NL_DGEMM_MAX_TOKENS=100: 65 tokens stay on dgemm_kernel, 130 and 320 take the long-run GEMM with the norms folded around it
    monkeypatch.setenv("NL_DGEMM_MAX_TOKENS", "100")
    monkeypatch.setenv("NL_SCORE_SLAB", "64")
    run_case(hip, orc, files, "mx_a", "q4_0", (65, 130, MX_A.seq_len), env="NL_DGEMM_MAX_TOKENS=100")


def test_q4_0_without_dgemm(hip, orc, files, monkeypatch):
    monkeypatch.setenv("NL_DGEMM", "0")
    monkeypatch.setenv("NL_SCORE_SLAB", "64")
    run_case(hip, orc, files, "mx_a", "q4_0", (65, 130, MX_A.seq_len), env="NL_DGEMM=0")


@pytest.mark.parametrize("name", ["hd32_gqa8", "mha_hd64"])
def test_other_head_shapes(hip, orc, files, name):
    run_case(hip, orc, files, name, "q4_0", (3, 65, 130, SHAPES[name].seq_len))


@pytest.mark.parametrize("wtype", ["q8_0", "f16", "q5_0"])
def test_other_weight_types_on_the_multi_token_path(hip, orc, files, wtype):
    run_case(hip, orc, files, "mx_a", wtype, (65, 130, MX_A.seq_len))


@pytest.mark.parametrize("name", ["tiny_qknorm_q8_0", "tiny_tied_q8_0"])
def test_goldens(hip, orc, files, name):
    run_case(hip, orc, files, name, "", (2, 3, 33, 64))


def test_single_token_fallback_on_a_k_quant_file(hip, orc, files):
    # Q6_K matrices are not on the multi-token path: every token is a single-token step and one reduction of its logits
    run_case(hip, orc, files, "mx_a", "q6_k", (1, 3, 40))


def test_single_token_fallback_under_batch_min(hip, orc, files):
    # NL_BATCH_MIN is read once per process: a child with it above n scores the Q4_0 file on single-token steps
    path, n = files("mx_a", "q4_0"), 40
    seq = sequence(MX_A.vocab, MX_A.seq_len, TOKEN_SEEDS[("mx_a", "q4_0")])
    env = dict(os.environ, NL_BATCH_MIN="1000")
    out = subprocess.run([sys.executable, os.path.join(HERE, "score_worker.py"), path, json.dumps(seq[:n]), json.dumps(seq[1:n + 1])],
                         env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    rows = reference(orc, path, seq[:-1])
    check(np.asarray(got["logprobs"], dtype=np.float32), np.asarray(got["argmax"]), rows[:n], seq[1:n + 1], "mx_a q4_0 NL_BATCH_MIN=1000")
    # the same call in this process runs the multi-token path: not the same bits, or the child did not take the fallback
    dev = hip.load_llama_model(gguf.load_gguf(path))
    lp, _ = dev.score(seq[:n], seq[1:n + 1])
    dev.close()
    assert lp.tobytes() != np.asarray(got["logprobs"], dtype=np.float32).tobytes()


def test_continuation_at_pos0_above_zero(hip, orc, files):
    path = files("mx_a", "q4_0")
    g = gguf.load_gguf(path)
    seq = sequence(MX_A.vocab, MX_A.seq_len, TOKEN_SEEDS[("mx_a", "q4_0")])
    rows = reference(orc, path, seq[:-1])
    dev = hip.load_llama_model(g)
    dev.prefill(seq[:40], pos0=0, want_logits=False)
    targets = [seq[41 + i] if i % 3 != 1 else -1 for i in range(30)]
    lp, am = dev.score(seq[40:70], targets, pos0=40)
    dev.close()
    assert sum(t < 0 for t in targets) == 10
    check(lp, am, rows[40:70], targets, "mx_a q4_0 prefill 40, score 30 at pos0 = 40")


@pytest.mark.parametrize("n", [2, 65, 300])
def test_leaves_the_stream_as_prefill_does(hip, files, n):
    g = gguf.load_gguf(files("mx_a", "q4_0"))
    seq = sequence(MX_A.vocab, MX_A.seq_len, TOKEN_SEEDS[("mx_a", "q4_0")])
    L, KV, hd, S, V = MX_A.n_layer, MX_A.n_kv_head, MX_A.head_dim, MX_A.seq_len, MX_A.vocab
    dev = hip.load_llama_model(g, max_streams=2)
    dev.score(seq[:n], seq[1:n + 1], stream=0)
    lg_score = dev.debug_read("logits", V).copy()
    cont_score = dev.decode_greedy(int(lg_score.argmax()), n, 16, stream=0)
    dev.prefill(seq[:n], pos0=0, stream=1)
    lg_prefill = dev.state.logits.copy()
    assert dev.debug_read("logits", V).tobytes() == lg_prefill.tobytes()
    cont_prefill = dev.decode_greedy(int(lg_prefill.argmax()), n, 16, stream=1)
    assert lg_score.tobytes() == lg_prefill.tobytes()
    assert len(cont_score) == 16 and cont_score == cont_prefill
    for which in ("k_cache", "v_cache"):
        a = dev.debug_read(which, L * KV * S * hd, stream=0).reshape(L, KV, S, hd)[:, :, :n]
        b = dev.debug_read(which, L * KV * S * hd, stream=1).reshape(L, KV, S, hd)[:, :, :n]
        assert np.abs(b).max() > 0 and a.tobytes() == b.tobytes(), which
    dev.close()


def test_errors_leave_the_handle_usable(hip, orc, files):
    from nanollama_amd import _lib
    path = files("mx_a", "q4_0")
    g = gguf.load_gguf(path)
    seq = sequence(MX_A.vocab, MX_A.seq_len, TOKEN_SEEDS[("mx_a", "q4_0")])
    rows = reference(orc, path, seq[:-1])
    dev = hip.load_llama_model(g)
    for targets in ([seq[1], MX_A.vocab, seq[3]], [seq[1], -2, seq[3]]):
        with pytest.raises(_lib.NlError) as ei:
            dev.score(seq[:3], targets)
        assert ei.value.code == -1
    with pytest.raises(_lib.NlError) as ei:
        dev.score(seq[:11], seq[1:12], pos0=MX_A.seq_len - 10)
    assert ei.value.code == -1
    lp, am = dev.score([], [])
    assert lp.size == 0 and am.size == 0
    lp, am = dev.score(seq[:65], seq[1:66])
    check(lp, am, rows[:65], seq[1:66], "after the refused calls")
    dev.close()
    grp = hip.load_llama_model(gguf.load_gguf(files("tiny_q8_0")), devices=[0, 0])      # every rank on device 0
    with pytest.raises(_lib.NlError) as ei:
        grp.score(seq[:3], seq[1:4])
    assert ei.value.code == -2
    grp.close()


def test_score_text_end_to_end_on_a_golden_model(hip, orc, files):
    from nanollama_amd.tokenizer import Tokenizer
    path = files("tiny_q8_0")
    g = gguf.load_gguf(path)
    tok = Tokenizer(g.meta)
    seq = sequence(g.meta.vocab_size, g.meta.seq_len, TOKEN_SEEDS[("tiny_q8_0", "")])
    ids = [1] + [t for t in seq if t >= 40][:49]
    text = "".join(g.meta.token_list[i] for i in ids[1:])          # synthetic vocabulary: one code point per token
    assert tok.encode(text, True) == ids
    rows = reference(orc, path, ids[:-1], key=(path, "text"))
    want = want_logprobs(rows, ids[1:])
    dev = hip.load_llama_model(g)
    r = score.score_text(dev, tok, text)
    dev.close()
    bound = float((2 * LOGIT_TOL * np.maximum(1.0, rows.std(axis=1))).sum())
    print(f"score_text: {r.n_tokens} tokens, logprob {r.logprob:.6f} (oracle {want.sum():.6f}, bound {bound:.2e}), bpb {r.bpb:.6f}")
    assert r.n_tokens == len(ids) - 1 and abs(r.logprob - want.sum()) <= bound
    n_bytes = len(text.encode("utf-8"))
    assert r.n_bytes == n_bytes and abs(r.bpb - (-want.sum() / n_bytes / np.log(2))) <= bound / n_bytes / np.log(2)
    assert abs(r.nll + want.sum() / r.n_tokens) <= bound / r.n_tokens and abs(r.ppl - np.exp(r.nll)) <= 1e-9 * r.ppl


def test_three_windows_score_every_id_once(hip, orc, files):
    path = files("mx_a", "q4_0")
    g = gguf.load_gguf(path)
    ids = [int(t) for t in np.random.Generator(np.random.PCG64(5)).integers(3, MX_A.vocab, size=700)]
    S = MX_A.seq_len
    want = []
    for k, lo in enumerate(range(0, 700, S)):
        rows = reference(orc, path, ids[lo:lo + S], key=(path, "window", k))
        want.append((rows, ids[lo + 1:lo + S + 1]))
    dev = hip.load_llama_model(g)
    r = score.score_ids(dev, ids)
    dev.close()
    assert r.n_tokens == 699 and len(r.token_logprobs) == 699
    at = 0
    for k, (rows, targets) in enumerate(want):
        n = len(targets)
        lp = np.asarray(r.token_logprobs[at:at + n], dtype=np.float32)
        exact = want_logprobs(rows[:n], targets)
        rel = np.abs(lp - exact) / (2 * LOGIT_TOL * np.maximum(1.0, rows[:n].std(axis=1)))
        print(f"window {k}: {n} ids, max|gpu - oracle| = {float(rel.max()):.3f} of the bound")
        assert (rel <= 1.0).all(), (k, int(rel.argmax()))
        at += n
    assert at == 699
