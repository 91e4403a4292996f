"""Sequence scoring on the device (web-rwkv-gguf_amd/csrc/wrk_score.hip) against the f64 restatement in
tests/score_ref.py: the kernel through `Context.score_logits`, the model jobs through `Runtime.score_raw` (against `infer_raw` on the
same job), the runtime loop `score_sequences` (against `infer` with Full output and a host log-softmax), the oracle on tiny models and
the C oracle at the 1.5B bench shape."""
import json
import os
import sys

import numpy as np
import pytest

import wrk
import score_ref as R
from oracle import gguf as ogguf
from oracle import rwkv7 as O
from oracle import synth
from oracle.rnn import stack_cursors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-2            # tests/test_gpu_model.py's bars on the logits; a log-softmax moves by at most twice the largest error
LOGIT_MEAN_TOL = 1.5e-3
RECORD_DIR = os.environ.get("WRK_RECORD_DIR", "")     # where the full-size parity record goes (DIR/score_parity.json); unset: printed only


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ 1. the kernel
def kernel_rows(V, n, seed):
    """n rows of kinds flat / peaked / half -inf / duplicated / target on a tied maximum, and their targets."""
    rng = np.random.default_rng(seed)
    rows, tg = np.empty((n, V), np.float32), np.empty(n, np.uint32)
    for r in range(n):
        kind = r % 5
        if kind == 0:
            x = rng.normal(0.0, 0.5, V)
        elif kind == 1:
            x = rng.normal(0.0, 3.0, V)
            x[rng.integers(V)] += 12.0
        elif kind == 2:
            x = rng.normal(0.0, 2.0, V)
            x[rng.random(V) < 0.5] = -np.inf
        else:
            x = np.round(rng.normal(0.0, 2.0, V) * 2.0) / 2.0
        t = int(rng.integers(V))
        if kind == 4:                                   # the maximum at several places, the target on one of them
            ties = rng.choice(V, min(V, 4), replace=False)
            x[ties] = x.max() + 1.0
            t = int(ties[r % ties.size])
        rows[r], tg[r] = x, t
    return rows, tg


@pytest.mark.parametrize("n", [1, 3, 64, 300])
@pytest.mark.parametrize("V", [1, 50, 1000, 65529, 65536])
def test_kernel_matches_the_restatement(ctx, V, n):
    x, t = kernel_rows(V, n, V * 1000 + n)
    lp, rk = ctx.score_logits(x, t)
    want_lp, want_rk = R.score_rows(x, t)
    ok = R.within_bar(lp, want_lp)
    assert ok.all(), (np.nonzero(~ok)[0][:5], lp[~ok][:5], want_lp[~ok][:5])
    assert (rk.astype(np.int64) == want_rk).all(), np.nonzero(rk != want_rk)[0][:5]
    lp2, rk2 = ctx.score_logits(x, t)                   # fixed reduction order: the same bits on every call
    assert lp2.tobytes() == lp.tobytes() and (rk2 == rk).all()
    live = x.max(axis=1) > -3e38                        # argmax_rows' answer: the first index of the maximum
    assert ((rk[live] == 0) == (x[live].argmax(axis=1) == t[live])).all()


def test_kernel_strided_rows_and_nan(ctx):
    """Rows of a stride that is not a multiple of 4 (the scalar-load form) and a NaN row."""
    V, stride, n = 65529, 65531, 5
    x, t = kernel_rows(V, n, 5)
    x[3, 17] = np.nan
    buf = np.full((n, stride), 7.0e3, np.float32)        # padding would dominate every row if it were read
    buf[:, :V] = x
    lp, rk = ctx.score_logits(ctx.buffer(buf), t, num_vocab=V, row_stride=stride)
    want_lp, want_rk = R.score_rows(x, t)
    assert np.isnan(lp[3])
    keep = np.arange(n) != 3
    assert R.within_bar(lp[keep], want_lp[keep]).all()
    assert (rk[keep].astype(np.int64) == want_rk[keep]).all()


def test_kernel_rejects_bad_targets(ctx):
    x = np.zeros((2, 10), np.float32)
    with pytest.raises(wrk.WrkError) as e:
        ctx.score_logits(x, [1, 10])
    assert e.value.code == wrk.E_ARG


# ------------------------------------------------------------------ 2. the model jobs
def make_runtime(ctx, version, name, num_batch):
    if version == 7:
        data = synth.make_v7_gguf(synth.CONFIGS[name], 42)
    else:
        data = synth.make_v6_gguf(synth.V6_CONFIGS[name], 42)
    return wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=num_batch, weights=wrk.WEIGHTS_INLINE)


def zero_state(rt):
    z = np.zeros_like(rt.state_back(0))
    for b in range(rt.num_batch):
        rt.state_load(z, b)


def states(rt):
    return np.stack([rt.state_back(b) for b in range(rt.num_batch)])


def full_logits(rt, seqs, chunk):
    """`infer` with Full output until the input is exhausted: every position's logits, per sequence."""
    inp = wrk.RnnInput(seqs, chunk, options=[wrk.RNN_FULL] * len(seqs))
    full = [[np.zeros((0, rt.info.num_vocab), np.float32)] for _ in seqs]
    while any(inp.remaining(b) for b in range(len(seqs))):
        for b, rows in enumerate(rt.infer(inp, mode=1)):
            full[b].append(rows)
    return [np.concatenate(f) for f in full]


# (lens per batch, which stacked rows are headers): engine (1 x 1), fused (4 x 1), a 70-token chunk, ragged batches
JOBS = {
    "engine": ([1], "all"),
    "fused4": ([1, 1, 1, 1], "all"),
    "chunk70": ([70], "all"),
    "ragged": ([5, 17, 3, 9], "some"),
}


def job(rt, lens, which, seed):
    rng = np.random.default_rng(seed)
    V = rt.info.num_vocab
    T = sum(lens)
    tokens = rng.integers(0, V, T).tolist()
    cursors = stack_cursors(lens)
    headers = list(range(T)) if which == "all" else sorted(rng.choice(T, T // 2, replace=False).tolist())
    targets = rng.integers(0, V, len(headers)).tolist()
    return tokens, cursors, headers, targets


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", list(JOBS))
@pytest.mark.parametrize("version,name", [(7, "tiny"), (7, "small"), (6, "tiny"), (6, "small")])
def test_score_raw_matches_infer_raw(ctx, version, name, shape, mode):
    lens, which = JOBS[shape]
    rt = make_runtime(ctx, version, name, len(lens))
    try:
        tokens, cursors, headers, targets = job(rt, lens, which, 11)
        zero_state(rt)
        logits = rt.infer_raw(tokens, cursors, headers, mode=mode)
        s_infer = states(rt)
        zero_state(rt)
        lp, rk = rt.score_raw(tokens, cursors, headers, targets, mode=mode)
        assert states(rt).tobytes() == s_infer.tobytes()          # only the epilogue differs
        want_lp, want_rk = R.score_rows(logits, targets)
        assert R.within_bar(lp, want_lp).all(), np.abs(lp - want_lp).max()
        assert (rk.astype(np.int64) == want_rk).all()
    finally:
        rt.close()


# ------------------------------------------------------------------ 3. the runtime loop
LENS = [1, 2, 33, 70, 129]


@pytest.mark.parametrize("version", [7, 6])
def test_score_sequences_matches_full_infer(ctx, version):
    rt = make_runtime(ctx, version, "tiny", len(LENS))
    try:
        V = rt.info.num_vocab
        rng = np.random.default_rng(version)
        seqs = [rng.integers(0, V, n).tolist() for n in LENS]
        zero_state(rt)
        full = full_logits(rt, seqs, 32)
        s_infer = states(rt)
        zero_state(rt)
        got = rt.score_sequences(seqs, token_chunk_size=32, mode=1)
        assert states(rt).tobytes() == s_infer.tobytes()
        for b, s in enumerate(seqs):
            lp, rk = got[b]
            assert lp.shape == rk.shape == (len(s) - 1,)
            assert full[b].shape[0] == len(s)
            if len(s) == 1:
                continue
            logits = full[b][: len(s) - 1]
            want = R.log_softmax_at(logits, s[1:])
            # the head of a score job sees other header rows than the Full job's: the logits agree to f32 summation order
            assert np.abs(lp - want).max() <= 1e-4, (b, np.abs(lp - want).max())
            x = logits.astype(np.float64)
            _, want_rk = R.score_rows(x, s[1:])
            xt = x[np.arange(len(s) - 1), s[1:]]
            gap = np.abs(x - xt[:, None])
            gap[np.arange(len(s) - 1), s[1:]] = np.inf
            clear = gap.min(axis=1) > 1e-4
            assert (rk[clear].astype(np.int64) == want_rk[clear]).all()
    finally:
        rt.close()


# ------------------------------------------------------------------ 4. the oracle (tiny models)
VARIANTS = [
    ("tiny", wrk.WEIGHTS_INLINE, {}),
    ("tiny", wrk.WEIGHTS_INLINE_F16, {}),
    ("tiny", wrk.WEIGHTS_REFERENCE, {}),
    ("small", wrk.WEIGHTS_INLINE, {}),
]


@pytest.mark.parametrize("name,weights,kw", VARIANTS)
def test_score_sequences_matches_the_oracle(ctx, name, weights, kw):
    data = synth.make_v7_gguf(synth.CONFIGS[name], 42, **kw)
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=1, weights=weights)
    try:
        oracle = O.V7Runtime(O.build_v7(ogguf.GgufReader(data), weights_f16=(weights != wrk.WEIGHTS_INLINE)), 1, act_f16=True)
        V = rt.info.num_vocab
        prompt = synth.tokens(5, "score", 40, V)
        want_logits = oracle.infer_chunk([prompt], list(range(len(prompt))))[:-1].astype(np.float64)
        zero_state(rt)
        err = np.abs(full_logits(rt, [prompt], 128)[0][:-1] - want_logits).max()
        zero_state(rt)
        lp, rk = rt.score_sequences([prompt], token_chunk_size=128)[0]
        want_lp, want_rk = R.score_rows(want_logits, prompt[1:])
        d = np.abs(lp - want_lp)
        assert d.max() <= 2 * LOGIT_TOL and d.mean() <= 2 * LOGIT_MEAN_TOL, (d.max(), d.mean())
        xt = want_logits[np.arange(len(prompt) - 1), prompt[1:]]
        gap = np.abs(want_logits - xt[:, None])
        gap[np.arange(len(prompt) - 1), prompt[1:]] = np.inf
        clear = gap.min(axis=1) > 2 * err
        assert clear.any()
        assert (rk[clear].astype(np.int64) == want_rk[clear]).all()
    finally:
        rt.close()


# ------------------------------------------------------------------ 5. full size against the C oracle
def record(key, stats):
    print(key, stats)
    if not RECORD_DIR:
        return
    path = os.path.join(RECORD_DIR, "score_parity.json")
    os.makedirs(RECORD_DIR, exist_ok=True)
    data = {}
    if os.path.exists(path):
        try:
            data = json.load(open(path))
        except Exception:
            data = {}
    data[key] = stats
    json.dump(data, open(path, "w"), indent=1, sort_keys=True)


def test_1p5b_score_matches_the_c_oracle():
    """The bench's 1.5B model (WEIGHTS_INLINE_F16, the arithmetic oracle/c restates), one 96-token sequence scored in one chunk,
    against the C oracle's teacher-forced logits at every position.  Bars: twice test_gpu_fullsize_oracle.py's logit bars."""
    sys.path.insert(0, ROOT)
    import bench
    from oracle import cport
    cport.lib.orc_set_threads(cport.usable_cpus())
    gg = bench.make_model_gguf("1.5B", seed=7)
    c = wrk.Context(0)
    rt = wrk.Runtime(c, wrk.GgufReader(gg), num_batch=1, weights=wrk.WEIGHTS_INLINE_F16)
    try:
        V = rt.info.num_vocab
        oracle = cport.CModel(gg)
        prompt = [(31 * i + 5) % (V - 1) for i in range(96)]
        zero_state(rt)
        oracle.state[:] = 0
        lp, rk = rt.score_sequences([prompt], token_chunk_size=128)[0]
        rows = np.stack([oracle.decode(int(t)).astype(np.float64) for t in prompt[:-1]])
        want_lp, want_rk = R.score_rows(rows, prompt[1:])
        d = np.abs(lp.astype(np.float64) - want_lp)
        st = {"max_abs_dlogprob": float(d.max()), "mean_abs_dlogprob": float(d.mean()), "positions": int(d.size),
              "nll_hip": float(-lp.astype(np.float64).mean()), "nll_oracle": float(-want_lp.mean()),
              "nll_difference": float(-lp.astype(np.float64).mean() + want_lp.mean()),
              "ppl_hip": float(np.exp(-lp.astype(np.float64).mean())), "ppl_oracle": float(np.exp(-want_lp.mean())),
              "rank_equal_fraction": float((rk.astype(np.int64) == want_rk).mean())}
        record("1.5B 96-token sequence", st)
        assert d.max() <= 2 * 6e-2 and d.mean() <= 2 * 8e-3, st
    finally:
        rt.close()
        c.close()


# ------------------------------------------------------------------ 6. interference and arguments
@pytest.mark.parametrize("shape", ["engine", "chunk70"])
def test_score_and_infer_programs_do_not_alias(ctx, shape):
    lens, which = JOBS[shape]
    rt = make_runtime(ctx, 7, "tiny", len(lens))
    try:
        tokens, cursors, headers, targets = job(rt, lens, which, 3)
        zero_state(rt)
        fresh_logits = rt.infer_raw(tokens, cursors, headers)
        rt2 = make_runtime(ctx, 7, "tiny", len(lens))
        try:
            zero_state(rt2)
            fresh_lp, fresh_rk = rt2.score_raw(tokens, cursors, headers, targets)
        finally:
            rt2.close()
        for _ in range(2):                  # a score job, then an infer job of the same shape, and the reverse
            zero_state(rt)
            lp, rk = rt.score_raw(tokens, cursors, headers, targets)
            assert lp.tobytes() == fresh_lp.tobytes() and (rk == fresh_rk).all()
            zero_state(rt)
            assert rt.infer_raw(tokens, cursors, headers).tobytes() == fresh_logits.tobytes()
    finally:
        rt.close()


@pytest.mark.parametrize("version", [7, 6])
def test_bad_arguments_launch_nothing(ctx, version):
    rt = make_runtime(ctx, version, "tiny", 1)
    try:
        V = rt.info.num_vocab
        tokens, cursors, headers, targets = job(rt, [9], "all", 5)
        zero_state(rt)
        rt.infer_raw(tokens[:3], stack_cursors([3]), [2])           # a non-zero state to keep
        before = states(rt)
        bad_target = list(targets)
        bad_target[4] = V
        fn, mdl = (wrk.hip.wrk_v6_score, rt.model6) if rt.model6 else (wrk.hip.wrk_v7_score, rt.model)
        t, c, h = wrk._u32(tokens), wrk._u32(cursors), wrk._u32(headers)
        lp, rk = np.zeros(len(headers), np.float32), np.zeros(len(headers), np.uint32)
        for call in (
            lambda: rt.score_raw(tokens, cursors, headers, bad_target),
            lambda: rt.score_raw(tokens, cursors, [0, 9], targets[:2]),
            lambda: rt.ctx.check(fn(rt.ctx.h, mdl, rt.state, wrk._ptr(t, wrk._u32p), None, wrk._ptr(c, wrk._u32p), t.size,
                                    wrk._ptr(h, wrk._u32p), h.size, None, wrk._ptr(lp, wrk._f32p), wrk._ptr(rk, wrk._u32p), 1)),
        ):
            with pytest.raises(wrk.WrkError) as e:
                call()
            assert e.value.code == wrk.E_ARG
            assert states(rt).tobytes() == before.tobytes()
        # NH = 0: the state advances as infer's does, nothing is scored
        rt.score_raw(tokens, cursors, [], [])
        after_score = states(rt)
        rt.state_load(before[0], 0)
        rt.infer_raw(tokens, cursors, [])
        assert after_score.tobytes() == states(rt).tobytes()
        assert after_score.tobytes() != before.tobytes()
    finally:
        rt.close()
