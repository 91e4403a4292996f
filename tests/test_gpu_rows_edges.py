"""The kernels that work on rows of f32 logits -- web-rwkv-gguf_amd/csrc/wrk_sample.hip, wrk_score.hip, wrk_logprob.hip, wrk_penalty.hip and
wrk_rows_dev.h under them -- over the whole f32 value range, through the C ABI, on the row profiles of tests/rows_edge_cases.py against
the expectations of tests/rows_edge_ref.py (checked on the CPU by tests/test_rows_edge_ref.py: the closed form equals the f64
references, every ordinary profile leaves 95 % of its cases unambiguous in every mode, four wrong readings of the contract fail).

Every row goes through twice: tight rows, and rows of stride V + 3 in a buffer whose padding holds +inf, NaN and 7.0e3 -- a kernel that
reads padding loses every row.  Which kernel a case runs on follows from V, the stride and the entry point:

| kernel                                        | selected by                                                       | cases                                        |
|-----------------------------------------------|-------------------------------------------------------------------|----------------------------------------------|
| sample_rows_kernel<1, PLAIN>                  | wrk_sample_logits, V = 1, 2, 1024                                 | test_plain[*-1] [*-2] [*-1024], test_temperature_and_top_p_edges[*-2] |
| sample_rows_kernel<4, PLAIN>                  | V = 1025, 4096                                                    | test_plain[*-1025] [*-4096], test_temperature_and_top_p_edges[*-1025] |
| sample_rows_kernel<16, PLAIN>                 | V = 4097, 8192, 8193, 16384                                       | test_plain[*-4097] .. [*-16384], test_temperature_and_top_p_edges[*-8193] |
| sample_rows_kernel<0, PLAIN>                  | V = 16385, 2^20                                                   | test_plain[*-16385], test_big_vocabulary     |
| sample_rows_kernel<1 / 4 / 8 / 0, FILT>       | wrk_sample_logits_filtered with a top_k or min_p array; V <= 1024 / <= 4096 / <= 8192 / >= 8193 | test_filtered[*]; its off rows (top_k = 0, min_p = 0): test_plain[*] |
| sample_rows_kernel<1 / 4 / 8 / 0, MIRO>       | wrk_sample_logits_mirostat, the same sizes                        | test_mirostat[*]; off rows (tau = 0): test_plain[*] |
| sample_rows_kernel<1 / 4 / 8 / 0, TYP>        | wrk_sample_logits_typical, the same sizes                         | test_typical[*]; off rows (typical_p = 1): test_plain[*] |
| score_slice_kernel<true>                      | stride % 4 == 0: tight V = 65536, 2^20; stride V + 3 at V = 1, 1025, 4097 | test_score_and_top_logprobs[*]       |
| score_slice_kernel<false>                     | the other strides of the same sizes                               | test_score_and_top_logprobs[*], test_greedy_agreement[*] |
| score_combine_kernel                          | more than one slice: V >= 4097                                    | test_score_and_top_logprobs[*-4097] ..       |
| logprob_slice_kernel<true> / <false>, logprob_combine_kernel | as the score kernels; the combine kernel runs at every size | test_score_and_top_logprobs[*], test_greedy_agreement[*] |
| penalize_rows_kernel<true>                    | V = 4096 at stride 4096                                           | test_penalize_is_bit_exact[4096-4096]        |
| penalize_rows_kernel<false>                   | V = 4096 at stride 4099; V = 4097                                 | test_penalize_is_bit_exact[4096-4099] [4097-*] |

profiles/rows_edges_kernel_stats.csv is a rocprofv3 --kernel-trace --stats run of this file and lists every instantiation of the table.

What this file found: DESIGN.md section 2, "Value range (logits rows)".
"""
import json
import os

import numpy as np
import pytest

import alt_cases as AC
import filter_cases as FC
import rows_edge_cases as RC
import rows_edge_ref as R
import score_ref as SC
import wrk
from oracle import synth

pytestmark = pytest.mark.gpu

WORST = {}          # (kernel, profile) -> worst error / bar
P_ = wrk._ptr
NAMES = sorted(RC.ORDINARY) + sorted(RC.EXACT)
SCORE_VOCABS = (1, 1025, 4097, 65536, RC.BIG_V)
NUM_TOP = 5


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def layouts(ctx, rows):
    """[(label, Buffer, stride)] of rows [n, V]: tight, and stride V + 3 with +inf, NaN and 7.0e3 in the padding"""
    rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.float32)
    flat, stride = RC.strided(rows)
    return [("tight", ctx.buffer(rows), rows.shape[1]), ("strided", ctx.buffer(flat), stride)]


def sample(ctx, buf, V, stride, T, P, seed, top_k=None, min_p=None, mirostat=None, typical_p=None):
    """One sampler call through the C ABI at `stride`; mirostat = (tau, eta, mu): returns (tokens, mu after)."""
    T, P, seed = f32(T), f32(P), u32(seed)
    n = T.size
    out = np.full(n, 0xFFFFFFFF, np.uint32)
    common = (ctx.h, buf.h, V, stride, n, P_(T, wrk._f32p), P_(P, wrk._f32p))
    tail = (P_(seed, wrk._u32p), R.STEP, P_(out, wrk._u32p))
    if mirostat is not None:
        tau, eta, mu = (np.array(np.broadcast_to(f32(a), n), np.float32) for a in mirostat)
        ctx.check(wrk.hip.wrk_sample_logits_mirostat(*common, P_(tau, wrk._f32p), P_(eta, wrk._f32p), P_(mu, wrk._f32p), *tail))
        assert (out < V).all()
        return out, mu
    if typical_p is not None:
        ty = np.array(np.broadcast_to(f32(typical_p), n), np.float32)
        ctx.check(wrk.hip.wrk_sample_logits_typical(*common, P_(ty, wrk._f32p), *tail))
    elif top_k is not None:
        K, mp = u32(top_k), f32(min_p)
        ctx.check(wrk.hip.wrk_sample_logits_filtered(*common, P_(K, wrk._u32p), P_(mp, wrk._f32p), *tail))
    else:
        ctx.check(wrk.hip.wrk_sample_logits(*common, *tail))
    assert (out < V).all()
    return out


def columns(cases):
    return [np.array([c[j] for c in cases]) for j in range(len(cases[0]))]


# ----------------------------------------------------------------------------- 1. the sampler, four modes
@pytest.mark.parametrize("V", RC.VOCABS)
@pytest.mark.parametrize("name", NAMES)
def test_plain(ctx, name, V):
    """The plain kernel against the references (the first direct comparison of its 4- and 16-per-thread variants with them), and the
    off rows of the three other kernels, bit-equal to it."""
    raw, cases, want = R.plain_cases(name, V)
    T, P, seed = columns(cases)
    n = len(cases)
    for label, buf, stride in layouts(ctx, np.tile(raw, (n, 1))):
        got = sample(ctx, buf, V, stride, T, P, seed)
        R.compare((name, V, label), got, want, cap=1.0 if name in RC.EXACT else 0.95)
        assert np.array_equal(sample(ctx, buf, V, stride, T, P, seed, top_k=np.zeros(n), min_p=np.zeros(n)), got), (name, V, label, "filtered")
        tok, mu = sample(ctx, buf, V, stride, T, P, seed, mirostat=(0.0, 0.3, 7.25))
        assert np.array_equal(tok, got) and (mu == np.float32(7.25)).all(), (name, V, label, "mirostat")
        assert np.array_equal(sample(ctx, buf, V, stride, T, P, seed, typical_p=1.0), got), (name, V, label, "typical")


@pytest.mark.parametrize("V", RC.VOCABS)
@pytest.mark.parametrize("name", NAMES)
def test_filtered(ctx, name, V):
    """top_k over filter_cases.top_ks(V) -- 0, 1, 2, 5, 40, V - 1, V, V + 7, 2^32 - 1 -- with every min_p, top_p and temperature of its grid"""
    raw, cases, want = R.filter_cases(name, V)
    T, P, K, mp, seed = columns(cases)
    for label, buf, stride in layouts(ctx, np.tile(raw, (len(cases), 1))):
        got = sample(ctx, buf, V, stride, T, P, seed, top_k=K, min_p=mp)
        R.compare((name, V, label), got, want, cap=1.0 if name in RC.EXACT else 0.95)


@pytest.mark.parametrize("V", RC.VOCABS)
@pytest.mark.parametrize("name", NAMES)
def test_mirostat(ctx, name, V):
    """Token and mu after the draw.  pos_inf_ties at mu >= log2(3): all three +inf tokens are candidates (the row-mass pass counts
    each with weight 1, so the candidate predicate has to let them through)."""
    raw, cases, want = R.mirostat_cases(name, V)
    T, mu, seed = columns(cases)
    for label, buf, stride in layouts(ctx, np.tile(raw, (len(cases), 1))):
        got, mu2 = sample(ctx, buf, V, stride, T, np.full(len(cases), AC.TOP_P), seed, mirostat=(AC.TAU, AC.ETA, mu))
        R.compare((name, V, label), got, [None if w is None else w[0] for w in want], cap=1.0 if name in RC.EXACT else 0.95)
        for i, w in enumerate(want):
            if w is not None:
                assert abs(float(mu2[i]) - w[1]) <= w[2], (name, V, label, i, cases[i], float(mu2[i]), w)


@pytest.mark.parametrize("name", ["all_equal_zero", "pos_inf_ties", "huge_span"])
def test_mirostat_tied_maximum_at_subnormal_temperature(ctx, name):
    """1 / T = +inf: a token tied with a finite maximum has (l - mx) / T = 0 * inf, NaN without the `l == mx` guard"""
    V, T = 1025, 1e-45
    raw = RC.row(name, V)
    ex = R.Exact(raw, float(np.float32(T)))
    assert ex.m_t > 1
    seeds = [3, 11, 19, R.SEED_U_ZERO, R.SEED_U_MAX]
    want = [ex.mirostat(20.0, AC.TAU, AC.ETA, s) for s in seeds]
    assert len({w[0] for w in want}) > 1
    for label, buf, stride in layouts(ctx, np.tile(raw, (len(seeds), 1))):
        got, mu2 = sample(ctx, buf, V, stride, np.full(len(seeds), T), np.ones(len(seeds)), seeds, mirostat=(AC.TAU, AC.ETA, 20.0))
        assert got.tolist() == [w[0] for w in want], (name, label)
        assert all(abs(float(m) - w[1]) <= w[2] for m, w in zip(mu2, want)), (name, label, mu2, want)


@pytest.mark.parametrize("V", RC.VOCABS)
@pytest.mark.parametrize("name", [n for n in NAMES if n not in RC.NOT_TYPICAL])
def test_typical(ctx, name, V):
    raw, cases, want = R.typical_cases(name, V)
    T, tp, seed = columns(cases)
    for label, buf, stride in layouts(ctx, np.tile(raw, (len(cases), 1))):
        got = sample(ctx, buf, V, stride, T, np.full(len(cases), AC.TOP_P), seed, typical_p=tp)
        R.compare((name, V, label), got, want, cap=1.0 if name in RC.EXACT else 0.95)


def test_big_vocabulary(ctx):
    """V = 2^20, SAMPLE_MAX_VOCAB: W = 2^60 on the constant row, whose u = 1 - 2^-24 draw is the last index"""
    cases = R.big_cases()
    rows = np.stack([RC.row(c[0], RC.BIG_V) for c in cases])
    _, T, P, seed, want = columns(cases)
    for label, buf, stride in layouts(ctx, rows):
        got = sample(ctx, buf, RC.BIG_V, stride, T, P, seed)
        assert got.tolist() == [int(w) for w in want], (label, [c[0] for c in cases])


# ----------------------------------------------------------------------------- 2. temperature and top-p edges
@pytest.mark.parametrize("V", R.EDGE_VOCABS)
@pytest.mark.parametrize("name", R.EDGE_PROFILES)
def test_temperature_and_top_p_edges(ctx, name, V):
    """T in {1e-45, 1.2e-38, 1e-30, 1e-3, 1e3, 3e38} x top_p in {1e-45, 1e-30, 1 - 2^-24, 1, 7, +inf}: 1 / T is +inf or subnormal at the
    ends, P * sum overflows nothing"""
    raw, cases, want = R.edge_cases(name, V)
    T, P, seed = columns(cases)
    clear, total = R.edge_cap(cases, want)
    assert clear >= 0.95 * total
    for label, buf, stride in layouts(ctx, np.tile(raw, (len(cases), 1))):
        got = sample(ctx, buf, V, stride, T, P, seed)
        R.compare((name, V, label), got, want, cap=0.0)


def test_infinite_temperature_is_rejected(ctx):
    """1 / T = 0 would turn a -inf logit inside the nucleus into (-inf) * 0 = NaN and a NaN into an integer mass: a non-finite
    temperature is an argument error in every mode, here on a half-masked row with top_p = 1"""
    V = 1025
    raw = RC.row("nan_mix", V)
    x = np.tile(raw, (2, 1))
    for kw in ({}, dict(top_k=40), dict(mirostat=(5.0, 0.1, None)), dict(typical_p=0.5)):
        for T in (np.inf, [1.0, np.inf]):
            with pytest.raises(wrk.WrkError) as e:
                ctx.sample_logits(x, T, 1.0, seed=3, step=R.STEP, **kw)
            assert e.value.code == wrk.E_ARG, kw
        out = ctx.sample_logits(x, 3e38, 1.0, seed=3, step=R.STEP, **kw)          # the largest finite temperatures still draw
        assert (np.asarray(out[0] if isinstance(out, tuple) else out) < V).all()
    rt = wrk.Runtime(ctx, wrk.GgufReader(synth.make_v7_gguf(synth.CONFIGS["tiny"], 42)), num_batch=1)
    with pytest.raises(wrk.WrkError) as e:
        rt.generate_sample([1], 2, temperature=np.inf, top_p=1.0)
    assert e.value.code == wrk.E_ARG
    rt.close()


# ----------------------------------------------------------------------------- 3. greedy agreement
@pytest.mark.parametrize("name", NAMES)
def test_greedy_agreement(ctx, name):
    """sample_logits(T = 0), score_logits' rank 0 and top_logprobs' first id name one token: the first index of the maximum after
    row_norm, or 0 when nothing exceeds -3e38.  A row with a NaN leaves top_ids unspecified."""
    for V in RC.VOCABS:
        raw = RC.row(name, V)
        want = R.greedy(raw)
        for label, buf, stride in layouts(ctx, raw):
            for T, P in ((0.0, 0.9), (1.0, 0.0)):
                assert sample(ctx, buf, V, stride, [T], [P], [1]).tolist() == [want], (name, V, label)
            assert sample(ctx, buf, V, stride, [1.3], [0.9], [1], top_k=[1], min_p=[0.3]).tolist() == [want], (name, V, label)
            _, rk = ctx.score_logits(buf, [want], num_vocab=V, row_stride=stride)
            assert rk.tolist() == [0], (name, V, label)
            if not np.isnan(raw).any():
                _, ids, _ = ctx.top_logprobs(buf, [want], 1, num_vocab=V, row_stride=stride)
                assert ids.tolist() == [[want]], (name, V, label)


# ----------------------------------------------------------------------------- 4. score and log-probs
def judge(kernel, name, got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (kernel, name, got, want)
    ok = SC.within_bar(got, want)
    with np.errstate(invalid="ignore"):
        ratio = np.abs(got - want) / (1e-5 + 1e-6 * np.abs(want))
    fin = np.isfinite(got) & np.isfinite(want)
    worst = float(ratio[fin].max()) if fin.any() else 0.0
    print(f"{kernel} {name}: worst error / bar = {worst:.4g}")
    WORST[(kernel, name)] = max(WORST.get((kernel, name), 0.0), worst)
    assert ok.all(), (kernel, name, got[~ok], want[~ok])


@pytest.mark.parametrize("V", SCORE_VOCABS)
@pytest.mark.parametrize("name", NAMES)
def test_score_and_top_logprobs(ctx, name, V):
    """Targets on the maximum, a tied maximum, a -inf, a NaN, the lowest finite value and the last index.  Log-probs: score_ref's bar
    against the f64 value rounded to f32 (-6e38 is -inf there, as in the kernel's f32); a +inf anywhere: NaN.  Ranks and ids: exact."""
    raw = RC.row(name, V)
    tg = R.targets_for(raw)
    lp_want, rk_want = R.score_expected(raw, tg)
    tlp_lp, ids_want, tlp_want = R.top_expected(raw, tg, NUM_TOP)
    for label, buf, stride in layouts(ctx, np.tile(raw, (len(tg), 1))):
        lp, rk = ctx.score_logits(buf, tg, num_vocab=V, row_stride=stride)
        assert rk.tolist() == rk_want.tolist(), (name, V, label)
        judge("score", name, lp, lp_want)
        lp2, rk2 = ctx.score_logits(buf, tg, num_vocab=V, row_stride=stride)
        assert np.array_equal(bits(lp), bits(lp2)) and np.array_equal(rk, rk2)
        y, ids, tlp = ctx.top_logprobs(buf, tg, NUM_TOP, num_vocab=V, row_stride=stride)
        judge("logprob", name, y, tlp_lp)
        judge("logprob", name, tlp, np.tile(tlp_want, (len(tg), 1)))
        if ids_want is not None:
            assert (ids == u32(ids_want & 0xFFFFFFFF)[None, :]).all(), (name, V, label, ids[0], ids_want)
        y2, ids2, tlp2 = ctx.top_logprobs(buf, tg, NUM_TOP, num_vocab=V, row_stride=stride)
        assert np.array_equal(bits(y), bits(y2)) and np.array_equal(ids, ids2) and np.array_equal(bits(tlp), bits(tlp2))


# ----------------------------------------------------------------------------- 5. penalties
@pytest.mark.parametrize("V,stride", [(4096, 4096), (4096, 4099), (4097, 4097), (4097, 4100)])
def test_penalize_is_bit_exact(ctx, V, stride):
    """x - (presence + count * frequency) in three roundings over counts {0, 1, 2^24, 3e38, a subnormal} and presence / frequency in
    {0, 1e-45, 3e38}^2, on nan_mix, pos_inf_one (+inf - inf = NaN) and huge_span rows; both forms of the kernel"""
    rng = np.random.default_rng(V + stride)
    pairs = [(ap, af) for ap in (0.0, 1e-45, 3e38) for af in (0.0, 1e-45, 3e38)]
    n = len(pairs)
    ap, af = f32([p[0] for p in pairs]), f32([p[1] for p in pairs])
    occ = wrk.Occurrence(ctx, n, V)
    slots = []
    for b in range(n):
        c = rng.choice(f32([0.0, 1.0, 2.0 ** 24, 3e38, 1e-45]), V)
        fl = rng.integers(0, 4, V).astype(np.uint32)
        fl[0] &= 1
        occ.load(b, c, fl)
        slots.append((c, fl))
    for name in ("nan_mix", "pos_inf_one", "huge_span"):
        raw = RC.row(name, V)
        x = np.empty((n, stride), np.float32)
        x[:, :V] = raw
        x[:, V:] = np.resize(f32(RC.PAD), (n, stride - V))
        buf = ctx.buffer(x.reshape(-1))
        ctx.penalize_logits(buf, occ, ap, af, num_vocab=V, row_stride=stride)
        got = buf.read(np.float32, n * stride).reshape(n, stride)
        for r in range(n):
            want = R.penalize32(raw, slots[r][0], slots[r][1], ap[r], af[r])
            assert np.array_equal(np.isnan(got[r, :V]), np.isnan(want)), (name, r)
            ok = ~np.isnan(want)
            assert np.array_equal(bits(got[r, :V])[ok], bits(want)[ok]), (name, r, pairs[r])
            assert np.array_equal(bits(got[r, V:]), bits(x[r, V:])), (name, r)         # the padding is not touched
    occ.close()


def test_zz_write_worst_ratios():
    """Not a check: prints the worst error / bar per kernel and profile (with -s) and, where WRK_ROWS_EDGES_JSON names a file, writes
    them there, for DESIGN.md."""
    fam = {}
    for (kernel, name), v in WORST.items():
        fam.setdefault(kernel, {})[name] = v
    out = os.environ.get("WRK_ROWS_EDGES_JSON")
    if out:
        with open(out, "w") as f:
            json.dump({"worst_ratio": fam}, f, indent=1, sort_keys=True)
    for kernel, d in sorted(fam.items()):
        print(kernel, "worst error / bar:", max(d.values()), {k: round(v, 4) for k, v in sorted(d.items())})
