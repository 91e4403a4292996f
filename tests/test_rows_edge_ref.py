"""CPU checks of tests/rows_edge_ref.py and tests/rows_edge_cases.py: `canonical` by hand, the integer closed form of the exact-weight
rows against sampling_ref / filter_ref / typical_ref / mirostat_ref on small rows, the 95 % condition of every (ordinary profile, V,
mode) as a property of the references alone, the committed end-of-range seeds, and four deliberately wrong readings of the contract
that the same comparisons reject."""
import math

import numpy as np
import pytest

import alt_cases as AC
import filter_ref as F
import mirostat_ref as M
import rows_edge_cases as RC
import rows_edge_ref as R
import sampling_ref as S
import typical_ref as TY

INF, NAN = np.inf, np.nan


def nan32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


# ----------------------------------------------------------------------------- canonical, by hand
def test_canonical_by_hand():
    row = np.array([1.0, nan32(0xFFC00001), -0.0, -INF, nan32(0x7F800001), 2.5], np.float32)
    c = R.canonical(row)
    assert c.tolist() == [1.0, -INF, -0.0, -INF, -INF, 2.5] and np.signbit(c[2])
    row = np.array([3.0e38, INF, NAN, -INF, INF, 0.0], np.float32)
    assert R.canonical(row).tolist() == [-INF, 0.0, -INF, -INF, 0.0, -INF]
    assert R.canonical(np.array([-INF, NAN], np.float32)).tolist() == [-INF, -INF]
    assert R.canonical(np.array([INF], np.float32)).tolist() == [0.0]
    assert row[1] == INF                                    # the input is not modified


def test_greedy_by_hand():
    assert R.greedy(np.array([NAN, 1.0, 1.0], np.float32)) == 1
    assert R.greedy(np.array([-0.0, 0.0, -1.0], np.float32)) == 0           # -0 ties with +0: the first index
    assert R.greedy(np.array([-3.2e38, -INF, NAN], np.float32)) == 0        # nothing above -3e38
    assert R.greedy(np.array([-INF, -3.2e38, -2.9e38], np.float32)) == 2
    assert R.greedy(np.array([5.0, INF, INF], np.float32)) == 1


def test_every_profile_is_what_its_name_says():
    for V in RC.VOCABS:
        x = RC.row("nan_mix", V)
        if V >= 1024:
            bits = x.view(np.uint32)
            assert 0.2 < np.isnan(x).mean() < 0.4 and 0.1 < (x == -INF).mean() < 0.3
            assert all((bits == b).any() for b in RC.NAN_BITS)
        assert (RC.row("pos_inf_one", V) == INF).sum() == 1
        assert (RC.row("pos_inf_ties", V) == INF).sum() == min(3, V)
        assert np.isfinite(RC.row("one_finite", V)).sum() == 1
        s = RC.row("subnormal", V)
        assert (np.abs(s) < np.finfo(np.float32).tiny).all()
        z = RC.row("signed_zero_floor", V)
        if V >= 1024:
            assert ((s == 0) & np.signbit(s)).any() and ((s == 0) & ~np.signbit(s)).any()
            assert ((z == 0) & np.signbit(z)).sum() > V // 4 and ((z == 0) & ~np.signbit(z)).sum() > V // 4
            assert (RC.row("huge_span", V) == np.float32(3.0e38)).sum() == 3
        d = RC.row("deep_tail", V)
        assert d.max() <= -30.5 and (np.sort(d)[::-1][min(24, max(1, V // 4)):] <= -60.0).all()
        for off, name in ((1.0e6, "offset_pos"), (-1.0e6, "offset_neg")):
            o = RC.row(name, V).astype(np.float64) - off
            assert np.array_equal(o * 4.0, np.round(o * 4.0))
    buf, stride = RC.strided(np.zeros((2, 5), np.float32))
    assert stride == 8 and buf.reshape(2, 8)[:, 5:].tolist()[0][0] == INF and np.isnan(buf[6]) and buf[7] == 7.0e3


def test_committed_seeds_sit_at_the_ends_of_u():
    assert S.splitmix(R.SEED_U_ZERO, R.STEP) >> 40 == 0
    assert S.splitmix(R.SEED_U_MAX, R.STEP) >> 40 == 2 ** 24 - 1
    assert R.search_seeds(R.STEP, limit=1 << 24) == (R.SEED_U_ZERO, R.SEED_U_MAX)


# ----------------------------------------------------------------------------- the closed form against the f64 references
def small_rows():
    rng = np.random.default_rng(5)
    rows = [np.zeros(7, np.float32), np.full(64, -3.2e38, np.float32), np.full(33, 65504.0, np.float32)]
    z = np.where(rng.random(16) < 0.5, -0.0, 0.0).astype(np.float32)
    z[0], z[1] = -0.0, 0.0
    rows.append(z)
    x = rng.normal(0, 2, 40).astype(np.float32)
    x[[3, 17, 31]] = INF
    x[[5, 9]] = NAN
    rows.append(x)
    x = rng.normal(0, 2, 50).astype(np.float32)
    x[[44, 2, 20]] = 3.0e38
    x[[7, 8]] = -3.0e38
    rows.append(x)
    x = np.full(20, -INF, np.float32)
    x[::3] = NAN
    x[13] = -2.0
    rows.append(x)
    k = rng.integers(-2 ** 20, 2 ** 20, 48)
    x = (k * 2.0 ** -149).astype(np.float32)
    x[10], x[30] = -0.0, 0.0
    rows.append(x)
    x = np.full(64, -1.0e30, np.float32)
    x[rng.random(64) < 0.5] = np.nextafter(np.float32(-1.0e30), np.float32(-INF))
    rows.append(x)
    return rows


def mid_seeds(count, n, salt):
    """seeds whose u sits in the middle half of its interval of a uniform draw over `count` tokens"""
    out, s = [], 1000 * salt
    while len(out) < n:
        u = S.uniform(s, R.STEP)
        if u > 0 and 0.25 < (u * count) % 1.0 < 0.75:
            out.append(s)
        s += 1
    return out


def closed_form_against_references(mutant=None):
    """The comparisons the mutants must fail: the closed form (read with `mutant`) equals the f64 references on the canonical row."""
    checked = 0
    for j, raw in enumerate(small_rows()):
        c = R.canonical(raw)
        assert R.greedy(raw, mutant) == S.greedy(c.astype(np.float64)), j
        frow, trow = F.Row(c), TY.Row(c)
        for T in (0.5, 1.0, 2.0):
            ex = R.Exact(raw, T, mutant)
            mrow = M.Row(c, T)
            for P in (0.05, 0.4, 0.77, 1.0):
                n = ex.nucleus(P)[0]
                for s in mid_seeds(min(n, ex.m_t), 3, j):
                    assert not S.ambiguous(c.astype(np.float64), T, P, s, R.STEP)
                    assert ex.sample(P, s) == S.sample(c.astype(np.float64), T, P, s, R.STEP), (j, T, P, s)
                    checked += 1
                for K, mp in ((2, 0.0), (5, 0.5), (0, 1.0)):
                    cnt = min(n, ex.m_t, F.top_k_count(K, c.size), F.min_p_count(c, mp))
                    for s in mid_seeds(cnt, 2, j):
                        assert ex.sample(P, s, top_k=K, min_p=mp) == frow.sample(T, P, K, mp, s, R.STEP), (j, T, P, K, mp, s)
                        checked += 1
            for tp in (0.2, 0.5, 0.9) if ex.one_value else ():
                cnt = min(ex.m_1, int(math.floor(float(np.float32(tp)) * ex.m_1)) + 1)
                for s in mid_seeds(cnt, 2, j):
                    assert ex.sample(0.7, s, typical_p=tp) == trow.sample(T, 0.7, tp, s, R.STEP), (j, T, tp, s)
                    checked += 1
            for mu in (0.5, 2.5, 20.0):
                cnt = ex.m_t if math.log2(ex.m_t) <= mu else 1
                for s in mid_seeds(cnt, 2, j):
                    tok, mu2, tol = ex.mirostat(mu, AC.TAU, AC.ETA, s)
                    wt, wmu, _ = mrow.step(mu, AC.TAU, AC.ETA, s, R.STEP)
                    assert tok == wt and abs(mu2 - wmu) <= tol, (j, T, mu, s)
                    checked += 1
    return checked


def test_closed_form_equals_the_references_on_small_rows():
    assert closed_form_against_references() > 1000


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_fail_the_same_comparisons(mutant):
    """NaN read as +inf; ties broken by the higher index; +inf ties collapsed to the first; -0 < +0."""
    with pytest.raises(AssertionError):
        closed_form_against_references(mutant)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_change_the_expected_tokens_of_the_profiles(mutant):
    """...and on the profiles themselves: `compare`, the GPU test's comparison, rejects the tokens a mutant reading expects."""
    name = {"nan_pos_inf": "one_finite", "tie_high_index": "all_equal_zero", "inf_ties_first": "pos_inf_ties", "neg_zero_below": "subnormal"}[mutant]
    V = 2 if mutant == "neg_zero_below" else 1025
    raw = RC.row(name, V)
    if mutant == "neg_zero_below":
        raw = np.array([-0.0, 0.0], np.float32)
        want = [R.Exact(raw, 1.0).sample(1.0, s) for s in range(8)]
        got = [R.Exact(raw, 1.0, mutant).sample(1.0, s) for s in range(8)]
    else:
        _, _, want = R.plain_cases(name, V)
        _, _, got = R.plain_cases(name, V, mutant)
    R.compare(name, want, want)
    with pytest.raises(AssertionError):
        R.compare(name, got, want)


# ----------------------------------------------------------------------------- the caps are conditions on the references
@pytest.mark.parametrize("name", sorted(RC.ORDINARY))
def test_ordinary_profiles_leave_95_percent_unambiguous(name):
    for V in RC.VOCABS:
        modes = [("plain", R.plain_cases), ("filtered", R.filter_cases), ("mirostat", R.mirostat_cases)]
        if name not in RC.NOT_TYPICAL:
            modes.append(("typical", R.typical_cases))
        for mode, fn in modes:
            _, g, want = fn(name, V)
            clear = sum(w is not None for w in want)
            assert clear >= 0.95 * len(want), (name, V, mode, clear, len(want))


@pytest.mark.parametrize("name", sorted(RC.EXACT))
def test_exact_profiles_leave_nothing_out(name):
    for V in RC.VOCABS:
        for fn in (R.plain_cases, R.filter_cases, R.mirostat_cases, R.typical_cases):
            if fn is R.typical_cases and name in RC.NOT_TYPICAL:
                continue
            _, g, want = fn(name, V)
            assert len(want) == len(g) and None not in want, (name, V, fn.__name__)
        seeds = {c[2] for c in R.plain_cases(name, V)[1]}
        assert {R.SEED_U_ZERO, R.SEED_U_MAX} <= seeds


@pytest.mark.parametrize("name", R.EDGE_PROFILES)
def test_temperature_and_top_p_edges_meet_the_cap(name):
    for V in R.EDGE_VOCABS:
        raw, g, want = R.edge_cases(name, V)
        assert len(g) == 72
        clear, total = R.edge_cap(g, want)
        assert total == 68 and clear >= 0.95 * total, (name, V, clear, total)
        for (T, P, s), w in zip(g, want):
            if T <= 1e-30 and name != "pos_inf_ties":
                assert w == R.greedy(raw), (name, V, T, P)          # weight 1 on the maximum alone: exact, whatever the nucleus
        if name == "pos_inf_ties":
            assert None not in want


def test_big_vocabulary_rows():
    """the V = 2^20 cases of the GPU test are exact or unambiguous"""
    for name, T, P, s, w in R.big_cases():
        assert w is not None, (name, T, P, s)
    got = {(n, P): w for n, T, P, s, w in R.big_cases()}
    assert got[("all_equal_zero", 1.0)] == 2 ** 20 - 1 and got[("all_equal_zero", 0.5)] == 2 ** 19


# ----------------------------------------------------------------------------- score, log-probs, penalties
def test_score_and_top_expectations_by_hand():
    x = np.array([0.0, 0.0, -INF, 3.0e38, -3.0e38], np.float32)
    lp, rk = R.score_expected(x, [3, 0, 2, 4])
    assert lp.tolist() == [0.0, float(np.float32(-3.0e38)), -INF, -INF] and rk.tolist() == [0, 1, 4, 3]       # -6e38 rounds to -inf in f32
    lp, rk = R.score_expected(np.array([1.0, INF, -INF], np.float32), [0, 1, 2])
    assert np.isnan(lp).all() and rk.tolist() == [1, 0, 2]
    lp, ids, tlp = R.top_expected(np.array([1.0, NAN, 2.0], np.float32), [0, 2], 2)
    assert ids is None and np.isnan(lp).all() and np.isnan(tlp).all()
    lp, ids, tlp = R.top_expected(np.array([-0.0, 0.0, -1.0], np.float32), [1], 3)
    assert ids.tolist() == [0, 1, 2] and tlp[0] == tlp[1] == lp[0]
    for name in RC.PROFILES:
        t = R.targets_for(RC.row(name, 1025))
        assert len(t) == 6 and t[-1] == 1024


def test_penalize32_is_penalty_ref_and_keeps_edge_values():
    import penalty_ref as PR
    rng = np.random.default_rng(2)
    x = rng.normal(0, 3, 64).astype(np.float32)
    c = rng.integers(0, 5, 64).astype(np.float32)
    fl = rng.integers(0, 4, 64).astype(np.uint32)
    assert np.array_equal(R.penalize32(x, c, fl, 0.3, 0.7), PR.penalize(x, c, fl, 0.3, 0.7))
    one = np.ones(3, np.uint32)
    out = R.penalize32(np.array([INF, 1.0, -3.0e38], np.float32), np.array([3e38, 2.0 ** 24, 1e-45], np.float32), one, 0.0, 3e38)
    assert np.isnan(out[0]) and out[1] == -INF and out[2] == np.float32(-3.0e38)     # inf - inf; 2^24 * 3e38 overflows; a subnormal count
