"""tests/typical_ref.py against hand-worked cases, sampling_ref (off rows), an f32 restatement of the device's evaluation and mutants
of the contract; the kernel test's rows leave 95 % of its cases unambiguous."""
import numpy as np
import pytest

import alt_cases as AC
import sampling_ref as S
import typical_ref as TY


def _row():
    # p = (0.5, 0.2, 0.2, 0.05, 0.05): H = 1.2899 nats; -ln p = 0.693, 1.609, 1.609, 2.996, 2.996; d = 0.597, 0.320, 0.320, 1.706, 1.706
    return np.log(np.array([0.5, 0.2, 0.2, 0.05, 0.05]))


def test_hand_worked_row():
    row = TY.Row(_row())
    H = -np.sum(row.p * np.log(row.p))
    assert np.isclose(H, 1.28992, atol=1e-5)
    assert np.allclose(row.d, np.abs(-np.log(row.p) - H))
    assert list(row.torder) == [1, 2, 0, 3, 4]                       # ties by index
    assert np.allclose(row.before, [0.0, 0.2, 0.4, 0.9, 0.95])
    assert [row.count(p) for p in (0.0, 0.1, 0.21, 0.39, 0.41, 0.89, 0.91, 0.99)] == [1, 1, 2, 2, 3, 3, 4, 5]
    # typical_p = 0.3: candidates {1, 2}; in the sampler's order 1 then 2, equal weights
    toks, c = row.candidates(1.0, 0.3)
    assert list(toks) == [1, 2] and np.allclose(c, [0.5, 1.0])
    assert row.sample(1.0, 0.9, 0.3, u=0.4) == 1 and row.sample(1.0, 0.9, 0.3, u=0.6) == 2
    # typical_p = 0.41: the crossing token 0 is in, and the draw goes in the sampler's order: 0 (5/9), 1, 2
    toks, c = row.candidates(1.0, 0.41)
    assert list(toks) == [0, 1, 2] and np.allclose(c, [5 / 9, 7 / 9, 1.0])
    # typical_p = 0: exactly one token, rank 0 of the typical order -- not the arg-max
    assert all(row.sample(1.0, 0.9, 0.0, u=u) == 1 for u in (0.0, 0.5, 0.999))
    # temperature reweights inside the candidates: p^2 = 25 : 4 : 4
    toks, c = row.candidates(0.5, 0.41)
    assert np.allclose(c, np.cumsum([25, 4, 4]) / 33.0)


def test_masked_tokens_and_nan():
    l = np.array([0.0, -np.inf, np.nan, 0.0, -1.0])
    row = TY.Row(l)
    assert np.isinf(row.d[1]) and np.isinf(row.d[2]) and np.isfinite(row.gbar)
    assert set(row.torder[-2:]) == {1, 2}
    assert all(row.sample(1.0, 1.0, 0.99, seed=s) in (0, 3, 4) for s in range(30))


def test_greedy_and_off_rows():
    rng = np.random.default_rng(0)
    l = rng.normal(0, 2, 50).astype(np.float32)
    assert TY.sample(l, 0.0, 0.3, 0.5) == S.greedy(l)
    assert TY.sample(np.full(5, -np.inf), 1.0, 0.3, 0.5) == 0
    for seed in range(20):
        assert TY.sample(l, 0.8, 0.6, 1.0, seed, 3) == S.sample(l, 0.8, 0.6, seed, 3)
        assert TY.ambiguous(l, 0.8, 0.6, 1.0, seed, 3) == S.ambiguous(l, 0.8, 0.6, seed, 3)
    assert TY.sample(l, 0.8, 0.0, 0.5, 4, 3) == TY.sample(l, 0.8, 1.0, 0.5, 4, 3)       # top_p is not read by a typical row


def _cases(V):
    for name, l, g, want in AC.typical_expected(V):
        for (t, p, s), w in zip(g, want):
            yield name, l, t, p, s, w


@pytest.mark.parametrize("V", [1, 50, 1000, 3000])
def test_f32_restatement_agrees_on_the_clear_cases(V):
    n = 0
    for name, l, t, p, s, w in _cases(V):
        if w is None or p >= 1.0:
            continue
        assert TY.sample32(l, t, p, s, AC.STEP) == w, (V, name, t, p, s)
        n += 1
    assert n


def test_mutants_disagree():
    """the crossing token left out, d without the absolute value, the draw made in typical order: each changes tokens of clear cases"""
    for kw in ({"crossing_out": True}, {"signed": True}, {"typical_order_draw": True}):
        diff = total = 0
        for name, l, g, want in AC.typical_expected(1000):
            bad = TY.Row(l, **kw)
            for (t, p, s), w in zip(g, want):
                if w is None or p >= 1.0:
                    continue
                total += 1
                diff += bad.sample(t, AC.TOP_P, p, s, AC.STEP) != w
        assert diff >= total // 10, (kw, diff, total)
    row = TY.Row(_row(), crossing_out=True)
    assert list(row.candidates(1.0, 0.41)[0]) == [1, 2]
    row = TY.Row(_row(), signed=True)
    assert row.torder[0] == 0
    row = TY.Row(_row(), typical_order_draw=True)
    assert list(row.candidates(1.0, 0.41)[0]) == [1, 2, 0]


@pytest.mark.parametrize("V", AC.VOCABS)
def test_the_gpu_rows_leave_95_percent_of_the_cases_clear(V):
    want = [w for _, _, _, ws in AC.typical_expected(V) for w in ws]
    assert len(want) == 4 * len(AC.TYPICAL_PS) * len(AC.TEMPS) * len(AC.SEEDS)
    clear = sum(w is not None for w in want)
    assert clear >= 0.95 * len(want), (V, clear, len(want))


def test_the_slack_is_the_derived_one():
    assert 1.0e-5 < TY.gbar_slack(65536) < 2.0e-5 and TY.gbar_slack(2 ** 20) < 4.0e-5
