"""CPU checks of the sampler restatement (tests/sampling_ref.py) on hand-worked cases, the SplitMix64 known answers, and the exports of
the sampling entry points."""
import numpy as np
import pytest

import wrk
import sampling_ref as S


def logp(*p):
    return np.log(np.asarray(p, np.float64))


def test_splitmix_known_answers():
    assert S.splitmix(0, 0) == 0xE220A8397B1DCDAF
    assert S.uniform(0, 0) == 0.8833107948303223
    assert S.splitmix(0, 1) == 0x910A2DEC89025CC1
    assert S.splitmix(42, 7) == 0x2C582B9E1961250F
    assert S.uniform(42, 7) == 0.17322033643722534
    for s, t in ((0, 0), (5, 9), (0xFFFFFFFF, 0xFFFFFFFF)):
        assert 0.0 <= S.uniform(s, t) < 1.0


def test_zero_top_p_or_temperature_is_argmax():
    l = [1.0, 3.0, 2.0, 3.0, -np.inf]
    for seed in range(8):
        assert S.sample(l, 1.0, 0.0, seed) == 1
        assert S.sample(l, 0.0, 0.9, seed) == 1
    assert S.sample([-np.inf, -np.inf], 0.0, 0.5) == 0       # argmax_rows: nothing above -3e38 -> 0


def test_ties_resolve_to_the_lower_index():
    l = [0.0, 5.0, 5.0, 0.0]
    toks, _, _ = S.nucleus(l, 1.0, 0.01)
    assert toks.tolist() == [1]
    toks, w, _ = S.nucleus(l, 1.0, 0.999)
    assert toks.tolist() == [1, 2, 0, 3]
    assert S.sample(l, 1.0, 0.01, u=0.999) == 1


def test_the_token_that_crosses_top_p_is_included():
    l = logp(0.2, 0.5, 0.3)                 # rank order 1, 2, 0; masses before them 0, 0.5, 0.8
    assert S.nucleus(l, 1.0, 0.55)[0].tolist() == [1, 2]
    assert S.nucleus(l, 1.0, 0.45)[0].tolist() == [1]       # token 1 crosses 0.45 and is in; token 2 starts above it
    assert S.nucleus(l, 1.0, 0.85)[0].tolist() == [1, 2, 0]
    assert S.nucleus(l, 1.0, 1.0)[0].tolist() == [1, 2, 0]
    assert S.nucleus(l, 1.0, 1e-9)[0].tolist() == [1]


def test_temperature_reweights_only_inside_the_nucleus():
    l = logp(0.2, 0.5, 0.3)
    toks, w, _ = S.nucleus(l, 0.5, 0.6)     # nucleus {1, 2}; weights p^2 = 0.25, 0.09
    assert toks.tolist() == [1, 2]
    np.testing.assert_allclose(w, [0.25 / 0.34, 0.09 / 0.34], rtol=1e-12)
    toks, w, _ = S.nucleus(l, 2.0, 0.6)     # p^0.5
    np.testing.assert_allclose(w, np.sqrt([0.5, 0.3]) / np.sqrt([0.5, 0.3]).sum(), rtol=1e-12)
    # token 0 is outside the nucleus: no u draws it, whatever the temperature
    for T in (0.1, 1.0, 10.0):
        assert {S.sample(l, T, 0.6, u=u) for u in np.linspace(0, 0.999999, 101)} <= {1, 2}
    assert S.sample(l, 0.5, 0.6, u=0.25 / 0.34 - 1e-9) == 1
    assert S.sample(l, 0.5, 0.6, u=0.25 / 0.34 + 1e-9) == 2


def test_find_or_first_fallback():
    l = logp(0.2, 0.5, 0.3)
    assert S.sample(l, 1.0, 1.0, u=1.5) == 1       # no rank reaches u * W: rank 0
    assert S.sample(l, 1.0, 1.0, u=0.0) == 1       # u = 0: rank 0


def test_ambiguity_predicate():
    l = logp(0.2, 0.5, 0.3)
    assert S.ambiguous(l, 1.0, 0.5 + 5e-5)         # prefix mass 0.5 within 1e-4 of P
    assert not S.ambiguous(l, 1.0, 0.0)
    flat = np.zeros(65536)
    assert S.ambiguous(flat, 1.0, 1.0)             # edges 1.5e-5 apart: u is always within 1e-5 of one


def test_sampling_symbols_are_exported():
    for name in ("wrk_sample_logits", "wrk_v7_generate_sample", "wrk_v6_generate_sample"):
        assert hasattr(wrk.hip, name), name
        assert name in wrk.HIP_SYMBOLS, name
    assert callable(wrk.Context.sample_logits) and callable(wrk.Runtime.generate_sample)


@pytest.mark.parametrize("T,P", [(0.7, 0.9), (1.0, 0.5), (1.5, 1.0)])
def test_draw_frequencies_follow_the_tempered_nucleus(T, P):
    rng = np.random.default_rng(3)
    l = rng.normal(0, 1.5, 40)
    toks, w, _ = S.nucleus(l, T, P)
    n = 20000
    counts = np.bincount([S.sample(l, T, P, seed=s) for s in range(n)], minlength=l.size)
    assert counts[np.setdiff1d(np.arange(l.size), toks)].sum() == 0
    np.testing.assert_allclose(counts[toks] / n, w, atol=0.015)
