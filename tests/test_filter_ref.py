"""Hand-worked cases of tests/filter_ref.py, the restatement the filtered device sampler (top-k / min-p) is held to, the check that
the GPU test's rows leave enough unambiguous cases, and the declarations of the ABI."""
import math
import os
import re

import numpy as np
import pytest

import filter_cases as FC
import filter_ref as F
import sampling_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN = math.log


def test_a_tie_across_the_top_k_boundary_keeps_the_lower_index():
    l = [1.0, 3.0, 2.0, 2.0, 0.0]                   # order 1, 2, 3, 0, 4
    toks, w = F.candidates(l, 1.0, 1.0, top_k=2)
    assert toks.tolist() == [1, 2]
    e = np.exp([0.0, -1.0])
    assert np.allclose(w, e / e.sum())
    assert F.candidates(l, 1.0, 1.0, top_k=3)[0].tolist() == [1, 2, 3]
    # exactly top_k tokens survive however many tie
    assert F.candidates([5.0] * 6, 1.0, 1.0, top_k=4)[0].tolist() == [0, 1, 2, 3]
    # the draw: u below the first weight is token 1, above it token 2
    assert F.sample(l, 1.0, 1.0, top_k=2, u=0.5) == 1
    assert F.sample(l, 1.0, 1.0, top_k=2, u=0.9) == 2


def test_top_k_larger_than_the_number_of_finite_logits():
    ninf = -np.inf
    l = [ninf, 2.0, ninf, 1.0, ninf, ninf]
    toks, w = F.candidates(l, 1.0, 1.0, top_k=4)
    assert toks.tolist() == [1, 3, 0, 2]            # the -inf tokens inside the prefix, by index
    assert w[2] == 0.0 and w[3] == 0.0
    for u in (0.0, 0.3, 0.9, 1.0):
        assert F.sample(l, 1.0, 1.0, top_k=4, u=u) in (1, 3)


def test_top_k_off_values_and_top_k_one():
    l = np.array([0.5, 2.0, 2.0, -1.0], np.float32)
    for k in (0, 4, 5, 2 ** 32 - 1):
        assert F.top_k_count(k, 4) == 4
        for u in (0.1, 0.6, 0.95):
            assert F.sample(l, 0.8, 0.9, top_k=k, u=u) == S.sample(l.astype(np.float64), 0.8, 0.9, u=u)
    assert F.sample(l, 0.8, 0.9, top_k=1, u=0.99) == 1                      # the arg-max: the first index of the maximum
    assert F.sample([-3.2e38, -3.3e38], 1.0, 1.0, top_k=1) == 0             # argmax_rows: 0 when nothing exceeds -3e38
    assert not F.ambiguous(l, 0.8, 0.9, top_k=1)


def test_min_p_one_keeps_exactly_the_maxima():
    l = [1.0, 4.0, 3.999, 4.0, -np.inf]
    assert F.min_p_count(l, 1.0) == 2
    assert F.candidates(l, 1.0, 1.0, min_p=1.0)[0].tolist() == [1, 3]
    assert F.min_p_count(l, 0.0) == 5                                       # off: the -inf token too
    assert F.ln_min_p(0.0) == -np.inf and F.ln_min_p(1.0) == 0.0
    assert F.ln_min_p(0.05) == np.float32(LN(float(np.float32(0.05))))


def test_min_p_is_an_f32_comparison_of_logit_differences():
    lnh = F.ln_min_p(0.5)
    mx = np.float32(3.0)
    at = np.float32(mx + lnh)                       # candidates around the threshold, decided by fl32(l - mx) >= lnh alone
    row = np.array([mx, at, np.nextafter(at, np.float32(-np.inf)), np.nextafter(at, np.float32(np.inf))], np.float32)
    want = int(np.count_nonzero((row - mx).astype(np.float32) >= lnh))
    assert F.min_p_count(row, 0.5) == want
    assert 2 <= want <= 4


def test_each_cut_binds_in_its_own_case():
    l = np.log(np.array([0.4, 0.3, 0.15, 0.1, 0.05]))
    r = F.Row(l)
    assert r.counts(0.5, 4, 0.2) == (2, 4, 4)       # before = 0, .4, .7, ...: the nucleus binds
    assert r.candidates(1.0, 0.5, 4, 0.2)[0].tolist() == [0, 1]
    assert r.counts(0.97, 3, 0.2) == (5, 3, 4)      # top-k binds
    assert r.candidates(1.0, 0.97, 3, 0.2)[0].tolist() == [0, 1, 2]
    assert r.counts(0.97, 4, 0.5) == (5, 4, 2)      # min-p binds: 0.3 / 0.4 >= 0.5 > 0.15 / 0.4
    toks, c = r.candidates(2.0, 0.97, 4, 0.5)
    assert toks.tolist() == [0, 1]
    w = np.array([0.4, 0.3]) ** 0.5                 # p^(1/T) inside the candidates
    assert np.allclose(c, np.cumsum(w / w.sum()))
    # the nucleus is not renormalised after the other cuts: with top_k = 2 the mass before rank 1 stays 0.4
    assert r.counts(0.39, 2, 0.0)[0] == 1


def test_filters_off_is_sampling_ref():
    rng = np.random.default_rng(3)
    for V in (1, 7, 300):
        l = rng.normal(0, 2, V).astype(np.float32)
        l[rng.random(V) < 0.2] = -np.inf
        l[0] = 1.0
        for T, P in ((0.7, 0.3), (1.0, 0.9), (1.5, 1.0), (0.0, 0.5), (1.0, 0.0)):
            for seed in range(12):
                a = F.sample(l, T, P, 0, 0.0, seed, 2)
                assert a == S.sample(l.astype(np.float64), T, P, seed, 2)
                assert a == F.sample(l, T, P, V + 3, 0.0, seed, 2)
    assert F.sample([-np.inf, np.nan], 1.0, 0.9, top_k=0, min_p=0.3) == 0


@pytest.mark.parametrize("V", FC.VOCABS)
def test_the_gpu_rows_leave_95_percent_of_the_cases_clear(V):
    for name, _, g, want in FC.expected(V):
        assert len(g) == 9 * 4 * 3 * 3 * 2
    total = sum(len(w) for _, _, _, w in FC.expected(V))
    clear = sum(x is not None for _, _, _, w in FC.expected(V) for x in w)
    assert clear >= 0.95 * total, (V, clear, total)


def test_filtered_entry_point_is_declared_exported_and_bound():
    import wrk
    text = open(os.path.join(ROOT, "include", "wrk_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(wrk_[a-z0-9_]+)\s*\(", text))
    name = "wrk_sample_logits_filtered"
    assert name in declared and hasattr(wrk.hip, name) and name in wrk.HIP_SYMBOLS
    assert len(wrk.HIP_SYMBOLS[name][1]) == 12
    for cname, cls in (("wrk_generate_options", wrk.GenerateOptions), ("wrk_queue_options", wrk.QueueOptions)):
        body = re.search(r"typedef\s+struct\s+" + cname + r"\s*\{(.*?)\}", text, flags=re.S).group(1)
        names = [n for stmt in body.split(";") if stmt.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", stmt.strip())]
        assert names == [n for n, _ in cls._fields_], cname
        assert names[-2:] == ["top_k", "min_p"]
