"""tests/logprob_ref.py against independent formulations (no GPU): the f64 restatement against a stable argsort, tests/score_ref.py and
the log-sum-exp identity; the f32 restatement of the kernel's sliced (max, sum) merge and per-slice candidate selection against the f64
one, inside score_ref's kernel bar with equal ids; and two mutants of it that must fall outside."""
import numpy as np
import pytest

import logprob_ref as L
import score_ref as R

ROWS = 15           # three of every row kind, every chosen-token kind on some of them


def logsumexp(a):
    a = np.asarray(a, np.float64)
    m = a.max()
    return m + np.log(np.exp(a - m).sum())


@pytest.mark.parametrize("V", [1, 7, 50, 1000, 5000])
def test_f64_restatement_against_independent_formulations(V):
    x, tok = L.kernel_rows(V, ROWS, V)
    n = min(L.MAX_TOP, V)
    lp, ids, tlp = L.top_rows(x, tok, n)
    for r in range(ROWS):
        row = x[r].astype(np.float64)
        order = sorted(range(V), key=lambda i: (-row[i], i))           # (-x, index), Python's stable sort
        assert ids[r].tolist() == order[:n]
        want_lp, rank = R.score_row(row, int(tok[r]))
        assert lp[r] == want_lp or abs(lp[r] - want_lp) <= 1e-12
        if rank < n:                                                    # a token of score rank r sits at top_ids[r]
            assert ids[r][rank] == tok[r] and tlp[r][rank] == lp[r]
        if row.max() > -np.inf:                                         # a row of nothing but -inf has no distribution
            assert abs(logsumexp(L.log_softmax(row))) <= 1e-12
        assert all(tlp[r][j] >= tlp[r][j + 1] for j in range(n - 1))


def test_more_alternatives_than_tokens_and_inf_rows():
    x = np.array([[0.5, -np.inf, 2.0, 0.5, -np.inf]], np.float32)
    lp, ids, tlp = L.top_rows(x, [1], 8)
    assert lp[0] == -np.inf
    assert ids[0].tolist() == [2, 0, 3, 1, 4, L.NO_ID, L.NO_ID, L.NO_ID]       # -inf after every finite logit, by index
    assert np.isfinite(tlp[0][:3]).all() and (tlp[0][3:] == -np.inf).all()
    assert tlp[0][1] == tlp[0][2]
    lp, ids, tlp = L.top_rows(np.array([[1.0, np.nan, 0.0]], np.float32), [0], 2)
    assert np.isnan(lp[0]) and np.isnan(tlp[0]).all()
    lp, ids, tlp = L.top_rows(x, [2], 0)                                        # n = 0: only logprob
    assert ids.shape == (1, 0) and tlp.shape == (1, 0) and np.isfinite(lp[0])
    lp, ids, tlp = L.top_rows(np.array([[-0.0, 0.0, -0.0]], np.float32), [2], 3)
    assert ids[0].tolist() == [0, 1, 2]                                         # -0 and +0 tie: by index


def sliced(x, tok, n, S, **mutant):
    out = [L.top_row_sliced(row, int(t), n, S, **mutant) for row, t in zip(x, tok)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


@pytest.mark.parametrize("S", [1, 3, 32])
@pytest.mark.parametrize("V,n", [(7, 5), (1000, 20), (5000, 20), (5000, 1)])
def test_f32_sliced_restatement_is_inside_the_kernel_bar(V, n, S):
    x, tok = L.kernel_rows(V, ROWS, 100 + V)
    want_lp, want_ids, want_tlp = L.top_rows(x, tok, n)
    lp, ids, tlp = sliced(x, tok, n, S)
    assert (ids == want_ids).all()
    assert R.within_bar(lp, want_lp).all(), np.abs(lp - want_lp).max()
    assert R.within_bar(tlp, want_tlp).all()
    assert L.slices(1, 65536) == 32 and L.slices(300, 65536) == 4 and L.slices(64, 1000) == 1


def test_a_merge_without_rescaling_falls_outside_the_bar():
    V, n, S = 5000, 5, 3
    x, tok = L.kernel_rows(V, ROWS, 100 + V)
    want_lp, _, want_tlp = L.top_rows(x, tok, n)
    lp, _, tlp = sliced(x, tok, n, S, rescale=False)
    assert not R.within_bar(lp, want_lp).all()
    assert not R.within_bar(tlp, want_tlp).all()


def test_a_tie_break_by_index_descending_gives_other_ids():
    V, n, S = 5000, 5, 3
    x, tok = L.kernel_rows(V, ROWS, 100 + V)
    _, want_ids, _ = L.top_rows(x, tok, n)
    _, ids, _ = sliced(x, tok, n, S, descending_index=True)
    assert not (ids == want_ids).all()
    tied = [r for r in range(ROWS) if r % 5 == 4]                  # the rows with a tied maximum
    assert all((ids[r] != want_ids[r]).any() for r in tied)
