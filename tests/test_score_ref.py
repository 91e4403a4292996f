"""CPU checks of sequence scoring: the f64 restatement (tests/score_ref.py) on hand-worked rows, and the host's scoring plan
(`wrk_rnn_score_plan`) against a Python restatement over ragged inputs fed through RnnIter::next / JobInput::step."""
import math

import numpy as np
import pytest

import wrk
import score_ref as R


def test_flat_row():
    lp, rk = R.score_row([0.0, 0.0, 0.0, 0.0], 2)
    assert lp == pytest.approx(-math.log(4.0), abs=1e-15)
    assert rk == 2                                   # two equal logits before it


def test_target_at_the_argmax():
    x = [1.0, 3.0, 2.0]
    lp, rk = R.score_row(x, 1)
    assert rk == 0
    assert lp == pytest.approx(-math.log(1.0 + math.exp(-2.0) + math.exp(-1.0)), abs=1e-15)
    assert R.score_row(x, 0)[1] == 2 and R.score_row(x, 2)[1] == 1


def test_ties_count_lower_indices_only():
    x = [5.0, 1.0, 5.0, 5.0]
    assert [R.score_row(x, t)[1] for t in range(4)] == [0, 3, 1, 2]
    assert R.score_row(x, 0)[0] == pytest.approx(R.score_row(x, 3)[0], abs=0)


def test_minus_infinity():
    x = [0.0, -np.inf, 1.0, -np.inf]
    lp, rk = R.score_row(x, 1)
    assert lp == -np.inf and rk == 2
    assert R.score_row(x, 3)[1] == 3                 # the -inf at index 1 is an equal before it
    lp, _ = R.score_row(x, 2)
    assert lp == pytest.approx(-math.log(1.0 + math.exp(-1.0)), abs=1e-15)   # -inf entries add no mass
    assert R.score_row([-np.inf, -np.inf], 1) == (-np.inf, 1)


def test_nan_anywhere():
    lp, _ = R.score_row([0.0, np.nan, 1.0], 2)
    assert math.isnan(lp)


def test_large_magnitudes():
    x = np.array([3.0e4, 3.0e4 - 1.0, -3.0e4])
    lp, rk = R.score_row(x, 1)
    assert rk == 1
    assert lp == pytest.approx(-1.0 - math.log(1.0 + math.exp(-1.0)), abs=1e-12)
    assert R.score_row(x, 2)[0] == pytest.approx(-6.0e4 - math.log(1.0 + math.exp(-1.0)), rel=1e-15)


def test_rows_agree_with_the_log_softmax():
    rng = np.random.default_rng(3)
    x = rng.normal(0.0, 3.0, (5, 300))
    t = rng.integers(0, 300, 5)
    lp, rk = R.score_rows(x, t)
    np.testing.assert_allclose(lp, R.log_softmax_at(x, t), rtol=0, atol=1e-12)
    assert ((rk == 0) == (x.argmax(axis=1) == t)).all()


def test_bar_helper():
    assert R.within_bar([np.nan, -np.inf, -1.0], [np.nan, -np.inf, -1.0 - 5e-6]).all()
    assert not R.within_bar([-1.0], [-1.0 - 2e-5]).any()


LENGTHS = [0, 1, 2, 31, 33, 70, 129, 300]


def run_plan(seqs, chunk):
    """Walk `seqs` chunk by chunk; check every plan against score_ref.plan; return the targets collected per sequence."""
    inp = wrk.RnnInput(seqs, chunk)
    rem = [list(s) for s in seqs]
    got = [[] for _ in seqs]
    big = False
    while True:
        info = next(inp.iter())
        lens = [l for l, _ in info]
        if sum(lens) == 0:
            break
        assert sum(lens) <= inp.token_chunk_size
        big = big or sum(lens) > 32
        if sum(lens) > 32:
            assert sum(lens) % 32 == 0                 # RnnIter rounds chunks above 32 tokens down to a multiple of 32
        h, t, rows = wrk.score_plan(inp, lens)
        wh, wt, wrows = R.plan(rem, lens)
        assert (h, t, rows) == (wh, wt, wrows)
        p = 0
        for b, n in enumerate(rows):
            got[b].extend(t[p:p + n])
            p += n
        inp.step()
        for b, n in enumerate(lens):
            rem[b] = rem[b][n:]
        assert [inp.remaining(b) for b in range(len(seqs))] == [len(r) for r in rem]
    return got, big


@pytest.mark.parametrize("chunk", [32, 128])
@pytest.mark.parametrize("seed", range(6))
def test_plan_over_ragged_inputs(chunk, seed):
    rng = np.random.default_rng(seed)
    nb = int(rng.integers(1, 6))
    seqs = [rng.integers(0, 1000, int(rng.choice(LENGTHS))).tolist() for _ in range(nb)]
    got, _ = run_plan(seqs, chunk)
    # across chunk boundaries, every token but the first is some position's target, in order
    assert got == [s[1:] for s in seqs]


@pytest.mark.parametrize("chunk", [32, 128])
def test_plan_every_length(chunk):
    seqs = [list(range(100 * i, 100 * i + n)) for i, n in enumerate(LENGTHS)]
    got, big = run_plan(seqs, chunk)
    assert got == [s[1:] for s in seqs]
    assert big == (chunk > 32)


def test_one_token_sequence_has_no_rows():
    inp = wrk.RnnInput([[5], [1, 2]], 32)
    lens = [l for l, _ in next(inp.iter())]
    assert lens == [1, 2]
    assert wrk.score_plan(inp, lens) == ([1], [2], [0, 1])


def test_plan_rejects_a_chunk_longer_than_the_input():
    inp = wrk.RnnInput([[1, 2, 3]], 32)
    with pytest.raises(wrk.WrkError):
        wrk.score_plan(inp, [4])
