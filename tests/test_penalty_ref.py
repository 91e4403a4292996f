"""Hand-worked cases of the repetition-penalty restatement (tests/penalty_ref.py)."""
import numpy as np

import penalty_ref as R

f32 = np.float32


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_decay_then_add():
    c = np.array([2.0, 4.0, 0.0], np.float32)
    f = np.zeros(3, np.uint32)
    w = np.array([1.0, 3.0, 1.0], np.float32)
    c2, f2 = R.update(c, f, 1, w, 0.5)
    assert c2.tolist() == [1.0, 2.0 + 3.0, 0.0]          # decayed first, then the drawn token's weight: not (4 + 3) * 0.5
    assert f2.tolist() == [0, R.PRESENT, 0]
    assert c.tolist() == [2.0, 4.0, 0.0] and f.tolist() == [0, 0, 0]      # inputs untouched
    c3, f3 = R.update_all(c, f, [1, 1], w, 0.5)
    assert c3.tolist() == [0.5, (4.0 * 0.5 + 3.0) * 0.5 + 3.0, 0.0]
    assert f3.tolist() == [0, R.PRESENT, 0]


def test_weight_zero_token_gets_only_the_presence_penalty():
    w = np.array([0.0, 1.0], np.float32)
    c, f = R.update(np.zeros(2, np.float32), np.zeros(2, np.uint32), 0, w, 1.0)
    assert c.tolist() == [0.0, 0.0] and f.tolist() == [R.PRESENT, 0]
    x = np.array([3.0, 3.0], np.float32)
    assert R.penalize(x, c, f, 0.25, 7.0).tolist() == [2.75, 3.0]


def test_penalty_expression_and_rounding():
    x = np.array([1.0, 1.0, 1.0], np.float32)
    c = np.array([3.0, 0.1, 2.0], np.float32)
    f = np.array([R.PRESENT, R.PRESENT, 0], np.uint32)
    y = R.penalize(x, c, f, 0.2, 0.3)
    want0 = f32(1.0) - (f32(0.2) + f32(3.0) * f32(0.3))
    want1 = f32(1.0) - (f32(0.2) + f32(0.1) * f32(0.3))
    assert bits(y).tolist() == bits([want0, want1, 1.0]).tolist()
    assert y.dtype == np.float32


def test_banned_is_minus_infinity():
    x = np.array([5.0, np.nan, -1.0, 2.0], np.float32)
    f = np.array([R.BANNED, R.BANNED, R.BANNED | R.PRESENT, 0], np.uint32)
    y = R.penalize(x, np.full(4, 9.0, np.float32), f, 1.0, 1.0)
    assert y[:3].tolist() == [-np.inf] * 3 and y[3] == 2.0


def test_zero_penalties_are_the_identity_bit_for_bit():
    rng = np.random.default_rng(3)
    x = rng.normal(0, 3, 64).astype(np.float32)
    x[[1, 7]] = np.nan
    x[[2, 9]] = -np.inf
    x[3] = np.inf
    x[4] = -0.0
    c = rng.uniform(0, 5, 64).astype(np.float32)
    f = rng.integers(0, 2, 64).astype(np.uint32)          # present or not, nothing banned
    f[[1, 2, 3, 4]] = R.PRESENT
    assert bits(R.penalize(x, c, f, 0.0, 0.0)).tolist() == bits(x).tolist()


def test_negative_frequency_raises_a_present_token():
    x = np.array([1.0, 1.0], np.float32)
    y = R.penalize(x, np.array([2.0, 2.0], np.float32), np.array([R.PRESENT, 0], np.uint32), 0.0, -0.5)
    assert y.tolist() == [2.0, 1.0]
    y = R.penalize(x, np.array([2.0, 0.0], np.float32), np.array([R.PRESENT, 0], np.uint32), -1.0, 0.0)
    assert y.tolist() == [2.0, 1.0]                      # negative presence too


def test_decay_zero_keeps_only_the_last_token():
    w = np.ones(4, np.float32)
    c, f = R.update_all(np.array([5.0, 1.0, 0.0, 2.0], np.float32), np.zeros(4, np.uint32), [0, 2, 2, 1], w, 0.0)
    assert c.tolist() == [0.0, 1.0, 0.0, 0.0]
    assert f.tolist() == [R.PRESENT, R.PRESENT, R.PRESENT, 0]     # presence stays once set


def test_decay_one_is_a_plain_count():
    w = np.array([1.0, 0.5, 2.0], np.float32)
    c, f = R.update_all(np.zeros(3, np.float32), np.zeros(3, np.uint32), [2, 1, 2, 2], w, 1.0)
    assert c.tolist() == [0.0, 0.5, 6.0] and f.tolist() == [0, R.PRESENT, R.PRESENT]
