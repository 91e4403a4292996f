"""CPU tests of the automaton bookkeeping of constrained decoding: `wrk.grammar_from_dense`, `wrk.grammar_from_choices`,
`wrk.grammar_walk`, and tests/grammar_ref.py, the restatement the GPU tests hold the kernels to.  No device is touched."""
import numpy as np
import pytest

import grammar_ref as G
import sampling_ref as S
import wrk


def every_state_allows_a_token(cls, trans):
    used = np.zeros(trans.shape[1], bool)
    used[np.asarray(cls, np.int64)] = True
    return all(((trans[s] != G.REJECT) & used).any() for s in range(trans.shape[0]))


# ----------------------------------------------------------------------------- grammar_from_dense
@pytest.mark.parametrize("S_", [1, 3, 40])
@pytest.mark.parametrize("V", [1, 50, 4099])
def test_from_dense_round_trip(S_, V):
    rng = np.random.default_rng(100 * S_ + V)
    for columns in (1, 2, 7):
        table = G.random_dense(rng, S_, V, columns)
        cls, trans = wrk.grammar_from_dense(table)
        assert cls.dtype == np.uint16 and trans.dtype == np.uint16 and cls.shape == (V,) and trans.shape[0] == S_
        assert np.array_equal(G.expand(cls, trans), table)
        distinct = len({table[:, v].tobytes() for v in range(V)})
        assert trans.shape[1] == distinct
        # classes are numbered by first occurrence: the class of token v is new exactly when it is the next unused number
        seen = 0
        for c in cls.tolist():
            assert c <= seen
            seen += c == seen
        assert every_state_allows_a_token(cls, trans)


def test_from_dense_identity_map_when_all_columns_differ():
    table = np.array([[0, 1, -1], [1, -1, 0]])
    cls, trans = wrk.grammar_from_dense(table)
    assert cls.tolist() == [0, 1, 2]
    assert trans.tolist() == [[0, 1, G.REJECT], [1, G.REJECT, 0]]


def test_from_dense_rejects_bad_tables():
    for bad in ([[2]], [[-2]], [], [[]], [0, 1]):
        with pytest.raises(ValueError):
            wrk.grammar_from_dense(bad)
    n = wrk.MAX_TOKEN_CLASSES + 1                                       # more distinct columns than classes: column v = the bits of v
    with pytest.raises(ValueError):
        wrk.grammar_from_dense((np.arange(n)[None, :] >> np.arange(14)[:, None] & 1) - 1)


# ----------------------------------------------------------------------------- grammar_from_choices
CASES = {
    "shared prefixes": ([[5, 6, 7], [5, 6, 9], [5, 2], [11, 6, 7]], 3),
    "a prefix of another": ([[4, 8], [4, 8, 15, 16], [23]], 0),
    "one one-token choice": ([[42]], 41),
    "repeated tokens": ([[7, 7, 7], [7, 7]], 1),
}


@pytest.mark.parametrize("name", list(CASES))
def test_from_choices_accepts_exactly_the_choices(name):
    V = 50
    choices, end = CASES[name]
    cls, trans, start = wrk.grammar_from_choices(V, choices, end)
    assert start == 0 and every_state_allows_a_token(cls, trans)
    for c in choices:
        assert G.accepts(cls, trans, start, c + [end] * 3), c
        final = G.walk(cls, trans, start, c + [end])
        assert G.allowed(cls, trans, final).nonzero()[0].tolist() == [end]          # finished: only end_token, forever
        assert G.walk(cls, trans, final, [end]) == final
    # every one-token deviation of every accepted sequence is rejected, unless it is itself a choice followed by end tokens
    ok = {tuple(c + [end] * k) for c in choices for k in range(1, 6)}
    for c in choices:
        seq = c + [end, end]
        for i in range(len(seq)):
            for t in range(V):
                dev = seq[:i] + [t] + seq[i + 1:]
                if t != seq[i] and tuple(dev) not in ok:
                    assert not G.accepts(cls, trans, start, dev), (dev, c)
    # the prefixes of the choices that are not choices do not allow end_token
    for c in choices:
        for k in range(len(c)):
            if c[:k] not in choices:
                assert not G.accepts(cls, trans, start, c[:k] + [end])


def test_from_choices_on_a_large_vocabulary_stays_small():
    cls, trans, start = wrk.grammar_from_choices(65536, [[70, 65535, 3], [70, 9]], 0)
    assert trans.shape[1] <= 6 and trans.shape[0] == 6
    assert G.accepts(cls, trans, start, [70, 65535, 3, 0, 0]) and not G.accepts(cls, trans, start, [70, 65534])


def test_from_choices_rejects_bad_arguments():
    for args in ((10, [], 1), (10, [[3, 1]], 1), (10, [[10]], 1), (10, [[3]], 10)):
        with pytest.raises(ValueError):
            wrk.grammar_from_choices(*args)


# ----------------------------------------------------------------------------- the walk and the restatement
def test_walk_agrees_with_the_restatement_and_raises_at_the_first_rejected_token():
    rng = np.random.default_rng(5)
    table = G.random_dense(rng, 6, 64, 9)
    cls, trans = wrk.grammar_from_dense(table)
    s, seq = 2, []
    for _ in range(20):
        t = int(rng.choice(np.flatnonzero(table[s] >= 0)))
        seq.append(t)
        s = int(table[s, t])
    assert wrk.grammar_walk(cls, trans, 2, seq) == G.walk(cls, trans, 2, seq) == s
    bad = int(np.flatnonzero(table[s] < 0)[0])
    with pytest.raises(ValueError, match=f"token {len(seq)} "):
        wrk.grammar_walk(cls, trans, 2, seq + [bad, seq[0]])
    assert G.advance(cls, trans, s, bad) == s                                         # the device's rule: a rejected token keeps the state


def test_mask_keeps_bits_and_writes_minus_infinity():
    cls = np.array([0, 1, 1, 0, 2], np.uint16)
    trans = np.array([[0, G.REJECT, 1], [G.REJECT, 0, G.REJECT]], np.uint16)
    row = np.array([0x7FC01234, 0x80000000, 0x00000001, 0xFF800000, 0x477FE000], np.uint32).view(np.float32)     # NaN payload, -0, subnormal, -inf, 65504
    assert G.mask(row, cls, trans, 0).view(np.uint32).tolist() == [0x7FC01234, 0xFF800000, 0xFF800000, 0xFF800000, 0x477FE000]
    assert G.mask(row, cls, trans, 1).view(np.uint32).tolist() == [0xFF800000, 0x80000000, 0x00000001, 0xFF800000, 0xFF800000]


def test_the_reference_loop_draws_only_allowed_tokens():
    rng = np.random.default_rng(9)
    V = 64
    table = G.random_dense(rng, 6, V, 12)
    cls, trans = wrk.grammar_from_dense(table)
    rows = rng.normal(0, 2, (12, V)).astype(np.float32)
    for family, kw in (("greedy", {}), ("sample", dict(temperature=1.1, top_p=0.9, seed=3)), ("filter", dict(temperature=0.9, top_p=1.0, seed=4, top_k=5)),
                       ("mirostat", dict(temperature=1.0, seed=5, tau=3.0, eta=0.2)), ("typical", dict(temperature=1.0, seed=6, typical_p=0.6))):
        toks, _, final = G.loop(lambda i, _: rows[i], cls, trans, 1, G.Pick(family, **kw), 12)
        assert G.walk(cls, trans, 1, toks) == final, family
        if family == "greedy":
            s = 1
            for i, t in enumerate(toks):
                assert t == S.greedy(np.where(table[s] >= 0, rows[i], -np.inf))
                s = int(table[s, t])
