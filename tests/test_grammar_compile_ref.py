"""tests/grammar_compile_ref.py (the reference of wrk_grammar_compile) on hand-built automata with known answers, and the
package's host-side pieces that need no device: `wrk.ByteDfa` and `wrk.regex_of_choices`."""
import re

import numpy as np
import pytest

import grammar_compile_ref as R
import grammar_ref as G
import wrk

REJECT = R.REJECT


def dfa(num_states, edges, accepting):
    """next [S][256] from {(state, byte string of alternatives): target}"""
    nx = np.full((num_states, 256), REJECT, np.int64)
    for (s, chars), t in edges.items():
        for c in chars:
            nx[s, c] = t
    acc = np.zeros(num_states, np.uint8)
    acc[list(accepting)] = 1
    return nx, acc


AB_STAR_C = dfa(2, {(0, b"ab"): 0, (0, b"c"): 1}, [1])         # (a|b)*c


def test_dense_table_by_hand():
    nx, acc = AB_STAR_C
    vocab = [b"", b"a", b"c", b"ab", b"bc", b"cc", b"abca", b"x", b""]      # token 0: the end token; token 8: an empty token
    t = R.dense_table(nx, acc, vocab, 0)
    assert t.tolist() == [
        [-1, 0, 1, 0, 1, -1, -1, -1, -1],       # cc and abca die on their last byte, x on its first; the empty token is allowed nowhere
        [2, -1, -1, -1, -1, -1, -1, -1, -1],    # accepting: only the end token, to FINAL
        [2, -1, -1, -1, -1, -1, -1, -1, -1],    # FINAL loops on the end token
    ]
    assert np.array_equal(R.dense_table_numpy(nx, acc, vocab, 0), t)


def test_end_token_bytes_are_ignored():
    nx, acc = AB_STAR_C
    vocab = [b"a", b"c", b"a"]                  # the end token spells "a", as token 0 does
    t = R.dense_table(nx, acc, vocab, 2)
    assert t.tolist() == [[0, 1, -1], [-1, -1, 2], [-1, -1, 2]]
    cls, trans, starts, fin = R.compile_ref(nx, acc, [0], vocab, 2, wrk.grammar_from_dense)
    assert cls.tolist() == [0, 1, 2] and starts == [0] and fin == 2
    assert trans.tolist() == [[0, 1, REJECT], [REJECT, REJECT, 2], [REJECT, REJECT, 2]]


def test_trim_removes_states_the_vocabulary_cannot_leave():
    # a(bc|de)f: 0 -a-> 1, 1 -b-> 2 -c-> 4, 1 -d-> 3 -e-> 4, 4 -f-> 5 (accepting)
    nx, acc = dfa(6, {(0, b"a"): 1, (1, b"b"): 2, (2, b"c"): 4, (1, b"d"): 3, (3, b"e"): 4, (4, b"f"): 5}, [5])
    vocab = [b"<end>", b"a", b"bc", b"d", b"f", b"ab", b"e!"]               # no single b, c, e: state 2 is never entered, 3 never left
    t = R.dense_table(nx, acc, vocab, 0)
    assert t[3].tolist() == [-1] * 7 and t[1, 3] == 3 and t[0, 5] == 2 and t[2].tolist() == [-1] * 7
    out, starts, fin = R.token_trim(t, [0])
    # states 2 and 3 go; a leads to 1, bc from there to 4 (now 2), f to 5 (now 3), end to FINAL (now 4); d and ab lead nowhere now
    assert starts == [0] and fin == 4 and out.shape == (5, 7)
    assert out.tolist() == [
        [-1, 1, -1, -1, -1, -1, -1],
        [-1, -1, 2, -1, -1, -1, -1],
        [-1, -1, -1, -1, 3, -1, -1],
        [4, -1, -1, -1, -1, -1, -1],
        [4, -1, -1, -1, -1, -1, -1],
    ]
    cls, trans, starts, fin = R.compile_ref(nx, acc, [0], vocab, 0, wrk.grammar_from_dense)
    assert cls.tolist() == [0, 1, 2, 3, 4, 3, 3]                            # d, ab and e! now share the all-REJECT column
    assert trans.shape == (5, 5) and (trans[:, 3] == REJECT).all()
    assert G.accepts(cls, trans, 0, [1, 2, 4, 0, 0]) and not G.accepts(cls, trans, 0, [1, 3])
    for s in range(5):
        assert (trans[s] != REJECT).any()                                   # wrk_grammar_create's rule holds by construction


def test_trim_is_a_fixed_point_over_chains():
    # 0 -a-> 1 -b-> 2 -c-> 3 -d-> 4 (accepting), the vocabulary lacks d: 3 goes, then nothing leaves 2, 1, 0 either
    nx, acc = dfa(5, {(0, b"a"): 1, (1, b"b"): 2, (2, b"c"): 3, (3, b"d"): 4}, [4])
    with pytest.raises(R.Unspellable) as e:
        R.compile_ref(nx, acc, [0], [b"", b"a", b"b", b"c"], 0, wrk.grammar_from_dense)
    assert e.value.pattern == 0


def test_unspellable_pattern_names_its_index():
    # two patterns in one automaton: "ab" (states 0-2) and "xy" (states 3-5)
    nx, acc = dfa(6, {(0, b"a"): 1, (1, b"b"): 2, (3, b"x"): 4, (4, b"y"): 5}, [2, 5])
    vocab = [b"", b"a", b"b", b"x"]
    with pytest.raises(R.Unspellable) as e:
        R.compile_ref(nx, acc, [0, 3], vocab, 0, wrk.grammar_from_dense)
    assert e.value.pattern == 1
    cls, trans, starts, fin = R.compile_ref(nx, acc, [0, 3], vocab + [b"xy"], 0, wrk.grammar_from_dense)
    assert starts == [0, 3] and fin == 5            # 0 1 2 | 3 . 5 -> 0 1 2 | 3 4 | FINAL: state 4 (after x) goes, xy still spells it
    assert G.walk(cls, trans, 3, [4, 0]) == fin and not G.accepts(cls, trans, 3, [3])


def test_numpy_walk_equals_the_plain_walk():
    rng = np.random.default_rng(5)
    nx = rng.integers(0, 40, (40, 256))
    nx[rng.random((40, 256)) < 0.7] = REJECT
    acc = (rng.random(40) < 0.3).astype(np.uint8)
    vocab = R.synthetic_vocab(11, 400)
    assert np.array_equal(R.dense_table(nx, acc, vocab, 7), R.dense_table_numpy(nx, acc, vocab, 7))


# ----------------------------------------------------------------------------- the package, host side
def test_byte_dfa_from_regex_and_arrays():
    d = wrk.ByteDfa.from_regex(["(a|b)*c", "é"])
    assert d.num_states == 5 and d.starts.tolist() == [0, 2] and d.accepting.tolist() == [0, 1, 0, 0, 1]
    nx, acc = AB_STAR_C
    assert np.array_equal(d.next[:2], nx)
    assert R.dfa_accepts(d.next, d.accepting, 2, "é".encode()) and not R.dfa_accepts(d.next, d.accepting, 2, b"\xc3")
    e = wrk.ByteDfa.from_arrays(d.next, d.accepting, d.starts)
    assert np.array_equal(e.next, d.next) and np.array_equal(e.accepting, d.accepting) and np.array_equal(e.starts, d.starts)
    assert wrk.ByteDfa.from_regex("a+").num_patterns == 1
    with pytest.raises(wrk.WrkError) as err:
        wrk.ByteDfa.from_regex(["a", "b(?=c)"])
    assert err.value.code == wrk.E_UNSUPPORTED and "pattern 1: unsupported: look-around at offset 1" in str(err.value)
    with pytest.raises(wrk.WrkError) as err:
        wrk.ByteDfa.from_regex("(a")
    assert err.value.code == wrk.E_ARG and "offset 0" in str(err.value)
    bad = d.next.copy()
    bad[0, 0] = 5
    with pytest.raises(wrk.WrkError) as err:
        wrk.ByteDfa.from_arrays(bad, d.accepting, d.starts)
    assert err.value.code == wrk.E_ARG
    with pytest.raises(ValueError):
        wrk.ByteDfa.from_arrays(d.next[:, :255], d.accepting, d.starts)


def test_regex_of_choices_escapes_only():
    choices = ["a.b", "x|y", "(1+1)*[2]{3}?", "tab\there", "naïve", b"\xff\x00raw", "back\\slash^$"]
    pat = wrk.regex_of_choices(choices)
    assert pat.isascii() and pat.count("|") == len(choices)          # one unescaped | per junction, one escaped inside x|y
    d = wrk.ByteDfa.from_regex(pat)
    for c in choices:
        raw = c.encode() if isinstance(c, str) else c
        assert R.dfa_accepts(d.next, d.accepting, 0, raw), c
        assert not R.dfa_accepts(d.next, d.accepting, 0, raw + b"!") and not R.dfa_accepts(d.next, d.accepting, 0, raw[:-1])
    assert not R.dfa_accepts(d.next, d.accepting, 0, b"aXb")
    ascii_only = [c for c in choices if isinstance(c, str) and c.isascii()]
    for c in ascii_only:                                             # for ASCII choices `re` reads the same pattern the same way
        assert re.fullmatch(wrk.regex_of_choices(ascii_only), c)
    with pytest.raises(ValueError):
        wrk.regex_of_choices([])
