"""wrk_grammar_compile on the device (web-rwkv-gguf_amd/csrc/wrk_grammar_compile.hip) against tests/grammar_compile_ref.py.

Equality is exact array equality: token_class, transitions, start_states, final_state.  The vocabularies hold every single byte plus
seeded strings of 0, 1, 3, 4, 5, 15, 16, 17 and 64 bytes (16 is the last length that stays in registers) over the bytes the patterns
use, so tokens die on their first, a middle and their last byte; V is 300 to 2 048 and mostly no multiple of 64 or 256.  The tables
cover S = 1, one byte class and 256 byte classes, tables staged in LDS (<= 64 KiB) and tables read through L2, one state tile and
several.  The end-to-end tests run the decode loops of the tiny RWKV-7 and RWKV-6 fixtures (V = 512) under compiled grammars.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import grammar_compile_ref as R
import wrk
from oracle import synth

pytestmark = pytest.mark.gpu

P_ = wrk._ptr
ALPHABET = b"abcdxy019_ -.\n!" + "é中".encode()


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def still_usable(ctx):
    g = wrk.Grammar.compile(ctx, [b"", b"a", b"b"], "a+b", 0)
    assert g.walk(int(g.start_states[0]), [1, 1, 2, 0]) == g.final_state
    g.close()


def check(ctx, dfa, vocab, end, table_fn=R.dense_table):
    want = R.compile_ref(dfa.next, dfa.accepting, dfa.starts.tolist(), vocab, end, wrk.grammar_from_dense, table_fn)
    g = wrk.Grammar.compile(ctx, vocab, dfa, end)
    try:
        assert (g.num_states, g.num_classes) == want[1].shape
        assert np.array_equal(g.token_class, want[0])
        assert np.array_equal(g.transitions, want[1])
        assert g.start_states.tolist() == want[2] and g.final_state == want[3]
        return g.num_states, g.num_classes
    finally:
        g.close()


SEEDS = [b"ab", b"abc", b"abd", b"aab", b"0199", b"no 1!", b"y 19!", b"no", b" 1", b"1!", b"9!x", b"bcd", b"abcx", b"xabc", "éé".encode(),
         "中é".encode(), "a中".encode(), "中".encode()[:2], b"a\n", b"\n\n", b"a_0-", b"..", b"ac", b"abbcd", b"dd"]


@functools.lru_cache(maxsize=None)
def vocabulary(V, seed=3):
    return R.synthetic_vocab(seed, V, alphabet=ALPHABET, seeds=SEEDS)


def test_the_pattern_set(ctx):
    """every pattern of the CPU set, one automaton each, V = 333: a partial wave in the second token tile"""
    vocab = vocabulary(333)                # every single byte is a token, so every pattern can be spelled
    states = sum(check(ctx, wrk.ByteDfa.from_regex(pat), vocab, 300)[0] for pat, _ in R.PATTERNS)
    assert states > 2 * len(R.PATTERNS)


@pytest.mark.parametrize("V", [300, 1000, 2048])
def test_three_patterns_in_one_automaton(ctx, V):
    dfa = wrk.ByteDfa.from_regex(["(no|y) [0-9]{1,2}!", "(a|ab)(c|bcd)|[^a-c]x|é+", "\\w*\\.\\s"])
    assert dfa.num_patterns == 3
    S, NC = check(ctx, dfa, vocabulary(V), V - 1)
    assert NC > 10


def test_one_state_and_one_byte_class(ctx):
    vocab = vocabulary(321)
    S, NC = check(ctx, wrk.ByteDfa.from_regex("a*"), vocab, 0)
    assert (S, NC) == (2, 3)                                    # a-strings, the end token, everything else
    every = wrk.ByteDfa.from_arrays(np.zeros((1, 256), np.uint16), [1], [0])        # any bytes at all: one byte class
    assert check(ctx, every, vocab, 5) == (2, 3)                # every token that has bytes, the end token, the empty ones


@pytest.mark.parametrize("S,V", [(100, 700), (300, 700), (2000, 300)])
def test_random_tables_with_256_byte_classes(ctx, S, V):
    """a random byte DFA: 256 byte classes; 100 states are 50 KiB (staged in LDS), 300 and 2 000 states go through L2"""
    rng = np.random.default_rng(S)
    nx = rng.integers(0, S, (S, 256)).astype(np.uint16)
    nx[rng.random((S, 256)) < 0.5] = R.REJECT
    acc = (rng.random(S) < 0.2).astype(np.uint8)
    acc[0] = 1
    dfa = wrk.ByteDfa.from_arrays(nx, acc, [0, S // 2, S - 1])
    vocab = R.synthetic_vocab(S + 1, V, lengths=(0, 1, 2, 2, 3, 4, 5, 15, 16, 17, 64))
    check(ctx, dfa, vocab, V - 2, R.dense_table_numpy)


@functools.lru_cache(maxsize=None)
def choices8(n, seed=12):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0, 256, 8).tolist()) for _ in range(n)]


def test_choice_lists_small_and_large(ctx):
    """300 random 8-byte alternatives: about 2 000 states x 256 byte classes, far beyond LDS; 6 of them fit"""
    big = choices8(300)
    seeds = [c[:k] for c in big[:40] for k in (2, 3, 8)] + [c[3:] for c in big[:40]] + [c[2:5] for c in big[40:80]] + \
            [c[:7] + b"\0" for c in big[:20]] + [c[:3] + bytes([c[3] ^ 1]) + c[4:] for c in big[:20]] + [big[0] + big[1], big[2] * 2 + b"\1"]
    vocab = R.synthetic_vocab(9, 777, lengths=(0, 2, 3, 17), seeds=seeds)
    dfa = wrk.ByteDfa.from_regex(wrk.regex_of_choices(big))
    assert dfa.num_states > 1500
    S, NC = check(ctx, dfa, vocab, 256, R.dense_table_numpy)
    assert NC > 100
    small = wrk.ByteDfa.from_regex(wrk.regex_of_choices(big[:6]))
    assert small.num_states < 60
    check(ctx, small, vocab, 256, R.dense_table_numpy)


def test_more_columns_than_classes_is_unsupported(ctx):
    """8 200 distinct 3-byte strings, the vocabulary exactly those strings, the automaton their trie with a leaf per string (arrays of
    the caller's: not minimised): every token leads from the root to a leaf of its own"""
    rng = np.random.default_rng(1)
    codes = rng.choice(64 * 256 * 256, 8200, replace=False)
    vocab = [bytes([c >> 16, (c >> 8) & 255, c & 255]) for c in codes.tolist()]
    nodes = {b"": 0}
    for w in vocab:
        for k in (1, 2, 3):
            nodes.setdefault(w[:k], len(nodes))
    S = len(nodes)
    assert S < 25000
    nx = np.full((S, 256), R.REJECT, np.uint16)
    acc = np.zeros(S, np.uint8)
    for w, s in nodes.items():
        if w:
            nx[nodes[w[:-1]], w[-1]] = s
        acc[s] = len(w) == 3
    dfa = wrk.ByteDfa.from_arrays(nx, acc, [0])
    with pytest.raises(wrk.WrkError) as e:
        wrk.Grammar.compile(ctx, vocab, dfa, 0)
    assert e.value.code == wrk.E_UNSUPPORTED and "8200" in str(e.value)
    still_usable(ctx)
    # 8 191 of them and the end token: 8 192 classes, the limit itself.  No 3-byte token leaves an inner node, so the trim keeps
    # the root, the 8 200 leaves (accepting: the end token leaves them) and FINAL
    g = wrk.Grammar.compile(ctx, vocab[:8192], dfa, 0)
    assert g.num_classes == 8192 and g.num_states == 8202 and g.final_state == 8201
    assert g.walk(0, [5, 0, 0]) == g.final_state
    g.close()


def test_vocabulary_without_single_bytes(ctx):
    """no b, d, e, n or o alone: the token-level trim drops the states that only they would leave"""
    vocab = [b"", b"a", b"bc", b"d", b"f", b"ab", b"e!", b"y", b" ", b"1", b"!", b"c", b"x", "é".encode(), b"#x", b"no ", b"de", b"19!"]
    dfa = wrk.ByteDfa.from_regex(["(no|y) [0-9]{1,2}!", "(a|ab)(c|bcd)|[^a-c]x|é+", "a(bc|de)f"])
    S, NC = check(ctx, dfa, vocab, 0)
    assert S < dfa.num_states + 1


def test_unspellable_pattern(ctx):
    vocab = [b"", b"a", b"b", b"x", b"xyz"]
    with pytest.raises(wrk.WrkError) as e:
        wrk.Grammar.compile(ctx, vocab, ["ab", "xy"], 0)
    assert e.value.code == wrk.E_ARG and "cannot spell pattern 1" in str(e.value)
    with pytest.raises(wrk.WrkError) as e:
        wrk.Grammar.compile(ctx, vocab, ["abc"], 0)
    assert e.value.code == wrk.E_ARG and "cannot spell pattern 0" in str(e.value)
    still_usable(ctx)


def test_argument_errors(ctx):
    dfa = wrk.ByteDfa.from_regex("a")
    data = np.frombuffer(b"ab", np.uint8)
    off = np.array([0, 1, 2], np.uint64)
    starts = np.zeros(1, np.uint32)
    fin = C.c_uint32()
    h = wrk._P()
    u8, u64, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)

    def call(c=ctx.h, d=dfa.h, V=2, b=P_(data, u8), o=P_(off, u64), end=1, out=C.byref(h), st=P_(starts, u32), f=C.byref(fin)):
        return wrk.hip.wrk_grammar_compile(c, d, V, b, o, end, out, st, f)
    assert call() == wrk.OK and h.value
    wrk.hip.wrk_grammar_destroy(h)
    assert call(c=None) == wrk.E_ARG and call(out=None) == wrk.E_ARG
    for kw in (dict(d=None), dict(b=None), dict(o=None), dict(st=None), dict(f=None), dict(V=0), dict(end=2), dict(end=2 ** 32 - 1),
               dict(o=P_(np.array([0, 2, 1], np.uint64), u64)), dict(o=P_(np.array([3, 1, 2], np.uint64), u64))):
        h.value = 1
        assert call(**kw) == wrk.E_ARG, kw
        assert not h.value and wrk.hip.wrk_last_error(ctx.h), kw
    assert call(V=(1 << 20) + 1) == wrk.E_UNSUPPORTED
    assert wrk.hip.wrk_grammar_export(None, None, None, None, None) == wrk.E_ARG
    assert wrk.hip.wrk_grammar_compile_last_ms(None) == wrk.E_ARG
    still_usable(ctx)


# ----------------------------------------------------------------------------- end to end
END = 0
REGEX = r"(yes|no|maybe) [0-9]{2,4}!"


@functools.lru_cache(maxsize=None)
def model_vocab():
    """token 0: empty, the end token; 1 - 255: single bytes; the rest: short ASCII strings"""
    rng = np.random.default_rng(21)
    words = [b"yes", b"no", b"maybe", b"ye", b"may", b"be", b"s ", b"o 1", b" 12", b"123", b"4567", b"12!", b"!", b"9!", b"abc", b"bcx", b"cx",
             b"aab", b"no 77!", b"yes 1", b"x", b"yes!", b"maybe 12345", b"be 0000!"]
    vocab = [b""] + [bytes([b]) for b in range(1, 256)] + words
    alpha = np.frombuffer(b"yesnomayb 0123456789!abcx", np.uint8)
    while len(vocab) < 512:
        vocab.append(bytes(alpha[rng.integers(0, alpha.size, int(rng.integers(2, 5)))].tolist()))
    return vocab


@functools.lru_cache(maxsize=None)
def model(v6):
    return synth.make_v6_gguf(synth.V6_CONFIGS["tiny"], 42) if v6 else synth.make_v7_gguf(synth.CONFIGS["tiny"], 42)


def reply_bytes(vocab, tokens):
    """(the bytes before the first end token, the tokens from it on)"""
    toks = [int(t) for t in tokens]
    cut = toks.index(END) if END in toks else len(toks)
    return b"".join(vocab[t] for t in toks[:cut]), toks[cut:]


@pytest.mark.parametrize("v6", [False, True])
def test_decode_loops_under_a_compiled_regex(ctx, v6):
    vocab = model_vocab()
    g = wrk.Grammar.compile(ctx, vocab, REGEX, END)
    dfa = wrk.ByteDfa.from_regex(REGEX)
    want = R.compile_ref(dfa.next, dfa.accepting, dfa.starts.tolist(), vocab, END, wrk.grammar_from_dense)
    assert np.array_equal(g.token_class, want[0]) and np.array_equal(g.transitions, want[1])
    B, steps = 4, 16
    rt = wrk.Runtime(ctx, wrk.GgufReader(model(v6)), num_batch=B)
    start = int(g.start_states[0])
    first = [7, 100, 300, 411]
    runs = [rt.generate_greedy(first, steps, mode=1, grammar=g, grammar_state=start)[0]]
    states = [rt.last_grammar_state.copy()]
    runs.append(rt.generate_sample(first, steps, temperature=[1.0, 1.3, 0.8, 2.0], top_p=[1.0, 0.95, 0.9, 1.0], seed=[1, 2, 3, 4], mode=1, grammar=g,
                                   grammar_state=start)[0])
    states.append(rt.last_grammar_state.copy())
    texts = set()
    for tok, st in zip(runs, states):
        for b in range(B):
            text, tail = reply_bytes(vocab, tok[:, b])
            assert re.fullmatch(REGEX, text.decode()), text
            assert tail and all(t == END for t in tail), tail           # the language is finite: the end is forced, and only ends follow
            assert g.walk(start, tok[:, b]) == g.final_state
            assert int(st[b]) == g.final_state
            texts.add(text)
    assert len(texts) > 1
    rt.close()
    g.close()


@pytest.mark.parametrize("v6", [False, True])
def test_queue_requests_under_their_own_patterns(ctx, v6):
    vocab = model_vocab()
    pats = [r"(yes|no) [0-9]{2}!", r"[a-c]{3,5}x"]
    g = wrk.Grammar.compile(ctx, vocab, pats, END)
    n = 5
    starts = [int(g.start_states[r % 2]) for r in range(n)]
    prompts = [[(7 + 13 * r + 29 * i) % 512 for i in range(2 + r % 3)] for r in range(n)]
    rt = wrk.Runtime(ctx, wrk.GgufReader(model(v6)), num_batch=2)
    got, _ = rt.generate_queue(prompts, stop=[END], max_new=16, mode=1, grammar=g, grammar_state=starts)
    for r in range(n):
        text, tail = reply_bytes(vocab, got[r][0])
        assert re.fullmatch(pats[r % 2], text.decode()), (r, text)
        assert not re.fullmatch(pats[1 - r % 2], text.decode())
        assert tail == [END] and got[r][1] == 1, r
        assert int(rt.last_grammar_state[r]) == g.final_state == g.walk(starts[r], got[r][0])
    rt.close()
    g.close()
