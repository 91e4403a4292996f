"""Plain-Python restatement of wrk_grammar_compile (include/wrk_hip.h): byte-DFA arrays x vocabulary -> the token
automaton.

  * dense [S + 1][V]: from state s token t leads where its bytes lead in next[S][256]; a missing byte transition or an empty token is
    -1; end_token leads from an accepting state to FINAL = S and is -1 elsewhere; FINAL allows only end_token and loops on it;
  * token-level trim: states from which FINAL cannot be reached through tokens go, transitions into them become -1, the kept states
    keep their order (FINAL last); a pattern whose start goes is an error;
  * the package's `grammar_from_dense` then merges equal columns, classes numbered by first token id.

Not a test module: tests/test_grammar_compile_ref.py proves it on hand-built automata, tests/test_gpu_grammar_compile.py holds the device
compiler to it, tools/grammar_compile_bench.py times its NumPy walk.  Also here: the pattern set, the vocabularies and the oracle of the
regex tests.
"""
import re

import numpy as np

REJECT = 0xFFFF


class Unspellable(ValueError):
    """The vocabulary cannot spell a pattern: .pattern is its index."""

    def __init__(self, pattern):
        super().__init__(f"the vocabulary cannot spell pattern {pattern}")
        self.pattern = pattern


def dense_table(next_, accepting, vocab, end_token):
    """[S + 1][V] int64 of next states, -1 where the token is not allowed: one byte at a time, in plain Python."""
    nx = np.asarray(next_, np.int64)
    S, V = nx.shape[0], len(vocab)
    table = np.full((S + 1, V), -1, np.int64)
    rows = nx.tolist()
    for t, tok in enumerate(vocab):
        if t == end_token or len(tok) == 0:
            continue
        for s in range(S):
            cur = s
            for b in tok:
                cur = rows[cur][b]
                if cur == REJECT:
                    cur = -1
                    break
            table[s, t] = cur
    for s in range(S):
        table[s, end_token] = S if accepting[s] else -1
    table[S, end_token] = S
    return table


def dense_table_numpy(next_, accepting, vocab, end_token):
    """The same table with the byte steps vectorised over (state, token): the yardstick of tools/grammar_compile_bench.py."""
    S, V = np.asarray(next_).shape[0], len(vocab)
    table = np.empty((S + 1, V), np.int64)
    table[:S] = walk_rows_numpy(next_, vocab, 0, S)
    table[:S, end_token] = np.where(np.asarray(accepting) != 0, S, -1)
    table[S] = -1
    table[S, end_token] = S
    return table


def walk_rows_numpy(next_, vocab, s0, s1):
    """rows [s0, s1) of the walk, [s1 - s0][V]: where every token's bytes lead from each of these states (-1: nowhere; an empty token:
    -1), the end token not yet treated"""
    nx = np.asarray(next_, np.int64)
    nx = np.where(nx == REJECT, -1, nx)
    V = len(vocab)
    lens = np.array([len(t) for t in vocab], np.int64)
    L = int(lens.max(initial=0))
    padded = np.zeros((V, max(L, 1)), np.int64)
    for t, tok in enumerate(vocab):
        padded[t, :len(tok)] = np.frombuffer(tok, np.uint8)
    cur = np.repeat(np.arange(s0, s1, dtype=np.int64)[:, None], V, 1)
    for i in range(L):
        step = nx[np.maximum(cur, 0), padded[None, :, i]]
        cur = np.where((lens[None, :] > i) & (cur >= 0), step, cur)
    cur[:, lens == 0] = -1
    return cur


def token_trim(table, starts):
    """(trimmed table, new start states, new final state); Unspellable when a start state goes."""
    t = np.asarray(table, np.int64)
    N = t.shape[0]
    live = np.zeros(N, bool)
    live[N - 1] = True
    while True:
        reach = np.where(t >= 0, live[np.maximum(t, 0)], False).any(axis=1) | live
        if (reach == live).all():
            break
        live = reach
    for p, s in enumerate(starts):
        if not live[s]:
            raise Unspellable(p)
    new = np.cumsum(live) - 1
    out = t[live]
    out = np.where((out >= 0) & live[np.maximum(out, 0)], new[np.maximum(out, 0)], -1)
    return out, [int(new[s]) for s in starts], int(new[N - 1])


def compile_ref(next_, accepting, starts, vocab, end_token, from_dense, table_fn=dense_table):
    """(token_class, transitions, start_states, final_state) as wrk_grammar_compile returns them; from_dense: wrk.grammar_from_dense."""
    table, st, fin = token_trim(table_fn(next_, accepting, vocab, end_token), starts)
    cls, trans = from_dense(table)
    return cls, trans, st, fin


# ----------------------------------------------------------------------------- the regex tests' patterns, strings and oracle
# every construct of the dialect; each entry: (pattern, the bytes it mentions that the enumeration uses)
PATTERNS = [
    ("abc", "abc"), ("a*", "a"), ("a+", "a"), ("a?b", "ab"), ("a{2}", "a"), ("a{2,}", "a"), ("a{2,3}", "a"), ("a{2,4}", "a"), ("a{0,2}b", "ab"),
    ("a|b|", "ab"), ("(a|b)*c", "abc"), ("(?:ab)+", "ab"), ("(a(b|c))?d", "abcd"), ("[a-c]", "abc"), ("[a-b]", "abc"), ("[^a]", "a\n"),
    ("[^a-c]x", "acx"), (".", "a\n"), (".*a", "a\n"), ("a.c", "ac\n"), ("\\d+", "09a"), ("\\D", "0a"), ("\\w*", "a_0-"), ("\\W", "a_-"),
    ("\\s", " \ta"), ("\\S\\s", " a\n"), ("[\\d_]+", "0_a"), ("[^\\d]", "0a"), ("[\\D]", "0a"), ("[\\Sa ]", " a"), ("\\.\\*\\\\", ".*\\"),
    ("\\n|\\t|\\r|\\f|\\v", "\n\t\r\f\v"), ("\\x41\\x0a", "A\n"), ("é+", "a"), ("中|é", "a"), ("a(é|中)*", "a"), ("[]a]", "]a"),
    ("[a-]", "a-"), ("[-a]", "a-"), ("(a|ab)(c|bcd)", "abcd"), ("x{0}y", "xy"), ("(|a)b", "ab"), ("[\\]\\^\\-]", "]^-"), ("a}", "a}"),
    ("(no|y) [0-9]{1,2}!", "noy 1!"),
]
# pairs a plausible bug would confuse (a negated class without the multi-byte sequences, a "." that takes \n): the oracle must
# separate them on the enumerated strings
PAIRS = [("a+", "a*", "a"), ("a{2,3}", "a{2,4}", "a"), ("[a-c]", "[a-b]", "abc"), ("[^a]", "[\\x00-\\x60b-\\x7f]", "a\n"),
         (".", "(?:.|\\n)", "a\n")]
OUTSIDER = "#"


def symbols(mentioned):
    """Up to 9 symbols as byte strings: the bytes the pattern mentions, one outsider, é and 中."""
    syms = []
    for ch in mentioned:
        if ch.encode() not in syms:
            syms.append(ch.encode())
    syms = syms[:6] + [OUTSIDER.encode(), "é".encode(), "中".encode()]
    assert len(syms) <= 9
    return syms


def enumerate_strings(syms, max_len=5):
    out = [b""]
    layer = [b""]
    for _ in range(max_len):
        layer = [s + y for s in layer for y in syms]
        out += layer
    return out


def random_strings(seed, syms, count=300):
    """Seeded random byte strings: symbols mixed with arbitrary bytes, so most are not UTF-8."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(0, 7))
        parts = []
        for _ in range(n):
            parts.append(syms[int(rng.integers(0, len(syms)))] if rng.random() < 0.6 else bytes([int(rng.integers(0, 256))]))
        out.append(b"".join(parts))
    return out


def oracle(pattern: str, b: bytes) -> bool:
    """b decodes as strict UTF-8 and the pattern full-matches the text under re.ASCII."""
    try:
        text = b.decode("utf-8")
    except UnicodeDecodeError:
        return False
    return re.fullmatch(pattern, text, re.ASCII) is not None


def dfa_accepts(next_, accepting, start, b: bytes) -> bool:
    s = int(start)
    for x in b:
        s = int(next_[s][x])
        if s == REJECT:
            return False
    return bool(accepting[s])


# ----------------------------------------------------------------------------- vocabularies
def synthetic_vocab(seed, V, lengths=(0, 1, 3, 4, 5, 15, 16, 17, 64), alphabet=None, seeds=()):
    """All 256 single bytes first, then seeded strings: `seeds` (given strings), then random ones over `alphabet` (bytes; None: all)
    with the lengths cycled.  V >= 256 + len(seeds)."""
    rng = np.random.default_rng(seed)
    vocab = [bytes([b]) for b in range(256)] + [bytes(s) for s in seeds]
    alpha = np.frombuffer(bytes(range(256)) if alphabet is None else alphabet, np.uint8)
    i = 0
    while len(vocab) < V:
        n = lengths[i % len(lengths)]
        i += 1
        vocab.append(bytes(alpha[rng.integers(0, alpha.size, n)].tolist()))
    return vocab[:V]
