"""The regex -> byte DFA compiler and the exact grouping of token columns (web-rwkv-gguf_amd/csrc/wrk_regex.h), on the CPU.

tests/host/regex_main.cpp includes that HIP-free header alone.  It is built with the host compiler under the address and
undefined-behaviour sanitizers, linked into the program: a stand-alone executable; nothing is loaded into Python.

Language: for every pattern of grammar_compile_ref.PATTERNS, every string of at most 5 symbols over up to 9 symbols (the bytes the
pattern mentions, one outsider, é and 中) and 300 seeded random byte strings, most of them not UTF-8.  The verdict of the exported arrays
must be the oracle's: the bytes decode as strict UTF-8 and re.fullmatch(pattern, text, re.ASCII) succeeds.  Python's `re` is the oracle,
not a second compiler.  \\xHH with HH >= 0x80 differs from `re` by design (one raw byte) and is checked by hand.
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import grammar_compile_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_ARG, E_UNSUPPORTED = 0, 1, 4
REJECT = R.REJECT


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host compiler g++ is required"
    exe = str(tmp_path_factory.mktemp("regex") / "regex_main")
    cmd = [cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "web-rwkv-gguf_amd", "csrc"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-g",
           os.path.join(ROOT, "tests", "host", "regex_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(text):
        ran = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-4000:]
        return [json.loads(line) for line in ran.stdout.splitlines()]
    return run


def compile_cmd(patterns, dump=1):
    raw = [p.encode("utf-8") if isinstance(p, str) else p for p in patterns]
    return f"compile {len(raw)} {dump}\n" + "".join((r.hex() or "-") + "\n" for r in raw)


def compile_many(tool, jobs, dump=1):
    """jobs: lists of patterns -> one result per job, arrays as NumPy"""
    out = tool("".join(compile_cmd(j, dump) for j in jobs))
    assert len(out) == len(jobs)
    for o in out:
        o["next"] = np.array(o["next"], np.int64).reshape(-1, 256)
        o["accepting"] = np.array(o["accepting"], np.int64)
    return out


def verdicts(dfa, start, strings):
    """bool per string: the exported arrays walked from `start`, all strings at once"""
    L = max(1, max(len(s) for s in strings))
    data = np.zeros((len(strings), L), np.int64)
    lens = np.array([len(s) for s in strings], np.int64)
    for i, s in enumerate(strings):
        data[i, :len(s)] = np.frombuffer(s, np.uint8)
    cur = np.full(len(strings), int(start), np.int64)
    for i in range(L):
        on = (lens > i) & (cur != REJECT)
        cur = np.where(on, dfa["next"][np.where(on, cur, 0), data[:, i]], cur)
    return (cur != REJECT) & (dfa["accepting"][np.where(cur == REJECT, 0, cur)] != 0)


ALL = [(p, m) for p, m in R.PATTERNS] + [(p, m) for a, b, m in R.PAIRS for p in (a, b)]


@pytest.fixture(scope="module")
def compiled(tool):
    return compile_many(tool, [[p] for p, _ in ALL])


def test_every_construct_of_the_dialect_is_in_the_set():
    text = " ".join(p for p, _ in R.PATTERNS)
    for piece in ("*", "+", "?", "{2}", "{2,}", "{2,3}", "|", "(?:", "(a", "[a-c]", "[^a", ".", "\\d", "\\D", "\\w", "\\W", "\\s", "\\S", "\\n", "\\t",
                  "\\r", "\\f", "\\v", "\\x41", "\\.", "é", "中", "[\\d", "[^\\d", "[\\D", "(|", "b|"):
        assert piece in text, piece
    assert len(R.PATTERNS) >= 30


def test_language_equals_the_oracle(compiled):
    positives = 0
    for k, ((pat, mentioned), dfa) in enumerate(zip(ALL, compiled)):
        assert dfa["rc"] == OK, (pat, dfa["err"])
        syms = R.symbols(mentioned)
        strings = R.enumerate_strings(syms) + R.random_strings(1000 + k, syms)
        got = verdicts(dfa, dfa["starts"][0], strings)
        want = np.array([R.oracle(pat, s) for s in strings])
        wrong = np.nonzero(got != want)[0]
        assert wrong.size == 0, (pat, [(strings[i], bool(got[i]), bool(want[i])) for i in wrong[:5]])
        assert want.any() or pat == "", pat          # every pattern accepts something that is enumerated
        positives += int(want.sum())
    assert positives > 1000


def test_the_oracle_separates_the_confusable_pairs():
    for a, b, mentioned in R.PAIRS:
        strings = R.enumerate_strings(R.symbols(mentioned), 4)
        va = [R.oracle(a, s) for s in strings]
        vb = [R.oracle(b, s) for s in strings]
        assert va != vb, (a, b)


def test_raw_bytes_by_hand(tool):
    """\\xHH is one raw byte: \\xe9 is not the code point é, and a raw byte may make text that is not UTF-8"""
    jobs = [["\\xe9"], ["\\xc3\\xa9"], ["a\\xffb"], ["\\x80*"], ["(\\xe4\\xb8\\xad)+"], ["\\x00\\x7f"]]
    out = compile_many(tool, jobs)
    cases = [
        (0, b"\xe9", True), (0, "é".encode(), False), (0, b"", False),
        (1, "é".encode(), True), (1, b"\xc3", False), (1, b"\xe9", False),
        (2, b"a\xffb", True), (2, b"ab", False), (2, b"a\xfeb", False),
        (3, b"", True), (3, b"\x80\x80\x80", True), (3, b"\x80\x81", False),
        (4, "中中".encode(), True), (4, "中".encode()[:2], False),
        (5, b"\x00\x7f", True), (5, b"\x00", False),
    ]
    for k, s, want in cases:
        assert out[k]["rc"] == OK, out[k]["err"]
        assert bool(verdicts(out[k], 0, [s])[0]) is want, (jobs[k], s)


# ----------------------------------------------------------------------------- canonical form, from the exported arrays
def check_canonical(nx, acc, start, lo, hi):
    """states [lo, hi) of one pattern: closed, reachable, co-reachable, pairwise distinguishable, numbered by BFS in byte order"""
    n = hi - lo
    assert start == lo
    sub = nx[lo:hi]
    assert ((sub == REJECT) | ((sub >= lo) & (sub < hi))).all()
    # BFS in byte order gives 0, 1, 2, ... exactly
    order, seen = [lo], {lo}
    for s in order:
        for b in range(256):
            t = int(nx[s, b])
            if t != REJECT and t not in seen:
                seen.add(t)
                order.append(t)
    assert order == list(range(lo, hi))                 # every state reachable, and numbered as met
    live = acc[lo:hi] != 0
    assert live.any()
    while True:
        more = live | np.where(sub != REJECT, live[np.where(sub == REJECT, lo, sub) - lo], False).any(axis=1)
        if (more == live).all():
            break
        live = more
    assert live.all()                                   # every state reaches an accepting state: no dead state
    # Moore refinement from {accepting, not}: no two states may stay together
    block = (acc[lo:hi] != 0).astype(np.int64)
    while True:
        succ = np.where(sub == REJECT, -1, block[np.where(sub == REJECT, lo, sub) - lo])
        keys = np.concatenate([block[:, None], succ], axis=1)
        _, nb = np.unique(keys, axis=0, return_inverse=True)
        nb = np.asarray(nb).reshape(-1)
        if len(set(nb.tolist())) == len(set(block.tolist())):
            break
        block = nb
    assert len(set(block.tolist())) == n, "two equivalent states"


def test_canonical_form(compiled):
    sizes = {}
    for (pat, _), dfa in zip(ALL, compiled):
        check_canonical(dfa["next"], dfa["accepting"], dfa["starts"][0], 0, dfa["num_states"])
        sizes[pat] = dfa["num_states"]
    # known minimal sizes; (a|ab)(c|bcd) = {ac, abc, abcd, abbcd}: start, a, ab, abc (accepting, d follows), abb, abbc, end
    assert sizes["a*"] == 1 and sizes["a+"] == 2 and sizes["abc"] == 4 and sizes["a{2,3}"] == 4 and sizes["(a|ab)(c|bcd)"] == 7, sizes
    # equal languages written differently give identical arrays
    a, b = [c for (p, _), c in zip(ALL, compiled) if p in ("[^\\d]", "[\\D]")]
    assert np.array_equal(a["next"], b["next"]) and np.array_equal(a["accepting"], b["accepting"])


def test_several_patterns_share_one_automaton(tool, compiled):
    pats = ["(no|y) [0-9]{1,2}!", "a*", "[^a-c]x", "é+"]
    multi = compile_many(tool, [pats])[0]
    assert multi["rc"] == OK
    single = {p: c for (p, _), c in zip(ALL, compiled)}
    base = 0
    for k, p in enumerate(pats):
        one = single[p]
        n = one["num_states"]
        assert multi["starts"][k] == base
        check_canonical(multi["next"], multi["accepting"], multi["starts"][k], base, base + n)
        want = np.where(one["next"] == REJECT, REJECT, one["next"] + base)
        assert np.array_equal(multi["next"][base:base + n], want), p
        assert np.array_equal(multi["accepting"][base:base + n], one["accepting"]), p
        base += n
    assert multi["num_states"] == base


# ----------------------------------------------------------------------------- errors
REFUSED = [     # (pattern, code, offset, a word of the message)
    ("^a", E_UNSUPPORTED, 0, "anchor"), ("a$", E_UNSUPPORTED, 1, "anchor"), ("a\\b", E_UNSUPPORTED, 1, "anchor"), ("\\Ba", E_UNSUPPORTED, 0, "anchor"),
    ("\\Aa", E_UNSUPPORTED, 0, "anchor"), ("a\\Z", E_UNSUPPORTED, 1, "anchor"), ("(a)\\1", E_UNSUPPORTED, 3, "back-reference"),
    ("a(?=b)", E_UNSUPPORTED, 1, "look-around"), ("a(?!b)", E_UNSUPPORTED, 1, "look-around"), ("(?<=a)b", E_UNSUPPORTED, 0, "look-around"),
    ("(?<!a)b", E_UNSUPPORTED, 0, "look-around"), ("ab*?", E_UNSUPPORTED, 3, "lazy"), ("ab+?", E_UNSUPPORTED, 3, "lazy"),
    ("ab??", E_UNSUPPORTED, 3, "lazy"), ("ab{2}?", E_UNSUPPORTED, 5, "lazy"), ("ab*+", E_UNSUPPORTED, 3, "possessive"),
    ("ab++", E_UNSUPPORTED, 3, "possessive"), ("(?P<n>a)", E_UNSUPPORTED, 0, "named group"), ("(?<n>a)", E_UNSUPPORTED, 0, "named group"),
    ("(?i)a", E_UNSUPPORTED, 0, "inline flags"), ("a(?s:.)", E_UNSUPPORTED, 1, "inline flags"), ("\\p{L}", E_UNSUPPORTED, 0, "Unicode"),
    ("a\\P{L}", E_UNSUPPORTED, 1, "Unicode"), ("[aé]", E_UNSUPPORTED, 2, "non-ASCII"), ("[a-é]", E_UNSUPPORTED, 3, "non-ASCII"),
    ("[\\x80]", E_UNSUPPORTED, 1, "non-ASCII"), ("a{1001}", E_UNSUPPORTED, 1, "1000"), ("a{2,1001}", E_UNSUPPORTED, 1, "1000"),
    ("a{1000}", OK, 0, ""), ("a{0,1000}", OK, 0, ""),
    ("(a", E_ARG, 0, "missing )"), ("a)", E_ARG, 1, "unmatched )"), ("a(b(c)", E_ARG, 1, "missing )"), ("[a", E_ARG, 0, "missing ]"),
    ("*a", E_ARG, 0, "nothing to repeat"), ("a|+", E_ARG, 2, "nothing to repeat"), ("a**", E_ARG, 2, "multiple repeat"),
    ("a{2}{3}", E_ARG, 4, "multiple repeat"), ("a{3,2}", E_ARG, 1, "n < m"), ("a{", E_ARG, 1, "malformed"), ("a{,2}", E_ARG, 1, "malformed"),
    ("a{2", E_ARG, 1, "malformed"), ("{2}", E_ARG, 0, "{"), ("a\\", E_ARG, 1, "at the end"), ("\\xg1", E_ARG, 0, "hex"), ("\\x4", E_ARG, 0, "hex"),
    ("a\\q", E_ARG, 1, "unknown escape"), ("a\\0", E_ARG, 1, "unknown escape"), ("[c-a]", E_ARG, 1, "reversed"), ("[a-\\d]", E_ARG, 3, "range end"),
    ("[\\d-z]", E_ARG, 1, "range end"), (b"a\xff", E_ARG, 1, "UTF-8"), (b"\xc3", E_ARG, 0, "UTF-8"), (b"\xed\xa0\x80", E_ARG, 0, "UTF-8"),
]


def test_refused_constructs_and_offsets(tool):
    out = compile_many(tool, [[p] for p, _, _, _ in REFUSED], dump=0)
    for (pat, code, off, word), got in zip(REFUSED, out):
        assert got["rc"] == code, (pat, got["rc"], got["err"])
        if code == OK:
            continue
        assert got["num_states"] == 0
        kind = "unsupported" if code == E_UNSUPPORTED else "syntax"
        assert got["err"].startswith(f"pattern 0: {kind}: "), (pat, got["err"])
        assert got["err"].endswith(f" at offset {off}"), (pat, got["err"])
        assert word in got["err"], (pat, got["err"])


def test_limits(tool):
    big = "(a|b)*a(a|b){12}"    # the 13th letter from the end is an a: 2^13 states, none to spare
    jobs = [[big] * 7, [big] * 8, ["a", "(b"], ["(" * 201 + "a" + ")" * 201], ["(" * 200 + "a" + ")" * 200], ["(a{1000}){1000}"]]
    ok, over, second, deep, deep_ok, nfa = compile_many(tool, jobs, dump=0)
    assert ok["rc"] == OK and ok["num_states"] == 7 * 8192 and ok["starts"] == [8192 * k for k in range(7)]
    assert over["rc"] == E_UNSUPPORTED and "65534" in over["err"] and over["err"].startswith("pattern 7:")
    assert second["rc"] == E_ARG and second["err"].startswith("pattern 1: syntax: missing )")
    assert deep["rc"] == E_UNSUPPORTED and "nested" in deep["err"] and deep["err"].endswith("at offset 200")
    assert deep_ok["rc"] == OK and deep_ok["num_states"] == 2
    assert nfa["rc"] == E_UNSUPPORTED


def test_from_arrays_checks_ranges_only(tool):
    def cmd(S, P, nx, acc, starts):
        return f"arrays {S} {P}\n" + " ".join(map(str, nx)) + "\n" + " ".join(map(str, acc)) + "\n" + " ".join(map(str, starts)) + "\n"
    good = [REJECT] * 512
    good[ord("a")] = 1
    good[256 + ord("b")] = 0
    bad_next = list(good)
    bad_next[5] = 2
    out = tool(cmd(2, 1, good, [0, 1], [0]) + cmd(2, 1, bad_next, [0, 1], [0]) + cmd(2, 2, good, [0, 0], [0, 2]) + cmd(2, 2, good, [0, 0], [1, 1]))
    assert [o["rc"] for o in out] == [OK, E_ARG, E_ARG, OK]
    assert out[0]["byte_classes"] == 3 and out[3]["num_states"] == 2       # a, b, every other byte; no accepting state is not an error here


# ----------------------------------------------------------------------------- the host half of wrk_grammar_compile
def tokens_cmd(dfa, starts, vocab, end, weak):
    S = dfa["num_states"]
    return (f"tokens {S} {len(starts)} {len(vocab)} {end} {weak}\n" + " ".join(map(str, dfa["next"].reshape(-1).tolist())) + "\n" +
            " ".join(map(str, dfa["accepting"].tolist())) + "\n" + " ".join(map(str, starts)) + "\n" + "".join((t.hex() or "-") + "\n" for t in vocab))


@pytest.mark.parametrize("weak", [0, 1])
def test_grouping_and_trim_around_a_plain_walk(tool, weak):
    """byte classes, grouping (weak = 1: the hash is the number of allowed states, so many different columns collide and are split),
    verify and the token-level trim give the reference's tables, whatever the hash"""
    from wrk import grammar_from_dense          # NumPy bookkeeping of the package; the code under test runs in the tool
    pats = ["(no|y) [0-9]{1,2}!", "(a|ab)(c|bcd)|[^a-c]x|é+", "a(bc|de)f"]
    dfa = compile_many(tool, [pats])[0]
    vocabs = [R.synthetic_vocab(4, 400, alphabet=b"abcdxy019 !noef" + "é".encode(), seeds=[b"no 1", b"9!", b"abc", b"bcd", b"de", b"ef", b"y 0"]),
              [b"", b"a", b"bc", b"d", b"f", b"ab", b"e!", b"y", b" ", b"1", b"!", b"c", b"x", "é".encode(), b"#x"],  # the trim drops states
              [b"", b"a", b"f", b"y", b"c", b"1", b"!", b" "]]                                                    # pattern 2 cannot be spelled
    out = tool("".join(tokens_cmd(dfa, dfa["starts"], v, 0 if k else 300, weak) for k, v in enumerate(vocabs)))
    for k, (v, got) in enumerate(zip(vocabs, out)):
        assert got["rc"] == OK
        try:
            cls, trans, starts, fin = R.compile_ref(dfa["next"], dfa["accepting"], dfa["starts"], v, 0 if k else 300, grammar_from_dense)
        except R.Unspellable as e:
            assert k == 2 and got["lost"] == e.pattern == 2
            continue
        assert got["lost"] == -1 and k < 2
        assert got["token_class"] == cls.tolist() and got["starts"] == starts and got["final"] == fin, k
        assert (got["num_states"], got["num_classes"]) == trans.shape
        assert got["transitions"] == trans.reshape(-1).tolist(), k
        assert (got["rounds"] > 0) == bool(weak), (k, got["rounds"])
        if k == 1:
            assert got["num_states"] < dfa["num_states"] + 1            # the vocabulary has no b, d or e alone


# ----------------------------------------------------------------------------- class grouping
def group_cmd(hashes, cols, max_classes=8192):
    return f"group {len(hashes)} {max_classes}\n" + " ".join(map(str, hashes)) + "\n" + " ".join(map(str, cols)) + "\n"


def exact_classes(cols):
    first = {}
    return [first.setdefault(c, len(first)) for c in cols]


def test_grouping_is_exact_under_colliding_hashes(tool):
    rng = np.random.default_rng(7)
    cases = []
    cols = rng.integers(0, 40, 500).tolist()
    cases.append(([1000 + c for c in cols], cols))                              # honest hashes: one round
    cases.append(([1000 + c // 2 for c in cols], cols))                         # every hash shared by two columns
    cases.append(([7] * 500, cols))                                             # one hash for everything
    cases.append(([c % 3 for c in cols], cols))                                 # 3 hashes for 40 columns
    cases.append(([5, 5, 5, 5], [0, 1, 0, 1]))
    cases.append(([5], [0]))
    cases.append(([2 ** 64 - 1, 0, 2 ** 64 - 1], [3, 3, 4]))                    # equal columns under different hashes stay apart: exact
    out = tool("".join(group_cmd(h, c) for h, c in cases))                      # for the walk, merged later by the trim's column merge
    for k, ((h, c), got) in enumerate(zip(cases, out)):
        assert got["rc"] == OK, k
        cls, reps = got["classes"], got["reps"]
        if k < 6:
            assert cls == exact_classes(c), k
            assert reps == [c.index(x) for x in dict.fromkeys(c)], k
        for t, q in enumerate(cls):
            assert c[reps[q]] == c[t] and reps[q] <= t, (k, t)                  # a token's representative has its column and comes first
        assert reps == sorted(reps)
    assert out[0]["rounds"] == 0 and out[0]["verify_calls"] == 1
    assert out[1]["rounds"] >= 1 and out[2]["rounds"] >= 39 and out[2]["verify_calls"] == out[2]["rounds"] + 1
    assert out[6]["classes"] == [0, 1, 2]


def test_grouping_reports_too_many_classes(tool):
    cols = list(range(20))
    out = tool(group_cmd(cols, cols, 19) + group_cmd([1] * 20, cols, 19) + group_cmd(cols, cols, 20))
    assert [o["rc"] for o in out] == [E_UNSUPPORTED, E_UNSUPPORTED, OK]
    assert out[0]["verify_calls"] == 0 and len(out[0]["reps"]) == 20           # refused before anything is walked
