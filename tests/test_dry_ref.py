"""CPU tests of tests/dry_ref.py, the restatement of DRY and the no-repeat-n-gram ban that the GPU tests hold the kernels to
(DESIGN.md §7n), and of the ABI's new fields and entry points.  No device is touched."""
import os
import re

import numpy as np
import pytest

import dry_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (window, breakers, M) -- the worked cases of the contract, then one case per rule that they leave open
CASES = [
    ([5, 6, 7, 9, 5, 6, 7], (), {9: 3}),
    ([1, 2, 3, 1, 2, 3, 1, 2], (), {3: 5}),
    ([7, 7, 7, 7], (), {7: 3}),
    ([1, 2] * 200, (), {1: 50}),
    ([1, 0, 2, 1, 0, 2], (0,), {1: 1}),
    ([1, 2, 0, 1, 2], (0,), {}),
    ([3, 4, 3, 5, 3], (), {4: 1, 5: 1}),
    ([1, 2, 3, 5, 2, 3, 1, 2], (), {3: 2}),         # the longer match comes first: the max, not the last value
    ([0, 5, 0], (0,), {}),                          # the last token is a breaker
    ([], (), {}),
    ([4], (), {}),
    ([4, 4], (), {4: 1}),
]


def variant(window, breakers=(), cap=True, breaker_in_match=False, last_value=False, skip_follower=True, skip_last=True):
    """match_lengths with one rule switched off at a time: what a wrong implementation would compute."""
    w = [int(x) for x in window]
    n = len(w)
    bk = set(breakers)
    M = {}
    if n < 2 or (skip_last and w[-1] in bk):
        return M
    for i in range(n - 1):
        if w[i] != w[-1] or (skip_follower and w[i + 1] in bk):
            continue
        m = 1
        while (not cap or m < D.MAX_MATCH) and i - m >= 0 and w[i - m] == w[n - 1 - m] and (breaker_in_match or w[n - 1 - m] not in bk):
            m += 1
        M[w[i + 1]] = m if last_value else max(M.get(w[i + 1], 0), m)
    return M


def test_worked_cases():
    for w, bk, want in CASES:
        assert D.match_lengths(w, bk) == want, (w[:12], bk)
        assert D.match_lengths_suffix(w, bk) == want, (w[:12], bk)
        assert variant(w, bk) == want


@pytest.mark.parametrize("mutant", [dict(cap=False), dict(breaker_in_match=True), dict(last_value=True), dict(skip_follower=False),
                                    dict(skip_last=False)])
def test_every_mutant_fails_a_case(mutant):
    assert any(variant(w, bk, **mutant) != want for w, bk, want in CASES), mutant


def test_the_two_statements_agree_on_random_windows():
    rng = np.random.default_rng(7)
    longest = 0
    for k in range(400):
        symbols = int(rng.integers(2, 5))
        n = int(rng.integers(0, 301))
        w = rng.integers(0, symbols, n).tolist()
        bk = () if k % 3 == 0 else tuple(rng.choice(symbols + 1, int(rng.integers(1, 3)), replace=False).tolist())
        a, b = D.match_lengths(w, bk), D.match_lengths_suffix(w, bk)
        assert a == b, (k, w, bk)
        longest = max([longest] + list(a.values()))
    assert longest >= 8
    # a seeded 300-token window over 4 symbols already reaches M = 4
    w = np.random.default_rng(2).integers(0, 4, 300).tolist()
    assert max(D.match_lengths(w).values()) >= 4
    # periodic windows reach the cap from both statements
    for period in (1, 2, 3, 7):
        w = list(range(period)) * (120 // period + 2)
        assert max(D.match_lengths(w).values()) == D.MAX_MATCH == max(D.match_lengths_suffix(w).values())


def test_exact_lengths_around_the_cap():
    for length in (49, 50, 51):
        body = list(range(100, 100 + length))
        w = [1] + body + [9, 2] + body              # the earlier copy is preceded by another token, so the match is exactly `length`
        assert D.match_lengths(w) == {9: min(length, D.MAX_MATCH)} == D.match_lengths_suffix(w)


def test_ring_push():
    w = []
    for t in range(10):
        w = D.push(w, t, 4)
    assert w == [6, 7, 8, 9]
    assert D.push([], 3, 1) == [3] and D.push([3], 4, 1) == [4]


def test_penalty_table():
    pen = D.penalty_table(0.8, 1.75, 2)
    assert pen.dtype == np.float32 and pen.shape == (D.MAX_MATCH + 1,)
    assert pen[0] == pen[1] == 0 and pen[2] == np.float32(0.8)
    p = np.float64(np.float32(0.8))
    for m in range(3, D.MAX_MATCH + 1):
        p = p * np.float64(np.float32(1.75))
        assert pen[m] == np.float32(p)
    # the clamp: a finite table whatever the base
    big = D.penalty_table(3.0, 1e30, 1)
    assert np.isfinite(big).all() and big[1] == 3.0 and big[3] == D.FLT_MAX and big[D.MAX_MATCH] == D.FLT_MAX
    assert (D.penalty_table(0.0, 1e30, 1) == 0).all()
    assert D.penalty_table(2.0, 1.0, D.MAX_MATCH)[D.MAX_MATCH] == 2.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_dry_row():
    x = np.arange(10, dtype=np.float32)
    w = [5, 6, 7, 9, 5, 6, 7]                       # M[9] = 3
    assert np.array_equal(bits(D.dry_row(x, w)), bits(x))                                           # all off
    y = D.dry_row(x, w, multiplier=0.5, base=2.0, allowed_length=2)
    assert y[9] == np.float32(9 - 0.5 * 2.0) and np.array_equal(np.delete(y, 9), np.delete(x, 9))
    assert np.array_equal(bits(D.dry_row(x, w, multiplier=0.5, base=2.0, allowed_length=4)), bits(x))  # M below allowed_length
    for n, banned in ((2, True), (3, True), (4, True), (5, False), (51, False)):
        y = D.dry_row(x, w, no_repeat_ngram=n)
        assert (y[9] == -np.inf) == banned, n       # the ban needs M >= n - 1, not n
    # the ban wins over the penalty; the penalty applies where the ban does not reach
    y = D.dry_row(x, w, multiplier=1.0, base=1.0, allowed_length=1, no_repeat_ngram=5)
    assert y[9] == 8.0
    # NaN payloads, -0 and infinities of untouched tokens keep their bits; +inf meets the clamped penalty as +inf
    s = np.array([0x7FC01234, 0x80000000, 0x7F800000, 0xFF800000, 0x7F800000], np.uint32).view(np.float32)
    w2 = [4, 4]                                     # M[4] = 1
    y = D.dry_row(s, w2, multiplier=1.0, base=1e30, allowed_length=1)
    assert np.array_equal(bits(y), bits(s))
    y = D.dry_row(s, [0, 1, 3, 2, 0, 1, 3, 2, 0, 1, 3], multiplier=3.0, base=1e30, allowed_length=1)   # M[2] >= 3: pen = FLT_MAX
    assert np.array_equal(bits(y), bits(s))         # +inf - FLT_MAX is +inf: the clamp keeps inf - inf away
    f = np.array([1.0, 2.0, -np.inf, np.float32(D.FLT_MAX)], np.float32)
    y = D.dry_row(f, [3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2], multiplier=3.0, base=1e30, allowed_length=1)    # M[3] is long: pen = FLT_MAX
    assert y[3] == 0.0 and np.array_equal(bits(y[:3]), bits(f[:3]))


def test_ban_threshold_mutant_fails():
    x = np.zeros(8, np.float32)
    got = D.dry_row(x, [5, 6, 5], no_repeat_ngram=2)
    assert got[6] == -np.inf                        # a repeated bigram (5, 6) would follow: M = 1 = n - 1
    wrong = x.copy()                                # the mutant: threshold n instead of n - 1
    for t, m in D.match_lengths([5, 6, 5]).items():
        if m >= 2:
            wrong[t] = -np.inf
    assert not np.array_equal(got, wrong)
    # Hugging Face's statement of the same ban: a token is banned iff it would complete an n-gram the window already holds
    rng = np.random.default_rng(3)
    for n in (2, 3, 4):
        for _ in range(50):
            w = rng.integers(0, 3, int(rng.integers(0, 40))).tolist()
            y = D.dry_row(np.zeros(3, np.float32), w, no_repeat_ngram=n)
            for t in range(3):
                assert (y[t] == -np.inf) == _completes(w, t, n), (w, t, n)


def _completes(w, t, n):
    """Whether w + [t] ends in an n-gram that w already holds."""
    if len(w) < n - 1:
        return False
    g = tuple(w[len(w) - (n - 1):] + [t])
    return any(tuple(w[i:i + n]) == g for i in range(len(w) - n + 1))


def test_parameter_ranges():
    assert D.check_params(0.0, 1.0, 1, 0) and D.check_params(5.0, 3.0, 50, 51) and D.check_params(0.8, 1.75, 2, 2)
    for bad in ((-0.1, 1.75, 2, 0), (np.inf, 1.75, 2, 0), (np.nan, 1.75, 2, 0), (1.0, 0.99, 2, 0), (1.0, np.inf, 2, 0), (1.0, 1.75, 0, 0),
                (1.0, 1.75, 51, 0), (1.0, 1.75, 2, 1), (1.0, 1.75, 2, 52)):
        assert not D.check_params(*bad), bad


# ------------------------------------------------------------------------------------------------ the ABI
NEW_FIELDS = ["window", "dry_multiplier", "dry_base", "dry_allowed_length", "no_repeat_ngram", "dry_breakers", "num_dry_breakers"]
NEW_SYMBOLS = {"wrk_token_window_create": 5, "wrk_token_window_destroy": 1, "wrk_token_window_add": 5, "wrk_token_window_back": 5,
               "wrk_token_window_load": 5, "wrk_dry_logits": 13}


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wrk_hip.h")).read(), flags=re.S)


def test_option_fields_match_the_ctypes_mirror():
    import wrk
    for cname, cls in (("wrk_generate_options", wrk.GenerateOptions), ("wrk_queue_options", wrk.QueueOptions)):
        body = re.search(r"typedef\s+struct\s+" + cname + r"\s*\{(.*?)\}", header(), flags=re.S).group(1)
        names = [n for stmt in body.split(";") if stmt.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", stmt.strip())]
        assert names == [n for n, _ in cls._fields_], cname
        at = names.index("grammar")
        assert names[at - len(NEW_FIELDS):at] == NEW_FIELDS, cname                  # directly before grammar ...
        assert names[at - len(NEW_FIELDS) - 1] == "out_top_logprobs", cname         # ... and behind the log-prob fields
    assert wrk.hip.wrk_abi_version() == 1


def test_entry_points_and_constants_are_declared_exported_and_bound():
    import wrk
    text = header()
    declared = set(re.findall(r"\b(wrk_[a-z0-9_]+)\s*\(", text))
    for name, nargs in NEW_SYMBOLS.items():
        assert name in declared and hasattr(wrk.hip, name) and name in wrk.HIP_SYMBOLS, name
        assert len(wrk.HIP_SYMBOLS[name][1]) == nargs, name
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(WRK_\w+)\s+(\d+)\s", text)}
    assert wrk.MAX_TOKEN_WINDOW == defs["WRK_MAX_TOKEN_WINDOW"] == D.MAX_WINDOW == 4096
    assert wrk.MAX_DRY_BREAKERS == defs["WRK_MAX_DRY_BREAKERS"] == D.MAX_BREAKERS == 16
    assert wrk.DRY_MAX_MATCH == defs["WRK_DRY_MAX_MATCH"] == D.MAX_MATCH == 50
    assert callable(wrk.Context.dry_logits) and all(callable(getattr(wrk.TokenWindow, f)) for f in ("add", "back", "load", "close"))
    for fn in ("generate_greedy", "generate_sample", "generate_penalized", "generate_stop", "generate_queue"):
        code = getattr(wrk.Runtime, fn).__code__
        assert {"window", "dry", "no_repeat_ngram", "dry_breakers"} <= set(code.co_varnames[:code.co_argcount]), fn
