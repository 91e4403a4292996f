"""NumPy restatement of DRY and the no-repeat-n-gram ban (web-rwkv-gguf_amd/csrc/wrk_dry.hip): the contract the GPU tests
hold the kernels to.

A token window holds the last `capacity` tokens that counted, oldest first.  With the window w[0..n), last = w[n-1], a breaker set Bk
and MAXM = 50:

  * n < 2, or last in Bk: nothing matches;
  * else for every i in [0, n-2] with w[i] == last and t = w[i+1] not in Bk:  m = 1; while m < MAXM and i - m >= 0 and
    w[i-m] == w[n-1-m] and w[n-1-m] not in Bk: m += 1;  M[t] = max(M[t], m).

pen[m] = 0 for m < allowed_length, else multiplier * base ** (m - allowed_length) as repeated f64 products, rounded to f32 and clamped
to FLT_MAX.  A token with M >= no_repeat_ngram - 1 (no_repeat_ngram != 0) becomes -inf; else one with M >= allowed_length (multiplier
!= 0) becomes fl32(x - pen[M]); every other token keeps its bits."""
import numpy as np

MAX_MATCH = 50              # WRK_DRY_MAX_MATCH
MAX_WINDOW = 4096           # WRK_MAX_TOKEN_WINDOW
MAX_BREAKERS = 16           # WRK_MAX_DRY_BREAKERS
FLT_MAX = np.finfo(np.float32).max
DEFAULTS = dict(multiplier=0.0, base=1.75, allowed_length=2, no_repeat_ngram=0)


def push(window, token, capacity):
    """The window after one push: a full window drops its oldest token."""
    w = list(window) + [int(token)]
    return w[-capacity:]


def match_lengths(window, breakers=(), max_match=MAX_MATCH):
    """{token: M} of the tokens some candidate reaches (M >= 1)."""
    w = [int(x) for x in window]
    n = len(w)
    bk = {int(x) for x in breakers}
    M = {}
    if n < 2 or w[n - 1] in bk:
        return M
    last = w[n - 1]
    for i in range(n - 1):
        if w[i] != last:
            continue
        t = w[i + 1]
        if t in bk:
            continue
        m = 1
        while m < max_match and i - m >= 0 and w[i - m] == w[n - 1 - m] and w[n - 1 - m] not in bk:
            m += 1
        M[t] = max(M.get(t, 0), m)
    return M


def penalty_table(multiplier, base, allowed_length):
    """pen f32 [MAX_MATCH + 1]."""
    pen = np.zeros(MAX_MATCH + 1, np.float32)
    p = np.float64(np.float32(multiplier))
    b = np.float64(np.float32(base))
    with np.errstate(over="ignore"):
        for m in range(int(allowed_length), MAX_MATCH + 1):
            pen[m] = FLT_MAX if p >= np.float64(FLT_MAX) else np.float32(p)
            p = p * b
    return pen


def check_params(multiplier, base, allowed_length, no_repeat_ngram):
    """True iff the ABI accepts the row's values."""
    return bool(np.isfinite(multiplier) and multiplier >= 0 and np.isfinite(base) and base >= 1 and 1 <= allowed_length <= MAX_MATCH
                and (no_repeat_ngram == 0 or 2 <= no_repeat_ngram <= MAX_MATCH + 1))


def dry_row(x, window, multiplier=0.0, base=1.75, allowed_length=2, no_repeat_ngram=0, breakers=(), matched=None):
    """The row after DRY and the ban; untouched elements are the input's bits.  matched: match_lengths(window, breakers) when the caller
    has it already."""
    out = np.array(x, np.float32, copy=True)
    if np.float32(multiplier) == 0 and no_repeat_ngram == 0:
        return out
    pen = penalty_table(multiplier, base, allowed_length)
    with np.errstate(over="ignore", invalid="ignore"):
        for t, m in (match_lengths(window, breakers) if matched is None else matched).items():
            if t >= out.size:
                continue
            if no_repeat_ngram != 0 and m >= no_repeat_ngram - 1:
                out[t] = -np.inf
            elif np.float32(multiplier) != 0 and m >= allowed_length:
                out[t] = np.float32(out[t]) - pen[m]
    return out


# ----------------------------------------------------------------------------- a second, independent statement
def match_lengths_suffix(window, breakers=()):
    """The same map from another angle: for every earlier position i the longest common suffix of w[:i+1] and w[:n], found by comparing
    reversed slices; a breaker inside the suffix of w[:n] cuts it, the cap cuts it, and the follower w[i+1] takes the max."""
    w = [int(x) for x in window]
    n = len(w)
    bk = {int(x) for x in breakers}
    if n < 2 or w[-1] in bk:
        return {}
    tail = w[::-1]                                  # tail[k] = w[n-1-k]
    # how far a suffix of the whole window may reach before it meets a breaker (the last token itself is not one)
    clean = next((k for k in range(1, n) if tail[k] in bk), n)
    M = {}
    for i in range(n - 1):
        head = w[i::-1]                             # head[k] = w[i-k]
        lcs = 0
        for a, b in zip(head, tail):
            if a != b:
                break
            lcs += 1
        m = min(lcs, clean, MAX_MATCH)
        if m >= 1 and w[i + 1] not in bk:
            M[w[i + 1]] = max(M.get(w[i + 1], 0), m)
    return M


def has_repeated_ngram(tokens, n):
    """Whether some n-gram occurs twice in `tokens`."""
    seen = set()
    t = [int(x) for x in tokens]
    for i in range(len(t) - n + 1):
        g = tuple(t[i:i + n])
        if g in seen:
            return True
        seen.add(g)
    return False
