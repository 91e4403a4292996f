"""NumPy restatement of classifier-free guidance (web-rwkv-gguf_amd/csrc/wrk_guide.hip): the guided row of a conditional
and an unconditional logits row.

The rows are mixed raw.  Hugging Face and llama.cpp mix log-softmaxed rows, lu + s (lc - lu); with lc = c - LSE(c) and lu = u - LSE(u)
that is u + s (c - u) - (s LSE(c) + (1 - s) LSE(u)): the raw mix minus one constant per row, which no link of the pick chain sees.

For one token, c = row_norm(xc), u = row_norm(xu) (NaN -> -inf, -0 -> +0), s the row's scale; the first case that applies:

    s == 1      the bits of xc, unchanged (NaN payloads and -0 included)
    c == -inf   -inf
    c == +inf   +inf
    u == -inf   c
    s == 0      u
    u == +inf   -inf if s > 1 else +inf
    otherwise   d = c - u, p = s * d, out = p + u: three f32 roundings, no fused multiply-add; an overflow of d or p is the result

Outside s == 1 rows the result is never NaN.  A scale is finite and >= 0.

Not a test module: tests/test_guide_ref.py checks it, tests/test_gpu_guide.py holds the kernel and the decode loops to it.
"""
import numpy as np

MAX_VOCAB = 1 << 20         # the sampler's limit
INF = np.float32(np.inf)


def row_norm(x) -> np.ndarray:
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), -INF, x + np.float32(0.0)).astype(np.float32)


def mix(cond, uncond, s) -> np.ndarray:
    """The guided row of the rows `cond` and `uncond` with the scale s."""
    xc = np.array(cond, np.float32, copy=True)
    s = np.float32(s)
    if s == np.float32(1.0):
        return xc
    c, u = row_norm(xc), row_norm(uncond)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (c - u).astype(np.float32)
        p = (s * d).astype(np.float32)
        out = (p + u).astype(np.float32)
    out = np.where(u == INF, -INF if s > np.float32(1.0) else INF, out)
    out = np.where(s == np.float32(0.0), u, out)
    out = np.where(u == -INF, c, out)
    out = np.where(np.isinf(c), c, out)
    return out.astype(np.float32)


def check_scale(scale) -> str:
    """"ok" or "arg" (WRK_E_ARG): what every call that takes scales answers to them."""
    if scale is None:
        return "arg"
    s = np.asarray(scale, np.float32).reshape(-1)
    return "ok" if bool(np.all(np.isfinite(s) & (s >= 0))) else "arg"


def check_vocab(num_vocab) -> str:
    return "unsupported" if num_vocab > MAX_VOCAB else "ok"


# ----------------------------------------------------------------------------- the rows both test modules use
SCALES = [1.0, 0.0, 0.5, 1.5, 7.5]      # one per row of a row-function call

# the hand-worked table: (conditional bits, unconditional bits, {scale: result bits}); every case of the contract.  At s == 1 the result is
# the conditional bits whatever the rest is
QNAN, QNAN2, NEG0, PINF, NINF = 0x7FC01234, 0xFFC00001, 0x80000000, 0x7F800000, 0xFF800000
ONE, TWO, THREE, HALF = 0x3F800000, 0x40000000, 0x40400000, 0x3F000000
BIG, NBIG = 0x7F61B1E6, 0xFF61B1E6      # +-3e38
HAND = [
    # c == -inf (a NaN is one): -inf, whatever u is
    (NINF, ONE, {0.0: NINF, 0.5: NINF, 1.5: NINF, 7.5: NINF}),
    (QNAN, PINF, {0.0: NINF, 0.5: NINF, 1.5: NINF, 7.5: NINF}),
    (QNAN2, NINF, {0.0: NINF, 0.5: NINF, 1.5: NINF, 7.5: NINF}),
    # c == +inf: +inf, whatever u is
    (PINF, PINF, {0.0: PINF, 0.5: PINF, 1.5: PINF, 7.5: PINF}),
    (PINF, NINF, {0.0: PINF, 0.5: PINF, 1.5: PINF, 7.5: PINF}),
    (PINF, QNAN, {0.0: PINF, 0.5: PINF, 1.5: PINF, 7.5: PINF}),
    # u == -inf (a NaN is one): c, normalised -- before s == 0
    (THREE, NINF, {0.0: THREE, 0.5: THREE, 1.5: THREE, 7.5: THREE}),
    (NEG0, QNAN, {0.0: 0, 0.5: 0, 1.5: 0, 7.5: 0}),
    # s == 0: u, normalised -- before u == +inf
    (ONE, NEG0, {0.0: 0}),
    (ONE, PINF, {0.0: PINF, 0.5: PINF, 1.5: NINF, 7.5: NINF}),
    # both finite: u + s (c - u)
    (THREE, ONE, {0.0: ONE, 0.5: TWO, 1.5: 0x40800000, 7.5: 0x41800000}),           # 1, 2, 4, 16
    (ONE, THREE, {0.0: THREE, 0.5: TWO, 1.5: 0, 7.5: 0xC1400000}),                  # 3, 2, 0, -12
    (NEG0, NEG0, {0.0: 0, 0.5: 0, 1.5: 0, 7.5: 0}),                                  # -0 is +0 once a row is on
    # d overflows: 3e38 - -3e38 = +inf, times s, plus u; at s == 0 the case above has taken it
    (BIG, NBIG, {0.0: NBIG, 0.5: PINF, 1.5: PINF, 7.5: PINF}),
    (NBIG, BIG, {0.0: BIG, 0.5: NINF, 1.5: NINF, 7.5: NINF}),
    # p overflows: d = 3e38 is finite, 7.5 d is not
    (BIG, 0, {0.0: 0, 0.5: 0x7EE1B1E6, 1.5: PINF, 7.5: PINF}),
]

# finite cases where a fused multiply-add rounds differently from the product and the sum, one per scale of SCALES whose product
# rounds (0.5 d is exact): (scale, conditional bits, unconditional bits, result bits, bits of the fused result)
FMA_CASES = [
    (1.5, 0x3F9E10EE, 0x4048299E, 0x3E93BF20, 0x3E93BF1C),
    (7.5, 0xC00EC07A, 0xC030F8A5, 0x3F9F593A, 0x3F9F593B),
]
HAND_LEN = len(HAND) + len(FMA_CASES)


def hand_rows(n: int):
    """The hand-worked table as a pair of rows of n >= HAND_LEN logits (zeros behind it), the FMA cases last."""
    c, u = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i, (cb, ub) in enumerate([x[:2] for x in HAND] + [x[1:3] for x in FMA_CASES]):
        c[i], u[i] = cb, ub
    return c.view(np.float32), u.view(np.float32)


def special_pairs(special_rows, rng, n: int, stride: int, V: int):
    """2n rows of `stride` logits for one row-function call of n guided rows, from `special_rows` (tests/test_gpu_grammar.py): the
    conditional rows first.  Row 3's pair (scale 1.5 in SCALES) is overwritten with +-3e38 rows, whose difference overflows, and wherever
    there is room the leading logits of every pair are the hand-worked table."""
    a = special_rows(rng, 2 * n, stride)
    if n > 3:
        a[3, :V] = np.float32(3e38) * np.where(rng.random(V) < 0.5, 1, -1).astype(np.float32)
        a[n + 3, :V] = -a[3, :V]
    if V >= HAND_LEN:
        hc, hu = hand_rows(HAND_LEN)
        for r in range(n):
            a[r, :HAND_LEN], a[n + r, :HAND_LEN] = hc, hu
    return a
