"""float64 references, error bounds and input profiles for the non-matmul kernels (norms, activations, element-wise ops, WKV), for NumPy.

Every reference restates the MATHEMATICS of a reference shader in float64 (the shader is cited by file and line, as oracle/rwkv7.py
does; nothing is imported from the product or from the oracle) and returns the value together with the quantity its error is measured
against.  There is no additive floor anywhere: `ulp16` is the true spacing of f16 at |want| (2^-24 in the subnormal range).

  element-wise (f16 out) ... |got - want| <= ulp16(want)/2 + n * 2^-24 * terms + ulp16(want) * 2^-11          (`bound16`)
       terms = sum of |addends| of the expression, n = number of f32 roundings of the kernel's expression (next to each op below),
       the last term is the double-rounding allowance (f32 result rounded again to f16).
  reductions ............... C_RED * sum|terms| per reduction (C_RED = 4e-6, the constant of the matmul edge tests, tied to f32
       accumulation in tests/test_blocks_ref.py), carried to the output by first-order propagation written out in each helper;
       an f16 store adds ulp16(want)/2, an f32 output (state) takes the propagated bound alone.
  activations .............. the shader's expression stage by stage, every stage in f64 and rounded to f32 (what the reference
       computes when its functions are exact), then rounded to the tensor's type (`act_expected`).  This defines the overflow zones
       of the reference's own formula: softplus = log(1 + exp(x)) is +inf from x = 88.73 on, opposite_exp = -exp(x) is -inf there
       (and -inf in an f16 tensor from x = 11.09 on), silu's x / (1 + exp(-x)) is -0 below x = -88.73.

A `want` that rounds beyond 65504 expects +-inf; within one bound of the overflow threshold (65520) either result is accepted
(`check16` counts those elements; tests cap their share).
"""
import numpy as np

F16_MAX = 65504.0
F16_OVER = 65520.0          # round-to-nearest-even threshold: |v| >= 65520 becomes inf
F16_TINY = 2.0 ** -24
U32 = 2.0 ** -24            # unit roundoff of f32
C_RED = 4e-6                # per-reduction constant (tests/test_gpu_matmul_edges.py: C)

NORMAL, TINY, LARGE, OFFSET, CONSTANT, ZERO_ROW, ONE_HOT, CANCELLING, MIXED_SCALE = (
    "normal", "tiny", "large", "offset", "constant", "zero_row", "one_hot", "cancelling", "mixed_scale")
PROFILES = (NORMAL, TINY, LARGE, OFFSET, CONSTANT, ZERO_ROW, ONE_HOT, CANCELLING, MIXED_SCALE)
ACTS = ("squared_relu", "tanh", "stable_exp", "opposite_exp", "softplus", "sigmoid", "silu")


def _rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ----------------------------------------------------------------------------- formats
def ulp16(x):
    """True spacing of f16 at |x|: 2^(floor(log2|x|) - 10), 2^-24 below 2^-14, 32 from 2^15 on (no floor, no constant)."""
    a = np.abs(np.asarray(x, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.clip(np.where(a > 0, e, -14), -14, 15)
    return 2.0 ** (e - 10)


def ulp32(x):
    a = np.abs(np.asarray(x, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.clip(np.where(a > 0, e, -126), -126, 127)
    return 2.0 ** (e - 23)


def r32(x):
    """f64 -> nearest f32 -> f64 (overflow gives inf, as the hardware's rounding does)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def r16(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float16)


def ordered16(h):
    """f16 bit patterns -> integers that are monotone in the value, -0 and +0 both 0, +inf = the successor of 65504: the distance of two
    such integers is the distance in f16 steps with the true spacing."""
    b = np.asarray(h, np.float16).view(np.uint16).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def finite_f16_patterns():
    """All 63 488 finite f16 values (both zeros, all subnormals, up to +-65504), as f16."""
    b = np.arange(1 << 16, dtype=np.uint32)
    b = b[(b & 0x7C00) != 0x7C00].astype(np.uint16)
    assert b.size == 63488
    return b.view(np.float16)


# ----------------------------------------------------------------------------- bounds and checks
def rnd32(terms, n=1):
    """n f32 roundings of values of size `terms`: 2^-24 relative each, and never less than half the subnormal spacing 2^-149"""
    return n * np.maximum(U32 * np.asarray(terms, np.float64), 2.0 ** -150)


def bound16(want, terms, n):
    u = ulp16(want)
    return u / 2 + n * U32 * np.asarray(terms, np.float64) + u * 2.0 ** -11


def check16(got, want, bound):
    """-> (ratio = |got - want| / bound per element, with inf where the element is wrong outright; number of elements near the overflow
    threshold where either result was accepted).  `want` f64, `got` f16."""
    got = np.asarray(got).astype(np.float64).reshape(np.shape(want))
    want, bound = np.asarray(want, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(want))
    a = np.abs(want)
    over = a - bound >= F16_OVER                      # must be +-inf
    near = ~over & (a + bound >= F16_OVER)            # either
    sign_ok = np.sign(got) == np.sign(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - want)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isnan(got), np.inf, ratio)
    ratio = np.where(over, np.where(np.isinf(got) & sign_ok, 0.0, np.inf), ratio)
    ratio = np.where(near & np.isinf(got), np.where(sign_ok, 0.0, np.inf), ratio)
    ratio = np.where(~over & ~near & np.isinf(got), np.inf, ratio)
    return ratio, int(near.sum())


def check32(got, want, bound):
    got = np.asarray(got, np.float64).reshape(np.shape(want))
    want, bound = np.asarray(want, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(want))
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - want)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(got), ratio, np.inf)


# ----------------------------------------------------------------------------- input profiles (f16 arrays; rows = last axis)
def make(profile, shape, *seed):
    r = _rng(profile, shape, seed)
    shape = tuple(shape)
    n = shape[-1]
    if profile == NORMAL:
        x = r.standard_normal(shape)
    elif profile == TINY:           # f16 subnormals of either sign mixed with +-0
        bits = r.integers(1, 1024, shape).astype(np.uint16)
        bits = np.where(r.random(shape) < 0.25, 0, bits).astype(np.uint16) | (r.integers(0, 2, shape).astype(np.uint16) << 15)
        return bits.view(np.float16).reshape(shape)
    elif profile == LARGE:          # up to 65504, some exactly there
        x = r.choice([-1.0, 1.0], shape) * F16_MAX * r.uniform(0.25, 1.0, shape)
        x = np.where(r.random(shape) < 0.005, np.sign(x) * F16_MAX, x)
    elif profile == OFFSET:         # mean 2^10, spread of one or two f16 ulps (1.0 at 1024): kills a one-pass variance
        x = 1024.0 + r.integers(-1, 2, shape) * np.where(r.integers(0, 2, shape) == 1, 1.0, 0.5)
    elif profile == CONSTANT:
        x = np.broadcast_to(np.asarray(3.0 * r.standard_normal(shape[:-1] + (1,)), np.float16), shape).astype(np.float64)
    elif profile == ZERO_ROW:
        x = np.where(r.integers(0, 2, shape) == 1, -0.0, 0.0)
    elif profile == ONE_HOT:
        x = np.zeros(shape)
        idx = r.integers(0, n, shape[:-1])
        np.put_along_axis(x, idx[..., None], 3.0 * r.choice([-1.0, 1.0], shape[:-1] + (1,)) * (1 + r.random(shape[:-1] + (1,))), -1)
    elif profile == CANCELLING:     # alternating signs: pairs cancel to ~2^-10 of their size, the sum is orders below sum|x|
        a = np.asarray(100.0 * (1.0 + r.random(shape)), np.float16).astype(np.float64)
        a[..., 1::2] = a[..., 0:n - (n % 2):2] * (1.0 + 2.0 ** -10 * r.integers(-1, 2, a[..., 1::2].shape))
        x = a * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    elif profile == MIXED_SCALE:    # one element 2^15 among 2^-14
        x = np.full(shape, 2.0 ** -14) * r.choice([-1.0, 1.0], shape)
        np.put_along_axis(x, r.integers(0, n, shape[:-1])[..., None], 2.0 ** 15, -1)
    else:
        raise KeyError(profile)
    return np.asarray(x, np.float64).astype(np.float16)


def factors(shape, *seed):
    """lerp / token-shift factors: f16 in [0, 1] with both ends present."""
    r = _rng("factors", shape, seed)
    f = r.random(shape)
    f = np.where(r.random(shape) < 0.1, np.round(f), f)
    return f.astype(np.float16)


# ----------------------------------------------------------------------------- element-wise references: (want, terms, n)
def _f(x):
    return np.asarray(x, np.float64)


def add(x, y):              # binary.wgsl:38-57  x + y: 1 rounding
    x, y = _f(x), _f(y)
    return x + y, np.abs(x) + np.abs(y), 1


def mul(x, y):              # binary.wgsl:60-78  x * y: 1 rounding
    x, y = _f(x), _f(y)
    return x * y, np.abs(x * y), 1


def affine(x, scale, bias):     # the reference's affine op: scale * x + bias, one fma: 1 rounding
    x, scale, bias = _f(x), float(np.float32(scale)), float(np.float32(bias))
    return scale * x + bias, np.abs(scale * x) + abs(bias), 1


def mix(x, y, a):           # WGSL mix(x, y, a) = x (1 - a) + y a (lerp.wgsl:74-92, token_shift.wgsl:85-117): (1 - a), two products, the sum: 4
    x, y, a = _f(x), _f(y), _f(a)
    return x * (1 - a) + y * a, np.abs(x * (1 - a)) + np.abs(y * a), 4


def control_k(k, a, p):     # control_k_v7.wgsl:60-75  k (1 + (a - 1) p) = k + k a p - k p: (a - 1), * p, 1 +, * k: 4
    k, a, p = _f(k), _f(a), _f(p)
    return k * (1 + (a - 1) * p), np.abs(k) + np.abs(k * a * p) + np.abs(k * p), 4


# exp(x) in the kernels is exp2(x log2 e): the product's rounding moves the exponent by |x| log2(e) 2^-24, i.e. |x| 2^-24 relative on
# the result.  sigma(r) differs from 0 or 1 by less than 2^-25 beyond |r| = 17.4, so 18 units cover the argument and 2 the instruction.
EXP_UNITS = 20


def channel_mix_v6(r, v):   # channel_mix.wgsl:83-107  sigmoid(r) v: exp, 1 +, 1 /, * v = 4 roundings + EXP_UNITS for the exponential
    r, v = _f(r), _f(v)
    with np.errstate(over="ignore"):
        want = v / (1 + np.exp(-r))
    return want, np.abs(want), 4 + EXP_UNITS


# ----------------------------------------------------------------------------- activations, stage by stage (ops.rs:206-234)
def act_expected(name, x):
    """x: f16 or f32 array -> f64 array holding the f32 the reference computes when exp / log / tanh / the division are exact."""
    x = _f(x)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore", under="ignore"):
        if name == "none":
            return x
        if name == "squared_relu":
            p = np.maximum(x, 0.0)
            return r32(p * p)
        if name == "tanh":
            return np.where(x > 42.0, 1.0, r32(np.tanh(x)))
        if name == "stable_exp":
            return r32(np.exp(-r32(np.exp(x))))
        if name == "opposite_exp":
            return -r32(np.exp(x))
        if name == "softplus":
            return r32(np.log(r32(1.0 + r32(np.exp(x)))))
        if name == "sigmoid":
            return r32(1.0 / r32(1.0 + r32(np.exp(-x))))
        if name == "silu":
            return r32(x / r32(1.0 + r32(np.exp(-x))))
    raise KeyError(name)


# ----------------------------------------------------------------------------- reductions: (want, bound before the store)
def layer_norm(x, w, b, eps):
    """layer_norm.wgsl:63-121 (group_norm: the same per head).  x [..., C]; w, b broadcastable to x.  First-order propagation:
         mean   m = sum x / C                      e_m   = C_RED sum|x| / C
         d = x - m                                 e_d   = e_m + 2^-24 |d|
         var = sum d^2 / C                         e_var = sum (2 |d| e_d + e_d^2) / C + C_RED var
         dev = (var + eps)^-1/2                    e_dev = dev e_var / (2 (var + eps)) + 2 * 2^-24 dev      (sqrt, division)
         out = d dev w + b                         e_out = (e_d dev + |d| e_dev) |w| + 2 * 2^-24 (|d dev w| + |b|)
    """
    x, w, b, eps = _f(x), _f(w), _f(b), float(np.float32(eps))
    C = x.shape[-1]
    m = x.sum(-1, keepdims=True) / C
    e_m = C_RED * np.abs(x).sum(-1, keepdims=True) / C
    d = x - m
    e_d = e_m + U32 * np.abs(d)
    var = (d * d).sum(-1, keepdims=True) / C
    e_var = (2 * np.abs(d) * e_d + e_d * e_d).sum(-1, keepdims=True) / C + C_RED * var
    dev = 1.0 / np.sqrt(var + eps)
    e_dev = dev * e_var / (2 * (var + eps)) + 2 * U32 * dev
    want = d * dev * w + b
    e_out = (e_d * dev + np.abs(d) * e_dev) * np.abs(w) + 2 * U32 * (np.abs(d * dev * w) + np.abs(b))
    return want, e_out, np.abs(d * dev * w) + np.abs(b)


def l2_norm(x, eps):
    """normalize.wgsl:117-152  x / sqrt(sum x^2 + eps):  e_s = C_RED s;  e_n = n e_s / (2 (s + eps)) + 2 * 2^-24 n;  e_out = |x| e_n + 2^-24 |x n|"""
    x, eps = _f(x), float(np.float32(eps))
    s = (x * x).sum(-1, keepdims=True)
    n = 1.0 / np.sqrt(s + eps)
    e_n = n * (C_RED * s) / (2 * (s + eps)) + 2 * U32 * n
    want = x * n
    return want, np.abs(x) * e_n + U32 * np.abs(want), np.abs(want)


def softmax(x):
    """softmax.wgsl: exp(x - max) / sum.  exp carries (|x - max| + 3) 2^-24 relative (EXP_UNITS' argument applied to the actual argument);
    e_s = C_RED s + sum e_exp;  out relative = e_exp / exp + e_s / s + 2^-24, plus one f32 spacing of the result (true spacing: the
    quotient of a subnormal numerator has no relative accuracy).  A result below 2^-126 may also be 0: WGSL lets an implementation
    flush subnormal f32 results, and the exponential instruction of the GPU has none.  -inf entries give exactly 0."""
    x = _f(x)
    m = x.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        d = np.where(np.isneginf(x), -np.inf, x - m)
    e = np.exp(d)
    rel = np.where(np.isfinite(d), (np.abs(d) + 3) * U32, 0.0)
    s = e.sum(-1, keepdims=True)
    e_s = C_RED * s + (e * rel).sum(-1, keepdims=True)
    want = e / s
    return want, np.where(want < 2.0 ** -126, want, 0.0) + want * (rel + e_s / s + U32) + np.where(want > 0, ulp32(want), 0.0)


def time_first(u, k, r, v, x):
    """time_mix_v7.wgsl:223-262  x_i + (sum_j u_j k_j r_j) v_i per head ([..., H, S]):  e_xx = (C_RED + 2 * 2^-24) sum|u k r|;
    e_out = |v| e_xx + 2 * 2^-24 (|x| + |xx v|)"""
    u, k, r, v, x = _f(u), _f(k), _f(r), _f(v), _f(x)
    xx = (u * k * r).sum(-1, keepdims=True)
    e_xx = (C_RED + 2 * U32) * np.abs(u * k * r).sum(-1, keepdims=True)
    want = x + xx * v
    terms = np.abs(x) + np.abs(xx * v)
    return want, np.abs(v) * e_xx + 2 * U32 * terms, terms


W_SCALE = -0.606531         # time_mix_v7.wgsl:69
DECAY_UNITS = 8             # w~ = exp(W_SCALE sigma(w)): sigma(1 - sigma)|w| <= 0.23, so the exponential inside sigma moves sigma by < 2^-24;
#                             with its three roundings, the product, and the outer exponential (argument <= 0.61) below 8 * 2^-24 relative


def cursors_of(lens):
    """packed cursors of stacked tokens (tensor/mod.rs:53-60): batch | token << 8 | len << 24; -> [(batch, start, len)] per sequence"""
    out, t = [], 0
    for b, n in enumerate(lens):
        if n:
            out.append((b, t, n))
        t += n
    return out


def stack_cursors(lens):
    cur = []
    for b, start, n in cursors_of(lens):
        cur += [b | (start << 8) | (n << 24)] * n
    return np.array(cur, np.uint32)


def wkv7(state, r, w, k, v, a, kk, lens, H):
    """time_mix_v7.wgsl:143-221 on stacked tokens.  state [B, S+1, D] (row 0: token-shift carry, rows 1..S: S[j, :]); r .. kk [T, D].
         w~ = exp(W_SCALE sigma(w)), a~ = -kk, b~ = kk a
         sa_i = sum_j S_ji a~_j ;  S_ji <- S_ji w~_j + k_j v_i + sa_i b~_j ;  y_i = sum_j r_j S_ji
    An absolute error bound E travels with the f64 state through the same recurrence on absolute values:
         e_sa = sum_j |a~_j| E_ji + C_RED sum_j |S_ji a~_j|
         E'   = E w~ + |S| w~ DECAY_UNITS 2^-24 + |b~| e_sa + rnd32(|S w~| + |k v| + |sa b~|, 4)          (b~, k v, two sums: 4 roundings)
         e_y  = sum_j |r_j| E'_ji + C_RED sum_j |r_j S'_ji|
    -> (y [T, D], e_y [T, D], sum_j|r_j S'_ji| [T, D], state' [B, S+1, D], E [B, S+1, D]); the carry row is the caller's."""
    S = 64
    st = _f(state).copy()
    E = np.zeros_like(st)
    r, w, k, v, a, kk = (_f(z).reshape(-1, H, S) for z in (r, w, k, v, a, kk))
    T = r.shape[0]
    with np.errstate(over="ignore"):
        wt = np.exp(W_SCALE / (1 + np.exp(-w)))
    y, ey, ty = (np.zeros((T, H, S)) for _ in range(3))
    for b, start, n in cursors_of(lens):
        Sm = st[b, 1:].reshape(S, H, S).transpose(1, 0, 2).copy()        # [H, j, i]
        Em = E[b, 1:].reshape(S, H, S).transpose(1, 0, 2).copy()
        for t in range(start, start + n):
            at, bt = -kk[t][:, :, None], (kk[t] * a[t])[:, :, None]
            sa = (Sm * at).sum(1, keepdims=True)
            e_sa = (np.abs(at) * Em).sum(1, keepdims=True) + C_RED * np.abs(Sm * at).sum(1, keepdims=True)
            wj, kv = wt[t][:, :, None], k[t][:, :, None] * v[t][:, None, :]
            Em = Em * wj + np.abs(Sm) * wj * DECAY_UNITS * U32 + np.abs(bt) * e_sa + rnd32(np.abs(Sm * wj) + np.abs(kv) + np.abs(sa * bt), 4)
            Sm = Sm * wj + kv + sa * bt
            rj = r[t][:, :, None]
            y[t] = (rj * Sm).sum(1)
            ty[t] = np.abs(rj * Sm).sum(1)
            ey[t] = (np.abs(rj) * Em).sum(1) + C_RED * ty[t]
        st[b, 1:] = Sm.transpose(1, 0, 2).reshape(S, H * S)
        E[b, 1:] = Em.transpose(1, 0, 2).reshape(S, H * S)
    D = H * S
    return y.reshape(T, D), ey.reshape(T, D), ty.reshape(T, D), st, E


def wkv6(state, decay, u, k, v, r, lens, H):
    """time_mix_v6.wgsl:83-155:  y_i = sum_j r_j (u_j k_j v_i + S_ji);  S_ji <- w_j S_ji + k_j v_i   (all operands f32)
         e_y = sum_j |r_j| (E_ji + 2 * 2^-24 (|u k v| + |S|)) + C_RED sum_j |r_j (u k v + S)|;   E' = w E + rnd32(|w S| + |k v|, 2)"""
    S = 64
    st = _f(state).copy()
    E = np.zeros_like(st)
    decay, k, v, r = (_f(z).reshape(-1, H, S) for z in (decay, k, v, r))
    u = _f(u).reshape(H, S)[:, :, None]
    T = r.shape[0]
    y, ey, ty = (np.zeros((T, H, S)) for _ in range(3))
    for b, start, n in cursors_of(lens):
        Sm = st[b, 1:].reshape(S, H, S).transpose(1, 0, 2).copy()
        Em = E[b, 1:].reshape(S, H, S).transpose(1, 0, 2).copy()
        for t in range(start, start + n):
            kv, rj, wj = k[t][:, :, None] * v[t][:, None, :], r[t][:, :, None], decay[t][:, :, None]
            y[t] = (rj * (u * kv + Sm)).sum(1)
            ty[t] = np.abs(rj * (u * kv + Sm)).sum(1)
            ey[t] = (np.abs(rj) * (Em + 2 * U32 * (np.abs(u * kv) + np.abs(Sm)))).sum(1) + C_RED * ty[t]
            Em = wj * Em + rnd32(np.abs(wj * Sm) + np.abs(kv), 2)
            Sm = wj * Sm + kv
        st[b, 1:] = Sm.transpose(1, 0, 2).reshape(S, H * S)
        E[b, 1:] = Em.transpose(1, 0, 2).reshape(S, H * S)
    D = H * S
    return y.reshape(T, D), ey.reshape(T, D), ty.reshape(T, D), st, E


# ----------------------------------------------------------------------------- WKV input profiles
WKV_PROFILES = (NORMAL, TINY, "decay_limits", LARGE, CANCELLING, "zero_r")
WKV_OPERANDS = ("r", "k", "v", "a", "kk", "state")


def _unit_heads(z, H):
    z = z.reshape(z.shape[0], H, 64)
    return (z / np.sqrt((z * z).sum(-1, keepdims=True) + 1e-12)).reshape(z.shape[0], -1)


def wkv7_inputs(profile, operand, lens, H, seed=0):
    """-> dict of f16 [T, D] r, w, k, v, a, kk, x (the carry source) and the f32 state [B, S+2, D].  `normal` is the layer's own range
    (kk unit per head, a in [0, 1]); the other profiles change `operand` alone (`tiny`) or the operands they are about."""
    S, B, T, D = 64, len(lens), sum(lens), 64 * H
    r_ = _rng("wkv7", profile, operand, tuple(lens), H, seed)
    g = lambda s=1.0: (s * r_.standard_normal((T, D))).astype(np.float16)
    d = {"r": g(), "w": g(), "k": g(0.5), "v": g(), "x": g(), "a": r_.random((T, D)).astype(np.float16),
         "kk": _unit_heads(r_.standard_normal((T, D)), H).astype(np.float16)}
    state = (0.3 * r_.standard_normal((B, S + 2, D))).astype(np.float32)
    if profile == TINY:
        if operand == "state":
            state[:, 1:S + 1] = make(TINY, (B, S, D), seed).astype(np.float32) * np.float32(2.0 ** -120)      # f32 subnormals and +-0
        else:
            d[operand] = make(TINY, (T, D), seed, operand)
    elif profile == "decay_limits":     # sigma = 0 / 1 exactly (decay exactly 1 / exactly exp(W_SCALE)) and between
        d["w"] = r_.choice(np.array([65504, -65504, 11, -11, 0.0, -0.0], np.float16), (T, D))
    elif profile == LARGE:              # |y| stays below 65504 and the state below 1e30 (asserted on the CPU by the tests)
        d["k"] = make(LARGE, (T, D), seed, "k")
        d["r"] = (2.0 ** -24 * make(LARGE, (T, D), seed, "r").astype(np.float64)).astype(np.float16)
        state[:, 1:S + 1] *= np.float32(1e5)
    elif profile == CANCELLING:         # r alternating over j so y cancels; kk a alternating so sa's second term cancels
        alt = np.where(np.arange(D) % 2 == 0, 1.0, -1.0)
        d["r"] = (alt * (1.0 + 2.0 ** -9 * r_.integers(0, 2, (T, D)))).astype(np.float16)
        d["kk"] = (alt * 0.125).astype(np.float16) * np.ones((T, 1), np.float16)
        d["a"] = np.ones((T, D), np.float16)
        state[:, 1:S + 1] = np.float32(0.5) + (2.0 ** -8 * r_.standard_normal((B, S, D))).astype(np.float32)
        d["k"] = np.full((T, D), 0.25, np.float16)
    elif profile == "zero_r":
        d["r"] = np.where(r_.integers(0, 2, (T, D)) == 1, -0.0, 0.0).astype(np.float16)
    elif profile != NORMAL:
        raise KeyError(profile)
    d["state"] = state
    return d


def wkv6_inputs(profile, lens, H, seed=0):
    """-> f32 [T, D] decay, k, v, r; f32 u [D]; f16 x [T, D]; f32 state [B, S+2, D]"""
    S, B, T, D = 64, len(lens), sum(lens), 64 * H
    r_ = _rng("wkv6", profile, tuple(lens), H, seed)
    g = lambda s=1.0: (s * r_.standard_normal((T, D))).astype(np.float32)
    d = {"k": g(0.5), "v": g(), "r": g(), "u": (0.3 * r_.standard_normal(D)).astype(np.float32), "x": g().astype(np.float16),
         "decay": np.exp(-np.exp(r_.uniform(-3, 0.5, (T, D)))).astype(np.float32)}
    state = (0.3 * r_.standard_normal((B, S + 2, D))).astype(np.float32)
    if profile == TINY:                 # f16 subnormal values (exact in f32) in k and r, f32 subnormals in the state
        d["k"], d["r"] = (make(TINY, (T, D), seed, z).astype(np.float32) for z in "kr")
        state[:, 1:S + 1] = make(TINY, (B, S, D), seed).astype(np.float32) * np.float32(2.0 ** -120)
    elif profile == "decay_limits":
        d["decay"] = r_.choice(np.array([0.0, 2.0 ** -149, 1.0 - 2.0 ** -24, 1.0], np.float32), (T, D))
    elif profile == LARGE:
        d["k"] = make(LARGE, (T, D), seed, "k").astype(np.float32)
        d["r"] = make(LARGE, (T, D), seed, "r").astype(np.float32) * np.float32(2.0 ** -24)
        state[:, 1:S + 1] *= np.float32(1e5)
    elif profile == CANCELLING:
        alt = np.where(np.arange(D) % 2 == 0, 1.0, -1.0)
        d["r"] = (alt * (1.0 + 2.0 ** -9 * r_.integers(0, 2, (T, D)))).astype(np.float32)
        d["k"] = np.full((T, D), 0.25, np.float32)
        d["u"] = np.full(D, 0.5, np.float32)
        state[:, 1:S + 1] = np.float32(0.5) + (2.0 ** -8 * r_.standard_normal((B, S, D))).astype(np.float32)
    elif profile != NORMAL:
        raise KeyError(profile)
    d["state"] = state
    return d
