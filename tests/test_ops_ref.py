"""tests/ops_ref.py proved on the CPU, before any GPU sees its bounds: they are neither wrong nor vacuous.

  * reference alone: the same expressions in float32 NumPy, in three summation orders (sequential, pairwise, the kernels' strided
    per-thread order followed by a tree), lie within the bound of the f64 value for every op and profile; at most 1 % of a case's
    elements are excused as "near the f16 overflow threshold".  The sequential order runs on rows of up to 64 elements (one head: group
    norm, l2 norm, WKV, the bonus; softmax on 5): a sequential f32 sum of n terms is only good for n 2^-24 sum|terms|, which is below
    C_RED = 4e-6 up to n = 67 -- at C = 1000 a `one_hot` row (one large square followed by 999 equal small ones, all rounded the same
    way) exceeds C_RED tenfold, and no kernel adds more than 16 elements in sequence before its tree;
  * tight: on the `normal` profile no bound exceeds 2 f16 ulps (see `tight`).  The ulp is that of the output wherever the output is of the size of its
    addends (|want| >= terms / 2) and that of sum|addends| elsewhere: an output that is itself a cancelled sum (d dev w + b near 0) has
    no relative accuracy in any arithmetic, and the existing tests grant such an element the spacing of its buffer;
  * mutants: deliberately wrong variants each violate the bound on a named profile (MUTANTS below names it).
"""
import numpy as np
import pytest

import ops_ref as R

f32 = np.float32
ORDERS = ("sequential", "pairwise", "strided")


def sum32(a, order, nt=256, dtype=np.float32):
    """sum over the last axis in `dtype` arithmetic, in one of three orders"""
    a = np.asarray(a, dtype)
    n = a.shape[-1]
    if order == "sequential":
        return np.cumsum(a, -1, dtype=dtype)[..., -1]
    if order == "strided":          # thread i adds elements i, i + nt, ... in that order; then a tree over the threads
        pad = (-n) % nt
        a = np.concatenate([a, np.zeros(a.shape[:-1] + (pad,), dtype)], -1).reshape(a.shape[:-1] + (-1, nt))
        a = np.cumsum(a, -2, dtype=dtype)[..., -1, :]
        n = nt
    p = 1
    while p < n:
        p *= 2
    a = np.concatenate([a, np.zeros(a.shape[:-1] + (p - n,), dtype)], -1)
    while a.shape[-1] > 1:
        a = (a[..., 0::2] + a[..., 1::2]).astype(dtype)
    return a[..., 0]


def h(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x).astype(np.float16)


# ----------------------------------------------------------------------------- float32 restatements (with their mutants)
def ln32(x, w, b, eps, order, mutant=None):
    st = np.float16 if mutant == "f16_stats" else np.float32
    x, w, b, eps = f32(x), f32(w), f32(b), f32(eps)
    C = f32(x.shape[-1])
    with np.errstate(all="ignore"):
        mean = f32(sum32(x, order, dtype=st))[..., None] / C
        d = x - mean
        if mutant == "one_pass":
            var = sum32(x * x, order)[..., None] / C - mean * mean
        else:
            var = f32(sum32(d * d, order, dtype=st))[..., None] / C
        if mutant == "eps_dropped":
            dev = f32(1) / np.sqrt(var)
        elif mutant == "eps_after_sqrt":
            dev = f32(1) / (np.sqrt(var) + eps)
        else:
            dev = f32(1) / np.sqrt(var + eps)
        return h((d * dev) * w + b)


def l2n32(x, eps, order):
    x = f32(x)
    return h(x * (f32(1) / np.sqrt(sum32(x * x, order, 64)[..., None] + f32(eps))))


def softmax32(x, order, mutant=None):
    x = f32(x)
    with np.errstate(all="ignore"):
        m = f32(0) if mutant == "no_max" else x.max(-1, keepdims=True)
        e = np.exp(x - m)
        return e / sum32(e, order)[..., None]


def mix32(x, y, a):
    x, y, a = f32(x), f32(y), f32(a)
    return h(x * (f32(1) - a) + y * a)


def flush16(x):
    x = np.asarray(x, np.float16)
    return np.where(np.abs(x) < f32(2.0 ** -14), np.float16(0), x)


def act32(name, x, mutant=None):
    x = f32(x)
    with np.errstate(all="ignore"):
        if name == "squared_relu":
            p = np.maximum(x, f32(0))
            return p * p
        if name == "tanh":
            return np.where(x > 42, f32(1), np.tanh(x))
        if name == "stable_exp":
            return np.exp(-np.exp(x))
        if name == "opposite_exp":
            return -np.exp(x)
        if name == "softplus":
            return np.log(f32(1) + np.exp(x))
        if name == "sigmoid":
            return np.exp(x) / (f32(1) + np.exp(x)) if mutant == "exp_over_one_plus_exp" else f32(1) / (f32(1) + np.exp(-x))
        if name == "silu":
            return x / (f32(1) + np.exp(-x))
    raise KeyError(name)


def wkv7_32(d, lens, H, order, mutant=None):
    S = 64
    st = d["state"][:, :S + 1].astype(np.float32).copy()
    r, w, k, v, a, kk = (f32(d[z]).reshape(-1, H, S) for z in ("r", "w", "k", "v", "a", "kk"))
    y = np.zeros(r.shape, np.float32)
    with np.errstate(over="ignore"):
        wt = np.exp(f32(R.W_SCALE) * (f32(1) / (f32(1) + np.exp(-w))))
    for b, start, n in R.cursors_of(lens):
        Sm = st[b, 1:].reshape(S, H, S).transpose(1, 0, 2).copy()       # [H, j, i]
        for t in range(start, start + n):
            at, bt = -kk[t][:, :, None], (kk[t] * a[t])[:, :, None]
            wj, kv = wt[t][:, :, None], k[t][:, :, None] * v[t][:, None, :]
            sa = sum32((Sm * at).transpose(0, 2, 1), order, 16)[:, None, :]
            if mutant == "sa_updated_state":
                Sm = Sm * wj + kv
                sa = sum32((Sm * at).transpose(0, 2, 1), order, 16)[:, None, :]
                Sm = Sm + sa * bt
            elif mutant == "decay_after_kv":
                Sm = (Sm + kv) * wj + sa * bt
            else:
                Sm = Sm * wj + kv + sa * bt
            y[t] = sum32((r[t][:, :, None] * Sm).transpose(0, 2, 1), order, 16)
        st[b, 1:] = Sm.transpose(1, 0, 2).reshape(S, H * S)
    return h(y.reshape(y.shape[0], -1)), st


def wkv6_32(d, lens, H, order):
    S = 64
    st = d["state"][:, :S + 1].astype(np.float32).copy()
    decay, k, v, r = (f32(d[z]).reshape(-1, H, S) for z in ("decay", "k", "v", "r"))
    u = f32(d["u"]).reshape(H, S)[:, :, None]
    y = np.zeros(r.shape, np.float32)
    for b, start, n in R.cursors_of(lens):
        Sm = st[b, 1:].reshape(S, H, S).transpose(1, 0, 2).copy()
        for t in range(start, start + n):
            kv = k[t][:, :, None] * v[t][:, None, :]
            y[t] = sum32((r[t][:, :, None] * (u * kv + Sm)).transpose(0, 2, 1), order, 16)
            Sm = decay[t][:, :, None] * Sm + kv
        st[b, 1:] = Sm.transpose(1, 0, 2).reshape(S, H * S)
    return h(y.reshape(y.shape[0], -1)), st


# ----------------------------------------------------------------------------- helpers
def inside(got16, want, bound, what):
    ratio, near = R.check16(got16, want, bound)
    assert near <= 0.01 * ratio.size, f"{what}: {near} of {ratio.size} elements near the f16 overflow threshold (cap 1 %)"
    assert ratio.max() <= 1.0, f"{what}: worst error / bound = {ratio.max():.3g}"
    return float(ratio.max())


def violates(got16, want, bound):
    return R.check16(got16, want, bound)[0].max() > 1.0


def tight(want, bound, terms, what, row=False):
    """`row` (the norms): the error of the row's mean and deviation is shared by every element of the row, so an element near the mean
    (|want| far below the row's rms) is measured with the spacing at the rms, as tests/test_gpu_layer_parity.py's `ulps` does."""
    want, bound, terms = (np.broadcast_to(np.asarray(z, np.float64), np.shape(want)) for z in (want, bound, terms))
    if row:
        terms = np.maximum(terms, np.sqrt((want * want).mean(-1, keepdims=True)) / 2)
    assert (bound <= 2 * R.ulp16(np.maximum(np.abs(want), terms))).all(), what
    own = np.abs(want) >= terms / 2
    assert own.mean() > 0.5 and (bound[own] <= 2 * R.ulp16(want[own])).all(), what


def ln_case(profile, C, rows=4):
    x = R.make(profile, (rows, C), "ln")
    w = (1.0 + 0.25 * R.make(R.NORMAL, (C,), "w").astype(np.float64)).astype(np.float16)
    b = (0.05 * R.make(R.NORMAL, (C,), "b").astype(np.float64)).astype(np.float16)
    return x, w, b


# ----------------------------------------------------------------------------- reference alone stays inside the bound
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("profile", R.PROFILES)
def test_norms_in_f32_stay_inside_the_bound(profile, order):
    for C, eps in ((1000, 1e-5), (64, 64e-5)):
        if order == "sequential" and C * R.U32 > R.C_RED:
            continue
        x, w, b = ln_case(profile, C)
        want, e, terms = R.layer_norm(x, w, b, eps)
        inside(ln32(x, w, b, eps, order), want, e + R.ulp16(want) / 2, f"layer_norm {profile} C={C} {order}")
    x = R.make(profile, (4, 64), "l2")
    want, e, _ = R.l2_norm(x, 1e-12)
    inside(l2n32(x, 1e-12, order), want, e + R.ulp16(want) / 2, f"l2_norm {profile} {order}")
    if profile == R.ZERO_ROW:
        assert not l2n32(x, 1e-12, order).astype(np.float32).any()


SOFTMAX_ROWS = ("normal", "span", "neg_inf", "one_hot_max", "constant", "large")


def softmax_rows(kind, C):
    r = R._rng("softmax", kind, C)
    x = (4 * r.standard_normal((2, C))).astype(np.float32)
    if kind == "span":                  # rows spanning +-3e38
        x = (r.uniform(-3e38, 3e38, (2, C))).astype(np.float32)
        x[:, 0], x[:, -1] = 3e38, -3e38
        x[1, 1] = np.nextafter(np.float32(3e38), np.float32(0))
    elif kind == "neg_inf":
        x[:, ::3] = -np.inf
    elif kind == "one_hot_max":
        x[:] = 0
        x[0, C // 2], x[1, 0] = np.finfo(np.float32).max, np.finfo(np.float32).max
    elif kind == "constant":
        x[:] = x[:, :1]
    elif kind == "large":
        x = R.make(R.LARGE, (2, C), "softmax").astype(np.float32)
    return x


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", SOFTMAX_ROWS)
def test_softmax_in_f32_stays_inside_the_bound(kind, order):
    for C in (1000, 5):
        if order == "sequential" and C * R.U32 > R.C_RED:
            continue
        x = softmax_rows(kind, C)
        want, e = R.softmax(x)
        ratio = R.check32(softmax32(x, order), want, e)
        assert ratio.max() <= 1.0, (kind, C, order, float(ratio.max()))
        assert abs(want.sum(-1) - 1).max() < 1e-12


@pytest.mark.parametrize("profile", R.PROFILES)
def test_elementwise_in_f32_stay_inside_the_bound(profile):
    C = 250
    x, y = R.make(profile, (3, C), "x"), R.make(profile, (3, C), "y")
    z, fa = R.make(R.NORMAL, (3, C), "z"), R.factors((3, C), profile)
    fx, fy, fz, ff = f32(x), f32(y), f32(z), f32(fa)
    with np.errstate(all="ignore"):
        cases = {"add": (R.add(x, y), h(fx + fy)), "mul": (R.mul(x, z), h(fx * fz)), "affine": (R.affine(x, 0.5, -3.0), h(f32(0.5) * fx + f32(-3.0))),
                 "mix": (R.mix(x, y, fa), mix32(x, y, fa)), "mix_z": (R.mix(x, z, fa), mix32(x, z, fa)),
                 "control_k": (R.control_k(x, fa, z), h(fx * (f32(1) + (ff - f32(1)) * fz))),
                 "channel_mix_v6": (R.channel_mix_v6(x, z), h((f32(1) / (f32(1) + np.exp(-fx))) * fz))}
    for name, ((want, terms, n), got) in cases.items():
        inside(got, want, R.bound16(want, terms, n), f"{name} {profile}")
        if profile == R.NORMAL:
            tight(want, R.bound16(want, terms, n), terms, name)


@pytest.mark.parametrize("act", R.ACTS)
def test_activations_in_f32_are_within_one_f16_step_of_the_staged_value(act):
    x = R.finite_f16_patterns()
    want = R.r16(R.act_expected(act, x))
    got = h(act32(act, x))
    assert not np.isnan(got).any()
    assert np.abs(R.ordered16(got) - R.ordered16(want)).max() <= 1


def test_activation_overflow_zones_of_the_reference_formula():
    e = lambda act, v: float(R.act_expected(act, np.array([v], np.float32))[0])
    assert e("softplus", 88.72) < np.inf and e("softplus", 88.73) == np.inf
    assert e("opposite_exp", 88.72) > -np.inf and e("opposite_exp", 88.73) == -np.inf
    assert np.isfinite(R.r16(e("opposite_exp", 11.08))) and np.isneginf(R.r16(e("opposite_exp", 11.0903)))
    assert e("silu", -88.73) == 0 and np.signbit(e("silu", -88.73)) and e("silu", -88.0) < 0
    assert e("sigmoid", -65504.0) == 0 and e("sigmoid", 65504.0) == 1 and e("stable_exp", 65504.0) == 0 and e("tanh", 65504.0) == 1


WKV_LENS, WKV_H = [3, 0, 2], 3


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("profile", R.WKV_PROFILES)
def test_wkv7_in_f32_stays_inside_the_bound(profile, order):
    for operand in (R.WKV_OPERANDS if profile == R.TINY else ("r",)):
        d = R.wkv7_inputs(profile, operand, WKV_LENS, WKV_H)
        y, ey, ty, st, E = R.wkv7(d["state"][:, :65], d["r"], d["w"], d["k"], d["v"], d["a"], d["kk"], WKV_LENS, WKV_H)
        assert np.abs(y).max() < R.F16_MAX and np.abs(st).max() < 1e30
        got_y, got_st = wkv7_32(d, WKV_LENS, WKV_H, order)
        inside(got_y, y, ey + R.ulp16(y) / 2, f"wkv7 y {profile}/{operand} {order}")
        assert R.check32(got_st[:, 1:], st[:, 1:], E[:, 1:]).max() <= 1.0, (profile, operand, order)
        if profile == "zero_r":
            assert not y.any() and not got_y.astype(np.float32).any()
        if profile == R.NORMAL:
            assert (ey + R.ulp16(y) / 2 <= 2 * R.ulp16(np.maximum(np.abs(y), ty))).all()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("profile", (R.NORMAL, R.TINY, "decay_limits", R.LARGE, R.CANCELLING))
def test_wkv6_in_f32_stays_inside_the_bound(profile, order):
    d = R.wkv6_inputs(profile, WKV_LENS, WKV_H)
    y, ey, ty, st, E = R.wkv6(d["state"][:, :65], d["decay"], d["u"], d["k"], d["v"], d["r"], WKV_LENS, WKV_H)
    assert np.abs(y).max() < R.F16_MAX and np.abs(st).max() < 1e30
    got_y, got_st = wkv6_32(d, WKV_LENS, WKV_H, order)
    inside(got_y, y, ey + R.ulp16(y) / 2, f"wkv6 y {profile} {order}")
    assert R.check32(got_st[:, 1:], st[:, 1:], E[:, 1:]).max() <= 1.0, (profile, order)
    if profile == R.NORMAL:
        assert (ey + R.ulp16(y) / 2 <= 2 * R.ulp16(np.maximum(np.abs(y), ty))).all()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("profile", R.PROFILES)
def test_time_first_in_f32_stays_inside_the_bound(profile, order):
    H, T, S = 3, 2, 64
    u, k, r = (R.make(profile if profile != R.LARGE else R.NORMAL, (T, H, S), z) for z in "ukr")
    if profile == R.LARGE:              # one large factor per product: u k r stays finite in f16 terms
        k = R.make(R.LARGE, (T, H, S), "k")
    u = np.broadcast_to(u[:1], u.shape)
    v, x = R.make(R.NORMAL, (T, H, S), "v"), R.make(R.NORMAL, (T, H, S), "x")
    want, e, terms = R.time_first(u, k, r, v, x)
    with np.errstate(all="ignore"):
        got = h(f32(x) + sum32(f32(u) * f32(k) * f32(r), order, 64)[..., None] * f32(v))
    inside(got, want, e + R.ulp16(want) / 2, f"time_first {profile} {order}")
    if profile == R.NORMAL:
        tight(want, e + R.ulp16(want) / 2, terms, "time_first")


def test_norm_bounds_are_tight_on_normal_inputs():
    for C, eps in ((64, 64e-5), (1000, 1e-5), (4104, 1e-5)):
        x, w, b = ln_case(R.NORMAL, C)
        want, e, terms = R.layer_norm(x, w, b, eps)
        tight(want, e + R.ulp16(want) / 2, terms, f"layer_norm C={C}", row=True)
    x = R.make(R.NORMAL, (4, 64), "l2")
    want, e, terms = R.l2_norm(x, 1e-12)
    tight(want, e + R.ulp16(want) / 2, terms, "l2_norm", row=True)


# ----------------------------------------------------------------------------- mutants
MUTANTS = {  # mutant -> the profile that catches it
    "one_pass": R.OFFSET, "f16_stats": R.NORMAL, "eps_dropped": R.TINY, "eps_after_sqrt": R.TINY, "lerp_swapped": R.NORMAL,
    "sa_updated_state": R.NORMAL, "decay_after_kv": R.NORMAL, "subnormals_flushed": R.TINY, "exp_over_one_plus_exp": R.LARGE, "no_max": R.LARGE,
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_violates_the_bound(mutant):
    profile = MUTANTS[mutant]
    if mutant in ("one_pass", "f16_stats", "eps_dropped", "eps_after_sqrt"):
        x, w, b = ln_case(profile, 1000)
        want, e, _ = R.layer_norm(x, w, b, 1e-5)
        assert not violates(ln32(x, w, b, 1e-5, "strided"), want, e + R.ulp16(want) / 2)
        assert violates(ln32(x, w, b, 1e-5, "strided", mutant), want, e + R.ulp16(want) / 2)
        if mutant == "eps_dropped":     # a constant row: 0 / 0
            x = R.make(R.CONSTANT, (4, 1000), "ln")
            assert np.isnan(ln32(x, w, b, 1e-5, "strided", mutant)).any()
    elif mutant == "lerp_swapped":
        x, y, a = R.make(profile, (3, 250), "x"), R.make(profile, (3, 250), "y"), R.factors((3, 250), 0)
        want, terms, n = R.mix(x, y, a)
        assert not violates(mix32(x, y, a), want, R.bound16(want, terms, n)) and violates(mix32(y, x, a), want, R.bound16(want, terms, n))
    elif mutant in ("sa_updated_state", "decay_after_kv"):
        d = R.wkv7_inputs(profile, "r", WKV_LENS, WKV_H)
        y, ey, ty, st, E = R.wkv7(d["state"][:, :65], d["r"], d["w"], d["k"], d["v"], d["a"], d["kk"], WKV_LENS, WKV_H)
        got_y, got_st = wkv7_32(d, WKV_LENS, WKV_H, "strided", mutant)
        assert violates(got_y, y, ey + R.ulp16(y) / 2) and R.check32(got_st[:, 1:], st[:, 1:], E[:, 1:]).max() > 1.0
    elif mutant == "subnormals_flushed":
        x, y = R.make(profile, (3, 250), "x"), R.make(profile, (3, 250), "y")
        want, terms, n = R.add(x, y)
        assert violates(h(f32(flush16(x)) + f32(flush16(y))), want, R.bound16(want, terms, n))
        d = R.wkv7_inputs(profile, "k", WKV_LENS, WKV_H)
        y7, ey, ty, st, E = R.wkv7(d["state"][:, :65], d["r"], d["w"], d["k"], d["v"], d["a"], d["kk"], WKV_LENS, WKV_H)
        got_st = wkv7_32(dict(d, k=flush16(d["k"])), WKV_LENS, WKV_H, "strided")[1]
        assert R.check32(got_st[:, 1:], st[:, 1:], E[:, 1:]).max() > 1.0
    elif mutant == "exp_over_one_plus_exp":
        x = R.make(profile, (3, 250), "x")
        want = R.r16(R.act_expected("sigmoid", x))
        assert np.abs(R.ordered16(h(act32("sigmoid", x))) - R.ordered16(want)).max() <= 1
        assert np.isnan(act32("sigmoid", x, mutant)).any()
    elif mutant == "no_max":
        x = softmax_rows("large", 1000)
        want, e = R.softmax(x)
        assert R.check32(softmax32(x, "strided"), want, e).max() <= 1.0 and R.check32(softmax32(x, "strided", mutant), want, e).max() > 1.0
    else:
        raise KeyError(mutant)
