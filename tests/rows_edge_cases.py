"""Row profiles that take the logits-row kernels (wrk_sample.hip, wrk_score.hip, wrk_logprob.hip, wrk_penalty.hip and wrk_rows_dev.h
under them) over the whole f32 value range, shared by tests/test_rows_edge_ref.py (CPU) and tests/test_gpu_rows_edges.py.  Not a test
module.

Every profile is a function of (V, seed) that returns an f32 row.  Profiles that need a softmax with spread are built on the recipe of
alt_cases.rows_for -- a head of up to 24 likely tokens on a floor -- so that the cuts fall among tokens that f32 can tell apart.

ORDINARY profiles are judged through the f64 references with their ambiguity rules, on `rows_edge_ref.canonical(row)`:
  peaked             the recipe itself (the temperature / top-p edge tests use it)
  offset_pos / _neg  the peaked row on a 1/4 grid, plus / minus 1.0e6 (ulp 1/16: every difference l - mx is exact; cancellation)
  nan_mix            about 30 % NaN of both signs and three payloads and about 20 % -inf off the head; NaN counts as -inf
  deep_tail          the head at about -32 (never above -30.5), every other token at -60 .. -100: exp(l - mx) of the tail truncates to a
                     fixed-point mass of 0, exp((l - mx) / T) of its upper part does not at T >= 2
  pos_inf_one        the peaked row with one +inf
  signed_zero_floor  the head over a floor of randomly signed zeros: -0 and +0 tie and go by index
  adjacent_one       half the head at 1.0, half at nextafter(1.0, -inf), weights one ulp apart, on a floor at about -13.  (With the whole
                     row on the two values every prefix mass and every interval of the draw lies inside the references' slack: 3 of 36
                     plain cases were unambiguous at V >= 4096.  The typical mode leaves this profile out: its cut orders tokens by
                     |g - gbar|, and two groups one ulp apart lie inside gbar's own rounding whenever the cut falls in the head.)

EXACT-WEIGHT profiles: every weight that feeds a decision is exactly 0 or 1 in f32 (rows_edge_ref.Exact asserts it), so the expected
token is an integer closed form and no case is left out:
  all_equal_zero / _low / _f16max   a constant row: 0.0, -3.2e38 (nothing exceeds the greedy floor of -3e38), 65504.0
  pos_inf_ties       three +inf at scattered indices of the peaked row
  huge_span          three tokens at 3.0e38, a few at -3.0e38, the peaked row between: mx - low overflows
  one_finite         one finite logit in a mix of -inf and NaN
  subnormal          k * 2^-149, k in [-2^20, 2^20], both zeros present: every weight is exactly 1, the order is by value
  adjacent_low       half the row at -1.0e30, half one ulp (7.6e22) below: that half weighs 0
"""
import numpy as np

VOCABS = (1, 2, 1024, 1025, 4096, 4097, 8192, 8193, 16384, 16385)       # both sides of every register-copy boundary of wrk_sample.hip
BIG_V = 1 << 20                                                         # SAMPLE_MAX_VOCAB
NAN_BITS = (0x7FC00000, 0xFFC00001, 0x7F800001)
PAD = (np.inf, np.nan, 7.0e3)                                           # what the padding of a strided buffer holds


def _head(V, seed):
    rng = np.random.default_rng(7919 * seed + V)
    head = rng.choice(V, min(24, max(1, V // 4)), replace=False)
    return rng, head


def _peaked(V, seed):
    rng, head = _head(V, seed)
    x = rng.normal(0.0, 2.0, V)
    x[head] += rng.normal(14.0, 1.0, head.size)
    return rng, head, x


def _off_head(rng, V, head, count):
    rest = np.setdiff1d(np.arange(V), head)
    return rng.choice(rest, min(count, rest.size), replace=False)


def peaked(V, seed):
    return _peaked(V, seed)[2].astype(np.float32)


def _offset(V, seed, off):
    x = np.round(_peaked(V, seed)[2] * 4.0) / 4.0 + off
    out = x.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), x)        # on the grid, exactly
    return out


def offset_pos(V, seed):
    return _offset(V, seed, 1.0e6)


def offset_neg(V, seed):
    return _offset(V, seed, -1.0e6)


def nan_mix(V, seed):
    rng, head, x = _peaked(V, seed)
    out = x.astype(np.float32)
    bits = out.view(np.uint32)
    r = rng.random(V)
    kind = rng.integers(len(NAN_BITS), size=V)
    off = np.ones(V, bool)
    off[head] = False
    for j, b in enumerate(NAN_BITS):
        bits[off & (r < 0.3) & (kind == j)] = b
    out[off & (r >= 0.3) & (r < 0.5)] = -np.inf
    return out


def deep_tail(V, seed):
    rng, head = _head(V, seed)
    x = rng.uniform(-100.0, -60.0, V)
    x[head] = np.minimum(rng.normal(-32.0, 1.0, head.size), -30.5)
    return x.astype(np.float32)


def pos_inf_one(V, seed):
    rng, head, x = _peaked(V, seed)
    x[_off_head(rng, V, head, 1)] = np.inf
    if V == 1:
        x[0] = np.inf
    return x.astype(np.float32)


def signed_zero_floor(V, seed):
    rng, head = _head(V, seed)
    x = np.where(rng.random(V) < 0.5, -0.0, 0.0)
    x[head] = rng.normal(14.0, 1.0, head.size)
    return x.astype(np.float32)


def _adjacent(V, seed, a):
    rng, _ = _head(V, seed)
    a = np.float32(a)
    x = np.full(V, a, np.float32)
    x[rng.random(V) < 0.5] = np.nextafter(a, np.float32(-np.inf))
    return x


def adjacent_one(V, seed):
    rng, head = _head(V, seed)
    x = rng.normal(-13.0, 2.0, V).astype(np.float32)
    x[head] = _adjacent(head.size, seed, 1.0)
    return x


def adjacent_low(V, seed):
    return _adjacent(V, seed, -1.0e30)


def _const(c):
    def f(V, seed):
        return np.full(V, c, np.float32)
    return f


def pos_inf_ties(V, seed):
    rng, head, x = _peaked(V, seed)
    x[rng.choice(V, min(3, V), replace=False)] = np.inf
    return x.astype(np.float32)


def huge_span(V, seed):
    rng, head, x = _peaked(V, seed)
    idx = rng.choice(V, min(8, V), replace=False)
    x[idx[3:]] = -3.0e38
    x[idx[:3]] = 3.0e38
    return x.astype(np.float32)


def one_finite(V, seed):
    rng, _ = _head(V, seed)
    out = np.full(V, -np.inf, np.float32)
    bits = out.view(np.uint32)
    r = rng.random(V)
    for j, b in enumerate(NAN_BITS):
        bits[(r > 0.2 * j) & (r < 0.2 * j + 0.15)] = b
    out[rng.integers(V)] = np.float32(rng.normal(0.0, 3.0))
    return out


def subnormal(V, seed):
    rng, _ = _head(V, seed)
    k = rng.integers(-2 ** 20, 2 ** 20 + 1, V)
    out = (k.astype(np.float64) * 2.0 ** -149).astype(np.float32)
    z = rng.choice(V, min(4, V), replace=False)
    out[z] = 0.0
    out[z[::2]] = -0.0
    return out


ORDINARY = {"offset_pos": offset_pos, "offset_neg": offset_neg, "nan_mix": nan_mix, "deep_tail": deep_tail, "pos_inf_one": pos_inf_one,
            "signed_zero_floor": signed_zero_floor, "adjacent_one": adjacent_one}
EXACT = {"all_equal_zero": _const(0.0), "all_equal_low": _const(-3.2e38), "all_equal_f16max": _const(65504.0), "pos_inf_ties": pos_inf_ties,
         "huge_span": huge_span, "one_finite": one_finite, "subnormal": subnormal, "adjacent_low": adjacent_low}
PROFILES = {"peaked": peaked, **ORDINARY, **EXACT}
NOT_TYPICAL = ("adjacent_one", "subnormal")         # adjacent_one: the note above; subnormal: its typical order is not specified (rows_edge_ref)
SEED = 1


def row(name, V, seed=SEED):
    out = PROFILES[name](V, seed)
    assert out.dtype == np.float32 and out.shape == (V,)
    return out


def strided(rows, pad=3):
    """[n, V] rows -> a flat f32 buffer of n rows of stride V + pad whose padding cycles through PAD, and the stride."""
    rows = np.atleast_2d(rows)
    n, V = rows.shape
    buf = np.empty((n, V + pad), np.float32)
    buf[:, :V] = rows
    buf[:, V:] = np.resize(np.array(PAD, np.float32), (n, pad))
    return buf.reshape(-1), V + pad
