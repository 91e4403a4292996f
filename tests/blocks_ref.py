"""Raw weight blocks and activation vectors over the whole value range of the formats, for NumPy.

The quantisers in oracle/quantize.py only emit a small corner of what the block formats can hold (positive d, scales clipped away from
0 / -128, Gaussian codes).  `make_blocks` writes the block BYTES directly, from the format descriptions (ggml's k-quants as restated in
gguf.rs:11-274; web-rwkv's Int8 / NF4 planes), so that a matmul kernel can be checked on encodings no quantiser here produces.
Nothing is imported from the product or from the oracle.

Layouts written here (little endian, rows of K elements, M rows):
  Q4_K  144 B / 256: d f16 | dmin f16 | scales[12] (8 x 6-bit sc, 8 x 6-bit m) | qs[128]           w = d*sc*q - dmin*m,  q in 0..15
  Q5_K  176 B / 256: d | dmin | scales[12] | qh[32] | ql[128]                                      same, q in 0..31
  Q6_K  210 B / 256: ql[128] | qh[64] | scales[16] i8 | d f16                                      w = d*sc*(q - 32), q in 0..63
  Q8_0   34 B / 32 : d f16 | q[32] i8                                                              w = d*q
  F16   2 B / element
  INT8  codes u8 [M*K] then (min, max) f16 per 128 FLATTENED elements                              w = c/255 * (max - min) + min
  NF4   nibbles [M*K/2] (element 2i low) then absmax f16 per 64 flattened elements                 w = level[c] * absmax

Every TERM of every decoded weight (d*sc*q, dmin*m, d*sc*(q-32), d*q, c/255*max, c/255*min, min, level*absmax) stays at or below
TERM_CAP = 2^10 in absolute value: the reference dequantises to f16, so an encoding whose weights leave the f16 range has no defined
expected value.  F16 weights are f16 by definition and go up to 65504.  Non-finite d / dmin / weights / inputs are out of scope for the
same reason: no generator here emits an inf or a NaN.
"""
import numpy as np

UNIFORM_BYTES = "uniform_bytes"
EXTREME_CODES = "extreme_codes"
SIGNED = "signed"
D_RANGE = "d_range"
ENCODINGS = (UNIFORM_BYTES, EXTREME_CODES, SIGNED, D_RANGE)

NORMAL = "normal"
LARGE = "large"
LARGE_SAME_SIGN = "large_same_sign"
TINY = "tiny"
SPARSE = "sparse"
CANCELLING = "cancelling"
INPUTS = (NORMAL, LARGE, LARGE_SAME_SIGN, TINY, SPARSE, CANCELLING)

KINDS = ("Q4_K", "Q5_K", "Q6_K", "Q8_0", "F16", "INT8", "NF4")
BLOCK_BYTES = {"Q4_K": 144, "Q5_K": 176, "Q6_K": 210, "Q8_0": 34}
BLOCK_ELEMS = {"Q4_K": 256, "Q5_K": 256, "Q6_K": 256, "Q8_0": 32, "F16": 1, "INT8": 128, "NF4": 64}
TERM_CAP = 2.0 ** 10
F16_MAX = 65504.0
F16_TINY = 2.0 ** -24
NF4_LEVELS = np.array([-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635,
                       -0.18477343022823334, -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725,
                       0.24611230194568634, 0.33791524171829224, 0.44070982933044434, 0.5626170039176941,
                       0.7229568362236023, 1.0], dtype=np.float32)


def _rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _f16_bytes(v):
    """float array [...] -> uint8 [..., 2] (little-endian f16)."""
    a = np.asarray(v, np.float64).astype("<f2")
    return a.view(np.uint8).reshape(a.shape + (2,))


def _log_uniform(r, lo, hi, shape):
    return np.exp2(r.uniform(np.log2(lo), np.log2(hi), shape))


def _zeros_pm(r, v):
    """Sprinkle exact +0.0 and -0.0 over ~1/8 of a float array (at least one of each when it has two elements)."""
    v = np.array(v, np.float64)
    f = v.reshape(-1)
    pick = r.random(f.size)
    f[pick < 1 / 16] = 0.0
    f[(pick >= 1 / 16) & (pick < 1 / 8)] = -0.0
    if f.size >= 2:
        i = r.permutation(f.size)[:2]
        f[i[0]], f[i[1]] = 0.0, -0.0
    return v


def _ends(r, v):
    """Put both ends of the d range, 2^-24 and 1.0, into a float array (two distinct places)."""
    i = r.permutation(v.size)[:2]
    v.reshape(-1)[i[0]], v.reshape(-1)[i[-1]] = F16_TINY, 1.0
    return v


def pack_scales_k4(sc, mn):
    """sc, mn: uint8 [..., 8] in 0..63 -> scales[12] of a Q4_K / Q5_K block (the inverse of get_scale_min_k4)."""
    sc, mn = np.asarray(sc, np.uint8), np.asarray(mn, np.uint8)
    out = np.zeros(sc.shape[:-1] + (12,), np.uint8)
    for j in range(4):
        out[..., j] = (sc[..., j] & 63) | ((sc[..., j + 4] >> 4) << 6)
        out[..., j + 4] = (mn[..., j] & 63) | ((mn[..., j + 4] >> 4) << 6)
        out[..., j + 8] = (sc[..., j + 4] & 0xF) | ((mn[..., j + 4] & 0xF) << 4)
    return out


def unpack_scales_k4(s):
    s = np.asarray(s, np.uint8)
    sc = np.zeros(s.shape[:-1] + (8,), np.uint8)
    mn = np.zeros_like(sc)
    for j in range(4):
        sc[..., j] = s[..., j] & 63
        mn[..., j] = s[..., j + 4] & 63
        sc[..., j + 4] = (s[..., j + 8] & 0xF) | ((s[..., j] >> 6) << 4)
        mn[..., j + 4] = (s[..., j + 8] >> 4) | ((s[..., j + 4] >> 6) << 4)
    return sc, mn


# ------------------------------------------------------------------------------------------------ K-quants with a min term
def _k4(kind, k, m, enc, r):
    nb = k // 256
    q5 = kind == "Q5_K"
    qmax = 31 if q5 else 15
    nq = 160 if q5 else 128                                   # qh + ql | qs
    sc = r.integers(0, 64, (m, nb, 8)).astype(np.uint8)
    mn = r.integers(0, 64, (m, nb, 8)).astype(np.uint8)
    qb = r.integers(0, 256, (m, nb, nq)).astype(np.uint8)
    d = _log_uniform(r, 2.0 ** -10, 2.0 ** -5, (m, nb))
    dmin = _log_uniform(r, 2.0 ** -10, 2.0 ** -5, (m, nb))
    if enc == UNIFORM_BYTES:
        scales = r.integers(0, 256, (m, nb, 12)).astype(np.uint8)
        sc, mn = unpack_scales_k4(scales)
    elif enc == EXTREME_CODES:
        # block (row i, block b) is of sort (i + b) % 6; a row of fewer than six blocks still differs from its neighbours
        sort = (np.arange(m)[:, None] + np.arange(nb)[None, :]) % 6
        s3 = sort[:, :, None]
        qb = np.where(s3 == 0, 0xFF, np.where(s3 == 1, 0x00, qb)).astype(np.uint8)             # all codes at maximum | all zero
        sc = np.where((s3 == 0) | (s3 == 1) | (s3 == 4), 63, sc)
        mn = np.where((s3 == 0) | (s3 == 1) | (s3 == 4), 63, mn)
        sc = np.where(s3 == 2, 0, sc)                                                           # sc = 0 with m != 0
        mn = np.where(s3 == 2, np.maximum(mn, 1), mn)
        mn = np.where(s3 == 3, 0, mn)                                                           # m = 0 with sc != 0
        sc = np.where(s3 == 3, np.maximum(sc, 1), sc)
        qb = np.where(s3 == 5, np.where(r.random((m, nb, 1)) < 0.5, 0xFF, 0x00), qb).astype(np.uint8)   # sort 5: random sc / m, codes all max or all zero
        sc, mn = sc.astype(np.uint8), mn.astype(np.uint8)
    elif enc == SIGNED:
        sd = np.where(r.random((m, nb)) < 0.5, -1.0, 1.0)
        sm = np.where(r.random((m, nb)) < 0.5, -1.0, 1.0)
        sd[:, 0], sm[:, 0] = -1.0, 1.0                        # every row: a negative d and a positive dmin ...
        if nb > 1:
            sd[:, 1], sm[:, 1] = 1.0, -1.0                    # ... and the other way round
        else:
            sm[:, 0] = -1.0
        d, dmin = d * sd, dmin * sm
    elif enc == D_RANGE:
        d = _zeros_pm(r, _log_uniform(r, F16_TINY, 1.0, (m, nb)))
        dmin = _zeros_pm(r, _log_uniform(r, F16_TINY, 1.0, (m, nb)))
        d, dmin = _ends(r, d), _ends(r, dmin)
    else:
        raise ValueError(enc)
    if enc != UNIFORM_BYTES:
        # keep |d * sc * q| <= TERM_CAP (|dmin * m| <= 63 always): only d_range comes near (Q5_K: 1 * 63 * 31)
        d16 = np.abs(np.asarray(d).astype(np.float16).astype(np.float64))
        lim = np.floor(TERM_CAP / np.maximum(d16 * qmax, 1e-30)).clip(0, 63)
        sc = np.minimum(sc, lim[:, :, None]).astype(np.uint8)
        scales = pack_scales_k4(sc, mn)
    raw = np.concatenate([_f16_bytes(d), _f16_bytes(dmin), scales, qb], axis=2)
    assert raw.shape[2] == BLOCK_BYTES[kind]
    return raw.reshape(-1)


def _q6k(k, m, enc, r):
    nb = k // 256
    ql = r.integers(0, 256, (m, nb, 128)).astype(np.uint8)
    qh = r.integers(0, 256, (m, nb, 64)).astype(np.uint8)
    sc = r.integers(-128, 128, (m, nb, 16)).astype(np.int64)
    d = _log_uniform(r, 2.0 ** -10, 2.0 ** -6, (m, nb))
    if enc == UNIFORM_BYTES:
        pass
    elif enc == EXTREME_CODES:
        sort = ((np.arange(m)[:, None] + np.arange(nb)[None, :]) % 5)[:, :, None]
        ql = np.where((sort == 0) | (sort == 4), 0xFF, np.where(sort == 1, 0x00, ql)).astype(np.uint8)
        qh = np.where((sort == 0) | (sort == 4), 0xFF, np.where(sort == 1, 0x00, qh)).astype(np.uint8)
        sc = np.where((sort == 2) | (sort == 4), 127, np.where(sort == 3, 0, np.clip(np.abs(sc), 1, 127)))   # scales at 127 | scale 0 | positive
    elif enc == SIGNED:
        sd = np.where(r.random((m, nb)) < 0.5, -1.0, 1.0)
        sd[:, 0] = -1.0
        if nb > 1:
            sd[:, 1] = 1.0
        d = d * sd
        rows = np.arange(m)
        sc[rows, r.integers(0, nb, m), r.integers(0, 16, m)] = -128
        sc[rows, r.integers(0, nb, m), (r.integers(0, 16, m) + 1) % 16] = 127
        d = np.minimum(np.abs(d), 2.0 ** -6) * np.sign(d)
    elif enc == D_RANGE:
        d = _zeros_pm(r, _log_uniform(r, F16_TINY, 1.0, (m, nb)))
        d = _ends(r, d)
    else:
        raise ValueError(enc)
    d16 = np.abs(np.asarray(d).astype(np.float16).astype(np.float64))
    lim = np.floor(TERM_CAP / np.maximum(d16 * 32.0, 1e-30)).clip(0, 128)[:, :, None]      # |d * sc * (q - 32)| <= TERM_CAP
    sc = np.clip(sc, -lim, np.minimum(lim, 127)).astype(np.int8)
    raw = np.concatenate([ql, qh, sc.view(np.uint8), _f16_bytes(d)], axis=2)
    assert raw.shape[2] == 210
    return raw.reshape(-1)


def _q80(k, m, enc, r):
    nb = k // 32
    q = r.integers(-128, 128, (m, nb, 32)).astype(np.int64)
    d = _log_uniform(r, 2.0 ** -10, 2.0 ** -4, (m, nb))
    if enc == UNIFORM_BYTES:
        pass
    elif enc == EXTREME_CODES:
        sort = ((np.arange(m)[:, None] + np.arange(nb)[None, :]) % 4)[:, :, None]
        q = np.where(sort == 0, 127, np.where(sort == 1, 0, np.where(sort == 2, -127, q)))
    elif enc == SIGNED:
        sd = np.where(r.random((m, nb)) < 0.5, -1.0, 1.0)
        sd[:, 0], sd[:, 1] = -1.0, 1.0
        d = d * sd
        rows = np.arange(m)
        q[rows, r.integers(0, nb, m), r.integers(0, 32, m)] = -128
    elif enc == D_RANGE:
        d = _zeros_pm(r, _log_uniform(r, F16_TINY, 1.0, (m, nb)))
        d = _ends(r, d)
    else:
        raise ValueError(enc)
    raw = np.concatenate([_f16_bytes(d), q.astype(np.int8).view(np.uint8)], axis=2)
    return raw.reshape(-1)


def _f16(k, m, enc, r):
    if enc == UNIFORM_BYTES:                                   # every finite bit pattern: subnormals .. 65504, both zeros
        bits = r.integers(0, 1 << 16, (m, k)).astype(np.uint16)
        inf = (bits & 0x7C00) == 0x7C00
        bits = np.where(inf, bits & 0xBFFF, bits).astype(np.uint16)      # exponent 31 -> 30
        return bits.view(np.uint8).reshape(-1).copy()
    sign = np.where(r.random((m, k)) < 0.5, -1.0, 1.0)
    if enc == EXTREME_CODES:                                   # near 65504 | subnormal | +0 | -0, in runs of eight along a row
        sort = ((np.arange(k)[None, :] // 8 + np.arange(m)[:, None]) % 4)
        big = r.uniform(60000.0, F16_MAX, (m, k))
        sub = r.integers(1, 1024, (m, k)) * F16_TINY
        w = np.where(sort == 0, big * sign, np.where(sort == 1, sub * sign, np.where(sort == 2, 0.0, -0.0)))
    elif enc == SIGNED:                                        # +a, -a pairs (the row sum cancels) and a -0.0 per row
        a = np.abs(r.standard_normal((m, k // 2))) / np.sqrt(k)
        w = np.stack([a, -a], axis=2).reshape(m, k)
        j = 2 * r.integers(0, k // 2, m)
        w[np.arange(m), j], w[np.arange(m), j + 1] = -0.0, 0.0
    elif enc == D_RANGE:
        w = _zeros_pm(r, _log_uniform(r, F16_TINY, 1.0, (m, k)) * sign)
    else:
        raise ValueError(enc)
    return _f16_bytes(w).reshape(-1)


def _side_values(enc, r, n, lo_hi=(2.0 ** -10, 1.0)):
    """n scale-like f16 fields (min / max / absmax) for the plane formats."""
    sign = np.where(r.random(n) < 0.5, -1.0, 1.0)
    if enc == UNIFORM_BYTES:
        return _log_uniform(r, *lo_hi, n)
    if enc == EXTREME_CODES:
        return r.choice(np.array([TERM_CAP, TERM_CAP / 2, 0.0, 1.0]), n)
    if enc == SIGNED:
        return _log_uniform(r, *lo_hi, n) * sign
    if enc == D_RANGE:
        return _zeros_pm(r, _log_uniform(r, F16_TINY, 1.0, n))
    raise ValueError(enc)


def _plane_codes(enc, r, nblk, per):
    c = r.integers(0, 256, (nblk, per)).astype(np.uint8)
    if enc == EXTREME_CODES:
        sort = (np.arange(nblk) % 3)[:, None]
        c = np.where(sort == 0, 0x00, np.where(sort == 1, 0xFF, c)).astype(np.uint8)
    return c


def _int8(k, m, enc, r):
    nblk = k * m // 128
    codes = _plane_codes(enc, r, nblk, 128)
    mn = _side_values(enc, r, nblk)
    mx = _side_values(enc, r, nblk)
    if enc == UNIFORM_BYTES:
        mn = -mn                                               # min < 0 < max, as a quantiser of centred weights gives
    elif enc == EXTREME_CODES:
        mn = -mn * np.where(np.arange(nblk) % 2 == 0, 1.0, 0.0)          # (-cap, cap), (0, cap), (0, 0), min == max == 0 ...
    elif enc == SIGNED and nblk > 1:
        mn[0], mx[0] = abs(mn[0]) + abs(mx[0]), -abs(mx[0])    # max < min: the format does not forbid it
        mn[1], mx[1] = -abs(mn[1]) - abs(mx[1]), -abs(mx[1])   # both negative
    return np.concatenate([codes.reshape(-1), _f16_bytes(np.stack([mn, mx], axis=1)).reshape(-1)])


def _nf4(k, m, enc, r):
    nblk = k * m // 64
    packed = _plane_codes(enc, r, nblk, 32)
    am = _side_values(enc, r, nblk)
    return np.concatenate([packed.reshape(-1), _f16_bytes(am).reshape(-1)])


def make_blocks(kind, k, m, encoding, seed):
    """Raw bytes of an [M, K] matrix of `kind` in encoding profile `encoding`; deterministic in its arguments."""
    assert k % BLOCK_ELEMS[kind] == 0 and (k * m) % BLOCK_ELEMS[kind] == 0, (kind, k, m)
    r = _rng("blocks", kind, k, m, encoding, seed)
    if kind in ("Q4_K", "Q5_K"):
        raw = _k4(kind, k, m, encoding, r)
    elif kind == "Q6_K":
        raw = _q6k(k, m, encoding, r)
    elif kind == "Q8_0":
        raw = _q80(k, m, encoding, r)
    elif kind == "F16":
        raw = _f16(k, m, encoding, r)
    elif kind == "INT8":
        raw = _int8(k, m, encoding, r)
    elif kind == "NF4":
        raw = _nf4(k, m, encoding, r)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(raw, np.uint8)


# ------------------------------------------------------------------------------------------------ field access, term magnitudes
def _f16_at(b, off):
    return np.ascontiguousarray(b[..., off:off + 2]).view("<f2")[..., 0].astype(np.float64)


def fields(kind, raw, k, m):
    """The decoded FIELDS of a raw matrix (no weights): dict of arrays, for terms_abs and for the profile-content tests."""
    raw = np.asarray(raw, np.uint8)
    if kind in ("Q4_K", "Q5_K"):
        b = raw.reshape(m, k // 256, BLOCK_BYTES[kind])
        sc, mn = unpack_scales_k4(b[:, :, 4:16])
        if kind == "Q4_K":
            qs = b[:, :, 16:144].reshape(m, -1, 4, 32)
            q = np.stack([qs & 0xF, qs >> 4], axis=3).reshape(m, -1, 8, 32)
        else:
            qh, ql = b[:, :, 16:48], b[:, :, 48:176].reshape(m, -1, 4, 32)
            q = np.empty((m, k // 256, 8, 32), np.uint8)
            for j in range(4):
                q[:, :, 2 * j] = (ql[:, :, j] & 0xF) | (((qh >> (2 * j)) & 1) << 4)
                q[:, :, 2 * j + 1] = (ql[:, :, j] >> 4) | (((qh >> (2 * j + 1)) & 1) << 4)
        return {"d": _f16_at(b, 0), "dmin": _f16_at(b, 2), "sc": sc, "m": mn, "q": q}
    if kind == "Q6_K":
        b = raw.reshape(m, k // 256, 210)
        ql, qh = b[:, :, 0:128], b[:, :, 128:192]
        q = np.empty((m, k // 256, 256), np.int64)
        for n in range(2):
            l, h = ql[:, :, 64 * n:64 * n + 64], qh[:, :, 32 * n:32 * n + 32]
            q[:, :, 128 * n + 0:128 * n + 32] = (l[:, :, :32] & 0xF) | ((h & 3) << 4)
            q[:, :, 128 * n + 32:128 * n + 64] = (l[:, :, 32:] & 0xF) | (((h >> 2) & 3) << 4)
            q[:, :, 128 * n + 64:128 * n + 96] = (l[:, :, :32] >> 4) | (((h >> 4) & 3) << 4)
            q[:, :, 128 * n + 96:128 * n + 128] = (l[:, :, 32:] >> 4) | (((h >> 6) & 3) << 4)
        return {"d": _f16_at(b, 208), "sc": b[:, :, 192:208].view(np.int8).astype(np.int64), "q": q}
    if kind == "Q8_0":
        b = raw.reshape(m, k // 32, 34)
        return {"d": _f16_at(b, 0), "q": b[:, :, 2:34].view(np.int8).astype(np.int64)}
    if kind == "F16":
        return {"w": raw.view("<f2").reshape(m, k).astype(np.float64)}
    if kind == "INT8":
        mm = raw[k * m:].view("<f2").reshape(-1, 2).astype(np.float64)
        return {"c": raw[:k * m].reshape(-1, 128), "min": mm[:, 0], "max": mm[:, 1]}
    if kind == "NF4":
        p = raw[:k * m // 2]
        c = np.empty(k * m, np.uint8)
        c[0::2], c[1::2] = p & 0xF, p >> 4
        return {"c": c.reshape(-1, 64), "absmax": raw[k * m // 2:].view("<f2").astype(np.float64)}
    raise ValueError(kind)


def terms_abs(kind, raw, k, m):
    """float64 [M, K]: the sum of the absolute values of the terms of each weight's decode formula.  A kernel may evaluate the terms
    separately (the K-quant min term is factored out as -dmin * m * sum(x)), so its rounding error scales with the parts, not with |w|."""
    f = fields(kind, raw, k, m)
    if kind in ("Q4_K", "Q5_K"):
        main = np.abs(f["d"])[:, :, None, None] * f["sc"].astype(np.float64)[:, :, :, None] * f["q"].astype(np.float64)
        mins = np.abs(f["dmin"])[:, :, None] * f["m"].astype(np.float64)
        return (main + mins[:, :, :, None]).reshape(m, k)
    if kind == "Q6_K":
        sc = np.repeat(f["sc"], 16, axis=2).astype(np.float64)
        return (np.abs(f["d"])[:, :, None] * np.abs(sc) * np.abs(f["q"] - 32)).reshape(m, k)
    if kind == "Q8_0":
        return (np.abs(f["d"])[:, :, None] * np.abs(f["q"])).reshape(m, k)
    if kind == "F16":
        return np.abs(f["w"])
    if kind == "INT8":
        c = f["c"].astype(np.float64) / 255.0
        return (c * (np.abs(f["max"]) + np.abs(f["min"]))[:, None] + np.abs(f["min"])[:, None]).reshape(m, k)
    if kind == "NF4":
        return (np.abs(NF4_LEVELS.astype(np.float64))[f["c"]] * np.abs(f["absmax"])[:, None]).reshape(m, k)
    raise ValueError(kind)


def max_term(kind, raw, k, m):
    """Largest single term of the matrix (what TERM_CAP bounds)."""
    f = fields(kind, raw, k, m)
    if kind in ("Q4_K", "Q5_K"):
        a = (np.abs(f["d"])[:, :, None] * f["sc"] * f["q"].max(axis=3)).max()
        return max(a, (np.abs(f["dmin"])[:, :, None] * f["m"]).max())
    if kind == "INT8":
        return max(np.abs(f["max"]).max(), np.abs(f["min"]).max())
    return terms_abs(kind, raw, k, m).max()


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(profile, shape, seed):
    """float16 activations of `shape` (last axis = K, a multiple of 32); deterministic in its arguments."""
    r = _rng("inputs", profile, tuple(shape), seed)
    shape = tuple(shape)
    n = int(np.prod(shape))
    sign = np.where(r.random(shape) < 0.5, -1.0, 1.0)
    if profile == NORMAL:
        x = r.standard_normal(shape)
    elif profile == LARGE:                         # log-uniform magnitude from the smallest normal f16 to the largest
        x = _log_uniform(r, 2.0 ** -14, F16_MAX, shape) * sign
        x.reshape(-1)[r.integers(0, n)] = F16_MAX
    elif profile == LARGE_SAME_SIGN:               # all in [2048, 65504]: every 32-element sum is beyond f16
        x = _log_uniform(r, 2048.0, F16_MAX, shape)
        x.reshape(-1)[r.integers(0, n)] = F16_MAX
    elif profile == TINY:                          # f16 subnormals (both signs) mixed with exact zeros
        x = r.integers(1, 1024, shape) * F16_TINY * sign
        x = np.where(r.random(shape) < 0.5, 0.0, x)
        x.reshape(-1)[0] = F16_TINY
    elif profile == SPARSE:                        # 90 % exact zeros (some -0.0), the rest relu(k)^2-like positives
        x = np.square(np.maximum(r.standard_normal(shape) * 4.0, 0.0)) + 2.0 ** -10
        z = r.random(shape)
        x = np.where(z < 0.8, 0.0, np.where(z < 0.9, -0.0, x))
    elif profile == CANCELLING:                    # adjacent (+a, -a): 32-element sums are 0 while sum|x| is huge
        a = _log_uniform(r, 2048.0, F16_MAX, shape[:-1] + (shape[-1] // 2,))
        a16 = a.astype(np.float16).astype(np.float64)
        x = np.stack([a16, -a16], axis=-1).reshape(shape)
    else:
        raise ValueError(profile)
    x16 = np.asarray(x, np.float64).astype(np.float16)
    assert np.isfinite(x16).all()
    return x16


# ------------------------------------------------------------------------------------------------ value-preserving re-encodings
def flippable(kind, raw, k, m):
    """A copy of a Q6_K / Q8_0 matrix whose scales (codes) avoid -128, so that `flip` can negate them."""
    raw = np.array(raw, np.uint8)
    if kind == "Q6_K":
        s = raw.reshape(-1, 210)[:, 192:208]
    elif kind == "Q8_0":
        s = raw.reshape(-1, 34)[:, 2:34]
    else:
        raise ValueError(kind)
    s[s == 0x80] = 0x81
    return raw


def flip(kind, raw, k, m):
    """The same weights with the other sign convention: Q6_K with d and every scale negated, Q8_0 with d and every code negated.
    (-d) * (-sc) is the same f32 product as d * sc, so every kernel must return the same bits for both."""
    raw = np.array(raw, np.uint8)
    b = raw.reshape(-1, 210 if kind == "Q6_K" else 34)
    lo, hi, dh = (192, 208, 209) if kind == "Q6_K" else (2, 34, 1)
    s = b[:, lo:hi].view(np.int8)
    assert (s != -128).all()
    b[:, lo:hi] = (-s.astype(np.int16)).astype(np.int8).view(np.uint8)
    b[:, dh] ^= 0x80                                           # sign bit of d
    return raw


def flip_tensor(name, kind, raw):
    """`reencode` hook of oracle/synth.py: every Q6_K / Q8_0 tensor of a model in the other sign convention (quantiser output has no -128)."""
    if kind not in ("Q6_K", "Q8_0"):
        return raw
    a = np.asarray(raw)
    return flip(kind, a.view(np.uint8).reshape(-1), 0, 0).view(a.dtype).reshape(a.shape)
