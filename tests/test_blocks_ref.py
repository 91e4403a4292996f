"""CPU checks of tests/blocks_ref.py, the raw-block generator behind tests/test_gpu_matmul_edges.py.

1. The oracle dequantisers (oracle/dequant.py, oracle/wrkquant.py) have only ever seen the output of oracle/quantize.py.  Before they
   serve as the GPU reference on signed scales, -128, zero scales and random scales[12] bytes, they are pinned to an independent scalar
   decoder written here: plain Python loops straight from the format description, a handful of blocks per profile.
2. The generators are deterministic and every profile contains what it promises.
3. Every term of every decoded weight stays <= 2^10 (F16 weights: <= 65504).
4. The bound of the GPU tests, |got - want| <= C * sum|terms||x| with C = 4e-6, is tied to a reference: an f32 accumulation in the C
   oracle's order (16-wide partial sums, then sequential) of exact f16 x f16 products stays within C / 2 of the f64 value on every input
   profile at the largest K used.  (A strictly sequential f32 sum does not: 6e-6 on same-signed inputs at K = 16384.)
"""
import struct

import numpy as np
import pytest

import blocks_ref as br
from oracle import dequant as dq
from oracle import wrkquant as wq

C = 4e-6
SHAPE = {"Q4_K": (1024, 6), "Q5_K": (1024, 6), "Q6_K": (1024, 6), "Q8_0": (256, 6), "F16": (64, 8), "INT8": (256, 4), "NF4": (128, 4)}


def oracle_decode(kind, raw, k, m):
    if kind == "INT8":
        return wq.dequantize_int8(raw[:k * m], raw[k * m:].view(np.float16).reshape(-1, 2)).reshape(m, k)
    if kind == "NF4":
        return wq.dequantize_nf4(raw[:k * m // 2], raw[k * m // 2:].view(np.float16)).reshape(m, k)
    return dq.dequantize(kind, raw, k * m, round_f16=False).reshape(m, k)


# ------------------------------------------------------------------------------------------------ the independent scalar decoder
def _h(b, off):
    return np.float32(struct.unpack_from("<e", bytes(b[off:off + 2]))[0])


def _i8(v):
    return v - 256 if v >= 128 else v


def _scale_min(j, s):
    if j < 4:
        return s[j] & 63, s[j + 4] & 63
    return (s[j + 4] & 0xF) | ((s[j - 4] >> 6) << 4), (s[j + 4] >> 4) | ((s[j] >> 6) << 4)


def scalar_block(kind, b):
    """One block (list of ints) -> list of np.float32 weights; f32 arithmetic in the reference's association."""
    f = np.float32
    out = []
    if kind == "Q8_0":
        d = _h(b, 0)
        return [f(_i8(b[2 + i])) * d for i in range(32)]
    if kind in ("Q4_K", "Q5_K"):
        d, dmin, s = _h(b, 0), _h(b, 2), b[4:16]
        q5 = kind == "Q5_K"
        qh = b[16:48] if q5 else None
        ql = b[48:176] if q5 else b[16:144]
        for j in range(4):                           # 64 elements: low nibbles then high nibbles of 32 bytes
            for half in range(2):
                sc, mn = _scale_min(2 * j + half, s)
                d1, m1 = d * f(sc), dmin * f(mn)
                for l in range(32):
                    q = (ql[32 * j + l] >> (4 * half)) & 0xF
                    if q5 and (qh[l] >> (2 * j + half)) & 1:
                        q += 16
                    out.append(f(d1 * f(q)) - m1)
        return out
    if kind == "Q6_K":
        ql, qh, sc, d = b[0:128], b[128:192], [_i8(v) for v in b[192:208]], _h(b, 208)
        out = [f(0)] * 256
        for n in range(2):
            for l in range(32):
                is_ = l // 16
                h = qh[32 * n + l]
                qs = [(ql[64 * n + l] & 0xF) | ((h & 3) << 4), (ql[64 * n + l + 32] & 0xF) | (((h >> 2) & 3) << 4),
                      (ql[64 * n + l] >> 4) | (((h >> 4) & 3) << 4), (ql[64 * n + l + 32] >> 4) | (((h >> 6) & 3) << 4)]
                for t in range(4):
                    out[128 * n + 32 * t + l] = f(d * f(sc[8 * n + is_ + 2 * t])) * f(qs[t] - 32)
        return out
    raise ValueError(kind)


def scalar_decode(kind, raw, k, m, rows):
    """Rows `rows` of the matrix, element by element."""
    f = np.float32
    raw = [int(v) for v in raw]
    got = []
    for i in rows:
        row = []
        if kind == "F16":
            row = [_h(raw, 2 * (i * k + e)) for e in range(k)]
        elif kind == "INT8":
            for e in range(i * k, (i + 1) * k):
                blk = e // 128
                mn, mx = _h(raw, k * m + 4 * blk), _h(raw, k * m + 4 * blk + 2)
                row.append(f(f(raw[e]) / f(255.0)) * f(mx - mn) + mn)
        elif kind == "NF4":
            for e in range(i * k, (i + 1) * k):
                c = (raw[e // 2] >> (4 * (e & 1))) & 0xF
                row.append(br.NF4_LEVELS[c] * _h(raw, k * m // 2 + 2 * (e // 64)))
        else:
            bb, be = br.BLOCK_BYTES[kind], br.BLOCK_ELEMS[kind]
            for blk in range(k // be):
                o = (i * (k // be) + blk) * bb
                row += scalar_block(kind, raw[o:o + bb])
        got.append(row)
    return np.array(got, np.float32)


@pytest.mark.parametrize("enc", br.ENCODINGS)
@pytest.mark.parametrize("kind", br.KINDS)
def test_oracle_dequantisers_match_scalar_decoder(kind, enc):
    k, m = SHAPE[kind]
    raw = br.make_blocks(kind, k, m, enc, 5)
    want = scalar_decode(kind, raw, k, m, range(m))
    got = oracle_decode(kind, raw, k, m)
    assert np.isfinite(got).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()       # same f32 bits, signs of zero included


def test_scale_packing_round_trip():
    r = np.random.default_rng(0)
    sc, mn = r.integers(0, 64, (50, 8)).astype(np.uint8), r.integers(0, 64, (50, 8)).astype(np.uint8)
    packed = br.pack_scales_k4(sc, mn)
    s2, m2 = br.unpack_scales_k4(packed)
    assert np.array_equal(sc, s2) and np.array_equal(mn, m2)
    for row, a, b in zip(packed.tolist(), sc, mn):                   # and the scalar decoder reads the same twelve bytes
        assert [_scale_min(j, row) for j in range(8)] == [(int(x), int(y)) for x, y in zip(a, b)]
    o1, o2 = dq.get_scale_min_k4(packed)
    assert np.array_equal(o1, sc) and np.array_equal(o2, mn)


# ------------------------------------------------------------------------------------------------ determinism, content, cap
@pytest.mark.parametrize("kind", br.KINDS)
def test_generators_are_deterministic(kind):
    k, m = SHAPE[kind]
    for enc in br.ENCODINGS:
        a, b = br.make_blocks(kind, k, m, enc, 1), br.make_blocks(kind, k, m, enc, 1)
        assert a.dtype == np.uint8 and np.array_equal(a, b)
        assert not np.array_equal(a, br.make_blocks(kind, k, m, enc, 2))
    for prof in br.INPUTS:
        a, b = br.make_inputs(prof, (3, k), 1), br.make_inputs(prof, (3, k), 1)
        assert a.dtype == np.float16 and np.array_equal(a.view(np.uint16), b.view(np.uint16))


def _neg_zero(v):
    return (np.asarray(v) == 0) & np.signbit(v)


def _pos_zero(v):
    return (np.asarray(v) == 0) & ~np.signbit(v)


@pytest.mark.parametrize("kind", ["Q4_K", "Q5_K"])
def test_k4_profiles_hold_what_they_promise(kind):
    k, m = 2048, 12
    qmax = 31 if kind == "Q5_K" else 15
    f = br.fields(kind, br.make_blocks(kind, k, m, br.UNIFORM_BYTES, 3), k, m)
    assert (f["d"] > 0).all() and (f["dmin"] > 0).all()
    for name in ("sc", "m"):
        assert set(np.unique(f[name])) == set(range(64))                # 6-bit packing of sub-blocks 4..7 over all its values
        assert set(np.unique(f[name][:, :, 4:])) == set(range(64))
    assert set(np.unique(f["q"])) == set(range(qmax + 1))
    f = br.fields(kind, br.make_blocks(kind, k, m, br.EXTREME_CODES, 3), k, m)
    q, sc, mn = f["q"].reshape(m, -1, 256), f["sc"], f["m"]
    for i in range(m):                                                  # per ROW
        allmax, allzero = (q[i] == qmax).all(axis=1), (q[i] == 0).all(axis=1)
        assert allmax.any() and allzero.any()
        assert ((sc[i] == 63).all(axis=1) & (mn[i] == 63).all(axis=1)).any()
        assert ((sc[i] == 0).all(axis=1) & (mn[i] != 0).all(axis=1)).any()
        assert ((mn[i] == 0).all(axis=1) & (sc[i] != 0).all(axis=1)).any()
    f = br.fields(kind, br.make_blocks(kind, k, m, br.SIGNED, 3), k, m)
    for i in range(m):
        assert (f["d"][i] < 0).any() and (f["d"][i] > 0).any() and (f["dmin"][i] < 0).any() and (f["dmin"][i] > 0).any()
    f = br.fields(kind, br.make_blocks(kind, k, m, br.D_RANGE, 3), k, m)
    for name in ("d", "dmin"):
        v = f[name]
        assert _neg_zero(v).any() and _pos_zero(v).any()
        nz = np.abs(v[v != 0])
        assert nz.min() == 2.0 ** -24 and nz.max() == 1.0 and (nz < 2.0 ** -14).sum() >= 5          # subnormal d


def test_q6k_profiles_hold_what_they_promise():
    kind, k, m = "Q6_K", 2048, 12
    f = br.fields(kind, br.make_blocks(kind, k, m, br.UNIFORM_BYTES, 3), k, m)
    assert (f["d"] > 0).all() and f["sc"].min() == -128 and f["sc"].max() == 127 and set(np.unique(f["q"])) == set(range(64))
    f = br.fields(kind, br.make_blocks(kind, k, m, br.EXTREME_CODES, 3), k, m)
    for i in range(m):
        assert (f["q"][i] == 63).all(axis=1).any() and (f["q"][i] == 0).all(axis=1).any()
        assert (f["sc"][i] == 127).all(axis=1).any() and (f["sc"][i] == 0).all(axis=1).any()
    f = br.fields(kind, br.make_blocks(kind, k, m, br.SIGNED, 3), k, m)
    for i in range(m):
        assert (f["sc"][i] == -128).any() and (f["sc"][i] == 127).any() and (f["d"][i] < 0).any() and (f["d"][i] > 0).any()
    f = br.fields(kind, br.make_blocks(kind, k, m, br.D_RANGE, 3), k, m)
    assert _neg_zero(f["d"]).any() and _pos_zero(f["d"]).any() and np.abs(f["d"][f["d"] != 0]).min() == 2.0 ** -24 and f["d"].max() == 1.0


def test_q80_profiles_hold_what_they_promise():
    kind, k, m = "Q8_0", 512, 12
    f = br.fields(kind, br.make_blocks(kind, k, m, br.UNIFORM_BYTES, 3), k, m)
    assert (f["d"] > 0).all() and f["q"].min() == -128 and f["q"].max() == 127
    f = br.fields(kind, br.make_blocks(kind, k, m, br.EXTREME_CODES, 3), k, m)
    for i in range(m):
        assert (f["q"][i] == 127).all(axis=1).any() and (f["q"][i] == 0).all(axis=1).any() and (f["q"][i] == -127).all(axis=1).any()
    f = br.fields(kind, br.make_blocks(kind, k, m, br.SIGNED, 3), k, m)
    for i in range(m):
        assert (f["q"][i] == -128).any() and (f["d"][i] < 0).any() and (f["d"][i] > 0).any()
    f = br.fields(kind, br.make_blocks(kind, k, m, br.D_RANGE, 3), k, m)
    assert _neg_zero(f["d"]).any() and _pos_zero(f["d"]).any() and np.abs(f["d"][f["d"] != 0]).min() == 2.0 ** -24 and f["d"].max() == 1.0


def test_f16_and_plane_profiles_hold_what_they_promise():
    k, m = 256, 8
    w = br.fields("F16", br.make_blocks("F16", k, m, br.EXTREME_CODES, 3), k, m)["w"]
    a = np.abs(w)
    assert np.isfinite(w).all() and a.max() > 60000 and ((a > 0) & (a < 2.0 ** -14)).any() and _neg_zero(w).any() and _pos_zero(w).any()
    w = br.fields("F16", br.make_blocks("F16", k, m, br.UNIFORM_BYTES, 3), k, m)["w"]
    assert np.isfinite(w).all() and np.abs(w).max() > 2.0 ** 14 and ((np.abs(w) > 0) & (np.abs(w) < 2.0 ** -14)).any()
    w = br.fields("F16", br.make_blocks("F16", k, m, br.SIGNED, 3), k, m)["w"]
    assert np.all(w.sum(axis=1) == 0) and _neg_zero(w).any()
    w = br.fields("F16", br.make_blocks("F16", k, m, br.D_RANGE, 3), k, m)["w"]
    assert _neg_zero(w).any() and ((np.abs(w) > 0) & (np.abs(w) < 2.0 ** -14)).any()
    f = br.fields("INT8", br.make_blocks("INT8", k, m, br.EXTREME_CODES, 3), k, m)
    assert (f["c"] == 0).all(axis=1).any() and (f["c"] == 255).all(axis=1).any() and f["max"].max() == br.TERM_CAP and f["min"].min() == -br.TERM_CAP
    assert ((f["min"] == 0) & (f["max"] == 0)).any()
    f = br.fields("INT8", br.make_blocks("INT8", k, m, br.SIGNED, 3), k, m)
    assert (f["max"] < f["min"]).any() and ((f["max"] < 0) & (f["min"] < 0)).any()
    f = br.fields("INT8", br.make_blocks("INT8", k, m, br.D_RANGE, 3), k, m)
    assert _neg_zero(f["min"]).any() and ((np.abs(f["max"]) > 0) & (np.abs(f["max"]) < 2.0 ** -14)).any()
    f = br.fields("NF4", br.make_blocks("NF4", k, m, br.EXTREME_CODES, 3), k, m)
    assert (f["c"] == 0).all(axis=1).any() and (f["c"] == 15).all(axis=1).any() and f["absmax"].max() == br.TERM_CAP and (f["absmax"] == 0).any()
    f = br.fields("NF4", br.make_blocks("NF4", k, m, br.SIGNED, 3), k, m)
    assert (f["absmax"] < 0).any() and (f["absmax"] > 0).any()
    f = br.fields("NF4", br.make_blocks("NF4", k, m, br.D_RANGE, 3), k, m)
    assert _neg_zero(f["absmax"]).any() and ((f["absmax"] > 0) & (f["absmax"] < 2.0 ** -14)).any()


def test_input_profiles_hold_what_they_promise():
    shape = (5, 2048)
    x = {p: br.make_inputs(p, shape, 4).astype(np.float64) for p in br.INPUTS}
    sums = {p: v.reshape(5, -1, 32).sum(axis=2) for p, v in x.items()}
    assert np.abs(x[br.LARGE]).max() == 65504 and np.abs(x[br.LARGE]).min() < 1e-3 and (x[br.LARGE] < 0).any() and (x[br.LARGE] > 0).any()
    assert x[br.LARGE_SAME_SIGN].min() >= 2048 and x[br.LARGE_SAME_SIGN].max() == 65504 and sums[br.LARGE_SAME_SIGN].min() > 65504
    t = x[br.TINY]
    assert np.abs(t).max() < 2.0 ** -14 and (t == 0).mean() > 0.3 and ((t != 0).mean() > 0.3) and (t < 0).any() and np.abs(t[t != 0]).min() == 2.0 ** -24
    s = x[br.SPARSE]
    assert 0.85 < (s == 0).mean() < 0.95 and _neg_zero(s).any() and _pos_zero(s).any() and (s >= 0).all() and s.max() > 16
    c = x[br.CANCELLING]
    assert np.all(sums[br.CANCELLING] == 0) and np.abs(c).min() >= 2048 and np.abs(c).reshape(5, -1, 32).sum(axis=2).min() > 65504
    assert np.array_equal(c[:, 0::2], -c[:, 1::2])


@pytest.mark.parametrize("enc", br.ENCODINGS)
@pytest.mark.parametrize("kind", br.KINDS)
def test_term_cap(kind, enc):
    k, m = (2048, 24) if br.BLOCK_ELEMS[kind] == 256 else (512, 24)
    for seed in (0, 1):
        raw = br.make_blocks(kind, k, m, enc, seed)
        cap = br.F16_MAX if kind == "F16" else br.TERM_CAP
        assert br.max_term(kind, raw, k, m) <= cap
        w = oracle_decode(kind, raw, k, m).astype(np.float64)
        t = br.terms_abs(kind, raw, k, m)
        assert np.isfinite(w).all() and np.all(np.abs(w) <= t * (1 + 1e-6) + 1e-30)        # |w| <= sum of its terms
        if kind in ("Q6_K", "Q8_0", "F16", "NF4"):
            assert np.allclose(np.abs(w), t, rtol=1e-6, atol=0)                               # one term: the same thing


# ------------------------------------------------------------------------------------------------ what C is checked against
def blocked_f32_dot(w, x):
    """f32 accumulation of exact f16 x f16 products in the C oracle's order: sixteen interleaved partial sums, then a sequential sum."""
    p = (w.astype(np.float32) * x.astype(np.float32)).reshape(-1, 16)           # f16 x f16 is exact in f32
    acc = np.zeros(16, np.float32)
    for row in p:
        acc = acc + row
    s = np.float32(0)
    for v in acc:
        s = np.float32(s + v)
    return s


@pytest.mark.parametrize("profile", br.INPUTS)
def test_blocked_f32_reference_is_within_half_the_bound(profile):
    k = 16384                                                                    # the largest K of tests/test_gpu_matmul_edges.py
    worst = 0.0
    for draw in range(20):
        x = br.make_inputs(profile, (k,), draw)
        w = (np.random.default_rng(draw).standard_normal(k) / np.sqrt(k)).astype(np.float16) if draw % 2 else \
            np.abs(np.random.default_rng(draw).standard_normal(k) / np.sqrt(k)).astype(np.float16)
        want = float(w.astype(np.float64) @ x.astype(np.float64))
        denom = float(np.abs(w).astype(np.float64) @ np.abs(x).astype(np.float64))
        worst = max(worst, abs(float(blocked_f32_dot(w, x)) - want) / denom)
    print(f"{profile}: blocked f32 reference, worst of 20 draws: {worst:.3e} of sum|w||x|")
    assert worst <= C / 2


@pytest.mark.parametrize("kind", ["Q6_K", "Q8_0"])
def test_sign_flip_keeps_every_weight(kind):
    k, m = SHAPE[kind]
    a = br.flippable(kind, br.make_blocks(kind, k, m, br.UNIFORM_BYTES, 9), k, m)
    b = br.flip(kind, a, k, m)
    assert not np.array_equal(a, b)
    fa, fb = br.fields(kind, a, k, m), br.fields(kind, b, k, m)
    assert np.array_equal(fa["d"], -fb["d"]) and np.array_equal(fa["sc" if kind == "Q6_K" else "q"], -fb["sc" if kind == "Q6_K" else "q"])
    wa, wb = oracle_decode(kind, a, k, m), oracle_decode(kind, b, k, m)
    nz = wa != 0                                               # (a zero weight may change the sign of its zero: 0 * d)
    assert np.array_equal(wa[nz].view(np.uint32), wb[nz].view(np.uint32)) and np.all(wb[~nz] == 0)
