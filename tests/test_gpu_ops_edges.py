"""Norms, activations, element-wise ops and the WKV kernels of web-rwkv-gguf_amd/csrc/wrk_ops.hip over the whole value range of their
formats, through the C ABI (`wrk.TensorOp.*`), against the float64 references and bounds of tests/ops_ref.py (proved on the CPU by
tests/test_ops_ref.py: float32 restatements stay inside every bound, the bounds are at most 2 f16 ulps on ordinary inputs, and ten
deliberately wrong variants violate them).  No additive floor anywhere: f16 subnormals, +-0 and 65504 are ordinary inputs here.

Which kernel a case runs on follows from its shape, type and view and from the switches that are read per call:

| kernel                                   | selected by                                                              | cases                                         |
|------------------------------------------|--------------------------------------------------------------------------|-----------------------------------------------|
| layer_norm_f16_kernel<8>                 | dense f16, C = 64, 1000 (tail), 2048 (limit)                             | test_layer_norm[64-*] [1000-*] [2048-*]       |
| layer_norm_f16_kernel<16>                | dense f16, C = 2056, 4096 (limit)                                        | test_layer_norm[2056-*] [4096-*]              |
| layer_norm_kernel<256> (generic)         | C = 4104 (> 4096); an f32 tensor; a row slice of a wider buffer          | test_layer_norm[4104-*], test_layer_norm_generic_kernel[f32-*] [strided-*] |
|                                          | (WRK_LN_FAST is read once per process: not used here)                    |                                               |
| layer_norm_kernel<64>, l2_norm_kernel    | group_norm H = 1, 3; l2_norm C = 64                                      | test_group_norm[*], test_l2_norm[*]           |
| binary / lerp / blit / token_shift _v8_kernel | dense f16, C = 256                                                  | [c256-*] of test_binary_lerp_affine_control_k, test_copies_are_bit_exact, test_token_shift; the f16 activation sweep's add / mul routes |
| binary / lerp / blit / token_shift element kernels | C = 250 (C % 8 != 0); a C = 256 view offset by 4 elements (not 16-byte aligned); f32 tensors | [c250-*] [c256_off4-*] of the same tests; test_activation_on_f32_tensors[*] |
| affine_kernel (affine, activate), control_k_kernel, transpose_kernel, channel_mix_v6 / v7_kernel | every layout (one kernel each) | test_binary_lerp_affine_control_k[*], test_activation_on_*[*], test_copies_are_bit_exact[*], test_channel_mix_v6[*] |
| softmax_kernel                           | C = 1000 (four strided passes), 5 (most lanes idle)                      | test_softmax[*]                               |
| time_mix_v7_wave_kernel                  | WRK_WKV_WAVE=1                                                           | test_time_mix_v7[*] ("wave")                  |
| time_mix_v7_fast_kernel<4, false> (quad) | WRK_WKV_WAVE=0 WRK_WKV_OCT=0                                             | test_time_mix_v7[*] ("quad")                  |
| time_mix_v7_fast_kernel<8, false> (oct)  | WRK_WKV_WAVE=0 WRK_WKV_OCT=1                                             | test_time_mix_v7[*] ("oct")                   |
| time_mix_v7_kernel (generic)             | f32 r, w, n, x; f16 r and x as views of [128, H, T] buffers (stride 128) | test_time_mix_v7[*] ("generic_f32", "generic_strided") |
| pre_wkv_v7_kernel, post_wkv_v7_kernel, time_mix_v7_fast_kernel<8, true> on 1 / 2 / 4 workgroups per head, <4, true> | infer_layer, mode 1, 3 tokens of one sequence, `tiny` synthetic model, layers 0 (v0 = v) and 1 (value residual); WRK_WKV_CSPLIT = 1, 2, 4; WRK_WKV_OCT = 0 | test_merged_wkv_stages_equal_the_op_chain[*] |
| time_mix_v6_fast_kernel<4>, <8>, time_mix_v6_wave_kernel, time_mix_v6_kernel | the switches of test_time_mix_v6; generic: the decay as a view of a [128, H, T] buffer | test_time_mix_v6[*] |
| time_first_v7_kernel                     | H = 1, 3                                                                 | test_time_first_v7[*]                         |

profiles/ops_edges_kernel_stats.csv is a rocprofv3 --kernel-trace --stats run of this file and lists every kernel of the table.

Activation bars.  f16 tensors: every finite f16 bit pattern, one step of f16 (true spacing; +-inf is the step after 65504) from the
stage-by-stage value of ops_ref.act_expected.  f32 tensors: relative to the same value where it is a normal f32, bars = twice the worst
measured on MI355X (F32_MEASURED, copied into DESIGN.md), never above 2^-12.

What this file found: DESIGN.md section 2, "Value range (norms, activations, element-wise ops, WKV)".
"""
import functools
import json
import os

import numpy as np
import pytest

import ops_ref as R
import wrk
from oracle import synth

pytestmark = pytest.mark.gpu

WORST = {}          # (family, profile) -> worst error / bound
NOTES = {}          # measurements that go into DESIGN.md


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def judge(case, family, profile, got, want, bound, f16=True):
    if f16:
        ratio, near = R.check16(got, want, bound)
        assert near <= 0.01 * ratio.size, f"{case}: {near} of {ratio.size} elements near the f16 overflow threshold (cap 1 %)"
    else:
        ratio = R.check32(got, want, bound)
    worst = float(ratio.max()) if ratio.size else 0.0
    WORST[(family, profile)] = max(WORST.get((family, profile), 0.0), worst)
    assert worst <= 1.0, f"{case}: worst error / bound = {worst:.4g} ({int((ratio > 1).sum())} of {ratio.size} elements beyond the bound)"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


# ----------------------------------------------------------------------------- norms
def ln_case(profile, shape, tag="ln"):
    C = shape[-1]
    x = R.make(profile, shape, tag)
    w = (1.0 + 0.25 * R.make(R.NORMAL, (C,), "w").astype(np.float64)).astype(np.float16)
    b = (0.05 * R.make(R.NORMAL, (C,), "b").astype(np.float64)).astype(np.float16)
    return x, w, b


@pytest.mark.parametrize("profile", R.PROFILES)
@pytest.mark.parametrize("C", [64, 1000, 2048, 2056, 4096, 4104])
def test_layer_norm(ctx, C, profile):
    for B in (1, 2):
        x, w, b = ln_case(profile, (B, 2, C))
        t = ctx.tensor(x)
        wrk.TensorOp.layer_norm(ctx.buffer(w), ctx.buffer(b), t, 1e-5)
        want, e, _ = R.layer_norm(x, w, b, 1e-5)
        judge(f"layer_norm C={C} B={B} {profile}", "layer_norm", profile, t.back().reshape(x.shape), want, e + R.ulp16(want) / 2)


@pytest.mark.parametrize("profile", R.PROFILES)
@pytest.mark.parametrize("kind", ["f32", "strided"])
def test_layer_norm_generic_kernel(ctx, kind, profile):
    C, T, B = 1000, 2, 2
    x, w, b = ln_case(profile, (B, T, C))
    want, e, terms = R.layer_norm(x, w, b, 1e-5)
    if kind == "f32":
        t = ctx.tensor(x.astype(np.float32))
        wrk.TensorOp.layer_norm(ctx.buffer(w), ctx.buffer(b), t, 1e-5)
        judge(f"layer_norm f32 {profile}", "layer_norm_generic", profile, t.back().reshape(x.shape), want, e + R.rnd32(terms), f16=False)
    else:                       # a row slice of a wider buffer: the rest of the buffer stays as it was
        wide = np.full((B, T, C + 24), 7.0, np.float16)
        wide[..., 8:8 + C] = x
        t = ctx.tensor(wide)
        wrk.TensorOp.layer_norm(ctx.buffer(w), ctx.buffer(b), t.view((8, 8 + C)), 1e-5)
        got = t.back().reshape(wide.shape)
        assert (got[..., :8] == 7.0).all() and (got[..., 8 + C:] == 7.0).all()
        judge(f"layer_norm strided {profile}", "layer_norm_generic", profile, got[..., 8:8 + C], want, e + R.ulp16(want) / 2)


@pytest.mark.parametrize("profile", R.PROFILES)
@pytest.mark.parametrize("H", [1, 3])
def test_group_norm(ctx, H, profile):
    S, T = 64, 2
    x = R.make(profile, (T, H, S), "gn")
    w = (1.0 + 0.25 * R.make(R.NORMAL, (H, S), "w").astype(np.float64)).astype(np.float16)
    b = (0.05 * R.make(R.NORMAL, (H, S), "b").astype(np.float64)).astype(np.float16)
    t = ctx.tensor(x)
    wrk.TensorOp.group_norm(ctx.buffer(w), ctx.buffer(b), t, 64e-5)
    want, e, _ = R.layer_norm(x, w[None], b[None], 64e-5)
    judge(f"group_norm H={H} {profile}", "group_norm", profile, t.back().reshape(x.shape), want, e + R.ulp16(want) / 2)


@pytest.mark.parametrize("profile", R.PROFILES)
def test_l2_norm(ctx, profile):
    x = R.make(profile, (2, 3, 64), "l2")
    t = ctx.tensor(x)
    wrk.TensorOp.l2_norm(t, 1e-12)
    got = t.back().reshape(x.shape)
    want, e, _ = R.l2_norm(x, 1e-12)
    judge(f"l2_norm {profile}", "l2_norm", profile, got, want, e + R.ulp16(want) / 2)
    if profile == R.ZERO_ROW:
        assert not got.astype(np.float32).any()         # exactly 0 (either sign), no NaN


# ----------------------------------------------------------------------------- activations
# f16 bar in f16 steps.  Measured: no activation, sigmoid included, has an element beyond 1 step on any of the seven routes (0 of 7 x 63 488
# each; squared_relu, tanh, opposite_exp and sigmoid are exact throughout), so the 2 that tests/test_gpu_ops.py grants sigmoid is not needed
F16_STEPS = {a: 1 for a in R.ACTS}
# worst |got - expected| / |expected| over the f32 sweep where the expected output is a normal f32, measured on MI355X (ROCm 7, gfx950);
# the test's bar is twice this and never above 2^-12
F32_MEASURED = {"squared_relu": 0.0, "tanh": 1.16e-7, "stable_exp": 2.33e-5, "opposite_exp": 3.80e-6, "softplus": 9.83e-5, "sigmoid": 3.76e-6,
                "silu": 3.77e-6}
F32_CEILING = 2.0 ** -12


def routes(ctx, act, x, dt):
    """the seven ways an activation is reached: `activate`, and the act_x / act_y / act_out slots of add (partner 0) and mul (partner 1)"""
    n = x.size
    dev = lambda a: ctx.tensor(np.ascontiguousarray(a, dt), [n, 1, 1])
    const = lambda c: dev(np.full(n, c))
    t = dev(x)
    wrk.TensorOp.activate(t, act)
    yield "activate", t.back().reshape(n)
    for op, name, unit in ((wrk.TensorOp.add_activate, "add", 0.0), (wrk.TensorOp.mul_activate, "mul", 1.0)):
        out = const(unit)
        op(dev(x), out, act, "none", "none")
        yield f"{name}.act_x", out.back().reshape(n)
        out = dev(x)
        op(const(unit), out, "none", act, "none")
        yield f"{name}.act_y", out.back().reshape(n)
        out = dev(x)
        op(const(unit), out, "none", "none", act)
        yield f"{name}.act_out", out.back().reshape(n)


@pytest.mark.parametrize("act", R.ACTS)
def test_activation_on_every_finite_f16(ctx, act):
    x = R.finite_f16_patterns()
    want = R.ordered16(R.r16(R.act_expected(act, x)))
    worst, beyond = 0, {}
    for route, got in routes(ctx, act, x, np.float16):
        assert not np.isnan(got).any(), f"{act} via {route}: NaN at {x[np.isnan(got)][:8]}"
        steps = np.abs(R.ordered16(got) - want)
        worst = max(worst, int(steps.max()))
        beyond[route] = int((steps > 1).sum())
    NOTES[f"f16_steps/{act}"] = {"worst_steps": worst, "beyond_one": beyond}
    print(f"{act}: worst {worst} f16 steps; elements beyond 1 step per route: {beyond}")
    assert worst <= F16_STEPS[act], f"{act}: {worst} f16 steps; beyond 1: {beyond}"


@pytest.mark.parametrize("act", R.ACTS)
def test_activation_on_f32_tensors(ctx, act):
    x = R.finite_f16_patterns().astype(np.float32)
    want = R.act_expected(act, x)
    normal = np.isfinite(want) & (np.abs(want) >= 2.0 ** -126)
    worst = 0.0
    for route, got in routes(ctx, act, x, np.float32):
        got = got.astype(np.float64)
        assert not np.isnan(got).any(), f"{act} via {route}: NaN"
        assert (np.isinf(got) <= (~np.isfinite(want) | (np.abs(want) > 3e38))).all(), f"{act} via {route}: inf where a finite value is expected"
        rel = np.abs(got[normal] - want[normal]) / np.abs(want[normal])
        worst = max(worst, float(rel.max()))
    NOTES[f"f32_rel/{act}"] = worst
    print(f"{act}: worst relative error on f32 tensors {worst:.3e} (2^-12 = {F32_CEILING:.3e})")
    assert worst <= F32_CEILING, f"{act}: {worst:.3e} relative > 2^-12"
    assert worst <= 2 * F32_MEASURED[act], f"{act}: {worst:.3e} relative, measured {F32_MEASURED[act]:.3e}"


# ----------------------------------------------------------------------------- element-wise ops
LAYOUTS = {"c256": (256, 0), "c250": (250, 0), "c256_off4": (256, 4)}
SHIFT_LENS = [3, 0, 4]


class Dev:
    """a host array [..., C] on the device in one of the LAYOUTS: dense, or a view offset by `off` elements into rows of C + 2 off
    elements (the rest of each row holds 7.0 and must still hold it afterwards).  `.t` is the [C, ...] tensor (axes reversed)."""

    def __init__(self, ctx, a, off):
        a = np.ascontiguousarray(a)
        self.C, self.off, self.shape = a.shape[-1], off, a.shape
        if off:
            wide = np.full(a.shape[:-1] + (self.C + 2 * off,), 7.0, a.dtype)
            wide[..., off:off + self.C] = a
            self.t = ctx.tensor(wide).view((off, off + self.C))
        else:
            self.t = ctx.tensor(a)

    def back(self):
        full = self.t.back()
        full = full.reshape(self.shape[:-1] + (full.shape[-1],))
        if self.off:
            assert (full[..., :self.off] == 7.0).all() and (full[..., self.off + self.C:] == 7.0).all(), "wrote outside its view"
        return full[..., self.off:self.off + self.C]


@pytest.mark.parametrize("profile", R.PROFILES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_binary_lerp_affine_control_k(ctx, layout, profile):
    C, off = LAYOUTS[layout]
    T = 3
    x, y, z = R.make(profile, (T, C), "x"), R.make(profile, (T, C), "y"), R.make(R.NORMAL, (T, C), "z")
    fa, p = R.factors((T, C), profile), R.make(R.NORMAL, (C,), "p")
    D = lambda a: Dev(ctx, a, off)

    def run(name, ref, launch, out_init):
        out = D(out_init)
        launch(out.t)
        want, terms, n = ref
        judge(f"{name} {layout} {profile}", name, profile, out.back(), want, R.bound16(want, terms, n))

    run("add", R.add(x, y), lambda o: wrk.TensorOp.add(D(x).t, o), y)
    run("add_broadcast", R.add(x[:1], y), lambda o: wrk.TensorOp.add(D(x[:1]).t, o), y)
    run("mul", R.mul(x, z), lambda o: wrk.TensorOp.mul(D(x).t, o), z)
    run("lerp", R.mix(x, y, fa), lambda o: wrk.TensorOp.lerp(D(x).t, o, D(fa).t, False), y)
    run("lerp", R.mix(y, x, fa), lambda o: wrk.TensorOp.lerp(D(x).t, o, D(fa).t, True), y)
    run("lerp", R.mix(x, z, fa[:1]), lambda o: wrk.TensorOp.lerp(D(x).t, o, D(fa[:1]).t, False), z)
    run("affine", R.affine(x, 0.5, -3.0), lambda o: wrk.TensorOp.affine(o, 0.5, -3.0), x)
    run("affine", R.affine(x, -1.0, 0.0), lambda o: wrk.TensorOp.affine(o, -1.0, 0.0), x)
    run("control_k_v7", R.control_k(x, fa, p[None]), lambda o: wrk.TensorOp.control_k_v7(ctx.buffer(p), D(fa).t, o), x)


@pytest.mark.parametrize("profile", R.PROFILES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_copies_are_bit_exact(ctx, layout, profile):
    """blit, transpose and the state carries of channel_mix: bit for bit, -0 and subnormals included"""
    C, off = LAYOUTS[layout]
    T, B = 3, 2
    x = R.make(profile, (B, T, C), "copy")
    D = lambda a: Dev(ctx, a, off)
    # blit f16 -> f16 and f16 -> f32 (exact widening)
    out = D(np.zeros((B, T, C), np.float16))
    wrk.TensorOp.blit(D(x).t, out.t)
    assert np.array_equal(bits(out.back()), bits(x))
    out = D(np.zeros((B, T, C), np.float32))
    wrk.TensorOp.blit(D(x).t, out.t)
    assert np.array_equal(bits(out.back()), bits(x.astype(np.float32)))
    # transpose: out[c, b, t] = in[c, t, b]
    out = D(np.zeros((T, B, C), np.float16))
    wrk.TensorOp.transpose(D(x).t, out.t)
    assert np.array_equal(bits(out.back()), bits(x.transpose(1, 0, 2)))
    # channel_mix_v7: state row <- x of each sequence's last token (f32, exact), x <- v
    lens = SHIFT_LENS
    Tn = sum(lens)
    xs, v = R.make(profile, (Tn, C), "cmx"), R.make(profile, (Tn, C), "cmv")
    state = R.make(R.NORMAL, (3, 66, C), "cmst").astype(np.float32)
    cur = ctx.buffer(R.stack_cursors(lens))
    st, xt = ctx.tensor(state), D(xs)
    wrk.TensorOp.channel_mix_v7(cur, st.view(None, 65), D(v).t, xt.t)
    got = st.back().reshape(3, 66, C)
    want = state.copy()
    want[0, 65], want[2, 65] = xs[2].astype(np.float32), xs[6].astype(np.float32)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(xt.back()), bits(v))


@pytest.mark.parametrize("profile", R.PROFILES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_channel_mix_v6(ctx, layout, profile):
    C, off = LAYOUTS[layout]
    lens = SHIFT_LENS
    T = sum(lens)
    r, v, xs = R.make(profile, (T, C), "r6"), R.make(R.NORMAL, (T, C), "v6"), R.make(profile, (T, C), "x6")
    state = R.make(R.NORMAL, (3, 66, C), "st6").astype(np.float32)
    st, xt = ctx.tensor(state), Dev(ctx, xs, off)
    wrk.TensorOp.channel_mix(ctx.buffer(R.stack_cursors(lens)), st.view(None, 65), Dev(ctx, r, off).t, Dev(ctx, v, off).t, xt.t)
    want_st = state.copy()
    want_st[0, 65], want_st[2, 65] = xs[2].astype(np.float32), xs[6].astype(np.float32)
    assert np.array_equal(bits(st.back().reshape(3, 66, C)), bits(want_st))
    want, terms, n = R.channel_mix_v6(r, v)
    judge(f"channel_mix_v6 {layout} {profile}", "channel_mix_v6", profile, xt.back(), want, R.bound16(want, terms, n))


@pytest.mark.parametrize("profile", R.PROFILES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_token_shift(ctx, layout, profile):
    """one factor vector and per-token factors [C, T, 5], both `reversed` values, ragged lens = [3, 0, 4]"""
    C, off = LAYOUTS[layout]
    lens = SHIFT_LENS
    T = sum(lens)
    x = R.make(profile, (T, C), "tsx")
    state = R.make(profile, (3, 66, C), "tsst").astype(np.float32)
    cur = ctx.buffer(R.stack_cursors(lens))
    st = ctx.tensor(state)
    prev = np.empty((T, C), np.float64)
    prev[1:] = x[:-1]
    prev[0], prev[3] = state[0, 0], state[2, 0]
    xin = Dev(ctx, x, off).t
    for I, mu in ((1, R.factors((1, 1, C), profile)), (5, R.factors((5, T, C), profile))):
        mt = Dev(ctx, mu, off).t
        for rev in (True, False):
            out = Dev(ctx, np.zeros((I, T, C), np.float16), off)
            wrk.TensorOp.token_shift(cur, mt, st.view(None, 0), xin, out.t, rev)
            want, terms, n = R.mix(x[None], prev[None], mu) if rev else R.mix(prev[None], x[None], mu)
            judge(f"token_shift I={I} reversed={rev} {layout} {profile}", "token_shift", profile, out.back(), want, R.bound16(want, terms, n))


# ----------------------------------------------------------------------------- softmax
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


@pytest.mark.parametrize("kind", SOFTMAX_ROWS)
@pytest.mark.parametrize("C", [1000, 5])
def test_softmax(ctx, C, kind):
    x = softmax_rows(kind, C)
    t = ctx.tensor(x, [C, 2, 1])
    wrk.TensorOp.softmax(t)
    got = t.back().reshape(2, C)
    want, e = R.softmax(x)
    judge(f"softmax C={C} {kind}", "softmax", kind, got, want, e, f16=False)
    if kind == "neg_inf":
        assert not got[:, ::3].any()


# ----------------------------------------------------------------------------- WKV7
WKV7_KERNELS = {"wave": ("1", "0"), "quad": ("0", "0"), "oct": ("0", "1")}
WKV7_CASES = [(p, o) for p in R.WKV_PROFILES for o in (R.WKV_OPERANDS if p == R.TINY else ("",))]


@functools.lru_cache(maxsize=4)
def wkv7_ref(profile, operand, lens, H):
    d = R.wkv7_inputs(profile, operand, list(lens), H)
    ref = R.wkv7(d["state"][:, :65], d["r"], d["w"], d["k"], d["v"], d["a"], d["kk"], list(lens), H)
    assert np.abs(ref[0]).max() < R.F16_MAX and np.abs(ref[3]).max() < 1e30        # `large` stays inside the formats
    return d, ref


def wkv7_run(ctx, d, lens, H, kind):
    S, B, T = 64, len(lens), sum(lens)
    dt = np.float32 if kind == "generic_f32" else np.float16
    cur = ctx.buffer(R.stack_cursors(lens))
    st = ctx.tensor(d["state"])
    dev = lambda a: ctx.tensor(np.ascontiguousarray(a, dt), [S, H, T])
    if kind == "generic_strided":       # r and x are the first 64 of 128-element rows
        wide = lambda a: ctx.tensor(np.concatenate([a.reshape(T, H, S), np.full((T, H, S), 7.0, dt)], -1), [2 * S, H, T]).view((0, S))
        rt, x = wide(d["r"]), wide(d["x"])
    else:
        rt, x = dev(d["r"]), dev(d["x"])
    n = ctx.tensor(np.stack([d["k"], d["v"], d["a"], d["kk"]]).astype(dt), [S, H, T, 4])
    wrk.TensorOp.time_mix_v7(cur, st.view(None, (0, S + 1)), rt, dev(d["w"]), n, x)
    y = x.back().reshape(T, H, -1)[..., :S].reshape(T, H * S)
    return y, st.back().reshape(B, S + 2, H * S)


def wkv_judge(case, family, profile, d, ref, lens, y, st, y_f16=True):
    want_y, ey, ty, want_st, E = ref
    S = 64
    if y_f16:
        judge(f"{case} y", family, profile, y, want_y, ey + R.ulp16(want_y) / 2)
    else:
        judge(f"{case} y", family, profile, y, want_y, ey + R.rnd32(ty), f16=False)
    judge(f"{case} state", family + ".state", profile, st[:, 1:S + 1], want_st[:, 1:], E[:, 1:], f16=False)
    carry = d["state"][:, 0].copy()
    for b, start, n in R.cursors_of(lens):
        carry[b] = d["x"][start + n - 1].astype(np.float32)
    assert np.array_equal(bits(st[:, 0]), bits(carry)), f"{case}: token-shift carry row"
    assert np.array_equal(bits(st[:, S + 1]), bits(d["state"][:, S + 1])), f"{case}: ffn row touched"
    for b, n in enumerate(lens):
        if n == 0:
            assert np.array_equal(bits(st[b]), bits(d["state"][b])), f"{case}: idle batch {b} touched"


@pytest.mark.parametrize("profile,operand", WKV7_CASES)
@pytest.mark.parametrize("lens,H", [((1,), 1), ((1,), 3), ((3, 0, 2), 1), ((3, 0, 2), 3), ((5,), 1), ((5,), 3)])
def test_time_mix_v7(ctx, lens, H, profile, operand, monkeypatch):
    d, ref = wkv7_ref(profile, operand, lens, H)
    lens = list(lens)
    name = profile + ("/" + operand if operand else "")
    got = {}
    for kern, (wave, octs) in WKV7_KERNELS.items():
        monkeypatch.setenv("WRK_WKV_WAVE", wave)
        monkeypatch.setenv("WRK_WKV_OCT", octs)
        got[kern] = wkv7_run(ctx, d, lens, H, "dense")
    for kern in ("generic_f32", "generic_strided"):
        got[kern] = wkv7_run(ctx, d, lens, H, kern)
    for kern, (y, st) in got.items():
        wkv_judge(f"wkv7 {kern} {lens} H={H} {name}", "wkv7_" + kern, name, d, ref, lens, y, st, y_f16=kern != "generic_f32")
        if profile == "zero_r":
            assert not y.astype(np.float32).any(), f"{kern}: y must be exactly 0"
    (yq, sq), (yw, sw) = got["quad"], got["wave"]
    same = np.array_equal(bits(sq), bits(sw)) and np.array_equal(bits(yq), bits(yw))
    NOTES.setdefault("quad_wave_bits_agree", {}).setdefault(name, True)
    NOTES["quad_wave_bits_agree"][name] &= bool(same)
    if profile != "zero_r":
        # v_fma_mix_f32 on raw f16 operands (wave) against convert-then-fma (quad): the same bits, f16 subnormals and signed zeros included
        assert same, f"quad and wave differ on {name}: state {int((bits(sq) != bits(sw)).sum())}, y {int((bits(yq) != bits(yw)).sum())} elements"
    else:
        assert np.array_equal(sq, sw) and np.array_equal(yq.astype(np.float32), yw.astype(np.float32)), f"quad and wave differ in value on {name}"


# ----------------------------------------------------------------------------- WKV7 merged stages (pre_wkv_v7, post_wkv_v7, WD = true chunk kernels)
@pytest.fixture(scope="module")
def tiny_rt(ctx):
    rt = wrk.Runtime(ctx, wrk.GgufReader(synth.make_v7_gguf(synth.CONFIGS["tiny"], 42)), num_batch=1, weights=wrk.WEIGHTS_INLINE)
    yield rt
    rt.close()


def layer_frames(rt, layer, x, v0, state, cursors, mode, merged_stages):
    """-> the stage outputs of one layer run: w, (k, v, a, kk), the gated WKV output, the state.  The op list updates att_k / att_v / att_a /
    att_kk in place; the merged pre-WKV stage writes the same four values into the planes of att_n only."""
    T, D = x.shape
    rt.state_load(state, 0)
    rt.infer_layer(layer, x, v0 if layer else None, cursors, mode=mode)
    n = rt.frame("att_n", T).reshape(4, T, D)
    out = {"att_w": rt.frame("att_w", T), "att_x": rt.frame("att_x", T), "state": rt.state_back(0)[layer]}
    for i, name in enumerate(("att_k", "att_v", "att_a", "att_kk")):
        out[name] = n[i] if merged_stages else rt.frame(name, T)
        if not merged_stages:
            assert np.array_equal(bits(out[name]), bits(n[i])), f"{name} and its plane of att_n differ in the op list"
    return out


@pytest.mark.parametrize("scale", [2.0 ** -12, 1.0, 2.0 ** 6])
@pytest.mark.parametrize("layer", [0, 1])
def test_merged_wkv_stages_equal_the_op_chain(ctx, tiny_rt, layer, scale, monkeypatch):
    """mode 1 on 3 tokens of one sequence runs pre_wkv_v7 -> time_mix_v7_fast_kernel<*, true> -> post_wkv_v7; mode 0 runs the op list.
    DESIGN.md 4.5 states that the merged stages are bit-identical to the op chain: asserted here on every stored stage output, at three
    input scales, for each WD = true instantiation.  (WRK_MERGE_MASK=115 is mode 1 with only these two stages taken apart again: the
    same comparison with every other launch of the layer shared.)"""
    rt = tiny_rt
    T, D = 3, rt.info.num_emb
    r = R._rng("merged", layer, scale)
    x = (scale * r.standard_normal((T, D))).astype(np.float16)
    v0 = r.standard_normal((T, D)).astype(np.float16)
    state = (0.3 * r.standard_normal(rt.state_back(0).shape)).astype(np.float32)
    cursors = R.stack_cursors([T])
    monkeypatch.setenv("WRK_WKV_WAVE", "0")
    monkeypatch.setenv("WRK_WKV_OCT", "1")
    monkeypatch.setenv("WRK_WKV_CSPLIT", "1")
    ops = layer_frames(rt, layer, x, v0, state, cursors, 0, False)
    assert all(np.isfinite(v.astype(np.float32)).all() for v in ops.values())
    monkeypatch.setenv("WRK_MERGE_MASK", "115")
    apart = layer_frames(rt, layer, x, v0, state, cursors, 1, False)
    monkeypatch.delenv("WRK_MERGE_MASK")
    for octs, cs in (("1", "1"), ("1", "2"), ("1", "4"), ("0", "1")):
        monkeypatch.setenv("WRK_WKV_OCT", octs)
        monkeypatch.setenv("WRK_WKV_CSPLIT", cs)
        merged = layer_frames(rt, layer, x, v0, state, cursors, 1, True)
        for name, want in ops.items():
            if octs == "0" and name in ("att_x", "state"):
                continue        # four threads per column sum in another order than the op list's eight: covered against `apart` below
            assert np.array_equal(bits(merged[name]), bits(want)), \
                f"layer {layer} scale {scale} oct={octs} csplit={cs}: {name} differs from mode 0 in {int((bits(merged[name]) != bits(want)).sum())} elements"
        for name in ("att_w", "att_k", "att_v", "att_a", "att_kk"):
            assert np.array_equal(bits(merged[name]), bits(apart[name])), f"{name} differs from the op chain inside mode 1"
    # four threads per column, decays precomputed (WD = true) against computed in the kernel (the op chain's kernel at the same setting)
    monkeypatch.setenv("WRK_WKV_OCT", "0")
    monkeypatch.setenv("WRK_MERGE_MASK", "115")
    apart4 = layer_frames(rt, layer, x, v0, state, cursors, 1, False)
    monkeypatch.delenv("WRK_MERGE_MASK")
    merged4 = layer_frames(rt, layer, x, v0, state, cursors, 1, True)
    for name in ("att_x", "state"):
        assert np.array_equal(bits(merged4[name]), bits(apart4[name])), f"quad WD kernel: {name} differs"


# ----------------------------------------------------------------------------- WKV6
WKV6_PROFILES = (R.NORMAL, R.TINY, "decay_limits", R.LARGE, R.CANCELLING)


@functools.lru_cache(maxsize=4)
def wkv6_ref(profile, lens, H):
    d = R.wkv6_inputs(profile, list(lens), H)
    ref = R.wkv6(d["state"][:, :65], d["decay"], d["u"], d["k"], d["v"], d["r"], list(lens), H)
    assert np.abs(ref[0]).max() < R.F16_MAX and np.abs(ref[3]).max() < 1e30
    return d, ref


def wkv6_run(ctx, d, lens, H, strided=False):
    S, B, T = 64, len(lens), sum(lens)
    st, x = ctx.tensor(d["state"]), ctx.tensor(d["x"], [S, H, T])
    f = lambda a: ctx.tensor(a, [S, H, T])
    decay = f(d["decay"])
    if strided:
        decay = ctx.tensor(np.concatenate([d["decay"].reshape(T, H, S), np.full((T, H, S), 7.0, np.float32)], -1), [2 * S, H, T]).view((0, S))
    wrk.TensorOp.time_mix_v6(ctx.buffer(R.stack_cursors(lens)), decay, ctx.buffer(d["u"]), st.view(None, (0, S + 1)), f(d["k"]), f(d["v"]), f(d["r"]), x)
    return x.back().reshape(T, H * S), st.back().reshape(B, S + 2, H * S)


@pytest.mark.parametrize("profile", WKV6_PROFILES)
@pytest.mark.parametrize("lens,H", [((1,), 1), ((1,), 3), ((3, 0, 2), 1), ((3, 0, 2), 3), ((5,), 1), ((5,), 3)])
def test_time_mix_v6(ctx, lens, H, profile, monkeypatch):
    d, ref = wkv6_ref(profile, lens, H)
    lens = list(lens)
    got = {}
    for kern, (wave, octs) in WKV7_KERNELS.items():
        monkeypatch.setenv("WRK_WKV_WAVE", wave)
        monkeypatch.setenv("WRK_WKV_OCT", octs)
        got[kern] = wkv6_run(ctx, d, lens, H)
    got["generic_strided"] = wkv6_run(ctx, d, lens, H, strided=True)
    for kern, (y, st) in got.items():
        wkv_judge(f"wkv6 {kern} {lens} H={H} {profile}", "wkv6_" + kern, profile, d, ref, lens, y, st)
    (yq, sq), (yw, sw) = got["quad"], got["wave"]
    assert np.array_equal(bits(sq), bits(sw)) and np.array_equal(bits(yq), bits(yw)), f"quad and wave differ on {profile}"


# ----------------------------------------------------------------------------- time_first_v7
@pytest.mark.parametrize("profile", R.PROFILES)
@pytest.mark.parametrize("H", [1, 3])
def test_time_first_v7(ctx, H, profile):
    T, S = 2, 64
    u, k, r = (R.make(profile if profile != R.LARGE else R.NORMAL, (T, H, S), z) for z in "ukr")
    if profile == R.LARGE:              # one large factor per product (u k r of three large factors has no f16-range result)
        k = R.make(R.LARGE, (T, H, S), "k")
    u = np.ascontiguousarray(np.broadcast_to(u[:1], u.shape))
    v, x = R.make(R.NORMAL, (T, H, S), "v"), R.make(R.NORMAL, (T, H, S), "x")
    n = ctx.tensor(np.stack([k, v, np.zeros_like(k), np.zeros_like(k)]), [S, H, T, 4])
    xt = ctx.tensor(x, [S, H, T])
    wrk.TensorOp.time_first_v7(ctx.buffer(u[0]), ctx.tensor(r, [S, H, T]), n, xt)
    want, e, _ = R.time_first(u, k, r, v, x)
    judge(f"time_first_v7 H={H} {profile}", "time_first_v7", profile, xt.back().reshape(T, H, S), want, e + R.ulp16(want) / 2)


def test_zz_write_worst_ratios():
    """Not a check: prints the worst error / bound per kernel family (with -s) and, where WRK_OPS_EDGES_JSON names a file, writes the
    ratios per family and profile and the activation measurements there, for DESIGN.md."""
    fam = {}
    for (family, profile), v in WORST.items():
        fam.setdefault(family, {})[profile] = v
    out = os.environ.get("WRK_OPS_EDGES_JSON")
    if out:
        with open(out, "w") as f:
            json.dump({"worst_ratio": fam, "notes": NOTES}, f, indent=1, sort_keys=True)
    print(json.dumps({f: max(p.values()) for f, p in fam.items()}, indent=1, sort_keys=True))
