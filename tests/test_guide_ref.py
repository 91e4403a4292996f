"""Classifier-free guidance, the restatement (tests/guide_ref.py) held to the contract of DESIGN.md §7r: the table of cases by bit pattern,
the three roundings of the finite case, the identity at scale 1, the agreement with the log-softmax formula of Hugging Face and
llama.cpp under a softmax, the mutants that the rows of tests/test_gpu_guide.py must tell apart, and the ABI."""
import os
import re
from fractions import Fraction

import numpy as np

import guide_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def f32(word):
    return np.array([word], np.uint32).view(np.float32)


# ----------------------------------------------------------------------------- the contract
def test_the_hand_worked_table():
    seen = set()
    for cb, ub, want in GR.HAND:
        for s, w in want.items():
            assert bits(GR.mix(f32(cb), f32(ub), s))[0] == w, (hex(cb), hex(ub), s)
        assert bits(GR.mix(f32(cb), f32(ub), 1.0))[0] == cb, "s == 1 comes first"
        seen |= set(want)
    assert seen == set(GR.SCALES) - {1.0}
    # the order of the cases, spelled out: c == -inf beats u == +inf at any scale, u == -inf beats s == 0, s == 0 beats u == +inf
    assert GR.mix([-INF], [INF], 0.5)[0] == -INF and GR.mix([-INF], [INF], 0.0)[0] == -INF
    assert GR.mix([2.0], [-INF], 0.0)[0] == 2.0
    assert GR.mix([2.0], [INF], 0.0)[0] == INF and GR.mix([2.0], [INF], 1.0000001)[0] == -INF and GR.mix([2.0], [INF], 0.99999994)[0] == INF


def round_once(exact):
    """The f32 nearest to a rational, found among the neighbours of its f64 rounding; a tie would need the even rule and is refused."""
    near = int(bits(np.float32(float(exact)))[0])
    dist = sorted((abs(Fraction(float(f32(near + k)[0])) - exact), near + k) for k in (-2, -1, 0, 1, 2))
    assert dist[0][0] < dist[1][0], "a tie"
    return dist[0][1]


def test_the_finite_case_is_three_roundings_not_a_fused_multiply_add():
    for s, cb, ub, want, fused in GR.FMA_CASES:
        c, u = f32(cb), f32(ub)
        d = np.float32(c[0] - u[0])
        assert bits(np.float32(np.float32(np.float32(s) * d) + u[0])) == want == bits(GR.mix(c, u, s))[0]
        # the fused result: the exact s d + u rounded once
        assert round_once(Fraction(float(s)) * Fraction(float(d)) + Fraction(float(u[0]))) == fused != want, s


def test_scale_one_is_a_bit_identity():
    rng = np.random.default_rng(1)
    words = np.array([0x7FC00000, 0x7FC01234, 0xFFC00001, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 1, 0x807FFFFF], np.uint32)
    c = rng.choice(words, 200).view(np.float32)
    u = rng.choice(words, 200).view(np.float32)
    assert np.array_equal(bits(GR.mix(c, u, 1.0)), bits(c))
    # ... and only there: the next scale on either side normalises the row
    for s in (np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0))):
        out = GR.mix(c, u, s)
        assert not np.isnan(out).any() and not (bits(out) == 0x80000000).any()


def test_no_nan_outside_scale_one():
    rng = np.random.default_rng(2)
    words = np.array([0x7FC00000, 0xFFC00001, 0x80000000, 0, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 1, 0x3F800000, 0xC0400000], np.uint32)
    c, u = np.meshgrid(words.view(np.float32), words.view(np.float32))
    for s in (0.0, 1e-30, 0.5, 1.0000001, 1.5, 7.5, 3e38):
        assert not np.isnan(GR.mix(c.ravel(), u.ravel(), s)).any(), s


def softmax64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max())
    return e / e.sum()


def test_softmax_of_the_mix_is_softmax_of_the_log_softmax_formula():
    """Why there is no log-sum-exp pass: lu + s (lc - lu) with log-softmaxed rows is the raw mix minus s LSE(c) + (1 - s) LSE(u), one
    constant per row, and a softmax (as the arg-max, bias, penalties, DRY and the mask) does not see a row constant.  The bound: the
    mix makes three f32 roundings on values of magnitude at most M = (1 + s) (max |c| + max |u|), so each logit is within 3 * 2^-24 M of
    the exact one, and a softmax probability moves by a factor of at most exp(2 * that)."""
    rng = np.random.default_rng(3)
    for s in (0.5, 1.5, 3.0, 7.5):
        c = rng.normal(0, 3, 512).astype(np.float32)
        u = rng.normal(0, 3, 512).astype(np.float32)
        lc = np.log(softmax64(c))
        lu = np.log(softmax64(u))
        want = softmax64(lu + s * (lc - lu))
        got = softmax64(GR.mix(c, u, s))
        M = (1 + s) * (np.abs(c).max() + np.abs(u).max())
        rel = np.expm1(2 * 3 * 2.0 ** -24 * M) + 1e-12
        assert np.all(np.abs(got - want) <= rel * want), s
        assert int(got.argmax()) == int(want.argmax())


# ----------------------------------------------------------------------------- mutants that the rows of the GPU test must reject
def m_swapped(c, u, s):
    return GR.mix(u, c, s)


def m_u_minus_c(c, u, s):
    out = GR.mix(c, u, s)
    cn, un = GR.row_norm(c), GR.row_norm(u)
    fin = np.isfinite(cn) & np.isfinite(un)
    with np.errstate(over="ignore", invalid="ignore"):
        wrong = ((np.float32(s) * (un - cn).astype(np.float32)).astype(np.float32) + un).astype(np.float32)
    return out if np.float32(s) in (np.float32(0), np.float32(1)) else np.where(fin, wrong, out).astype(np.float32)


def m_fused(c, u, s):
    out = GR.mix(c, u, s)
    cn, un = GR.row_norm(c), GR.row_norm(u)
    fin = np.isfinite(cn) & np.isfinite(un)
    with np.errstate(over="ignore", invalid="ignore"):
        d = (cn - un).astype(np.float32).astype(np.float64)
        # s d is exact in f64 (24 x 24 bits); the sum is rounded to f64 and then to f32, a fused multiply-add up to double rounding
        wrong = (np.float64(np.float32(s)) * d + un.astype(np.float64)).astype(np.float32)
    return out if np.float32(s) in (np.float32(0), np.float32(1)) else np.where(fin & np.isfinite(d), wrong, out).astype(np.float32)


def m_no_identity(c, u, s):
    return GR.mix(c, u, s) if np.float32(s) != 1 else GR.mix(c, u, np.nextafter(np.float32(1), np.float32(2)))


def m_no_neg_inf_case(c, u, s):
    out = GR.mix(c, u, s)
    if np.float32(s) == 1:
        return out
    cn, un = GR.row_norm(c), GR.row_norm(u)
    hit = (cn == -INF) & (un != -INF)
    # without the case a row of s == 0 gives u, one with u == +inf the sign rule, and a finite u gives -inf - u = -inf all the same
    wrong = np.where(np.float32(s) == 0, un, np.where(un == INF, -INF if np.float32(s) > 1 else INF, -INF))
    return np.where(hit, wrong, out).astype(np.float32)


def m_no_zero_case(c, u, s):
    if np.float32(s) != 0:
        return GR.mix(c, u, s)
    cn, un = GR.row_norm(c), GR.row_norm(u)
    with np.errstate(over="ignore", invalid="ignore"):
        wrong = ((np.float32(0) * (cn - un).astype(np.float32)).astype(np.float32) + un).astype(np.float32)    # 0 * inf: NaN
    out = np.where(un == INF, INF, wrong)
    out = np.where(un == -INF, cn, out)
    return np.where(np.isinf(cn), cn, out).astype(np.float32)


MUTANTS = [m_swapped, m_u_minus_c, m_fused, m_no_identity, m_no_neg_inf_case, m_no_zero_case]


def test_mutants_are_rejected_by_the_rows_of_the_gpu_test():
    """One call of tests/test_gpu_guide.py's row-function test, rebuilt here at a small V: five guided rows with GR.SCALES on
    GR.special_pairs.  Every mutant differs from mix in at least one bit of that call, so a kernel that equals a mutant fails there."""
    import test_gpu_grammar as TG
    V = 50
    a = GR.special_pairs(TG.special_rows, np.random.default_rng(V), 5, V, V)
    want = [GR.mix(a[r], a[5 + r], s) for r, s in enumerate(GR.SCALES)]
    for m in MUTANTS:
        got = [m(a[r], a[5 + r], s) for r, s in enumerate(GR.SCALES)]
        assert any(not np.array_equal(bits(g), bits(w)) for g, w in zip(got, want)), m.__name__
    # and each for its own reason, on the hand-worked pairs alone
    hc, hu = GR.hand_rows(GR.HAND_LEN)
    assert not np.array_equal(bits(m_fused(hc, hu, 1.5)), bits(GR.mix(hc, hu, 1.5)))
    assert not np.array_equal(bits(m_no_identity(hc, hu, 1.0)), bits(GR.mix(hc, hu, 1.0)))
    assert not np.array_equal(bits(m_no_neg_inf_case(hc, hu, 0.5)), bits(GR.mix(hc, hu, 0.5)))
    assert not np.array_equal(bits(m_no_zero_case(hc, hu, 0.0)), bits(GR.mix(hc, hu, 0.0)))


# ----------------------------------------------------------------------------- validation
def test_check_scale():
    assert GR.check_scale([0.0, 1.0, 7.5, 3e38]) == "ok" and GR.check_scale([]) == "ok"
    for bad in ([-1e-45], [np.nan], [np.inf], [-np.inf], [1.0, -0.5], None):
        assert GR.check_scale(bad) == "arg", bad
    assert GR.check_scale([-0.0]) == "ok"                                       # -0 >= 0
    assert GR.check_vocab(2 ** 20) == "ok" and GR.check_vocab(2 ** 20 + 1) == "unsupported"


# ----------------------------------------------------------------------------- the ABI
def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wrk_hip.h")).read(), flags=re.S)


def fields(cname):
    body = re.search(r"typedef\s+struct\s+" + cname + r"\s*\{(.*?)\}", header(), flags=re.S).group(1)
    return [n for stmt in body.split(";") if stmt.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", stmt.strip())]


def test_the_header_declares_the_row_function_and_the_option_fields():
    import wrk
    text = header()
    assert re.search(r"int32_t\s+wrk_guide_logits\s*\(\s*wrk_ctx\s*\*\s*ctx,\s*const\s+wrk_buf\s*\*\s*logits,\s*uint32_t\s+num_vocab,\s*uint32_t\s+row_stride,"
                     r"\s*uint32_t\s+num_rows,\s*const\s+float\s*\*\s*scale,\s*wrk_buf\s*\*\s*out,\s*uint32_t\s+out_stride\s*\)", text)
    assert hasattr(wrk.hip, "wrk_guide_logits") and len(wrk.HIP_SYMBOLS["wrk_guide_logits"][1]) == 8
    names = fields("wrk_generate_options")
    assert names == [n for n, _ in wrk.GenerateOptions._fields_]
    at = names.index("bias_set")
    # directly behind the bias fields, which stay directly behind `occ`; every field behind them keeps its order
    assert names[at - 2:at + 4] == ["occ", "bias", "bias_set", "guidance_scale", "guidance_first_tokens", "stop_tokens"]
    assert re.search(r"const\s+float\s*\*\s*guidance_scale\s*;\s*const\s+uint32_t\s*\*\s*guidance_first_tokens\s*;", text)
    f = dict(wrk.GenerateOptions._fields_)
    assert f["guidance_scale"] is wrk._f32p and f["guidance_first_tokens"] is wrk._u32p
    assert not wrk.GenerateOptions().guidance_scale and not wrk.GenerateOptions().guidance_first_tokens       # NULL in a zeroed struct: off
    # the queue only carries the scale, to refuse it
    names = fields("wrk_queue_options")
    assert names == [n for n, _ in wrk.QueueOptions._fields_]
    at = names.index("bias_set")
    assert names[at + 1:at + 3] == ["guidance_scale", "init_state"] and "guidance_first_tokens" not in names
    assert callable(wrk.Context.guide_logits)
    code = wrk.Runtime.generate_guided.__code__
    stop_code = wrk.Runtime.generate_stop.__code__
    mine = set(code.co_varnames[:code.co_argcount])
    assert {"guidance_scale", "negative_first_tokens", "stop"} <= mine
    assert set(stop_code.co_varnames[:stop_code.co_argcount]) - {"groups"} <= mine, "every pick argument of generate_stop"
