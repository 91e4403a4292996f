"""RWKV-6, layer by layer: what tests/test_v6_layer_ref.py (CPU) and tests/test_gpu_v6_layer_parity.py (GPU) share.  NumPy only.

  * CASES ........ the fixtures and shapes of the GPU file, one entry per (fixture, chunk lengths); the CPU file runs the reference
                   through every one of them before the GPU sees the bars.
  * replay ....... the oracle's whole-model run of a case: warm-up, then per step the pre-token state, the trace and the end state.
  * RefRuntime ... oracle/rwkv6.py's layer restated with two switches: the summation ORDER of its matmuls (the GPU's order is neither
                   NumPy's nor these two: the bars must hold for any order) and one deliberate MUTANT (a wrong layer the bars must catch).
                   With both switches off it is the oracle bit for bit (test_restatement_is_the_oracle).
  * grade ........ teacher-forced comparison of one layer's buffers and state at the fixed bars of tests/layer_parity.py.
"""
import numpy as np

from layer_parity import DIRECT_MAX_ULP, DOWNSTREAM_FRAC_LE1, DOWNSTREAM_MAX_ULP, STATE_REL, check, ulps
from oracle import gguf as ogguf
from oracle import rwkv6 as O6
from oracle import synth
from oracle.rwkv7 import ACT, GN_EPS, LN_EPS, layer_norm, mix, r16, sigmoid

RANK_SHAPE = lambda R, W: synth.V6Config(2, 256, 1024, 512, 64, R, W)          # noqa: E731
RANKS = [(8, 8), (40, 72), (96, 104), (128, 128)]       # time_mix rank R, time_decay rank W: the masked 8-wide loads of v6_mix / v6_head
RANK_FALLBACK = (136, 64)                               # R > 128: the fused layer declines

# id -> (config name or V6Config, make_v6_gguf keywords, weights rounded to f16?, chunk lengths, modes, steps, WRK_GEMM_KS, warm-up tokens)
CASES = {}


def _case(cid, cfg, kw, f16, lens, modes, steps, ks=None, warm=8):
    CASES[cid] = dict(cfg=cfg, kw=kw, f16=f16, lens=lens, modes=modes, steps=steps, ks=ks, warm=warm)


# decode [1], 4 steps: the basic fused and op-list layers; small = 7 layers: layer 6 (index 5, halved output) and layer 7 (index 6,
# discounted w_o / ffn value), each in isolation
_case("decode-tiny-q5k", "tiny", {}, False, [1], (0, 1), 4)
_case("decode-tiny-q8_0-f16head", "tiny", {"mat": "Q8_0", "head": "F16"}, False, [1], (0, 1), 4)
_case("decode-tiny-inline-f16", "tiny", {}, True, [1], (0, 1), 4)
_case("decode-small-q4k", "small", {"mat": "Q4_K"}, False, [1], (0, 1), 4)
# batch addressing, mode 1: T = 1 with batch0 = 2 | cursor-indexed with batch != token | multi-token matvec | MFMA | 9 tokens over 11 slots
for _lens in ([0, 0, 1], [1, 0, 1], [1] * 3, [1] * 5, [1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 1]):
    _case("batch-tiny-" + "".join(map(str, _lens)), "tiny", {}, False, _lens, (1,), 2)
# RWKV-6 on the K-sliced GEMM (WRK_GEMM_KS=2)
for _n in (9, 20):
    for _mat in ("Q4_K", "Q8_0"):
        _case(f"ks-small-{_mat.lower()}-{_n}", "small", {"mat": _mat}, False, [1] * _n, (1,), 2, ks="2")
# LoRA ranks that are no multiple of 32, the smallest and the largest the fused kernels take, and one they decline
for _R, _W in RANKS:
    for _lens in ([1], [1] * 3):
        _case(f"rank-{_R}-{_W}-x{len(_lens)}", RANK_SHAPE(_R, _W), {}, False, _lens, (0, 1), 2)
for _lens in ([1], [1] * 3):
    _case(f"rank-fallback-{RANK_FALLBACK[0]}-{RANK_FALLBACK[1]}-x{len(_lens)}", RANK_SHAPE(*RANK_FALLBACK), {}, False, _lens, (1,), 2)
# chunks: every op-list buffer (mode 1 = the merged op list)
_case("chunk-small-70", "small", {"mat": "Q4_K"}, False, [70], (0, 1), 1)
_case("chunk-tiny-9-0-23", "tiny", {}, False, [9, 0, 23], (0, 1), 2)
# no warm-up: the first two tokens of a sequence.  After 8 tokens every head's WKV output has a variance above 2 and the group norm's eps
# (64e-5) is a 1e-4 effect, below one f16 ulp; on the zero state the variance is 1e-3 .. 3e-2 and eps decides the value (a layer with
# eps = 1e-5 is off by 20 .. 3800 ulp there, and by at most 1 ulp in every warmed-up case)
_case("cold-tiny-q5k", "tiny", {}, False, [1], (0, 1), 2, warm=0)
_case("cold-tiny-111", "tiny", {}, False, [1] * 3, (1,), 2, warm=0)

# every stage oracle/rwkv6.py records per layer
KEYS = ["att_x_ln", "att_xx", "tmx", "tm", "att_sx", "k", "v", "r", "g", "att_w", "time_decay", "wkv", "gn", "att_x", "att_o", "x_att", "ffn_x_ln",
        "ffn_kx", "ffn_rx", "ffn_k", "ffn_v", "ffn_r", "ffn_x", "x"]


# One replacement of a fixed bar, for an arithmetic reason.  att_sx = x + (prev - x) tm: a 1-ulp flip of tm (2^-10 where tm > 1) is multiplied
# by |prev - x|, which reaches 3 .. 6 for two LN rows of opposite sign, and is then measured with the spacing of the shifted value, 2^-11
# below 1 -- e.g. x = -2.42, prev = +0.76, tm 1.0137 -> 1.0146: att_sx = 0.804 moves by 3.1e-3 = 6.4 spacings, 7 after its own rounding (the
# 70-token chunk on an MI355X, 1 element of 1.25 million; the same att_sx is bit for bit the token shift of the GPU's own tm).  The bar is
# NOT taken from that run: it is the worst att_sx of the CPU reference in its two other summation orders over all cases (5 ulp,
# test_v6_layer_ref.py), times 2 -- the GPU's order is one more draw from the same distribution.  The share within 1 ulp stays at 80 %.
BUFFER_MAX_ULP = {"att_sx": 10.0}


def is_direct(key, lens):
    """One rounding away from the layer's exact inputs: LN1(x), and for one token per sequence the first shift (LN1 row and a state row)."""
    return key == "att_x_ln" or (key == "att_xx" and all(n <= 1 for n in lens))


def fixture(case):
    """(GGUF bytes, oracle model) of a case."""
    c = CASES[case]
    cfg = synth.V6_CONFIGS[c["cfg"]] if isinstance(c["cfg"], str) else c["cfg"]
    data = synth.make_v6_gguf(cfg, 42, **c["kw"])
    return data, O6.build_v6(ogguf.GgufReader(data), weights_f16=c["f16"])


def replay(model, lens, steps, warm=8):
    """The oracle's run of a case: `warm` warm-up tokens per live sequence (8: a generic recurrent state, as the RWKV-7 file argues), then
    per step (pre-token state [L, B, S+2, D], trace, end state)."""
    oracle = O6.V6Runtime(model, len(lens), act_f16=True)
    V = model.info.num_vocab
    if warm:
        oracle.infer_chunk([synth.tokens(99, f"w{b}", warm if n else 0, V) for b, n in enumerate(lens)], [])
    for step in range(steps):
        chunk = [synth.tokens(100 + step, f"b{b}", n, V) for b, n in enumerate(lens)]
        before = oracle.state.copy()
        oracle.trace = {}
        oracle.infer_chunk(chunk, [])
        trace, oracle.trace = oracle.trace, None
        yield before, trace, oracle.state.copy()


def layer_input(trace, li):
    return trace["emb_x"] if li == 0 else trace[f"{li - 1}_x"]


# ----------------------------------------------------------------------------- summation orders
def mm_f64(x, w):
    return (x.astype(np.float64) @ w.T.astype(np.float64)).astype(np.float32)


def mm_rev32(x, w):
    """f32, the K axis in chunks of 32 taken from the last to the first, each chunk's partial sum added to one f32 accumulator."""
    x, w = x.astype(np.float32), w.astype(np.float32)
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for k1 in range(x.shape[1], 0, -32):
        k0 = max(k1 - 32, 0)
        acc = (acc + np.matmul(x[:, k0:k1][:, ::-1], w[:, k0:k1][:, ::-1].T)).astype(np.float32)
    return acc


ORDERS = {"numpy": lambda x, w: np.matmul(x.astype(np.float32), w.T.astype(np.float32)).astype(np.float32), "f64": mm_f64, "rev32": mm_rev32}

MUTANTS = ["u_on_state", "decay_before_read", "gn_eps_1e-5", "gate_sigmoid", "shift_state_from_x", "w2_product_not_stored", "mix_swapped",
           "no_halving", "w_o_not_discounted", "time_decay_f16"]


class RefRuntime(O6.V6Runtime):
    def __init__(self, model, num_batch, order="numpy", mutant=None):
        super().__init__(model, num_batch, act_f16=True)
        assert order in ORDERS and (mutant is None or mutant in MUTANTS)
        self.order, self.mutant = order, mutant

    def _mm(self, w, x, act="none", f32_out=False):
        y = ACT[act](ORDERS[self.order](x, w))
        return y if f32_out else self.rnd(y)

    def _layer(self, li, x, where):
        """oracle/rwkv6.py V6Runtime._layer, line by line, with the mutants spliced in (`mu`)."""
        m, info, rnd, mu = self.model, self.model.info, self.rnd, self.mutant
        D, S, H, R = info.num_emb, info.head_size, info.num_head, info.custom["time_mix"]
        batches, starts, clens, firsts, lasts = where
        T = len(x)
        p, st = m.layers[li], self.state[li]
        rec = lambda name, val: self._rec(li, name, val)       # noqa: E731

        def shift(xv, state_row, fac):
            prev = np.empty_like(xv)
            prev[1:] = xv[:-1]
            for t in np.nonzero(firsts)[0]:
                prev[t] = state_row[batches[t]]
            fac = fac if fac.ndim == 2 else fac[None, :]
            return rnd(mix(prev, xv, fac) if mu == "mix_swapped" else mix(xv, prev, fac))

        x_in = x
        att_x = rnd(layer_norm(x, p["ln1_w"], p["ln1_b"], LN_EPS))
        rec("att_x_ln", att_x)
        row0 = st[:, 0, :]
        att_xx = shift(att_x, row0, p["time_mix_x"])
        rec("att_xx", att_xx)
        tmx = self._mm(p["time_mix_w1"], att_xx, "tanh")
        rec("tmx", tmx)
        tmx = tmx.reshape(T, 5, R)
        tm = np.stack([self._mm(p["time_mix_w2"][i], tmx[:, i, :], f32_out=(mu == "w2_product_not_stored")) for i in range(5)])
        tm = rnd(p["time_mix"][:, None, :] + tm)
        rec("tm", tm)
        sx = [shift(att_x, row0, tm[i]) for i in range(5)]
        rec("att_sx", np.stack(sx))
        k = self._mm(p["w_k"], sx[1], f32_out=True)
        v = self._mm(p["w_v"], sx[2], f32_out=True)
        r = self._mm(p["w_r"], sx[3], f32_out=True)
        g = self._mm(p["w_g"], sx[4])
        aw = self._mm(p["time_decay_w1"], sx[0], "tanh")
        td = self._mm(p["time_decay_w2"], aw, f32_out=True)
        td = (p["time_decay"][None, :] + td).astype(np.float32)
        td = np.exp(-np.exp(td, dtype=np.float32), dtype=np.float32)
        if mu == "time_decay_f16":
            td = r16(td)
        rec("k", k); rec("v", v); rec("r", r); rec("g", g); rec("att_w", aw); rec("time_decay", td)
        u = p["time_first"].reshape(H, S)
        y = np.empty((T, D), np.float32)
        for t in range(T):
            b = batches[t]
            if lasts[t]:
                st[b, 0, :] = (x_in if mu == "shift_state_from_x" else att_x)[starts[t] + clens[t] - 1]
            Sm = st[b, 1:S + 1, :].reshape(S, H, S).transpose(1, 0, 2)
            kt, vt, rt, wt = (z[t].reshape(H, S) for z in (k, v, r, td))
            kv = kt[:, :, None] * vt[:, None, :]
            if mu == "u_on_state":
                seen = kv + u[:, :, None] * Sm
            elif mu == "decay_before_read":
                seen = u[:, :, None] * kv + wt[:, :, None] * Sm
            else:
                seen = u[:, :, None] * kv + Sm
            y[t] = np.einsum("hj,hji->hi", rt, seen).reshape(D)
            st[b, 1:S + 1, :] = (wt[:, :, None] * Sm + kv).astype(np.float32).transpose(1, 0, 2).reshape(S, D)
        aux = rnd(y)
        rec("wkv", aux)
        gn_eps = np.float32(1e-5) if mu == "gn_eps_1e-5" else GN_EPS
        aux = rnd(layer_norm(aux.reshape(T, H, S), p["gn_w"].reshape(H, S)[None], p["gn_b"].reshape(H, S)[None], gn_eps).reshape(T, D))
        rec("gn", aux)
        att_x = rnd((sigmoid(g) if mu == "gate_sigmoid" else O6.silu(g)) * aux)
        rec("att_x", att_x)
        w_o = p["w_o"]
        if mu == "w_o_not_discounted":
            w_o = (w_o * np.float32(2.0 ** (li // m.rescale))).astype(np.float32)      # exact: a power of two
        o = self._mm(w_o, att_x)
        rec("att_o", o)
        x = rnd(o + x)
        rec("x_att", x)
        ffn_x = rnd(layer_norm(x, p["ln2_w"], p["ln2_b"], LN_EPS))
        rec("ffn_x_ln", ffn_x)
        rowf = st[:, S + 1, :]
        kx, rx = shift(ffn_x, rowf, p["ffn_mix_k"]), shift(ffn_x, rowf, p["ffn_mix_r"])
        fk = self._mm(p["ffn_w_k"], kx, "squared_relu")
        fv = self._mm(p["ffn_w_v"], fk)
        fr = self._mm(p["ffn_w_r"], rx)
        rec("ffn_kx", kx); rec("ffn_rx", rx); rec("ffn_k", fk); rec("ffn_v", fv); rec("ffn_r", fr)
        for t in np.nonzero(lasts)[0]:
            st[batches[t], S + 1, :] = ffn_x[t]
        ffn_x = rnd(sigmoid(fr) * fv)
        rec("ffn_x", ffn_x)
        x = rnd(ffn_x + x)
        if (li + 1) % m.rescale == 0 and mu != "no_halving":
            x = rnd(np.float32(0.5) * x)
        rec("x", x)
        return x


def run_layer(ref, li, x_in, before, lens):
    """Teacher-forced: layer li of `ref` alone on the oracle's layer input and pre-token state -> (trace, the layer's end state [B, S+2, D])."""
    ref.state[li] = before[li]
    ref.trace = {}
    ref.infer_layer(li, x_in, lens)
    trace, ref.trace = ref.trace, None
    return trace, ref.state[li].copy()


# ----------------------------------------------------------------------------- grading
def breaks(got, want, direct, max_ulp=None):
    """Does `got` break the buffer's bar?  (check() without the assert and the statistics: the mutant tests need the answer.)"""
    u = ulps(np.asarray(got).reshape(np.shape(want)), want)
    if direct:
        return bool(u.max() > DIRECT_MAX_ULP)
    return bool(u.max() > (max_ulp or DOWNSTREAM_MAX_ULP) or (u <= 1.0).mean() < DOWNSTREAM_FRAC_LE1)


def state_error(got, want):
    """max |delta| of one sequence's layer state [S+2, D], relative to max |state| (floored as in the RWKV-7 file)."""
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-3)


def grade_state(case, li, got, want, lens, stats):
    for b, n in enumerate(lens):
        if n:
            e = state_error(got[b], want[b])
            s = stats.setdefault(case, {}).setdefault("state", {"max_rel": 0.0})
            s["max_rel"] = max(s["max_rel"], e)
            assert e <= STATE_REL, f"{case} layer {li} sequence {b}: state off by {e:.3e} of max|state| (limit 2^-9)"


def grade(case, li, trace, got, lens, stats, keys=KEYS):
    """Every recorded stage of layer li at its bar."""
    for key in keys:
        check(case, key, got[f"{li}_{key}"], trace[f"{li}_{key}"], is_direct(key, lens), BUFFER_MAX_ULP.get(key), stats=stats)


# ----------------------------------------------------------------------------- stage-local checks
# The layer bars above compare with the oracle's buffers, so they carry the layer's own f16 flips (up to 5 ulp on the CPU alone) and cannot
# see a fault below that: WHERE a rounding sits, or an f32 buffer kept in f16.  Two stages are therefore also recomputed, in f64, from the
# inputs the layer under test stored itself -- no flip is carried in, only the stage's own arithmetic differs:
#   * tm (op list) / att_sx (fused layer) from the stored tmx: round16(round16(time_mix_w2 . tmx) + time_mix), then the five token shifts.
#     An f32 sum of R <= 136 products is within R * 2^-24 (8e-6) of the exact one, relative to sum |w x|; an f16 store flips only where the
#     exact value lies that close to a rounding boundary (spacing 2^-11 .. 2^-10 relative): a share of at most 2 * 8e-6 / 2^-11 = 3.3 % even
#     if every element had the worst-case error and no cancellation helped.  Bar: >= 95 % of the elements bit-identical; tm: none beyond
#     1 ulp (a flipped product moves the sum by one spacing at the most); att_sx = x + (prev - x) tm: a 1-ulp flip of tm is multiplied by
#     |prev - x|, which is several times the shifted value where the two nearly cancel, so its maximum is att_sx's layer bar (BUFFER_MAX_ULP).
#   * time_decay (f32; the op list stores it) from the stored att_w: exp(-exp(time_decay_w2 . att_w + time_decay)).  The f32 sum (W <= 136
#     terms) and two exponentials at a few f32 ulp each leave a relative error below 1e-5, the f16 spacing is at least 4.9e-4 relative:
#     bar 1/8 of an f16 ulp (6e-5 relative at the least).  A time_decay that went through f16 is off by up to 1/2 ulp.
LOCAL_EXACT_SHARE, LOCAL_F32_ULP = 0.95, 0.125


def local_tm(p, tmx):
    """tm [5, T, D] from a stored tmx [T, 5R]."""
    T = len(tmx)
    t = np.asarray(tmx, np.float32).reshape(T, 5, -1)
    prod = np.stack([r16(mm_f64(t[:, i, :], p["time_mix_w2"][i])) for i in range(5)])
    return r16(p["time_mix"][:, None, :] + prod)


def local_att_sx(p, tmx, att_x_ln, prev):
    """att_sx [5, T, D] of one token per sequence from the stored tmx and LN1(x); prev [T, D] = each token's att shift-state row."""
    tm = local_tm(p, tmx)
    x = np.asarray(att_x_ln, np.float32)
    return np.stack([r16(mix(x, prev, tm[i])) for i in range(5)])


def local_time_decay(p, att_w):
    a = np.asarray(att_w, np.float64) @ p["time_decay_w2"].T.astype(np.float64) + p["time_decay"][None, :].astype(np.float64)
    return np.exp(-np.exp(a)).astype(np.float32)


def local_breaks_exact(got, want, max_ulp=1.0):
    got, want = np.asarray(got, np.float32).reshape(np.shape(want)), np.asarray(want, np.float32)
    return bool(ulps(got, want).max() > max_ulp or (got == want).mean() < LOCAL_EXACT_SHARE)


def local_breaks_f32(got, want):
    return bool(ulps(np.asarray(got).reshape(np.shape(want)), want).max() > LOCAL_F32_ULP)


def grade_local(case, name, got, want, exact, stats, max_ulp=1.0):
    got, want = np.asarray(got, np.float32).reshape(np.shape(want)), np.asarray(want, np.float32)
    u = ulps(got, want)
    s = stats.setdefault(case, {}).setdefault(name, {"max_ulp": 0.0, "min_frac_exact": 1.0, "n": 0})
    s["max_ulp"] = max(s["max_ulp"], float(u.max()))
    s["min_frac_exact"] = min(s["min_frac_exact"], float((got == want).mean()))
    s["n"] += 1
    if exact:
        assert u.max() <= max_ulp and (got == want).mean() >= LOCAL_EXACT_SHARE, \
            f"{case} {name}: {u.max():.2f} ulp, {(got == want).mean():.4f} bit-identical (limits {max_ulp} ulp, {LOCAL_EXACT_SHARE})"
    else:
        assert u.max() <= LOCAL_F32_ULP, f"{case} {name}: {u.max():.4f} f16 ulp (limit {LOCAL_F32_ULP})"
