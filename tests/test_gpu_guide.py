"""Classifier-free guidance on the device (web-rwkv-gguf_amd/csrc/wrk_guide.hip) against the restatement in
tests/guide_ref.py: the row function (`wrk_guide_logits`, `Context.guide_logits`), the validation, and guidance in the decode loops
(`Runtime.generate_guided`) of both runners.

Every comparison is exact: token ids and bit patterns.  The loops run on the tiny fixtures (V = 512), RWKV-7 and RWKV-6, modes 0 and
1, B in {1, 3} guided sequences on 2B state slots -- the helpers, pick families, first tokens and sampler parameters of
tests/test_gpu_grammar.py.

  rows        five rows per call with the scales [1, 0, 0.5, 1.5, 7.5], input and output stride V and V + 3, on guide_ref.special_pairs:
              special_rows, a pair of +-3e38 rows whose difference overflows, and the hand-worked table;
  errors      every WRK_E_ARG and WRK_E_UNSUPPORTED case of the contract, and nothing launched by a refused call;
  identity    with every scale 1 a guided call returns what the same call without guidance returns on slots [0, B), in every family:
              tokens, lengths, last logits, log-probs, mu, grammar states, windows, state slots.  The call without guidance runs on the
              same frame of 2B sequences (run_plain says why);
  replay      scales (0.5, 1.5, 3) per sequence and a random bias set per sequence; the partner slots are primed with another prompt; a
              second runtime is fed the device's own tokens on all 2B slots, and the reference pick of the family on bias_ref.apply of
              guide_ref.mix of its rows (penalised through penalty_ref for "pen") must be the device's token.  A step is excused only
              where the reference's own ambiguous(...) says so (greedy: never), and at B = 3 at least 95 % of the steps, summed over the
              six families, must be checked.  Prompts, scales and the seed of the bias sets are chosen on the CPU: with the oracle's
              logits in place of the device's, the reference loop calls REPLAY_CPU_AMBIGUOUS steps ambiguous and guidance changes
              REPLAY_CPU_CHANGED of the greedy picks (below; at least a third in every configuration).  On the device (MI355X) the
              replay checked, at B = 3, 175 (mode 0) and 173 (mode 1) of 180 steps on RWKV-7 and 177 of 180 on RWKV-6 in both modes,
              and guidance changed 24 (RWKV-7) and 29 (RWKV-6) of the 30 greedy picks, 9 and 10 of 10 at B = 1;
  stops       with stop tokens and with stop sequences the tokens are a prefix of the guided call without stops, and slots b and B + b are
              bit for bit what the guided call without stops of lengths[b] steps leaves."""
import ctypes as C
import functools

import numpy as np
import pytest

import bias_ref as BR
import guide_ref as GR
import penalty_ref as R
import test_gpu_grammar as TG
import wrk
from oracle.rnn import pack_cursor, stack_cursors

pytestmark = pytest.mark.gpu

P_ = wrk._ptr
FAMILIES, FIRST, STEPS = TG.FAMILIES, TG.FIRST, TG.STEPS
bits, vocab, fresh, same, cut = TG.bits, TG.vocab, TG.fresh, TG.same, TG.cut
# (v6, mode, B): B guided sequences on 2B slots
CONFIGS = [(v6, mode, B) for v6 in (False, True) for mode in (0, 1) for B in (1, 3)]
NEG_FIRST = [33, 250, 9]                            # what the partners feed at step 0
NEG_PROMPT = [[5, 440, 17], [301, 2, 77], [129, 64, 400]]      # what the partner slots are primed with
SCALES = [1.5, 3.0, 0.5]
REPLAY_BIAS_SEED = 7
# measured on the CPU with the oracle's logits at B = 3 (the cap allows 9 of 180): {v6: steps of 180 the reference loop calls ambiguous} --
# RWKV-7: 1 sample + 4 pen, RWKV-6: 1 sample + 1 typical + 1 pen -- and {v6: greedy picks of 30 that guidance changes}; at B = 1 it
# changes 9 (RWKV-7) and 10 (RWKV-6) of 10
REPLAY_CPU_AMBIGUOUS = {False: 5, True: 3}
REPLAY_CPU_CHANGED = {False: 24, True: 29}


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


# ----------------------------------------------------------------------------- 1. the row function
@pytest.mark.parametrize("V", [1, 3, 50, 1023, 1024, 1025, 4099, 65536, 70001, 2 ** 20])
def test_guide_logits_matches_the_restatement(ctx, V):
    """Both instantiations (16-byte accesses when V and both strides are multiples of 4; scalar otherwise), the odd tail, more than one
    workgroup span per row (V > 4096), the last span cut short; the input rows are only read and the pad of the output is not written."""
    rng = np.random.default_rng(V)
    sc = np.array(GR.SCALES, np.float32)
    for in_stride in (V, V + 3):
        a = GR.special_pairs(TG.special_rows, rng, 5, in_stride, V)
        want = [GR.mix(a[r, :V], a[5 + r, :V], s) for r, s in enumerate(GR.SCALES)]
        src = ctx.buffer(a)
        for out_stride in (V, V + 3):
            canary = np.full((5, out_stride), 0x7FA5A5A5, np.uint32).view(np.float32)
            dst = ctx.buffer(canary)
            ctx.check(wrk.hip.wrk_guide_logits(ctx.h, src.h, V, in_stride, 5, P_(sc, wrk._f32p), dst.h, out_stride))
            got = dst.read(np.float32, canary.size).reshape(5, out_stride)
            for r in range(5):
                assert np.array_equal(bits(got[r, :V]), bits(want[r])), (in_stride, out_stride, r)
                assert np.array_equal(bits(got[r, V:]), bits(canary[r, V:])), "the padding between rows is not touched"
            assert not np.isnan(got[1:, :V]).any(), "outside s == 1 rows the result is never NaN"
        assert np.array_equal(bits(src.read(np.float32, a.size)), bits(a).reshape(-1)), "the input rows are only read"
    if V <= 4099:
        dense = GR.special_pairs(TG.special_rows, rng, 5, V, V)
        out = ctx.guide_logits(dense, GR.SCALES)
        assert all(np.array_equal(bits(out[r]), bits(GR.mix(dense[r], dense[5 + r], s))) for r, s in enumerate(GR.SCALES))
    if V >= GR.HAND_LEN:        # the hand-worked table, by its own expected words
        hc, hu = GR.hand_rows(V)
        for s in GR.SCALES[1:]:
            got = bits(ctx.guide_logits(np.stack([hc, hu]), s))[0]
            for i, (_, _, res) in enumerate(GR.HAND):
                assert s not in res or got[i] == res[s], (s, i)
            for i, (fs, _, _, w, fused) in enumerate(GR.FMA_CASES):
                assert fs != s or (got[len(GR.HAND) + i] == w != fused), "three roundings, not a fused multiply-add"


# ----------------------------------------------------------------------------- 2. validation
def test_argument_errors_leave_the_model_usable(ctx):
    V = vocab()
    rt = fresh(ctx, False, 4)
    rt.generate_greedy([1, 2, 3, 4], 3)
    before = [rt.state_back(b).copy() for b in range(4)]
    rows = np.zeros((4, V), np.float32)

    def code(call):
        with pytest.raises(wrk.WrkError) as e:
            call()
        return e.value.code

    # a scale must be finite and >= 0, from every call that takes one
    for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-45):
        assert GR.check_scale([1.5, bad]) == "arg"
        assert code(lambda: ctx.guide_logits(rows, [1.5, bad])) == wrk.E_ARG, bad
        assert code(lambda: rt.generate_guided([1, 2], 3, [1.5, bad])) == wrk.E_ARG, bad
    assert GR.check_scale([0.0, -0.0, 3e38]) == "ok"
    assert ctx.guide_logits(rows, [0.0, 3e38]).shape == (2, V)
    # the vocabulary limit, and one buffer for both
    big = ctx.buffer(np.zeros(2 * (2 ** 20 + 1), np.float32))
    out = ctx.buffer(np.zeros(2 ** 20 + 1, np.float32))
    one = np.array([1.5], np.float32)
    assert wrk.hip.wrk_guide_logits(ctx.h, big.h, 2 ** 20 + 1, 2 ** 20 + 1, 1, P_(one, wrk._f32p), out.h, 2 ** 20 + 1) == wrk.E_UNSUPPORTED
    assert wrk.hip.wrk_guide_logits(ctx.h, big.h, 2 ** 20, 2 ** 20, 1, P_(one, wrk._f32p), out.h, 2 ** 20) == wrk.OK
    assert wrk.hip.wrk_guide_logits(ctx.h, big.h, 8, 8, 1, P_(one, wrk._f32p), big.h, 8) == wrk.E_ARG                 # in place
    assert wrk.hip.wrk_guide_logits(ctx.h, big.h, 8, 8, 1, None, out.h, 8) == wrk.E_ARG                                # no scales
    assert wrk.hip.wrk_guide_logits(ctx.h, big.h, 2 ** 20, 2 ** 20, 2, P_(np.ones(2, np.float32), wrk._f32p), out.h, 8) == wrk.E_ARG   # 4 rows do not fit
    assert wrk.hip.wrk_guide_logits(ctx.h, big.h, 8, 8, 2, P_(np.ones(2, np.float32), wrk._f32p), out.h, 7) == wrk.E_ARG   # out_stride < V
    # lanes, the queue and beam search: WRK_E_UNSUPPORTED before any launch
    assert code(lambda: rt.generate_guided([1, 2], 3, 1.5, mode=1 | (2 << 8))) == wrk.E_UNSUPPORTED
    assert code(lambda: rt.generate_queue([[1, 2], [3]], max_new=2, guidance_scale=1.5)) == wrk.E_UNSUPPORTED
    assert code(lambda: rt.generate_beam([1], 3, 2, guidance_scale=1.5)) == wrk.E_UNSUPPORTED
    gen = wrk.GenerateOptions()
    nf = np.array([1], np.uint32)
    gen.guidance_first_tokens = P_(nf, wrk._u32p)           # either field of `gen`
    arrs = [np.zeros(8, np.uint32) for _ in range(8)]
    run = C.c_uint32()
    res = wrk.BeamResult(P_(arrs[0], wrk._u32p), P_(arrs[1], wrk._u32p), P_(np.zeros(8, np.float32), wrk._f32p), P_(arrs[2], wrk._u32p),
                         P_(arrs[3], wrk._u32p), P_(arrs[4], wrk._u32p), C.pointer(run), None, None, None)
    bo = wrk.BeamOptions(2, 0.0, C.pointer(gen))
    assert wrk.hip.wrk_v7_generate_beam(ctx.h, rt.model, rt.state, P_(nf, wrk._u32p), 1, 3, C.byref(bo), C.byref(res), None, 1) == wrk.E_UNSUPPORTED
    # a state of fewer than 2B slots
    assert code(lambda: rt.generate_guided([1, 2, 3], 3, 1.5)) == wrk.E_ARG
    # a partner's first token outside the vocabulary
    assert code(lambda: rt.generate_guided([1, 2], 3, 1.5, negative_first_tokens=[3, V])) == wrk.E_ARG
    with pytest.raises(ValueError):
        rt.generate_guided([1, 2], 3, None, negative_first_tokens=[3, 4])
    with pytest.raises(ValueError):
        rt.generate_guided([1, 2], 3, [1.0, 2.0, 3.0])
    # guidance_first_tokens without guidance_scale, through the ABI
    ft, out_t, lens = np.array([1, 2], np.uint32), np.zeros((3, 2), np.uint32), np.zeros(2, np.uint32)
    opt = wrk.GenerateOptions()
    opt.guidance_first_tokens = P_(ft, wrk._u32p)
    assert wrk.hip.wrk_v7_generate_stop(ctx.h, rt.model, rt.state, P_(ft, wrk._u32p), 2, 3, C.byref(opt), P_(out_t, wrk._u32p), P_(lens, wrk._u32p),
                                        None, C.byref(run), None, 1) == wrk.E_ARG
    for b in range(4):
        assert np.array_equal(bits(rt.state_back(b)), bits(before[b])), "a refused call launched nothing"
    # still usable: a guided call runs, and the unguided loop from zero states equals a fresh runtime's
    tok, lens = rt.generate_guided([1, 2], 4, [1.5, 0.0])
    assert tok.shape == (4, 2) and lens.tolist() == [4, 4]
    TG.zero_states(rt, 4)
    t, _ = rt.generate_greedy([1, 2, 3, 4], 4)
    fresh_rt = fresh(ctx, False, 4)
    assert np.array_equal(t, fresh_rt.generate_greedy([1, 2, 3, 4], 4)[0])
    fresh_rt.close()
    rt.close()
    # RWKV-6 refuses alike
    rt6 = fresh(ctx, True, 2)
    assert code(lambda: rt6.generate_guided([1, 2], 3, 1.5)) == wrk.E_ARG                                          # 2 slots, 4 needed
    assert code(lambda: rt6.generate_guided([1], 3, np.nan)) == wrk.E_ARG
    assert code(lambda: rt6.generate_guided([1], 3, 1.5, mode=1 | (2 << 8))) == wrk.E_UNSUPPORTED
    assert code(lambda: rt6.generate_queue([[1, 2], [3]], max_new=2, guidance_scale=1.5)) == wrk.E_UNSUPPORTED
    assert code(lambda: rt6.generate_beam([1], 3, 2, guidance_scale=1.5)) == wrk.E_UNSUPPORTED
    rt6.close()


# ----------------------------------------------------------------------------- the guided loop
def prime(rt, B, mode):
    """Zero states on all 2B slots, then the negative prompts into the partner slots [B, 2B), as one job."""
    TG.zero_states(rt, 2 * B)
    toks, cur, hdr = [], [], []
    for b in range(B):
        n = len(NEG_PROMPT[b])
        cur += [pack_cursor(B + b, len(toks), n)] * n
        toks += NEG_PROMPT[b]
        hdr.append(len(toks) - 1)
    rt.infer_raw(toks, cur, hdr, mode=mode)


def run_guided(ctx, rt, family, B, mode, scale, stop=None, occ=None, steps=STEPS, primed=True, **extra):
    """One guided call of the loop that belongs to `family`: everything it leaves behind, the states of all 2B slots included."""
    if primed:
        prime(rt, B, mode)
    else:
        TG.zero_states(rt, 2 * B)
    kw = cut(FAMILIES[family], B)
    if family == "pen":
        for b in range(B):
            occ.load(b)
        kw["occurrence"] = occ
    tok, lens, logits = rt.generate_guided(FIRST[:B], steps, scale, negative_first_tokens=NEG_FIRST[:B], stop=stop, mode=mode, want_logits=True,
                                           **kw, **extra)
    return dict(tok=tok, lens=lens, logits=logits, lp=rt.last_logprobs, mu=rt.last_mirostat_mu, gs=rt.last_grammar_state,
                match=rt.last_stop_match, tail=rt.last_stop_tail, states=[rt.state_back(b).copy() for b in range(2 * B)])


# ----------------------------------------------------------------------------- 3. identity
def run_plain(ctx, rt, family, B, mode, stop=None, occ=None, **extra):
    """The call without guidance on the frame the guided call runs: 2B sequences from zero states, the B conditional ones first and behind
    them B more that start from the partners' first tokens, with the families' parameters repeated.  A frame's matmul kernels are chosen
    by the number of stacked sequences, so the logits of a frame of B and of a frame of 2B sequences differ in their last bits (measured:
    RWKV-7, mode 0, B = 1: equal tokens, last logits apart by 1e-4); a sequence's row does not depend on its neighbours' rows, so columns
    [0, B) of this call are what guidance at scale 1 has to reproduce bit for bit."""
    n = 2 * B
    TG.zero_states(rt, n)
    kw = {k: (tuple(np.resize(x, n) for x in v) if k == "mirostat" else np.resize(v, n)) for k, v in FAMILIES[family].items()}
    if family == "pen":
        for b in range(n):
            occ.load(b)
        kw["occurrence"] = occ
    for k in ("grammar_state", "bias_set"):
        if k in extra:
            extra[k] = list(extra[k]) * 2
    stops = [] if not stop else list(stop) + [[] for _ in range(B)]
    tok, lens, logits = rt.generate_stop(FIRST[:B] + NEG_FIRST[:B], STEPS, stops, mode=mode, want_logits=True, **kw, **extra)
    lp = None if rt.last_logprobs is None else tuple(x[:, :B] for x in rt.last_logprobs)
    head = lambda x: None if x is None else x[:B]
    return dict(tok=tok[:, :B], lens=lens[:B], logits=logits[:B], lp=lp, mu=head(rt.last_mirostat_mu), gs=head(rt.last_grammar_state),
                states=[rt.state_back(b).copy() for b in range(B)])


@pytest.mark.parametrize("v6,mode,B", CONFIGS)
def test_scale_one_is_the_call_without_guidance(ctx, v6, mode, B):
    V = vocab(v6)
    rt = fresh(ctx, v6, 2 * B)
    occ = wrk.Occurrence(ctx, 2 * B, V)
    cls, trans = TG.free_tables(V)
    g = wrk.Grammar(ctx, V, cls, trans)
    starts = [2, 0, 5][:B]
    win = wrk.TokenWindow(ctx, 2 * B, V, 16)
    for family in FAMILIES:
        plain = run_plain(ctx, rt, family, B, mode, occ=occ, logprobs=2)
        got = run_guided(ctx, rt, family, B, mode, 1.0, stop=[], occ=occ, logprobs=2, primed=False)
        same(plain, got, family)
        for b in range(B):
            assert np.array_equal(bits(got["states"][b]), bits(plain["states"][b])), (family, b)
        # with stop sets: sequence 0 ends on its fourth token
        stops = [[int(plain["tok"][3, 0])]] + [[] for _ in range(B - 1)]
        plain = run_plain(ctx, rt, family, B, mode, stop=stops, occ=occ, logprobs=2)
        assert plain["lens"][0] <= 4
        got = run_guided(ctx, rt, family, B, mode, [1.0] * B, stop=stops, occ=occ, logprobs=2, primed=False)
        same(plain, got, (family, "with stops"))
        for b in range(B):
            assert np.array_equal(bits(got["states"][b]), bits(plain["states"][b])), (family, b, "with stops")
        # with a grammar and a window: the states and the windows the call leaves
        left = []
        for guided in (False, True):
            for b in range(2 * B):
                win.load(b)
            kw = dict(grammar=g, grammar_state=starts, window=win, dry=(0.8, 1.75, 2), no_repeat_ngram=3)
            out = (run_guided(ctx, rt, family, B, mode, 1.0, stop=[], occ=occ, primed=False, **kw) if guided
                   else run_plain(ctx, rt, family, B, mode, occ=occ, **kw))
            left.append((out["tok"].tolist(), out["gs"].tolist(), [win.back(b).tolist() for b in range(B)], bits(out["logits"]).tolist()))
        assert left[0] == left[1], (family, "grammar states and windows")
    win.close()
    g.close()
    occ.close()
    rt.close()


# ----------------------------------------------------------------------------- 4. replay
@functools.lru_cache(maxsize=None)
def replay_sets(v6):
    V = vocab(v6)
    rng = np.random.default_rng(REPLAY_BIAS_SEED)
    sets = []
    for n in (48, 1, 120):
        ids = rng.choice(V, n, replace=False)
        vals = rng.uniform(-3, 3, n).astype(np.float32)
        vals[rng.random(n) < 0.25] = -np.inf
        sets.append((ids, vals))
    return sets


def replay(ctx, v6, B, mode, family, sets, out):
    """A second runtime, primed alike, is fed the device's own tokens on all 2B slots; the reference pick of `family` on the guided,
    biased (and for "pen" penalised) row of its logits must give the device's token wherever the reference does not call the row
    ambiguous.  (checked, steps)"""
    V = vocab(v6)
    rt = fresh(ctx, v6, 2 * B)
    prime(rt, B, mode)
    pk = TG.picks_of(family, B)
    pen = cut(FAMILIES["pen"], B) if family == "pen" else None
    counts = [np.zeros(V, np.float32) for _ in range(B)]
    flags = [np.zeros(V, np.uint32) for _ in range(B)]
    ones = np.ones(V, np.float32)
    cur = FIRST[:B] + NEG_FIRST[:B]
    checked = total = 0
    for step in range(out["tok"].shape[0]):
        logits = rt.infer_raw(cur, stack_cursors([1] * (2 * B)), list(range(2 * B)), mode=mode)
        for b in range(B):
            y = int(out["tok"][step, b])
            x = BR.apply(GR.mix(logits[b], logits[B + b], SCALES[b]), *sets[b])
            assert x[y] != -np.inf, f"step {step} sequence {b}: token {y} is banned"
            if pen:
                x = R.penalize(x, counts[b], flags[b], pen["presence"][b], pen["frequency"][b])
                counts[b], flags[b] = R.update(counts[b], flags[b], y, ones, pen["decay"][b])
            tok, ambiguous = pk[b].draw(x, step)
            total += 1
            if not ambiguous:
                assert y == tok, (family, step, b)
                checked += 1
        cur = out["tok"][step].tolist() * 2
    # the last logits of the call are the raw conditional rows of the last step
    assert np.array_equal(bits(out["logits"]), bits(logits[:B])), "last_logits: the raw head rows of the conditional sequences"
    rt.close()
    return checked, total


@pytest.mark.parametrize("v6,mode,B", CONFIGS)
def test_guided_picks_match_the_replay(ctx, v6, mode, B):
    V = vocab(v6)
    sets = replay_sets(v6)
    lb = wrk.LogitBias(ctx, V, sets)
    rt = fresh(ctx, v6, 2 * B)
    occ = wrk.Occurrence(ctx, B, V)
    checked = total = 0
    for family in FAMILIES:
        out = run_guided(ctx, rt, family, B, mode, SCALES[:B], occ=occ, logit_bias=lb, bias_set=list(range(B)))
        assert out["lens"].tolist() == [STEPS] * B
        c, t = replay(ctx, v6, B, mode, family, sets, out)
        print(f"{family}: {c} of {t} steps checked")
        checked, total = checked + c, total + t
        if family == "greedy":
            assert c == t, "greedy has no excused step"
            off = run_guided(ctx, rt, family, B, mode, 1.0, occ=occ, logit_bias=lb, bias_set=list(range(B)))
            changed = int((out["tok"] != off["tok"]).sum())
            print(f"guidance changes {changed} of {t} greedy picks")
            assert 3 * changed >= t, "guidance changes too few greedy picks: a kernel that does nothing would nearly pass"
    assert B != 3 or checked >= 0.95 * total, (checked, total)
    occ.close()
    rt.close()
    lb.close()


def test_one_program_serves_any_scales(ctx):
    """The scales are device data: other scales replay the program the first call captured, and calls without guidance in between run
    the programs they ran before."""
    rt = fresh(ctx, False, 4)
    plain = run_plain(ctx, rt, "greedy", 2, 1)["tok"]
    seen = []
    for _ in range(2):
        a = run_guided(ctx, rt, "greedy", 2, 1, [3.0, 0.0], primed=False)["tok"]
        b = run_guided(ctx, rt, "greedy", 2, 1, [1.0, 1.0], primed=False)["tok"]
        c = run_guided(ctx, rt, "greedy", 2, 1, [0.0, 3.0], primed=False)["tok"]
        assert np.array_equal(b, plain) and np.array_equal(run_plain(ctx, rt, "greedy", 2, 1)["tok"], plain)
        assert not np.array_equal(a, plain) and not np.array_equal(c, a)
        seen.append((a.tolist(), c.tolist()))
    assert seen[0] == seen[1]
    rt.close()


# ----------------------------------------------------------------------------- 5. stops
@pytest.mark.parametrize("v6,mode,B", CONFIGS)
@pytest.mark.parametrize("family", ["greedy", "sample"])
def test_stops_freeze_both_slots(ctx, family, v6, mode, B):
    V = vocab(v6)
    rt = fresh(ctx, v6, 2 * B)
    free = run_guided(ctx, rt, family, B, mode, SCALES[:B])
    tok = free["tok"]
    # sequence 0 ends on its fifth token, the last sequence on its seventh (B = 3; the middle one never ends)
    ends = {0: 4, B - 1: 6} if B > 1 else {0: 4}
    stop_ids = [[int(tok[ends[b], b])] if b in ends else [] for b in range(B)]
    stop_seqs = [[[int(tok[ends[b] - 1, b]), int(tok[ends[b], b])]] if b in ends else [] for b in range(B)]
    by_len = {}
    for what, kw in (("tokens", dict(stop=stop_ids)), ("sequences", dict(stop=[], stop_sequences=stop_seqs))):
        got = run_guided(ctx, rt, family, B, mode, SCALES[:B], poll_steps=2, **kw)
        for b in range(B):
            n = int(got["lens"][b])
            assert n <= (ends[b] + 1 if b in ends else STEPS), (what, b)
            assert got["tok"][:n, b].tolist() == tok[:n, b].tolist(), (what, b, "a prefix of the call without stops")
            if n not in by_len:
                by_len[n] = run_guided(ctx, rt, family, B, mode, SCALES[:B], steps=n)
            ref = by_len[n]
            for slot in (b, B + b):
                assert np.array_equal(bits(got["states"][slot]), bits(ref["states"][slot])), (what, slot, "frozen as the call of lengths[b] steps leaves it")
            assert np.array_equal(bits(got["logits"][b]), bits(ref["logits"][b])), (what, b)
        assert got["lens"][0] <= 5 and got["tok"].shape[1] == B and got["logits"].shape == (B, V)
        if what == "sequences":
            assert got["match"].shape == (B,) and got["tail"].shape == (B, wrk.STOP_TAIL_LEN)
            assert [int(m) != wrk.STOP_MATCH_NONE for m in got["match"]] == [b in ends for b in range(B)]
    rt.close()
