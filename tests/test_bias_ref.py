"""CPU tests of tests/bias_ref.py, the restatement the GPU tests hold the logit-bias kernel and the decode loops to,
and of the ABI the feature adds.  No device is touched."""
import os
import re

import numpy as np

import bias_ref as B
import dry_ref as D
import grammar_ref as G
import penalty_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- hand-worked rows
# logits by bit pattern: a quiet NaN with a payload, a negative NaN, +0, -0, +inf, -inf, 1.5, the smallest subnormal, the largest
# negative subnormal, the smallest normal, -2.25
ROW = f32([0x7FC01234, 0xFFC00001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x3FC00000, 0x00000001, 0x807FFFFF, 0x00800000, 0xC0100000])


def test_tokens_off_the_set_keep_their_bits():
    out = B.apply(ROW, [6], [1.0])
    assert bits(out)[6] == 0x40200000                                          # 1.5 + 1 = 2.5
    assert np.array_equal(np.delete(bits(out), 6), np.delete(bits(ROW), 6))     # NaN payloads, -0 and the subnormals included
    assert bits(ROW)[6] == 0x3FC00000, "the input is not modified"


def test_a_ban_is_a_ban_whatever_the_logit():
    out = B.apply(ROW, [0, 1, 4, 5, 6, 3], [-INF] * 6)
    assert all(bits(out)[t] == 0xFF800000 for t in (0, 1, 4, 5, 6, 3))          # on NaN, on +inf (not NaN), on -inf, on a finite logit
    assert np.array_equal(bits(out)[[2, 7, 8, 9, 10]], bits(ROW)[[2, 7, 8, 9, 10]])


def test_a_finite_bias_is_one_f32_addition():
    out = B.apply(ROW, [2, 3, 7, 8, 9, 4, 5, 0, 10], [-0.0, 0.0, f32(0x00000001), f32(0x007FFFFF), -f32(0x00800000), -1e30, 1e30, 2.0, 0.75])
    got = bits(out)
    assert got[2] == 0x00000000                                                 # +0 + -0 = +0
    assert got[3] == 0x00000000                                                 # -0 + +0 = +0 (round to nearest)
    assert got[7] == 0x00000002                                                 # subnormal + subnormal, exact
    assert got[8] == 0x00000000                                                 # -max subnormal + max subnormal = +0
    assert got[9] == 0x00000000                                                 # min normal - min normal = +0
    assert got[4] == 0x7F800000 and got[5] == 0xFF800000                        # +-inf stay +-inf under a finite bias
    assert np.isnan(out[0]) and np.isnan(out[1])                                # NaN stays NaN
    assert got[10] == 0xBFC00000                                                # -2.25 + 0.75 = -1.5
    assert B.apply(f32([0x80000000]), [0], [-0.0]).view(np.uint32)[0] == 0x80000000      # -0 + -0 = -0
    big = B.apply(np.array([3e38], np.float32), [0], [3e38])
    assert bits(big)[0] == 0x7F800000                                           # overflow rounds to +inf, as the addition does


def test_the_empty_set_and_none_are_the_identity():
    assert np.array_equal(bits(B.apply(ROW, [], [])), bits(ROW))
    assert np.array_equal(bits(B.apply(ROW, None, None)), bits(ROW))
    assert B.apply(ROW, None, None) is not ROW


# ----------------------------------------------------------------------------- composition, in the contract's order
def chain(row, ids, vals, counts, flags, ap, af, window, dry, cls, trans, state):
    x = B.apply(row, ids, vals)
    x = R.penalize(x, counts, flags, ap, af)
    x = D.dry_row(x, window, **dry)
    return G.mask(x, cls, trans, state)


def test_composition_bias_then_penalties_then_dry_then_mask():
    V = 8
    row = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0], np.float32)
    counts = np.array([0, 2, 0, 1, 0, 0, 0, 3], np.float32)
    flags = np.array([0, 1, 0, 1, 0, 0, 0, 1], np.uint32)
    window = [5, 6, 2, 5, 6]                                                    # token 2 would extend the repeat "5 6" (M = 2)
    dry = dict(multiplier=1.0, base=2.0, allowed_length=2)
    cls = np.arange(V, dtype=np.uint16)
    trans = np.zeros((1, V), np.uint16)
    trans[0, 4] = G.REJECT
    out = chain(row, [1, 2, 7, 4, 6], [0.5, 0.25, -INF, 100.0, -1.0], counts, flags, 0.5, 0.25, window, dry, cls, trans, 0)
    want = np.array([1.0,                                                       # untouched
                     (2.0 + 0.5) - (0.5 + 2 * 0.25),                            # (x + v) - t
                     (3.0 + 0.25) - 1.0,                                        # bias, then DRY's pen[2] = 1 * 2 ** 0
                     4.0 - (0.5 + 1 * 0.25),                                    # penalty alone
                     -np.inf,                                                   # the mask beats a bias of +100
                     6.0,
                     6.0,                                                       # 7 - 1
                     -np.inf], np.float32)                                      # banned by the set, then "penalised": -inf - t = -inf
    assert np.array_equal(bits(out), bits(want))


def test_the_order_of_rounding_is_bias_then_penalty():
    # (x + v) - t and (x - t) + v differ in f32 for these values: the contract is the first
    x, v, t = np.float32(1.0), np.float32(2.0 ** -24), np.float32(1.0)
    first = np.float32(np.float32(x + v) - t)
    second = np.float32(np.float32(x - t) + v)
    assert first != second
    counts, flags = np.array([1.0], np.float32), np.array([1], np.uint32)
    out = R.penalize(B.apply(np.array([x]), [0], [v]), counts, flags, 0.0, 1.0)
    assert out[0] == first


# ----------------------------------------------------------------------------- mutants that the row cases must reject
def mutant_ban_by_addition(row, ids, vals):
    out = np.array(row, np.float32, copy=True)
    with np.errstate(invalid="ignore"):
        for t, v in zip(ids, vals):
            out[t] = out[t] + np.float32(v)
    return out


def mutant_twice(row, ids, vals):
    return B.apply(B.apply(row, ids, vals), ids, vals)


def mutant_rewrite_all(row, ids, vals):
    dense = np.zeros(len(row), np.float32)
    out = np.array(row, np.float32, copy=True)
    ban = np.zeros(len(row), bool)
    for t, v in zip(ids, vals):
        dense[t], ban[t] = (0.0, True) if v == -np.inf else (v, False)
    with np.errstate(invalid="ignore"):
        out = (out + dense).astype(np.float32)
    out[ban] = -np.inf
    return out


def test_mutants_are_rejected_by_the_row_cases():
    ids, vals = [4, 6, 3], [-INF, 1.0, 0.0]
    want = B.apply(ROW, ids, vals)
    # a ban computed as x + (-inf): NaN on the +inf logit
    assert not np.array_equal(bits(mutant_ban_by_addition(ROW, ids, vals)), bits(want))
    assert np.isnan(mutant_ban_by_addition(ROW, ids, vals)[4]) and bits(want)[4] == 0xFF800000
    # an entry applied twice
    assert bits(mutant_twice(ROW, ids, vals))[6] == 0x40600000 != bits(want)[6]
    # the off-set tokens rewritten as x + 0: -0 becomes +0 (a NaN payload may survive an addition, the sign of zero does not)
    assert bits(mutant_rewrite_all(ROW, [6], [1.0]))[3] == 0x00000000 != bits(B.apply(ROW, [6], [1.0]))[3]
    # bias applied after the penalties: the other order of rounding
    x, v = np.float32(1.0), np.float32(2.0 ** -24)
    counts, flags = np.array([1.0], np.float32), np.array([1], np.uint32)
    after = B.apply(R.penalize(np.array([x]), counts, flags, 0.0, 1.0), [0], [v])
    right = R.penalize(B.apply(np.array([x]), [0], [v]), counts, flags, 0.0, 1.0)
    assert after[0] != right[0]
    # ... and a ban of the table's is lifted by nothing, but a bias applied after a DRY ban would be -inf + v = -inf either way: the
    # place in the chain shows where the grammar's mask meets a positive bias
    cls, trans = np.arange(2, dtype=np.uint16), np.array([[0, G.REJECT]], np.uint16)
    assert G.mask(B.apply(np.zeros(2, np.float32), [1], [5.0]), cls, trans, 0)[1] == -np.inf
    assert B.apply(G.mask(np.zeros(2, np.float32), cls, trans, 0), [1], [5.0])[1] == -np.inf       # -inf + 5: also -inf ...
    assert B.apply(G.mask(np.zeros(2, np.float32), cls, trans, 0), [0], [5.0])[0] == 5.0           # ... the allowed token is biased


# ----------------------------------------------------------------------------- validation
def test_check_sets():
    V = 6
    ok = ([0, 2, 2, 5], [1, 4, 0, 5, 3], [0.5, -INF, -3.0, -INF, 0.0])
    assert B.check_sets(V, *ok) == "ok"                                         # an empty set in the middle
    assert B.check_sets(V, [0, 0], [], []) == "ok"                              # one empty set
    assert B.check_sets(V, None, [], []) == "arg"                               # NULL arrays, even where nothing would be read
    assert B.check_sets(V, [0, 1], None, [1.0]) == "arg" and B.check_sets(V, [0, 0], [], None) == "arg"
    assert B.check_sets(V, [0], [], []) == "arg"                                # num_sets 0
    assert B.check_sets(V, [1, 2], [0, 1], [0.0, 0.0]) == "arg"                 # offsets that do not start at 0
    assert B.check_sets(V, [0, 2, 1], [0, 1], [0.0, 0.0]) == "arg"              # offsets that decrease
    assert B.check_sets(V, [0, 1], [V], [0.0]) == "arg"                         # an id >= num_vocab
    assert B.check_sets(V, [0, 2], [3, 3], [0.0, 1.0]) == "arg"                 # the same id twice in one set
    assert B.check_sets(V, [0, 1, 2], [3, 3], [0.0, 1.0]) == "ok"               # ... in two sets it is fine
    assert B.check_sets(V, [0, 1], [0], [np.nan]) == "arg" and B.check_sets(V, [0, 1], [0], [np.inf]) == "arg"
    assert B.check_sets(V, [0, V], list(range(V)), [-INF] * V) == "arg"         # a set that bans every token
    assert B.check_sets(V, [0, V], list(range(V)), [-INF] * (V - 1) + [-1e30]) == "ok"
    assert B.check_sets(2 ** 20, [0, 0], [], []) == "ok" and B.check_sets(2 ** 20 + 1, [0, 0], [], []) == "unsupported"
    assert B.check_sets(V, [0] * (B.MAX_SETS + 1), [], []) == "ok" and B.check_sets(V, [0] * (B.MAX_SETS + 2), [], []) == "arg"
    assert B.check_set_words(3, [0, 2, B.NONE]) and not B.check_set_words(3, [3]) and not B.check_set_words(3, [B.NONE - 1])


# ----------------------------------------------------------------------------- the ABI
NEW_FIELDS = ["bias", "bias_set"]
NEW_SYMBOLS = {"wrk_logit_bias_create": 7, "wrk_logit_bias_destroy": 1, "wrk_bias_logits": 7}


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wrk_hip.h")).read(), flags=re.S)


def test_option_fields_match_the_ctypes_mirror():
    import wrk
    for cname, cls in (("wrk_generate_options", wrk.GenerateOptions), ("wrk_queue_options", wrk.QueueOptions)):
        body = re.search(r"typedef\s+struct\s+" + cname + r"\s*\{(.*?)\}", header(), flags=re.S).group(1)
        names = [n for stmt in body.split(";") if stmt.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", stmt.strip())]
        assert names == [n for n, _ in cls._fields_], cname
        at = names.index("occ")
        assert names[at + 1:at + 3] == NEW_FIELDS, cname                            # directly behind occ
        assert dict(cls._fields_)["bias"] is wrk._P and dict(cls._fields_)["bias_set"] is wrk._u32p
        assert not cls().bias and not cls().bias_set                                # NULL in a zeroed struct: off
    assert wrk.hip.wrk_abi_version() == 1


def test_entry_points_and_constants_are_declared_exported_and_bound():
    import wrk
    text = header()
    declared = set(re.findall(r"\b(wrk_[a-z0-9_]+)\s*\(", text))
    for name, nargs in NEW_SYMBOLS.items():
        assert name in declared and hasattr(wrk.hip, name) and name in wrk.HIP_SYMBOLS, name
        assert len(wrk.HIP_SYMBOLS[name][1]) == nargs, name
    assert re.search(r"#define\s+WRK_BIAS_NONE\s+0xFFFFFFFFu", text) and wrk.BIAS_NONE == B.NONE == wrk.LogitBias.NONE == 0xFFFFFFFF
    assert int(re.search(r"#define\s+WRK_MAX_BIAS_SETS\s+(\d+)", text).group(1)) == wrk.MAX_BIAS_SETS == B.MAX_SETS == 65536
    assert callable(wrk.Context.bias_logits) and callable(wrk.LogitBias.close)
    for fn in ("generate_greedy", "generate_sample", "generate_penalized", "generate_stop", "generate_queue"):
        code = getattr(wrk.Runtime, fn).__code__
        assert {"logit_bias", "bias_set"} <= set(code.co_varnames[:code.co_argcount]), fn


def test_bias_csr_of_dicts_and_pairs():
    import wrk
    off, ids, vals = wrk._bias_csr([{5: -np.inf, 2: 1.5}, {}, ([7], [0.25])])
    assert off.tolist() == [0, 2, 2, 3] and ids.tolist() == [5, 2, 7] and off.dtype == ids.dtype == np.uint32
    assert vals.dtype == np.float32 and vals.tolist() == [-np.inf, 1.5, 0.25]
    assert B.check_sets(8, off, ids, vals) == "ok"
    off, ids, vals = wrk._bias_csr([{}])
    assert off.tolist() == [0, 0] and ids.size == 0 and vals.size == 0
