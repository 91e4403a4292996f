"""Hand-worked groups of the beam step (the contract of wrk_v7_generate_beam in include/wrk_hip.h), shared by tests/test_beam_ref.py, which
checks tests/beam_ref.py against them, and tests/test_beam_select_host.py, which checks the C++ rule against them.  Every value is exact in
f32; expectations are written out slot by slot, never computed by the code under test.

A case: W, alpha (length_penalty), stop ids, slots [(score, key, length, status)], rows [[(id, lp)] * W] and `want`: per slot
(score, key, length, status, token, parent, ended)."""
import numpy as np

DEAD, LIVE, DONE = 0, 1, 2
NO = 0xFFFFFFFF
INF = float("inf")
NAN = float("nan")
_dead = (-INF, -INF, 0, DEAD)
_none = [(0, -INF)]

# f32(1/3) = 0x3EAAAAAB = 0.33333334327: -3.75 * it = -1.2500000373, below the midpoint 1.2500000596 of (1.25, 1.25 + 2^-23): -1.25;
# -4.5 * it = -1.5000000447: -1.5.
# f32(1/7) = 0x3E124925 = 0.14285714924: -5.25 * it = -0.7500000335, above the midpoint 0.7500000298 of (0.75, 0.75 + 2^-24):
# -0.75000006 = 0xBF400001, where -5.25 / 7 = -0.75 = 0xBF400000 exactly; -7 * it = -1.0000000447, below the midpoint 1.0000000596: -1.
KEY_MUL_7 = float(np.array([0xBF400001], np.uint32).view(np.float32)[0])

CASES = {
    # equal keys from two slots: the lower slot of origin first; nothing moves
    "tie_by_slot": dict(W=2, alpha=0.0, stop=[], slots=[(0.0, 0.0, 3, LIVE), (-0.5, -0.5, 3, LIVE)],
                        rows=[[(10, -1.0), (11, -1.5)], [(20, -0.5), (21, -1.0)]],
                        want=[(-1.0, -1.0, 4, LIVE, 10, 0, 0), (-1.0, -1.0, 4, LIVE, 20, 1, 0)]),
    # equal keys from one slot: j ascending; slot 1 takes slot 0's state
    "tie_by_j": dict(W=2, alpha=0.0, stop=[], slots=[(0.0, 0.0, 1, LIVE), (-4.0, -4.0, 1, LIVE)],
                     rows=[[(5, -1.0), (7, -1.0)], [(8, -0.5), (9, -0.5)]],
                     want=[(-1.0, -1.0, 2, LIVE, 5, 0, 0), (-1.0, -1.0, 2, LIVE, 7, 0, 0)]),
    # order: (0,0) -1.5, (3,0) -1.75, then -2.0 twice: candidate (0,1) of slot 0 before the DONE slot 1; the DONE slot 2 (-8) is pushed out.
    # slot 1 stays; slots 0, 2, 3 take (0,0) = 99: a stop id, DONE; (3,0) = 31: a stop id, DONE in the freed slot 2; (0,1) = 12: LIVE.
    # slot 3 is source (of slot 2) and destination (from slot 0) in one step
    "done_stays_and_pushed_out": dict(W=4, alpha=0.0, stop=[99, 31],
                                      slots=[(-1.0, -1.0, 2, LIVE), (-2.0, -2.0, 2, DONE), (-8.0, -8.0, 1, DONE), (-1.5, -1.5, 2, LIVE)],
                                      rows=[[(99, -0.5), (12, -1.0), (13, -4.0), (14, -5.0)], _none * 4, _none * 4,
                                            [(31, -0.25), (32, -1.0), (33, -3.0), (34, -7.0)]],
                                      want=[(-1.5, -1.5, 3, DONE, 99, 0, 1), (-2.0, -2.0, 2, DONE, NO, 1, 0), (-1.75, -1.75, 3, DONE, 31, 3, 1),
                                            (-2.0, -2.0, 3, LIVE, 12, 0, 0)]),
    # the start of a call, and a row with two finite logits: -inf and NaN log-probs are no candidates; two slots become DEAD
    "fewer_than_w": dict(W=4, alpha=0.0, stop=[], slots=[(0.0, 0.0, 0, LIVE), _dead, _dead, _dead],
                         rows=[[(3, -0.5), (4, -1.0), (5, -INF), (6, NAN)], _none * 4, _none * 4, _none * 4],
                         want=[(-0.5, -0.5, 1, LIVE, 3, 0, 0), (-1.0, -1.0, 1, LIVE, 4, 0, 0), _dead + (NO, 2, 0), _dead + (NO, 3, 0)]),
    # length_penalty 0: keys are the raw scores: the DONE slot (-2) leads, (0,0) = -3.75 follows
    "penalty_0": dict(W=2, alpha=0.0, stop=[], slots=[(-3.0, -3.0, 2, LIVE), (-2.0, -2.0, 1, DONE)],
                      rows=[[(7, -0.75), (8, -1.5)], _none * 2],
                      want=[(-3.75, -3.75, 3, LIVE, 7, 0, 0), (-2.0, -2.0, 1, DONE, NO, 1, 0)]),
    # length_penalty 1, the same group: keys -3.75 / 3 = -1.25 and -4.5 / 3 = -1.5 both beat the DONE slot's -2, which is pushed out
    "penalty_1": dict(W=2, alpha=1.0, stop=[], slots=[(-3.0, -1.5, 2, LIVE), (-2.0, -2.0, 1, DONE)],
                      rows=[[(7, -0.75), (8, -1.5)], _none * 2],
                      want=[(-3.75, -1.25, 3, LIVE, 7, 0, 0), (-4.5, -1.5, 3, LIVE, 8, 0, 0)]),
    # key = raw * inv_norm[7], not raw / 7: -5.25 gives 0xBF400001, so the DONE slot's -0.75 = 0xBF400000 leads (division would tie)
    "key_is_a_product": dict(W=2, alpha=1.0, stop=[], slots=[(-5.0, -5.0 / 6, 6, LIVE), (-3.0, -0.75, 4, DONE)],
                             rows=[[(40, -0.25), (41, -1.75)], _none * 2],
                             want=[(-5.25, KEY_MUL_7, 7, LIVE, 40, 0, 0), (-3.0, -0.75, 4, DONE, NO, 1, 0)]),
    # W = 1 is greedy with a score; the stop id ends it
    "w1": dict(W=1, alpha=0.0, stop=[], slots=[(-2.5, -2.5, 5, LIVE)], rows=[[(77, -0.125)]], want=[(-2.625, -2.625, 6, LIVE, 77, 0, 0)]),
    "w1_stop": dict(W=1, alpha=0.0, stop=[77], slots=[(-2.5, -2.5, 5, LIVE)], rows=[[(77, -0.125)]], want=[(-2.625, -2.625, 6, DONE, 77, 0, 1)]),
    "w1_done": dict(W=1, alpha=0.0, stop=[77], slots=[(-2.625, -2.625, 6, DONE)], rows=[_none], want=[(-2.625, -2.625, 6, DONE, NO, 0, 0)]),
}


def arrays(case):
    """(score, key, length, status, ids [W][W], lp [W][W]) of a case as the arrays the rule takes"""
    s = case["slots"]
    score, key = np.array([x[0] for x in s], np.float32), np.array([x[1] for x in s], np.float32)
    length, status = np.array([x[2] for x in s], np.uint32), np.array([x[3] for x in s], np.uint32)
    ids = np.array([[p[0] for p in r] for r in case["rows"]], np.uint32)
    lp = np.array([[p[1] for p in r] for r in case["rows"]], np.float32)
    return score, key, length, status, ids, lp


def want_words(case):
    """the expectation as words: slots [W * 4] (score bits, key bits, length, status), token [W], parent [W], ended [W]"""
    f = lambda x: int(np.array([x], np.float32).view(np.uint32)[0])
    w = case["want"]
    slots = [v for x in w for v in (f(x[0]), f(x[1]), x[2], x[3])]
    return dict(slots=slots, token=[x[4] for x in w], parent=[x[5] for x in w], ended=[x[6] for x in w])


def got_words(out):
    """beam_ref.select_group's result in the same words"""
    W = len(out["status"])
    sb, kb = out["score"].astype(np.float32).view(np.uint32), out["key"].astype(np.float32).view(np.uint32)
    slots = [int(v) for q in range(W) for v in (sb[q], kb[q], out["length"][q], out["status"][q])]
    return dict(slots=slots, token=[int(x) for x in out["token"]], parent=[int(x) for x in out["parent"]], ended=[int(x) for x in out["ended"]])
