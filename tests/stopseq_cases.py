"""The hand-worked stop-sequence cases shared by tests/test_stopseq_ref.py (on the CPU, against stopseq_ref and a brute force) and
tests/test_gpu_stopseq.py (scripted through a forced-chain grammar in every decode loop).  Not a test module.

Each case is the reply stream behind the first token, padded with the end token END to STEPS steps; `want` = (length, match word)
is worked out by hand from the contract, not computed."""
import stopseq_ref as Q

END = 3
STEPS = 16
NONE, TOKEN = Q.NONE, Q.TOKEN

#         name        first  stream                                              stop sequences                             stop ids  want
CASES = [("overlap",   1, [7, 7, 7, 9, 11, 12],                                   [[7, 7, 9]],                                   [],   (4, 0)),
         ("decoys",    1, [20, 21, 22, 21, 22, 20, 21, 23, 20, 21, 22, 23, 30],   [[20, 21, 22, 23]],                            [],   (12, 0)),
         ("longest",   1, [40, 41, 42, 43, 44],                                   [[42, 43], [41, 42, 43], [99, 43]],            [43], (4, 1)),
         ("never",     1, [50, 51, 52, 53, 54, 55, 56, 57, 58, 60],               [[51, 50], [52, 53, 54, 55, 56, 57, 58, 59]],  [],   (16, NONE)),
         ("full 8",    1, [60, 61, 62, 63, 64, 65, 66, 67, 68],                   [[60, 61, 62, 63, 64, 65, 66, 67]],            [],   (8, 0)),
         ("x_0",       70, [71, 72, 70, 71, 5],                                   [[70, 71]],                                    [],   (4, 0)),
         ("step 0",    1, [80, 81],                                               [[80]],                                        [],   (1, 0))]

NAMES = [c[0] for c in CASES]


def stream(i: int) -> list:
    """The STEPS draws of case i without stops."""
    s = CASES[i][2]
    return (s + [END] * STEPS)[:STEPS]


def want_tail(i: int) -> list:
    """The tail case i leaves: the last draws up to and including the one that ended it, right aligned -- a slice, not stopseq_ref."""
    n = CASES[i][5][0]
    t = stream(i)[:n][-Q.TAIL_LEN:]
    return [Q.EMPTY] * (Q.TAIL_LEN - len(t)) + t


# the decoys case split into two calls: what the first call leaves and what the second must and must not do with it
SPLIT = 10
SPLIT_TAIL = [21, 22, 20, 21, 23, 20, 21]
