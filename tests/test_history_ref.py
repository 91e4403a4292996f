"""Hand-worked cases of tests/history_ref.py, the validation errors, and the ABI's new fields and entry points (no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import history_ref as H
import queue_ref as Q
import wrk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 8
ONES = np.ones(V, np.float32)


def flags_of(present=(), banned=()):
    f = np.zeros(V, np.uint32)
    f[list(present)] |= H.PRESENT
    f[list(banned)] |= H.BANNED
    return f


# ----------------------------------------------------------------------------------------------------------------- prompt intake
def test_a_repeated_prompt_token_with_decay_one_half():
    # prompt 3 5 3, f = 0, decay 0.5, weights 1, cold start.  By hand:
    #   3 enters: counts * 0.5 = 0, count[3] = 1
    #   5 enters: count[3] = 0.5, count[5] = 1
    #   3 enters: count[3] = 0.25 + 1 = 1.25, count[5] = 0.5
    counts, flags, window = H.context_before_draw(flags_of(), None, [3, 5, 3], 0, [], 0, ONES, 0.5, 4)
    want = np.zeros(V, np.float32)
    want[3], want[5] = 1.25, 0.5
    assert np.array_equal(counts, want) and flags.tolist() == flags_of(present=[3, 5]).tolist() and window == [3, 5, 3]
    # the row of y_1 has also counted y_0 = 5: count[3] = 0.625, count[5] = 0.25 + 1
    counts, flags, window = H.context_before_draw(flags_of(), None, [3, 5, 3], 0, [5, 1], 1, ONES, 0.5, 4)
    want[3], want[5] = 0.625, 1.25
    assert np.array_equal(counts, want) and window == [3, 5, 3, 5]


def test_a_prompt_longer_than_the_window_wraps_the_ring():
    # capacity 4, six prompt tokens: the two oldest are dropped, the order of the rest is kept; every token is still counted
    counts, flags, window = H.context_before_draw(flags_of(), None, [1, 2, 3, 4, 5, 6], 0, [], 0, ONES, 1.0, 4)
    assert window == [3, 4, 5, 6]
    assert counts.tolist() == [0, 1, 1, 1, 1, 1, 1, 0]
    # one draw more drops the 3
    _, _, window = H.context_before_draw(flags_of(), None, [1, 2, 3, 4, 5, 6], 0, [7, 0], 1, ONES, 1.0, 4)
    assert window == [4, 5, 6, 7]


def test_the_offset_says_where_the_intake_begins():
    prompt = [4, 4, 6]
    assert H.events(prompt, 0, [2]) == [("prompt", 4), ("prompt", 4), ("prompt", 6), ("draw", 2)]
    assert H.events(prompt, 1, [2]) == [("prompt", 4), ("prompt", 6), ("draw", 2)]
    assert H.events(prompt, 3, [2]) == H.events(prompt, 99, [2]) == H.events(prompt, None, [2]) == [("draw", 2)]
    c0 = H.context_before_draw(flags_of(), None, prompt, 0, [], 0, ONES, 1.0, 4)
    c1 = H.context_before_draw(flags_of(), None, prompt, 1, [], 0, ONES, 1.0, 4)
    c3 = H.context_before_draw(flags_of(), None, prompt, 3, [], 0, ONES, 1.0, 4)
    assert c0[0][4] == 2 and c1[0][4] == 1 and c3[0][4] == 0
    assert c0[2] == [4, 4, 6] and c1[2] == [4, 6] and c3[2] == []
    # f = 1 is what a continued turn passes: the entry has counted y_last as a draw, and the turn's prompt opens with it
    entry = H.entry_of(H.context_before_draw(flags_of(), None, [1], 0, [7, 4], 2, ONES, 1.0, 4))        # has seen 1, 7, 4
    counts, _, window = H.context_before_draw(flags_of(), entry, [4, 6], 1, [], 0, ONES, 1.0, 4)
    assert counts[4] == 1 and window == [1, 7, 4, 6]


def test_bans_are_the_slots_and_never_enter_an_entry():
    slot = flags_of(present=[0, 1], banned=[1, 2])
    entry = (np.arange(V, dtype=np.float32), flags_of(present=[5]), [5])
    counts, flags, window = H.begin(slot, entry)
    assert flags.tolist() == flags_of(present=[5], banned=[1, 2]).tolist() and counts[7] == 7 and window == [5]
    counts, flags, window = H.begin(slot, None)
    assert flags.tolist() == flags_of(banned=[1, 2]).tolist() and not counts.any() and window == []
    ctx = H.take(H.begin(slot, entry), 2, ONES, 1.0, 4)
    _, present, _ = H.entry_of(ctx)
    assert present.tolist() == flags_of(present=[2, 5]).tolist()


# ----------------------------------------------------------------------------------------------------------------- the pool
def entries(n):
    out = []
    for k in range(n):
        c = np.zeros(V, np.float32)
        c[k] = 10 + k
        out.append((c, flags_of(present=[k]), [k]))
    return out


def test_start_equals_save_reads_before_it_writes():
    # one request, in place on entry 1: it begins with what the entry held, and leaves that plus its prompt tail and its draws
    E = entries(2)
    got, after, written = H.run([[6, 3]], [[2, 2]], [[]], [2], 1, [1], [1], E, [flags_of(banned=[7])], [1], ONES, [1.0], 4)
    assert written == {1: 0} and got[0][1] == Q.MAX_NEW
    c, p, w = after[1]
    assert c.tolist() == [0, 11, 2, 1, 0, 0, 0, 0] and p.tolist() == flags_of(present=[1, 2, 3]).tolist() and w == [1, 3, 2, 2]
    assert np.array_equal(after[0][0], E[0][0]) and after[0][2] == [0]                       # the other entry keeps its bits


def test_two_readers_of_an_entry_nobody_saves():
    E = entries(3)
    got, after, written = H.run([[1], [1]], [[4], [5]], [[], []], [1, 1], 2, [0, 0], [1, 2], E, [flags_of(), flags_of()], None, ONES,
                                [1.0, 0.5], 4)
    assert written == {1: 0, 2: 1}
    assert after[0][2] == [0] and after[0][0][0] == 10                                        # read twice, unchanged
    assert after[1][2] == [0, 4] and after[1][0][0] == 10 and after[1][0][4] == 1
    assert after[2][2] == [0, 5] and after[2][0][0] == 5 and after[2][0][5] == 1              # its own decay


def test_cut_and_never_dispatched_requests_write_nothing():
    E = entries(3)
    # one slot, three steps: request 0 ends (stop), request 1 is cut after one draw, request 2 is never dispatched
    got, after, written = H.run([[1], [2], [3]], [[4], [5, 6, 7], [1]], [[4], [], []], [3, 3, 1], 1, [None] * 3, [0, 1, 2], E,
                                [flags_of()], [0, 0, 0], ONES, [1.0] * 3, 4, max_steps=3)
    assert [why for _, why, *_ in got] == [Q.STOP, Q.CAP, Q.NEVER] and written == {0: 0}
    assert after[0][2] == [1, 4]
    for k in (1, 2):
        assert np.array_equal(after[k][0], E[k][0]) and after[k][2] == E[k][2]


def test_validation():
    ok = dict(start=[0, None], save=[0, 1], state_entries=2, history_entries=2, history_capacity=4, has_pool=True, has_occ=True,
              window_capacity=4, count_prompt=[1, 0])
    H.validate(**ok)
    H.validate(**(ok | dict(has_occ=False)))                                     # a window alone will do
    H.validate(**(ok | dict(window_capacity=None, history_capacity=0)))          # and so will a table alone
    H.validate(**(ok | dict(history_entries=None, has_pool=False)))              # intake without any pool
    bad = [(dict(has_pool=False), "without a state pool"), (dict(has_occ=False, window_capacity=None, history_capacity=0, count_prompt=None), "needs an occurrence"),
           (dict(history_entries=3), "3 entries"), (dict(history_capacity=8), "capacity 8"), (dict(history_capacity=0), "without windows"),
           (dict(window_capacity=None), "no token window"), (dict(has_occ=False, window_capacity=None, history_entries=None), "count_prompt needs"),
           (dict(save=[0, 0]), "both save"), (dict(start=[1, None]), "which request")]
    for change, what in bad:
        with pytest.raises(ValueError, match=what):
            H.validate(**(ok | change))


# ----------------------------------------------------------------------------------------------------------------- the ABI
def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wrk_hip.h")).read(), flags=re.S)


def fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header(), flags=re.S).group(1)
    names = []
    for stmt in body.split(";"):
        names += [d.replace("*", "").split()[-1] for d in stmt.split(",") if d.strip()]
    return names


def test_the_new_fields_sit_where_the_header_says():
    want = fields("wrk_queue_options")
    at = want.index("prompt_context_from")
    assert want[at - 1] == "max_steps" and want[at + 1:at + 3] == ["history", "num_top"] and want[-2:] == ["top_k", "min_p"]
    assert [n for n, _ in wrk.QueueOptions._fields_] == want
    # the pool struct keeps its five fields: the history pool travels with the options, NULL in a zeroed struct
    assert fields("wrk_queue_pool") == [n for n, _ in wrk.QueuePool._fields_] == ["states", "num_entries", "start", "save", "saved"]
    assert not wrk.QueueOptions().history and not wrk.QueueOptions().prompt_context_from


def test_the_history_pool_entry_points_are_declared_and_exported():
    for name in ("create", "destroy", "load", "back", "put", "get"):
        assert re.search(r"\bwrk_history_pool_%s\s*\(" % name, header()), name
        assert hasattr(wrk.hip, "wrk_history_pool_" + name) and "wrk_history_pool_" + name in wrk.HIP_SYMBOLS
    assert callable(wrk.HistoryPool.put) and callable(wrk.HistoryPool.get)


def test_history_and_count_prompt_are_arguments_of_generate_queue():
    import inspect
    sig = inspect.signature(wrk.Runtime.generate_queue)
    assert sig.parameters["count_prompt"].default is None and sig.parameters["history"].default is None
