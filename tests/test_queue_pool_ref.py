"""Hand-worked cases of tests/queue_pool_ref.py, and the declared-symbol check of the two pool entry points (no GPU)."""
import ctypes as C
import os
import re

import pytest

import queue_pool_ref as P
import wrk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_shared_read_only_entry_is_accepted():
    # three replies from one prefix: all read entry 0, nobody saves to it; two of them keep their end states elsewhere
    P.validate([0, 0, 0], [None, 1, 2], 3)
    P.validate([0, 0, 0], [None, None, None], 1)


def test_an_in_place_entry_is_accepted():
    # every conversation has its own entry: the read at a request's start precedes the write at its end
    P.validate([0, 1, 2], [0, 1, 2], 3)
    P.validate([2, None, 0], [2, 1, 0], 3)


def test_two_savers_of_one_entry_are_rejected():
    with pytest.raises(ValueError, match="both save"):
        P.validate([None, None], [1, 1], 2)
    with pytest.raises(ValueError, match="both save"):
        P.validate([0, 1, 2], [0, 2, 2], 3)          # request 2 in place, request 1 onto the same entry


def test_a_reader_of_another_requests_save_target_is_rejected():
    # whether request 1 saw entry 0 before or after request 0's end would depend on the schedule
    with pytest.raises(ValueError, match="request 1 starts from entry 0, which request 0 saves to"):
        P.validate([None, 0], [0, None], 1)
    with pytest.raises(ValueError, match="request 0 starts from entry 1, which request 2 saves to"):
        P.validate([1, None, 1], [None, None, 1], 2)    # request 2 itself may; request 0 may not
    with pytest.raises(ValueError, match="which request"):
        P.validate([0, 1], [1, 0], 2)                   # swapped entries


def test_out_of_range_and_shape_errors_are_rejected():
    with pytest.raises(ValueError, match="start entry 3 of 3"):
        P.validate([3], [None], 3)
    with pytest.raises(ValueError, match="save entry 3 of 3"):
        P.validate([None], [3], 3)
    with pytest.raises(ValueError, match="save entry -1"):
        P.validate([None], [-1], 3)
    with pytest.raises(ValueError):
        P.validate([P.NO_ENTRY], [None], 3)             # "none" is None on this side, never the C constant
    with pytest.raises(ValueError, match="empty pool"):
        P.validate([None], [None], 0)
    with pytest.raises(ValueError):
        P.validate([None, None], [None], 2)


def test_which_entries_are_written():
    save = [4, None, 0, 2, 1, 3]
    reasons = [P.STOP, P.MAX_NEW, P.MAX_NEW, P.CAP, P.NEVER, P.STOP]
    # request 1 names no entry; request 3 was cut and request 4 never dispatched: entries 2 and 1 keep their bits
    assert P.saved(save, reasons) == [True, False, True, False, False, True]
    assert P.written(save, reasons) == {4: 0, 0: 2, 3: 5}
    assert P.written([None] * 3, [P.STOP] * 3) == {}
    assert P.written([0, 1], [P.CAP, P.NEVER]) == {}


def test_none_is_the_c_constant():
    assert wrk.QUEUE_NO_ENTRY == P.NO_ENTRY == 0xFFFFFFFF
    text = open(os.path.join(ROOT, "include", "wrk_hip.h")).read()
    assert re.search(r"#define\s+WRK_QUEUE_NO_ENTRY\s+0xFFFFFFFFu", text)


def test_the_pool_entry_points_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wrk_hip.h")).read(), flags=re.S)
    plain = re.search(r"wrk_v7_generate_queue\s*\(([^;]*)\)\s*;", text).group(1)
    for name, model in (("wrk_v7_generate_queue_pool", "wrk_v7_model"), ("wrk_v6_generate_queue_pool", "wrk_v6_model")):
        m = re.search(name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, name
        # the plain entry point's signature plus the pool
        want = " ".join(plain.split()).replace("wrk_v7_model", model) + ", const wrk_queue_pool* pool"
        assert " ".join(m.group(1).split()) == want
        assert hasattr(wrk.hip, name) and wrk.HIP_SYMBOLS[name][1][-1] == C.POINTER(wrk.QueuePool)
        assert wrk.HIP_SYMBOLS[name][1][:-1] == wrk.HIP_SYMBOLS[name.replace("_pool", "")][1]
    fields = [n for n, _ in wrk.QueuePool._fields_]
    assert fields == ["states", "num_entries", "start", "save", "saved"]
    struct = re.search(r"typedef struct wrk_queue_pool \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", struct) == fields
    assert C.sizeof(wrk.QueuePool) == 40
