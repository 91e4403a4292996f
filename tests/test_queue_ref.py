"""Hand-worked cases of tests/queue_ref.py, and the declared-symbol check of the two queue entry points (no GPU)."""
import os
import re

import numpy as np

import queue_ref as Q
import wrk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows(prompt_lens, lengths, B, max_steps=None):
    got, needed = Q.schedule(prompt_lens, lengths, B, max_steps)
    return [(r["slot"], r["start_step"], r["length"], r["cut"]) for r in got], needed


def test_two_slots_ending_in_the_same_step_take_requests_in_slot_order():
    # slot 0: prompt 2 + reply 2 -> draws at steps 1, 2; slot 1: prompt 1 + reply 3 -> draws at steps 0, 1, 2: both end in step 2
    got, needed = rows([2, 1, 1, 1], [2, 3, 1, 2], 2)
    assert got == [(0, 0, 2, False), (1, 0, 3, False), (0, 3, 1, False), (1, 3, 2, False)]
    assert needed == 5                              # request 3 draws at steps 3 and 4


def test_fewer_requests_than_slots():
    got, needed = rows([3, 1], [1, 4], 4)
    assert got == [(0, 0, 1, False), (1, 0, 4, False)]
    assert needed == 4


def test_prompt_of_length_one_draws_its_reply_in_the_step_that_feeds_it():
    got, needed = rows([1], [3], 1)
    assert got == [(0, 0, 3, False)] and needed == 3


def test_max_new_one_and_a_slot_serving_three_requests_in_a_row():
    # one slot: r0 feeds at 0, 1 and draws y_0 at 1; r1 feeds at 2 and draws at 2; r2 feeds at 3, 4, 5 and draws at 5, 6
    got, needed = rows([2, 1, 3], [1, 1, 2], 1)
    assert got == [(0, 0, 1, False), (0, 2, 1, False), (0, 3, 2, False)]
    assert needed == 7


def test_a_stop_on_the_first_reply_token():
    assert Q.reply_length([9, 4, 5], [9], 3) == (1, Q.STOP)
    assert Q.reply_length([1, 4, 5], [5, 8], 3) == (3, Q.STOP)         # stop on the last allowed token: the stop wins
    assert Q.reply_length([1, 4, 5], [5], 2) == (2, Q.MAX_NEW)
    assert Q.reply_length([1, 4, 5], [], 3) == (3, Q.MAX_NEW)
    out, needed = Q.run([[7, 7], [8]], [[9, 4, 5], [1, 2]], [[9], []], [3, 2], 1)
    assert [(t.tolist(), why, slot, start) for t, why, slot, start in out] == [([9], Q.STOP, 0, 0), ([1, 2], Q.MAX_NEW, 0, 2)]
    assert needed == 4


def test_a_cap_that_cuts_a_request():
    # one slot: r0 (prompt 2, reply 3) draws at steps 1, 2, 3; r1 starts at 4 with a prompt of 2; r2 never starts
    full, needed = rows([2, 2, 1], [3, 2, 1], 1)
    assert full == [(0, 0, 3, False), (0, 4, 2, False), (0, 7, 1, False)] and needed == 8
    got, _ = rows([2, 2, 1], [3, 2, 1], 1, max_steps=3)
    assert got == [(0, 0, 2, True), (None, None, 0, False), (None, None, 0, False)]
    got, _ = rows([2, 2, 1], [3, 2, 1], 1, max_steps=5)                 # r1 is still in its prompt: dispatched, nothing drawn yet
    assert got == [(0, 0, 3, False), (0, 4, 0, True), (None, None, 0, False)]
    got, _ = rows([2, 2, 1], [3, 2, 1], 1, max_steps=4)                 # r0 ends in the last step: r1 never feeds its p_0
    assert got == [(0, 0, 3, False), (None, None, 0, False), (None, None, 0, False)]
    out, _ = Q.run([[1, 2], [3, 4], [5]], [[6, 7, 8], [9, 9], [3]], [[], [], []], [3, 2, 1], 1, max_steps=3)
    assert [(t.tolist(), why, slot, start) for t, why, slot, start in out] == [([6, 7], Q.CAP, 0, 0), ([], Q.NEVER, 0, 0), ([], Q.NEVER, 0, 0)]


def test_steps_run_bound():
    assert Q.steps_run_bound(5, 2, 100) == (3 + 2) * 2
    assert Q.steps_run_bound(5, 2, 6) == 6
    assert Q.steps_run_bound(1, 16, 1000) == 48


def test_steps_run_is_one_block_past_the_last_end():
    # poll 2, the last request ends in step 4 (needed 5): blocks 0..2 cover it, the host reads block 2's live count before block 4,
    # so blocks 0..3 run
    assert Q.steps_run(5, 2, 100) == 8
    assert Q.steps_run(4, 2, 100) == 6                     # ends with the last step of block 1: blocks 0..2 run
    assert Q.steps_run(5, 2, 7) == 7                       # the cap cuts the last block
    assert Q.steps_run(1, 16, 1000) == 32
    assert Q.steps_run(50, 4, 20) == 20
    for needed in range(1, 40):
        for poll in (1, 3, 4, 16):
            assert needed <= Q.steps_run(needed, poll, 10 ** 6) <= Q.steps_run_bound(needed, poll, 10 ** 6)


def test_queue_entry_points_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "wrk_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(wrk_[a-z0-9_]+)\s*\(", text))
    for name in ("wrk_v7_generate_queue", "wrk_v6_generate_queue"):
        assert name in declared, f"{name} is not declared in include/wrk_hip.h"
        assert hasattr(wrk.hip, name), f"{name} is not exported"
        assert name in wrk.HIP_SYMBOLS, f"{name} has no ctypes signature"
        assert len(wrk.HIP_SYMBOLS[name][1]) == 8
    # the ctypes structures follow the header's field order
    for cname, cls in (("wrk_queue_options", wrk.QueueOptions), ("wrk_queue_result", wrk.QueueResult)):
        body = re.search(r"typedef\s+struct\s+" + cname + r"\s*\{(.*?)\}", text, flags=re.S).group(1)
        names = [n for stmt in body.split(";") if stmt.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", stmt.strip())]
        assert names == [n for n, _ in cls._fields_], cname
    assert hasattr(wrk.Runtime, "generate_queue")
    assert wrk.hip.wrk_abi_version() == 1
