"""Hand-worked cases of tests/guided_queue_ref.py (the schedule of wrk_v7_generate_queue_guided), its equality with
tests/queue_ref.py whenever no negative prompt is longer than its prompt, and the ABI of the guided queue (no GPU)."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import guided_queue_ref as G
import queue_ref as Q
import wrk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows(ns, ms, lengths, B, max_steps=None):
    """per request (slot, f, the step that feeds p_0 = the conditional half's reset step, the step that feeds q_0 = the partner's reset
    step, step_base, length, cut)"""
    got, needed = G.schedule(ns, ms, lengths, B, max_steps)
    return [(r["slot"], r["dispatch_step"], r["start_step"], r["neg_start_step"], r["step_base"], r["length"], r["cut"]) for r in got], needed


def test_negative_prompt_shorter_than_the_prompt():
    # n = 3, m = 1, L = 3: p_0 at 0, p_2 at 2; q_0 at 2 (the partner waits two steps and is reset in front of step 2); y_0 at step 2
    got, needed = rows([3], [1], [2], 1)
    assert got == [(0, 0, 0, 2, 2, 2, False)] and needed == 4


def test_negative_prompt_as_long_as_the_prompt():
    got, needed = rows([2], [2], [3], 1)
    assert got == [(0, 0, 0, 0, 1, 3, False)] and needed == 4


def test_negative_prompt_longer_than_the_prompt():
    # n = 1, m = 4, L = 4: q_0 at 0 .. q_3 at 3; p_0 at 3 (the conditional half waits three steps, reset in front of step 3); y_0 at 3
    got, needed = rows([1], [4], [2], 1)
    assert got == [(0, 0, 3, 0, 3, 2, False)] and needed == 5


def test_no_negative_prompt():
    # an unguided request: the partner is neither reset nor fed
    got, needed = rows([2], [0], [2], 1)
    assert got == [(0, 0, 0, None, 1, 2, False)] and needed == 3


def test_two_pairs_ending_in_the_same_step_take_requests_in_slot_order():
    # pair 0: n 1, m 2, reply 2 -> y at steps 1, 2; pair 1: n 3, m 1, reply 1 -> y_0 at step 2: both end in step 2, f = 3 for both
    got, needed = rows([1, 3, 2, 1], [2, 1, 3, 0], [2, 1, 1, 2], 2)
    assert got == [(0, 0, 1, 0, 1, 2, False), (1, 0, 0, 2, 2, 1, False),
                   (0, 3, 4, 3, 5, 1, False),       # L = 3: q_0 at 3, p_0 at 4, y_0 at 5
                   (1, 3, 3, None, 3, 2, False)]    # unguided: p_0 at 3, y at 3, 4
    assert needed == 6


def test_a_pair_serving_three_requests_in_a_row_with_alternating_late_halves():
    # r0: n 1, m 3 (the conditional half is late): f 0, q at 0..2, p_0 at 2, y at 2, 3          -> ends in step 3
    # r1: n 3, m 1 (the partner is late):          f 4, p at 4..6, q_0 at 6, y_0 at 6           -> ends in step 6
    # r2: n 2, m 4 (the conditional half again):   f 7, q at 7..10, p at 9, 10, y at 10, 11, 12 -> ends in step 12
    got, needed = rows([1, 3, 2], [3, 1, 4], [2, 1, 3], 1)
    assert got == [(0, 0, 2, 0, 2, 2, False), (0, 4, 4, 6, 6, 1, False), (0, 7, 9, 7, 10, 3, False)]
    assert needed == 13


def test_start_step_step_base_and_reset_steps_of_every_request():
    ns, ms, lengths = [3, 1, 5, 2, 4, 1, 2], [1, 4, 5, 0, 2, 3, 2], [4, 6, 12, 5, 9, 1, 7]
    for B in (1, 2, 4):
        got, needed = G.schedule(ns, ms, lengths, B)
        busy = {}
        for r, row in enumerate(got):
            n, m, L, f = ns[r], ms[r], max(ns[r], ms[r]), row["dispatch_step"]
            assert row["start_step"] == f + L - n and row["step_base"] == f + L - 1 == row["start_step"] + n - 1
            assert row["neg_start_step"] == (None if m == 0 else f + L - m)
            assert min(row["start_step"], row["neg_start_step"] if m else row["start_step"]) == f       # one half starts at once
            busy.setdefault(row["slot"], []).append((f, row["step_base"] + row["length"] - 1))
        for b, spans in busy.items():                   # a pair's requests follow each other without a gap or an overlap
            assert spans[0][0] == 0
            for (_, end), (f, _) in zip(spans, spans[1:]):
                assert f == end + 1
        assert needed == max(end for spans in busy.values() for _, end in spans) + 1


@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_equals_the_plain_queue_whenever_no_negative_prompt_is_longer(B):
    rng = np.random.default_rng(B)
    for _ in range(50):
        R = int(rng.integers(1, 9))
        ns = [int(x) for x in rng.integers(1, 6, R)]
        ms = [int(rng.integers(0, n + 1)) for n in ns]
        lengths = [int(x) for x in rng.integers(1, 7, R)]
        for cap in (None, int(rng.integers(1, 30))):
            got, needed = G.schedule(ns, ms, lengths, B, cap)
            want, want_needed = Q.schedule(ns, lengths, B, cap)
            assert needed == want_needed
            assert [(g["slot"], g["start_step"], g["length"], g["cut"]) for g in got] == [(w["slot"], w["start_step"], w["length"], w["cut"]) for w in want]
        prompts, negs = [[1] * n for n in ns], [[2] * m for m in ms]
        replies = [list(rng.integers(3, 9, k + 2)) for k in lengths]
        stops = [[5] if r % 2 else [] for r in range(R)]
        got, needed = G.run(prompts, negs, replies, stops, lengths, B)
        want, want_needed = Q.run(prompts, replies, stops, lengths, B)
        assert needed == want_needed
        assert [(t.tolist(), why, s, st) for t, why, s, st in got] == [(t.tolist(), why, s, st) for t, why, s, st in want]


def test_a_longer_negative_prompt_delays_exactly_by_the_difference():
    got, needed = rows([2, 2], [5, 0], [3, 3], 1)
    plain, plain_needed = Q.schedule([2, 2], [3, 3], 1)
    assert got[0][2] == plain[0]["start_step"] + 3 and got[1][2] == plain[1]["start_step"] + 3 and needed == plain_needed + 3


def test_a_cap_that_cuts_a_request():
    # one pair: r0 (n 1, m 3, reply 2) draws at 2, 3; r1 (n 2, m 0, reply 2) has f = 4, y at 5, 6
    full, needed = rows([1, 2], [3, 0], [2, 2], 1)
    assert full == [(0, 0, 2, 0, 2, 2, False), (0, 4, 4, None, 5, 2, False)] and needed == 7
    got, _ = rows([1, 2], [3, 0], [2, 2], 1, max_steps=2)          # q_0, q_1 were fed, p_0 was not: never dispatched
    assert got == [(None, None, None, None, None, 0, False)] * 2
    got, _ = rows([1, 2], [3, 0], [2, 2], 1, max_steps=3)          # y_0 drawn
    assert got[0] == (0, 0, 2, 0, 2, 1, True) and got[1][0] is None
    got, _ = rows([1, 2], [3, 0], [2, 2], 1, max_steps=5)          # r1 is in its prompt
    assert got == [(0, 0, 2, 0, 2, 2, False), (0, 4, 4, None, 5, 0, True)]
    out, _ = G.run([[1], [2, 3]], [[4, 5, 6], []], [[7, 8], [9, 9]], [[], []], [2, 2], 1, max_steps=3)
    assert [(t.tolist(), why, s, st) for t, why, s, st in out] == [([7], Q.CAP, 0, 2), ([], Q.NEVER, 0, 0)]


def test_request_conditions():
    assert G.check_request(1, 0, 1.0) and G.check_request(1, 3, 0.0) and G.check_request(2, 2, 7.5)
    for n, m, s in ((0, 1, 1.0), (1, 0, 1.5), (1, 0, 0.0), (1, 1, -0.5), (1, 1, float("nan")), (1, 1, float("inf"))):
        assert not G.check_request(n, m, s), (n, m, s)


# ------------------------------------------------------------------ the ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wrk_hip.h")).read(), flags=re.S)


def _fields(text, cname):
    body = re.search(r"typedef\s+struct\s+" + cname + r"\s*\{(.*?)\}", text, flags=re.S).group(1)
    return [n for stmt in body.split(";") if stmt.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", stmt.strip())]


def test_guided_queue_entry_points_are_declared_exported_and_bound():
    text = _header()
    declared = set(re.findall(r"\b(wrk_[a-z0-9_]+)\s*\(", text))
    plain = re.search(r"wrk_v7_generate_queue\s*\(([^;]*)\)\s*;", text).group(1)
    for name, model in (("wrk_v7_generate_queue_guided", "wrk_v7_model"), ("wrk_v6_generate_queue_guided", "wrk_v6_model")):
        assert name in declared, f"{name} is not declared in include/wrk_hip.h"
        assert hasattr(wrk.hip, name), f"{name} is not exported"
        assert name in wrk.HIP_SYMBOLS, f"{name} has no ctypes signature"
        assert len(wrk.HIP_SYMBOLS[name][1]) == 9
        args = re.search(name + r"\s*\(([^;]*)\)\s*;", text).group(1)
        # the leading arguments are wrk_v7_generate_queue's, the guidance last
        assert " ".join(args.split()) == " ".join(plain.replace("wrk_v7_model", model).split()) + ", const wrk_queue_guidance* guide"
    assert _fields(text, "wrk_queue_guidance") == ["scale", "negative_tokens", "negative_offsets", "negative_init_state"]
    assert [n for n, _ in wrk.QueueGuidance._fields_] == _fields(text, "wrk_queue_guidance")


def test_queue_options_are_unchanged():
    """The guided queue takes its guidance beside the options: wrk_queue_options keeps its fields and their pinned order, the scale
    field of the refusal included, and wrk_queue_result its six arrays."""
    text = _header()
    names = _fields(text, "wrk_queue_options")
    assert names == [n for n, _ in wrk.QueueOptions._fields_]
    assert len(names) == 44 and names[0] == "num_requests" and names[-2:] == ["top_k", "min_p"]
    assert names[names.index("bias_set") + 1] == "guidance_scale" and names[names.index("guidance_scale") + 1] == "init_state"
    assert not any(n.startswith("negative") for n in names)
    assert _fields(text, "wrk_queue_result") == ["lengths", "reasons", "slots", "start_steps", "out_tokens", "steps_run"]


def test_python_entry_point_takes_generate_queues_arguments_without_the_pool_ones():
    guided = inspect.signature(wrk.Runtime.generate_queue_guided).parameters
    plain = inspect.signature(wrk.Runtime.generate_queue).parameters
    assert list(guided)[1:5] == ["requests", "negative_prompts", "guidance_scale", "negative_init_state"]
    pool_ones = {"pool", "start_state", "save_state", "history"}
    assert set(plain) - set(guided) == pool_ones
    for name in set(plain) & set(guided) - {"guidance_scale"}:
        assert guided[name].default == plain[name].default or name == "requests", name
