"""Hand-worked cases of tests/stop_ref.py, and the declared-symbol check of the two stop entry points (no GPU)."""
import os
import re

import numpy as np

import stop_ref as R
import wrk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def col(*t):
    return np.array(t, np.uint32).reshape(-1, 1)


def test_stop_at_step_zero():
    out, n = R.apply(col(7, 3, 4, 5), [[7]])
    assert n.tolist() == [1]
    assert out[:, 0].tolist() == [7, 7, 7, 7]


def test_stop_at_the_last_step():
    out, n = R.apply(col(1, 2, 3, 9), [[9]])
    assert n.tolist() == [4]
    assert out[:, 0].tolist() == [1, 2, 3, 9]


def test_no_stop_at_all():
    t = col(1, 2, 3, 4)
    for stops in ([[]], [[8, 0]]):
        out, n = R.apply(t, stops)
        assert n.tolist() == [4]
        assert np.array_equal(out, t)


def test_stop_token_that_also_occurs_after_the_end():
    out, n = R.apply(col(5, 2, 6, 2, 8), [[2]])
    assert n.tolist() == [2]                       # the first occurrence ends the sequence, the later one is never drawn
    assert out[:, 0].tolist() == [5, 2, 2, 2, 2]


def test_two_sequences_with_different_stop_sets():
    t = np.array([[1, 1], [2, 2], [3, 3], [4, 4]], np.uint32)
    out, n = R.apply(t, [[3, 9], [2]])
    assert n.tolist() == [3, 2]
    assert out.tolist() == [[1, 1], [2, 2], [3, 2], [3, 2]]
    out, n = R.apply(t, [[4, 2], []])              # two ids: the one drawn first ends it; an empty set never does
    assert n.tolist() == [2, 4]
    assert out.tolist() == [[1, 1], [2, 2], [2, 3], [2, 4]]


def test_early_exit_rows_and_bound():
    t = np.array([[1, 1], [2, 2], [3, 3], [4, 4], [5, 5], [6, 6]], np.uint32)
    out, n = R.apply(t, [[2], [3]], steps_run=4)
    assert out.shape == (4, 2) and n.tolist() == [2, 3]
    assert out.tolist() == [[1, 1], [2, 2], [2, 3], [2, 3]]
    assert R.steps_run_bound([2, 3], 2, 6) == 6     # (ceil(3 / 2) + 2) * 2 = 8, capped by steps
    assert R.steps_run_bound([40, 63], 8, 2048) == (8 + 2) * 8
    assert R.steps_run_bound([1], 8, 2048) == 24


def test_stop_entry_points_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "wrk_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(wrk_[a-z0-9_]+)\s*\(", text))
    for name in ("wrk_v7_generate_stop", "wrk_v6_generate_stop"):
        assert name in declared, f"{name} is not declared in include/wrk_hip.h"
        assert hasattr(wrk.hip, name), f"{name} is not exported"
        assert name in wrk.HIP_SYMBOLS, f"{name} has no ctypes signature"
        res, args = wrk.HIP_SYMBOLS[name]
        assert len(args) == 13
    m = re.search(r"#define\s+WRK_MAX_STOP_TOKENS\s+(\d+)", text)
    assert m and int(m.group(1)) == R.MAX_STOP_TOKENS == wrk.MAX_STOP_TOKENS
    assert wrk.hip.wrk_abi_version() == 1
