"""tests/beam_ref.py -- the beam step in NumPy -- against the hand-worked groups of tests/beam_cases.py (written from the contract of
wrk_v7_generate_beam in include/wrk_hip.h), and three mutants of it that those groups must catch: a wrong tie order, a DONE slot
that moves, a key formed by division."""
import numpy as np
import pytest

import beam_cases as bc
import beam_ref as br


def run(case, **kw):
    score, key, length, status, ids, lp = bc.arrays(case)
    inv = br.inv_norm_table(case["alpha"], int(length.max()) + 1)
    return bc.got_words(br.select_group(score, key, length, status, ids, lp, inv, case["stop"], **kw))


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_hand_worked_groups(name):
    case = bc.CASES[name]
    got, want = run(case), bc.want_words(case)
    for k in want:
        assert got[k] == want[k], (name, k)


def test_inv_norm_table():
    assert br.inv_norm_table(0.0, 5).tolist() == [1.0] * 6                          # penalty 0: key == raw bit for bit
    t = br.inv_norm_table(1.0, 8)
    assert t[1] == 1.0 and t[2] == 0.5 and t[4] == 0.25 and t[8] == 0.125
    assert t[3].view(np.uint32) == 0x3EAAAAAB and t[7].view(np.uint32) == 0x3E124925  # 1/3 and 1/7 rounded to f32 once
    assert br.inv_norm_table(0.5, 4)[4] == 0.5
    raw = np.float32(-5.25)
    assert br.make_key(raw, br.inv_norm_table(0.0, 7), 7).view(np.uint32) == raw.view(np.uint32)
    assert br.make_key(raw, t, 7).view(np.uint32) == 0xBF400001                     # a product: the quotient is 0xBF400000


def test_copy_sources_and_global_indices():
    """select() over two groups: parents and copy sources are slot indices of the whole batch; a slot whose parent is itself moves no bytes"""
    a, b = bc.CASES["tie_by_j"], bc.CASES["penalty_1"]
    parts = [bc.arrays(a), bc.arrays(b)]
    score, key, length, status, ids, lp = (np.concatenate([p[i] for p in parts]) for i in range(6))
    out = br.select(score, key, length, status, ids, lp, 2, br.inv_norm_table(1.0, 4), stops=[[], []])
    assert out["parent"].tolist() == [0, 0, 2, 2]
    assert out["copy_src"].tolist() == [br.NO_COPY, 0, br.NO_COPY, 2]
    one = bc.CASES["done_stays_and_pushed_out"]
    o = br.select_group(*bc.arrays(one), br.inv_norm_table(0.0, 3), one["stop"])
    assert o["copy_src"].tolist() == [br.NO_COPY, br.NO_COPY, 3, 0]                # the staying DONE slot and slot 0 move nothing


def test_start_hypotheses_and_backtrack():
    score, key, length, status = br.start_records(2, 3)
    assert status.tolist() == [br.LIVE, br.DEAD, br.DEAD] * 2 and score[0] == 0 and np.isneginf(score[1]) and length.tolist() == [0] * 6
    # by key descending, ties by slot, DEAD slots left out
    assert br.hypotheses(np.array([-2, -1, -1, -9, 0, -3], np.float32), np.array([1, 2, 1, 0, 0, 2]), 3) == [[1, 2, 0], [5]]
    # two steps of W = 2: step 0 fills both slots from slot 0; step 1 puts (slot 1's child) in slot 0 and leaves slot 1 not filled
    toks, pars = [[5, 7], [9, br.NO_TOKEN]], [[0, 0], [1, 1]]
    assert br.backtrack(toks, pars, 0, 2) == [7, 9]
    assert br.backtrack(toks, pars, 1, 1) == [7]


MUTANTS = {
    "ties_by_slot_descending": dict(order=lambda c: (-float(c[0]), -c[1], c[2])),
    "ties_by_j_descending": dict(order=lambda c: (-float(c[0]), c[1], -c[2])),
    "done_slot_moves": dict(done_stays=False),
}


def mutant(name, case):
    if name == "key_by_division":       # key = raw / len ** length_penalty, one f32 division
        return dict(make_key=lambda raw, inv, n: np.float32(np.float32(raw) / np.float32(float(n) ** case["alpha"])))
    return MUTANTS[name]


@pytest.mark.parametrize("name", sorted(MUTANTS) + ["key_by_division"])
def test_mutants_are_caught(name):
    """every mutant differs from the hand-worked expectation in at least one group, in a word the device comparison looks at"""
    caught = [c for c in sorted(bc.CASES) if any(run(bc.CASES[c], **mutant(name, bc.CASES[c]))[k] != v for k, v in bc.want_words(bc.CASES[c]).items())]
    assert caught, name
    expect = {"ties_by_slot_descending": "tie_by_slot", "ties_by_j_descending": "tie_by_j", "done_slot_moves": "done_stays_and_pushed_out",
              "key_by_division": "key_is_a_product"}[name]
    assert expect in caught, (name, caught)
