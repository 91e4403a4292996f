"""tests/stopseq_ref.py, the restatement the device's stop-sequence matcher is held to, against an independent brute force and the
hand-worked cases of tests/stopseq_cases.py; the Python builders of the ABI's CSR of a CSR with the argument errors the host raises
without a device; and the declarations of the ABI."""
import os
import re

import numpy as np
import pytest

import stopseq_cases as K
import stopseq_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute(stream, seqs, ids=()):
    """(length, match word) from the definition alone: at draw i sequence k matches when stream[i + 1 - l : i + 1] == seq_k."""
    for i, y in enumerate(stream):
        found = []                                   # (length, a stop id beats a sequence, then the lower index)
        if y in ids:
            found.append((1, 1, 0, Q.TOKEN))
        for k, q in enumerate(seqs):
            l = len(q)
            if i + 1 - l >= 0 and list(stream[i + 1 - l:i + 1]) == list(q):
                found.append((l, 0, -k, k))
        if found:
            return i + 1, max(found)[3]
    return len(stream), Q.NONE


def test_step_agrees_with_the_brute_force_on_random_streams():
    rng = np.random.default_rng(7)
    ended = never = token = 0
    for _ in range(5000):
        stream = rng.integers(0, 3, 24).tolist()
        seqs = [rng.integers(0, 3, int(rng.integers(1, 9))).tolist() for _ in range(int(rng.integers(0, 9)))]
        ids = [int(rng.integers(0, 3))] if rng.random() < 0.2 else []
        n, m, tail = Q.run(stream, seqs, ids)
        assert (n, m) == brute(stream, seqs, ids), (stream, seqs, ids)
        t = stream[:n][-Q.TAIL_LEN:]
        assert tail == [Q.EMPTY] * (Q.TAIL_LEN - len(t)) + t
        ended += m != Q.NONE
        never += m == Q.NONE
        token += m == Q.TOKEN
    assert ended > 1000 and never > 300 and token > 100, (ended, never, token)     # the draw covers every outcome


@pytest.mark.parametrize("i", range(len(K.CASES)), ids=K.NAMES)
def test_hand_worked_case(i):
    name, first, _, seqs, ids, want = K.CASES[i]
    stream = K.stream(i)
    assert len(stream) == K.STEPS
    n, m, tail = Q.run(stream, seqs, ids)
    assert (n, m) == want, name
    assert brute(stream, seqs, ids) == want, name
    assert tail == K.want_tail(i), name
    lens, match, tails = Q.lengths(np.array([stream], np.uint32).T, [seqs], [ids])
    assert (int(lens[0]), int(match[0])) == want and tails[0].tolist() == K.want_tail(i)


def test_the_first_fed_token_is_not_in_the_tail():
    i = K.NAMES.index("x_0")
    _, first, _, seqs, ids, want = K.CASES[i]
    # were x_0 = 70 a drawn token, [70 71] would match at the first draw
    assert Q.run([first] + K.stream(i), seqs, ids)[0] - 1 == 1
    assert want == (4, 0)


def test_longest_then_stop_id_then_lower_index():
    t = Q.empty_tail()[:-2] + [41, 42]
    assert Q.step(t, 43, [[42, 43], [41, 42, 43], [99, 43]], [43])[0] == 1          # the longest
    assert Q.step(t, 43, [[43], [43]], [43])[0] == Q.TOKEN                          # equal length: the stop id
    assert Q.step(t, 43, [[43], [43]], [])[0] == 0                                  # equal length: the lower index
    assert Q.step(t, 43, [[42, 43], [43], [42, 43]], [43])[0] == 0
    assert Q.step(t, 44, [[42, 43]], [43])[0] == Q.NONE
    # EMPTY equals no id: a sequence cannot match across the start of the tail
    assert Q.step(Q.empty_tail(), 43, [[42, 43]], [])[0] == Q.NONE
    assert Q.step(Q.empty_tail(), 43, [[42, 43]], []) == (Q.NONE, Q.empty_tail()[1:] + [43])


def test_decoys_split_into_two_calls():
    i = K.NAMES.index("decoys")
    stream, seqs = K.stream(i), K.CASES[i][3]
    n, m, tail = Q.run(stream[:K.SPLIT], seqs)
    assert (n, m) == (K.SPLIT, Q.NONE) and tail == K.SPLIT_TAIL                     # the first call does not end
    assert Q.run(stream[K.SPLIT:], seqs, tail=tail)[:2] == (2, 0)                   # the second, with the tail, ends at length 2
    assert Q.run(stream[K.SPLIT:], seqs)[:2] == (K.STEPS - K.SPLIT, Q.NONE)         # and without it does not


def test_apply_pads_with_the_token_that_ended_the_sequence():
    tok = np.array([K.stream(0), K.stream(3)], np.uint32).T
    out, n, m, _ = Q.apply(tok, [K.CASES[0][3], K.CASES[3][3]])
    assert n.tolist() == [4, 16] and m.tolist() == [0, Q.NONE]
    assert out[:4, 0].tolist() == [7, 7, 7, 9] and set(out[4:, 0].tolist()) == {9} and np.array_equal(out[:, 1], tok[:, 1])
    assert Q.reply([5, 6, 7, 8], [[6, 7]], [], 4) == (3, 1, 0) and Q.reply([5, 6, 7, 8], [[9]], [], 3) == (3, 2, Q.NONE)


# ------------------------------------------------------------------------------------------------ the Python builders
def test_builders_make_the_csr_of_a_csr():
    import wrk
    ids, off, own = wrk._stop_seq_csr([[1, 2], [3]], 2, "sequences")                # one list for both owners
    assert ids.tolist() == [1, 2, 3, 1, 2, 3] and off.tolist() == [0, 2, 3, 5, 6] and own.tolist() == [0, 2, 4]
    ids, off, own = wrk._stop_seq_csr([[[1, 2]], [], [[4], [5, 6, 7]]], 3, "sequences")     # one list per owner
    assert ids.tolist() == [1, 2, 4, 5, 6, 7] and off.tolist() == [0, 2, 3, 6] and own.tolist() == [0, 1, 1, 3]
    ids, off, own = wrk._stop_seq_csr([], 3, "requests")                            # nobody owns a sequence: the arrays still exist
    assert ids.size >= 1 and off.tolist() == [0] and own.tolist() == [0, 0, 0, 0]
    _, off, own = wrk._stop_seq_csr([[], []], 2, "requests")
    assert off.tolist() == [0] and own.tolist() == [0, 0, 0]
    assert all(a.dtype == np.uint32 for a in (ids, off, own))
    t = wrk._stop_tails(None, 2)
    assert t.shape == (2, wrk.STOP_TAIL_LEN) and t.dtype == np.uint32 and (t == wrk.STOP_TAIL_EMPTY).all()
    t = wrk._stop_tails([[5, 6], K.SPLIT_TAIL], 2)
    assert t[0].tolist() == [wrk.STOP_TAIL_EMPTY] * 5 + [5, 6] and t[1].tolist() == K.SPLIT_TAIL


def test_builders_reject_what_the_host_can_see():
    import wrk
    S, L = wrk.MAX_STOP_SEQUENCES, wrk.MAX_STOP_SEQUENCE_LEN
    bad = [([[1]] * (S + 1), 2),                        # too many for an owner
           ([list(range(L + 1))], 2),                   # too long
           ([[1], []], 3),                              # an empty sequence
           ([[[1]], [[2]]], 3),                         # two owners' lists for three owners
           ([1, 2], 2),                                 # ids where id lists belong
           ([[-1]], 1)]
    for seqs, n in bad:
        with pytest.raises(ValueError):
            wrk._stop_seq_csr(seqs, n, "sequences")
    wrk._stop_seq_csr([[1]] * S, 2, "sequences")
    wrk._stop_seq_csr([list(range(L))], 2, "sequences")
    with pytest.raises(ValueError):
        wrk._stop_tails([[1] * (wrk.STOP_TAIL_LEN + 1)], 1)
    with pytest.raises(ValueError):
        wrk._stop_tails([[1]], 2)


# ------------------------------------------------------------------------------------------------ the ABI
def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wrk_hip.h")).read(), flags=re.S)


def test_option_fields_match_the_ctypes_mirror():
    import wrk
    new = {"wrk_generate_options": ["stop_seq_tokens", "stop_seq_offsets", "stop_seq_owners", "out_stop_match", "stop_tail"],
           "wrk_queue_options": ["stop_seq_tokens", "stop_seq_offsets", "stop_seq_owners", "out_stop_match"]}
    for cname, cls in (("wrk_generate_options", wrk.GenerateOptions), ("wrk_queue_options", wrk.QueueOptions)):
        body = re.search(r"typedef\s+struct\s+" + cname + r"\s*\{(.*?)\}", header(), flags=re.S).group(1)
        names = [n for stmt in body.split(";") if stmt.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", stmt.strip())]
        assert names == [n for n, _ in cls._fields_], cname
        at = names.index("grammar_state") + 1
        assert names[at:at + len(new[cname])] == new[cname], cname                  # between grammar_state and mirostat_tau
        assert names[at + len(new[cname])] == "mirostat_tau", cname
        assert all(dict(cls._fields_)[n] is wrk._u32p for n in new[cname])
    assert wrk.hip.wrk_abi_version() == 1


def test_entry_point_and_constants_are_declared_and_bound():
    import wrk
    text = header()
    name = "wrk_stop_sequences_advance"
    assert name in set(re.findall(r"\b(wrk_[a-z0-9_]+)\s*\(", text)) and hasattr(wrk.hip, name) and name in wrk.HIP_SYMBOLS
    assert len(wrk.HIP_SYMBOLS[name][1]) == 11
    assert callable(wrk.Context.stop_sequences_advance)
    defs = {k: int(v.rstrip("u"), 0) for k, v in re.findall(r"#define\s+(WRK_\w+)\s+(0x[0-9A-Fa-f]+u?|\d+)\s", text)}
    for py, c, ref in (("MAX_STOP_SEQUENCES", "WRK_MAX_STOP_SEQUENCES", Q.MAX_STOP_SEQUENCES),
                       ("MAX_STOP_SEQUENCE_LEN", "WRK_MAX_STOP_SEQUENCE_LEN", Q.MAX_STOP_SEQUENCE_LEN),
                       ("STOP_TAIL_LEN", "WRK_STOP_TAIL_LEN", Q.TAIL_LEN), ("STOP_TAIL_EMPTY", "WRK_STOP_TAIL_EMPTY", Q.EMPTY),
                       ("STOP_MATCH_NONE", "WRK_STOP_MATCH_NONE", Q.NONE), ("STOP_MATCH_TOKEN", "WRK_STOP_MATCH_TOKEN", Q.TOKEN)):
        assert getattr(wrk, py) == defs[c] == ref, py
    assert (defs["WRK_MAX_STOP_SEQUENCES"], defs["WRK_MAX_STOP_SEQUENCE_LEN"], defs["WRK_STOP_TAIL_LEN"]) == (8, 8, 7)
