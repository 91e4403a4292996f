"""The guided queue's dispatch rule (web-rwkv-gguf_amd/csrc/wrk_queue_dispatch.h queue_dispatch_guided), on the CPU.

tests/host/queue_dispatch_guided_main.cpp includes that HIP-free header alone, runs one dispatch per case over host arrays pre-filled
with a canary and prints every word the arrays then hold.  It is built with the host compiler under the address and undefined-behaviour
sanitizers, linked into the program: a stand-alone executable that runs the same whatever the environment preloads.

Every expectation here is worked from the contract of wrk_v7_generate_queue_guided in include/wrk_hip.h -- never read off the function:
  - "request slot b is the pair (state slot b, state slot B + b)": the conditional half's record, token and start answer are entry b,
    the partner's entry B + b.
  - "A pair given request r at step f ... feeds p_0 at step f + L - n and q_0 at step f + L - m ... both halves feed their last prompt
    token at step f + L - 1 ... The sampler step of y_j is j (the step base is f + L - 1), and start_steps[r] stays ... f + L - n".
  - "The half that starts late waits until its first token: it feeds a valid id": the record says WAIT with the number of steps to wait,
    L - n or L - m, and the half's first token already sits in `tokens`; its state slot is not to be reset yet (start answer 0).  A half
    that starts at f has start answer 1 and the record of the plain rule: REPLY at once iff its prompt has one token.
  - "A partner with m == 0 is neither reset nor fed": record IDLE, start answer 0, tokens[B + b] untouched.
  - "The pair's pick rows ... are the conditional request's and are written by the dispatch": everything the plain rule writes for
    (r, b, first step f + L - n), B wide, plus the pair's scale; prompt intake: p_0 enters iff prompt_context_from[r] == 0, and only once
    it is fed -- a waiting conditional half has no intake flag yet.
  - "started" / "pair_started" are the advance's to write, never the rule's.
The world: 3 pairs, 5 requests with the values of REQS, every one exact in f32; word-wise dumps, floats as their bits."""
import json
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5A5A5A5
TAIL_LEN, TAIL_EMPTY, DRY_MAX_MATCH = 7, 0xFFFFFFFF, 50        # WRK_STOP_TAIL_LEN, WRK_STOP_TAIL_EMPTY, WRK_DRY_MAX_MATCH
IDLE, PROMPT, REPLY, WAIT = 0, 1, 2, 3
B, R = 3, 5
#        prompts: r0 [11]  r1 [21 22 23]  r2 [31 32]  r3 [41 42 43]  r4 [51]    negatives: r0 [61 62 63]  r1 [71]  r2 [81 82]  r3 -  r4 [91]
POOL = [11, 21, 22, 23, 31, 32, 41, 42, 43, 51, 61, 62, 63, 71, 81, 82, 91]
OFFSETS, LENGTHS = [0, 1, 4, 6, 9], [1, 3, 2, 3, 1]
NEG_OFFSETS, NEG_LENGTHS = [10, 13, 14, 16, 16], [3, 1, 2, 0, 1]
SCALES = [1.5, 0.5, 2.0, 1.0, 0.0]
REQS = [dict(prompt_off=OFFSETS[r], prompt_len=LENGTHS[r], max_new=4 + r, seed=1000 + r, temperature=0.5 + 0.25 * r, top_p=0.5 + 0.125 * r,
             presence=0.25 * (r + 1), frequency=0.125 * (r + 1), decay=1 - 0.0625 * (r + 1), top_k=10 + r, ln_min_p=-(1.5 + r), tau=2.0 + r,
             eta=0.125 * (r + 1), typical_p=0.5 + 0.0625 * r, mu=4 + 0.5 * r, gram=7 + r, ctx_from=[0, 2, 0, 1, 0][r],
             dry_allowed=2 + r, dry_no_repeat=3 + r, dry_multiplier=0.5 * (r + 1), dry_pen0=100.0 * (r + 1),
             neg_off=NEG_OFFSETS[r], neg_len=NEG_LENGTHS[r], scale=SCALES[r]) for r in range(R)]
OPTIONAL = ["sample", "pen", "filter", "alt", "mu", "gram", "dry", "seq", "intake"]


def f32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


@pytest.fixture(scope="module")
def dispatch(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host compiler g++ is required"
    exe = str(tmp_path_factory.mktemp("queue_dispatch_guided") / "queue_dispatch_guided")
    cmd = [cxx, "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "web-rwkv-gguf_amd", "csrc"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-g",
           os.path.join(ROOT, "tests", "host", "queue_dispatch_guided_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(cases):
        """cases: [dict(r, b, first_step, rule, off)] -> one dump per case"""
        lines = []
        for i, c in enumerate(cases):
            lines.append(f"case c{i} {c.get('rule', 'guided')} {B} {R} {c['r']} {c['b']} {c['first_step']} {','.join(c.get('off', ())) or '-'}")
            lines += ["req " + " ".join(repr(v) for v in q.values()) for q in REQS]
            lines.append(f"pool {len(POOL)} " + " ".join(map(str, POOL)))
        ran = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert ran.returncode == 0, ran.stdout + ran.stderr
        out = [json.loads(line) for line in ran.stdout.splitlines()]
        assert len(out) == len(cases), ran.stdout + ran.stderr
        return out
    return run


def untouched():
    """the dump of a world no dispatch has written"""
    per_pair = dict(pair_started=1, scale=1, sample=4, filter=2, alt=4, gram_state=1, tail=TAIL_LEN, take=1, pen=4, dry=4 + DRY_MAX_MATCH + 2)
    w = {k: [CANARY] * (n * B) for k, n in per_pair.items()}
    w.update(tokens=[CANARY] * (2 * B), started=[CANARY] * (2 * B), slots=[CANARY] * (4 * 2 * B))
    w.update(log=[CANARY] * (4 * R), seq_match=[CANARY] * R, pointers_kept=True, start_cond=0, start_part=0)
    return w


def put(w, key, index, words):
    n = len(words)
    w[key][index * n:(index + 1) * n] = words


def plain_rows(w, r, b, first_step, off):
    """what the plain rule writes for (r, slot b, p_0 fed at first_step): the contract of wrk_v7_generate_queue, as
    tests/test_queue_dispatch_host.py states it"""
    q, n = REQS[r], LENGTHS[r]
    put(w, "tokens", b, [POOL[OFFSETS[r]]])
    put(w, "slots", b, [r, 0, 0, REPLY if n == 1 else PROMPT])
    put(w, "log", r, [0, 3, b, first_step])
    if "sample" not in off:
        put(w, "sample", b, [f32(q["temperature"]), f32(q["top_p"]), q["seed"], first_step + n - 1])
    if "filter" not in off:
        put(w, "filter", b, [q["top_k"], f32(q["ln_min_p"])])
    if "alt" not in off:
        put(w, "alt", b, [f32(q["tau"]), f32(q["eta"]), f32(0.0 if "mu" in off else q["mu"]), f32(q["typical_p"])])
    if "gram" not in off:
        put(w, "gram_state", b, [q["gram"]])
    if "seq" not in off:
        put(w, "tail", b, [TAIL_EMPTY] * TAIL_LEN)
    if "intake" not in off:
        put(w, "take", b, [int(q["ctx_from"] == 0)])
    if "pen" not in off:
        put(w, "pen", b, [f32(q["presence"]), f32(q["frequency"]), f32(q["decay"]), CANARY])
    if "dry" not in off:
        put(w, "dry", b, [CANARY, q["dry_allowed"], q["dry_no_repeat"], f32(q["dry_multiplier"])] +
            [f32(q["dry_pen0"] + m) for m in range(DRY_MAX_MATCH + 1)] + [CANARY])
    w["wipe"] = "dry" not in off


def expected(r, b, first_step, rule="guided", off=()):
    """the world after request r went to pair b with f = first_step, clause by clause from the contract (module docstring)"""
    w = untouched()
    if rule == "plain":
        plain_rows(w, r, b, first_step, off)
        return w
    n, m = LENGTHS[r], NEG_LENGTHS[r]
    L = max(n, m)
    plain_rows(w, r, b, first_step + L - n, off)            # start_step and the sampler base f + L - 1 follow from it
    if L > n:                                               # the conditional half waits L - n steps on its p_0; nothing has entered yet
        put(w, "slots", b, [r, L - n, 0, WAIT])
        if "intake" not in off:
            put(w, "take", b, [0])
    else:
        w["start_cond"] = 1
    if m == 0:
        put(w, "slots", B + b, [r, 0, 0, IDLE])
    else:
        put(w, "tokens", B + b, [POOL[NEG_OFFSETS[r]]])     # q_0
        if L > m:
            put(w, "slots", B + b, [r, L - m, 0, WAIT])
        else:
            put(w, "slots", B + b, [r, 0, 0, REPLY if m == 1 else PROMPT])
            w["start_part"] = 1
    put(w, "scale", b, [f32(SCALES[r])])
    return w


def check(got, want, what):
    got = {k: v for k, v in got.items() if k != "name"}
    assert got.keys() == want.keys(), what
    for k in want:
        assert got[k] == want[k], (what, k)


@pytest.mark.parametrize("first_step", [0, 6])
def test_step_0_and_refill_for_every_relation_of_the_two_lengths(dispatch, first_step):
    """r0: m > n (n = 1); r1: m < n; r2: m == n; r3: m == 0; r4: n == m == 1 -- at the host's step 0 and at a refill."""
    b = 1
    got = dispatch([dict(r=r, b=b, first_step=first_step) for r in range(R)])
    f = first_step
    # (conditional record, partner record, sampler base, start_step, start answers), worked by hand
    want = {0: ([0, 2, 0, WAIT], [0, 0, 0, PROMPT], f + 2, f + 2, (0, 1)),          # q_0 q_1 q_2 at f .. f + 2, p_0 at f + 2
            1: ([1, 0, 0, PROMPT], [1, 2, 0, WAIT], f + 2, f, (1, 0)),              # p_0 p_1 p_2 at f .. f + 2, q_0 at f + 2
            2: ([2, 0, 0, PROMPT], [2, 0, 0, PROMPT], f + 1, f, (1, 1)),
            3: ([3, 0, 0, PROMPT], [3, 0, 0, IDLE], f + 2, f, (1, 0)),
            4: ([4, 0, 0, REPLY], [4, 0, 0, REPLY], f, f, (1, 1))}
    for r, g in enumerate(got):
        cond, part, base, start, (sc, sp) = want[r]
        assert g["slots"][4 * b:4 * b + 4] == cond and g["slots"][4 * (B + b):4 * (B + b) + 4] == part, r
        assert g["sample"][4 * b + 3] == base and g["log"][4 * r:4 * r + 4] == [0, 3, b, start], r
        assert (g["start_cond"], g["start_part"]) == (sc, sp), r
        assert g["tokens"][b] == POOL[OFFSETS[r]], r                                 # p_0, also while the half waits
        assert g["tokens"][B + b] == (CANARY if NEG_LENGTHS[r] == 0 else POOL[NEG_OFFSETS[r]]), r
        assert g["scale"][b] == f32(SCALES[r]), r
        check(g, expected(r, b, first_step), (first_step, r))


def test_intake_flag_waits_with_the_conditional_half(dispatch):
    got = dispatch([dict(r=r, b=2, first_step=3) for r in range(R)])
    # prompt_context_from = 0, 2, 0, 1, 0: p_0 enters for r0, r2 and r4 -- but r0's conditional half waits, so not yet
    assert [g["take"][2] for g in got] == [0, 0, 1, 0, 1]


def test_only_the_pair_is_written_and_the_flags_are_the_advances(dispatch):
    for b in range(B):
        g = dispatch([dict(r=2, b=b, first_step=4)])[0]
        assert g["started"] == [CANARY] * (2 * B) and g["pair_started"] == [CANARY] * B
        assert g["pointers_kept"]
        for other in set(range(B)) - {b}:
            assert g["slots"][4 * other:4 * other + 4] == [CANARY] * 4 and g["slots"][4 * (B + other):4 * (B + other) + 4] == [CANARY] * 4
            assert g["tokens"][other] == CANARY and g["tokens"][B + other] == CANARY and g["scale"][other] == CANARY
        check(g, expected(2, b, 4), b)


def test_every_optional_array_null_in_turn(dispatch):
    """Nothing of a feature the call is without is dereferenced -- the sanitizers decide -- and everything else is written as with it."""
    for r in (0, 1, 3):
        cases = [dict(r=r, b=0, first_step=5, off=(name,)) for name in OPTIONAL]
        cases.append(dict(r=r, b=0, first_step=5, off=tuple(OPTIONAL)))               # the arg-max queue
        for c, g in zip(cases, dispatch(cases)):
            check(g, expected(**c), (r, c["off"]))


def test_a_call_without_the_new_arrays_writes_what_the_rule_wrote_before(dispatch):
    """queue_dispatch over a QueueBufs that names none of the guided arrays: slot b's rows as the contract of wrk_v7_generate_queue
    has them, and not a word of the partner's entries, the scales or the flags."""
    cases = [dict(rule="plain", r=r, b=b, first_step=f) for r in range(R) for b, f in ((0, 0), (2, 7))]
    cases += [dict(rule="plain", r=1, b=1, first_step=2, off=(name,)) for name in OPTIONAL]
    for c, g in zip(cases, dispatch(cases)):
        check(g, expected(**c), c)
        b = c["b"]
        assert g["tokens"][B:] == [CANARY] * B and g["slots"][4 * B:] == [CANARY] * (4 * B) and g["scale"] == [CANARY] * B
        assert g["slots"][4 * b + 3] in (PROMPT, REPLY) and (g["start_cond"], g["start_part"]) == (0, 0)
