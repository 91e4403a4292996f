"""The request queue's dispatch rule (web-rwkv-gguf_amd/csrc/wrk_queue_dispatch.h queue_dispatch), on the CPU.

tests/host/queue_dispatch_main.cpp includes that HIP-free header alone, runs one dispatch per case over host arrays pre-filled with a
canary and prints every word the arrays then hold.  It is built with the host compiler under the address and undefined-behaviour
sanitizers, linked into the program: a stand-alone executable that runs the same whatever the environment preloads.

Every expectation here is worked from the contract of wrk_v7_generate_queue in include/wrk_hip.h -- never read off the function:
  - "A slot that holds request r feeds p_0 .. p_{n-1} on consecutive steps; the draws of the first n - 1 of them are discarded ... The
    draw of the step that feeds p_{n-1} is reply token y_0 ... The sampler step of y_j is j".  With p_0 fed at step f, y_j is drawn at
    step f + n - 1 + j, and the sampler numbers a draw `step - step_base`: step_base = f + n - 1.  The slot is in the reply phase at
    once iff n == 1.
  - results: "slots, start_steps (the step that fed p_0)", reason 3 while running, length 0 so far.
  - mu, the automaton state, the stop tail and the DRY window: "request r starts from mirostat_mu[r] / in grammar_state[r] / the tail
    starts empty / a slot's window is set to length 0 when a request is dispatched ... never what its slot's previous request left".
  - prompt intake: "with f = prompt_context_from[r] the tokens p_f .. p_{n-1} enter": p_0 enters iff f == 0.
  - a pool: "Request r with start[r] = k begins from a copy of entry k"; with a history the turnover sets the window, not the dispatch.
The world: 3 slots, 4 requests with the values of REQS, every one exact in f32; word-wise dumps, floats as their bits."""
import json
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5A5A5A5
NO_ENTRY = 0xFFFFFFFF
TAIL_LEN, TAIL_EMPTY, DRY_MAX_MATCH = 7, 0xFFFFFFFF, 50        # WRK_STOP_TAIL_LEN, WRK_STOP_TAIL_EMPTY, WRK_DRY_MAX_MATCH
IDLE, PROMPT, REPLY = 0, 1, 2
B, R = 3, 4
POOL = [11, 21, 22, 23, 31, 32, 41, 42, 43]
OFFSETS, LENGTHS = [0, 1, 4, 6], [1, 3, 2, 3]
REQS = [dict(prompt_off=OFFSETS[r], prompt_len=LENGTHS[r], max_new=4 + r, seed=1000 + r, temperature=0.5 + 0.25 * r, top_p=0.5 + 0.125 * r,
             presence=0.25 * (r + 1), frequency=0.125 * (r + 1), decay=1 - 0.0625 * (r + 1), top_k=10 + r, ln_min_p=-(1.5 + r), tau=2.0 + r,
             eta=0.125 * (r + 1), typical_p=0.5 + 0.0625 * r, mu=4 + 0.5 * r, gram=7 + r, ctx_from=[0, 2, 0, 1][r], start=[5, NO_ENTRY, 6, 7][r],
             dry_allowed=2 + r, dry_no_repeat=3 + r, dry_multiplier=0.5 * (r + 1), dry_pen0=100.0 * (r + 1)) for r in range(R)]
OPTIONAL = ["sample", "pen", "filter", "alt", "mu", "gram", "dry", "seq", "intake"]


def f32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


@pytest.fixture(scope="module")
def dispatch(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host compiler g++ is required"
    exe = str(tmp_path_factory.mktemp("queue_dispatch") / "queue_dispatch")
    cmd = [cxx, "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "web-rwkv-gguf_amd", "csrc"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-g",
           os.path.join(ROOT, "tests", "host", "queue_dispatch_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(cases):
        """cases: [dict(r, b, first_step, pool, history, turn_at, save, off)] -> one dump per case"""
        lines = []
        for i, c in enumerate(cases):
            lines.append(f"case c{i} {B} {R} {c['r']} {c['b']} {c['first_step']} {int(c.get('pool', False))} {int(c.get('history', False))} "
                         f"{c.get('turn_at', 0)} {c.get('save', NO_ENTRY)} {','.join(c.get('off', ())) or '-'}")
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
    per_slot = dict(tokens=1, started=1, slots=4, sample=4, filter=2, alt=4, gram_state=1, tail=TAIL_LEN, take=1, pen=4, dry=4 + DRY_MAX_MATCH + 2,
                    turn=4)
    w = {k: [CANARY] * (n * B) for k, n in per_slot.items()}
    w.update(log=[CANARY] * (4 * R), seq_match=[CANARY] * R, pointers_kept=True)
    return w


def put(w, key, index, words):
    n = len(words)
    w[key][index * n:(index + 1) * n] = words


def expected(r, b, first_step, pool=False, history=False, turn_at=0, save=NO_ENTRY, off=()):
    """the world after request r went to slot b with p_0 fed at first_step, clause by clause from the contract (module docstring)"""
    q, n, w = REQS[r], LENGTHS[r], untouched()
    put(w, "tokens", b, [POOL[OFFSETS[r]]])                             # p_0
    put(w, "slots", b, [r, 0, 0, REPLY if n == 1 else PROMPT])          # nothing fed, nothing drawn yet
    put(w, "log", r, [0, 3, b, first_step])
    if "sample" not in off:
        put(w, "sample", b, [f32(q["temperature"]), f32(q["top_p"]), q["seed"], first_step + n - 1])
    if "filter" not in off:
        put(w, "filter", b, [q["top_k"], f32(q["ln_min_p"])])
    if "alt" not in off:                                                # without the mu array (a typical pick): mu 0, never read
        put(w, "alt", b, [f32(q["tau"]), f32(q["eta"]), f32(0.0 if "mu" in off else q["mu"]), f32(q["typical_p"])])
    if "gram" not in off:
        put(w, "gram_state", b, [q["gram"]])
    if "seq" not in off:
        put(w, "tail", b, [TAIL_EMPTY] * TAIL_LEN)
    if "intake" not in off:
        put(w, "take", b, [int(q["ctx_from"] == 0)])
    if "pen" not in off:                                                # the values; the pad word is nobody's
        put(w, "pen", b, [f32(q["presence"]), f32(q["frequency"]), f32(q["decay"]), CANARY])
    if "dry" not in off:                                                # the values and the table [0, 50]; cap and the padding entry are the slot's
        put(w, "dry", b, [CANARY, q["dry_allowed"], q["dry_no_repeat"], f32(q["dry_multiplier"])] +
            [f32(q["dry_pen0"] + m) for m in range(DRY_MAX_MATCH + 1)] + [CANARY])
    if pool:
        put(w, "turn", turn_at, [b, save, 1, q["start"]])
    w["wipe"] = "dry" not in off and not (pool and history)
    return w


def check(got, want, what):
    got = {k: v for k, v in got.items() if k != "name"}
    assert got.keys() == want.keys(), what
    for k in want:
        assert got[k] == want[k], (what, k)


@pytest.mark.parametrize("first_step", [0, 5])
@pytest.mark.parametrize("n", [1, 3])
def test_sampler_row_slot_record_and_log(dispatch, first_step, n):
    r, b = {1: 0, 3: 1}[n], 2
    assert LENGTHS[r] == n
    got = dispatch([dict(r=r, b=b, first_step=first_step)])[0]
    assert got["slots"][4 * b:4 * b + 4] == [r, 0, 0, REPLY if n == 1 else PROMPT]      # pos = reply = 0
    assert got["tokens"][b] == {0: 11, 1: 21}[r]
    assert got["log"][4 * r:4 * r + 4] == [0, 3, b, first_step]
    # y_j is drawn at step first_step + n - 1 + j and must have sampler step j
    base = {(0, 1): 0, (0, 3): 2, (5, 1): 5, (5, 3): 7}[(first_step, n)]
    assert got["sample"][4 * b:4 * b + 4] == [f32(0.5 + 0.25 * r), f32(0.5 + 0.125 * r), 1000 + r, base]
    check(got, expected(r, b, first_step), (first_step, n))


def test_other_slot_rows(dispatch):
    r, b = 2, 1
    got = dispatch([dict(r=r, b=b, first_step=9)])[0]
    assert got["filter"][2 * b:2 * b + 2] == [12, f32(-3.5)]
    assert got["alt"][4 * b:4 * b + 4] == [f32(4.0), f32(0.375), f32(5.0), f32(0.625)]          # (tau, eta, mu_start[r], typical_p)
    assert got["gram_state"][b] == 9                                                            # start_state[r]
    assert got["tail"][TAIL_LEN * b:TAIL_LEN * (b + 1)] == [TAIL_EMPTY] * TAIL_LEN
    check(got, expected(r, b, 9), "request 2 to slot 1")


def test_slot_pointers_kept(dispatch):
    r, b = 3, 0
    got = dispatch([dict(r=r, b=b, first_step=1)])[0]
    assert got["pointers_kept"]        # count / flags / weight of every penalty row, ring / meta of every DRY row, and the requests' mu / states
    assert got["pen"][4 * b:4 * b + 3] == [f32(1.0), f32(0.5), f32(0.75)]
    row = got["dry"][(4 + DRY_MAX_MATCH + 2) * b:(4 + DRY_MAX_MATCH + 2) * (b + 1)]
    assert row[0] == CANARY and row[1:4] == [5, 6, f32(2.0)]                                    # capacity kept; allowed, no_repeat, multiplier
    assert row[4:4 + DRY_MAX_MATCH + 1] == [f32(400.0 + m) for m in range(DRY_MAX_MATCH + 1)] and row[-1] == CANARY
    check(got, expected(r, b, 1), "request 3 to slot 0")


def test_intake_flag(dispatch):
    got = dispatch([dict(r=r, b=1, first_step=3) for r in range(R)])
    assert [g["take"][1] for g in got] == [1, 0, 1, 0]                  # prompt_context_from = 0, 2, 0, 1
    for r, g in enumerate(got):
        check(g, expected(r, 1, 3), r)


def test_pool_turn_entry_and_window_answer(dispatch):
    cases = [dict(r=0, b=2, first_step=0, pool=True, turn_at=2),                                    # the host's step 0: nothing to save
             dict(r=2, b=1, first_step=6, pool=True, turn_at=0, save=3),                             # a refill: the slot's last request saves to 3
             dict(r=1, b=0, first_step=6, pool=True, history=True, turn_at=1, save=NO_ENTRY),        # no start entry, with a history pool
             dict(r=3, b=0, first_step=6, history=True)]                                             # the flag of a pool that is not there
    got = dispatch(cases)
    assert got[0]["turn"][8:12] == [2, NO_ENTRY, 1, 5] and got[0]["wipe"] is True
    assert got[1]["turn"][0:4] == [1, 3, 1, 6] and got[1]["wipe"] is True
    assert got[2]["turn"][4:8] == [0, NO_ENTRY, 1, NO_ENTRY] and got[2]["wipe"] is False
    assert got[3]["turn"] == [CANARY] * (4 * B) and got[3]["wipe"] is True
    for c, g in zip(cases, got):
        check(g, expected(**c), c)


@pytest.mark.parametrize("pool", [False, True])
def test_every_optional_array_null_in_turn(dispatch, pool):
    """Nothing of a feature the call is without is dereferenced -- the sanitizers decide -- and everything else is written as with it."""
    cases = [dict(r=1, b=2, first_step=4, pool=pool, turn_at=1, save=2, off=(name,)) for name in OPTIONAL]
    cases.append(dict(r=1, b=2, first_step=4, pool=pool, turn_at=1, save=2, off=tuple(OPTIONAL)))       # the arg-max queue
    for c, g in zip(cases, dispatch(cases)):
        check(g, expected(**c), c["off"])
    assert expected(**cases[-1])["wipe"] is False                       # no window: nothing to empty
