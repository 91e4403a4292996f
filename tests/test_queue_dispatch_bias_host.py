"""The bias word of the request queue's dispatch rule (web-rwkv-gguf_amd/csrc/wrk_queue_dispatch.h queue_dispatch), on the CPU.

tests/host/queue_dispatch_bias_main.cpp includes that HIP-free header alone, runs one dispatch per case over host arrays pre-filled
with a canary and prints every word the arrays then hold.  It is built with the host compiler under the address and
undefined-behaviour sanitizers, linked into the program: a stand-alone executable that runs the same whatever the environment preloads.

Every expectation here is worked from the contract of wrk_queue_options in include/wrk_hip.h -- never read off the function:
  - "Request r's rows are biased with set bias_set[r] from the step it is dispatched, at step 0 or at a refill on the device, and never
    with what its slot's previous request used": after request r goes to slot b, the slot's word is request r's, whatever it held.
  - "bias NULL exactly the programs it ran before": without the two arrays nothing of them is read or written and everything else a
    dispatch writes is what it writes with them.
  - a dispatch writes its own slot: the other slots' words stay.
The world of the program: request i has a prompt of i + 1 tokens 100 + 10 i .., seed 1000 + i, temperature 0.5 + 0.25 i, top_p 0.5 and
automaton state 7 + i; the call has a sampler and a grammar."""
import json
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5A5A5A5
NONE = 0xFFFFFFFF           # WRK_BIAS_NONE
PROMPT, REPLY = 1, 2
B, R = 3, 4
WORDS = [5, NONE, 0, 5]     # the requests' set words: two share a set, one has none


def f32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


@pytest.fixture(scope="module")
def dispatch(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host compiler g++ is required"
    exe = str(tmp_path_factory.mktemp("queue_dispatch_bias") / "queue_dispatch_bias")
    cmd = [cxx, "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "web-rwkv-gguf_amd", "csrc"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-g",
           os.path.join(ROOT, "tests", "host", "queue_dispatch_bias_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(cases):
        """cases: [dict(r, b, first_step, bias)] -> one dump per case"""
        lines = [f"case c{i} {B} {R} {c['r']} {c['b']} {c['first_step']} {int(c['bias'])} " + " ".join(map(str, WORDS)) for i, c in enumerate(cases)]
        ran = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert ran.returncode == 0, ran.stdout + ran.stderr
        out = [json.loads(line) for line in ran.stdout.splitlines()]
        assert len(out) == len(cases), ran.stdout + ran.stderr
        return out
    return run


def rest_of_the_world(r, b, first_step):
    """what the dispatch leaves in the arrays that are not the bias's, clause by clause from the queue's contract: p_0 in the slot's
    token, the slot record with nothing fed or drawn, the log entry (length 0, reason 3 while running, slot, the step that fed p_0),
    the sampler row with step base first_step + n - 1, the request's automaton state"""
    n = r + 1
    w = dict(tokens=[CANARY] * B, slots=[CANARY] * (4 * B), log=[CANARY] * (4 * R), sample=[CANARY] * (4 * B), gram_state=[CANARY] * B)
    w["tokens"][b] = 100 + 10 * r
    w["slots"][4 * b:4 * b + 4] = [r, 0, 0, REPLY if n == 1 else PROMPT]
    w["log"][4 * r:4 * r + 4] = [0, 3, b, first_step]
    w["sample"][4 * b:4 * b + 4] = [f32(0.5 + 0.25 * r), f32(0.5), 1000 + r, first_step + n - 1]
    w["gram_state"][b] = 7 + r
    return w


@pytest.mark.parametrize("first_step", [0, 6])
def test_the_slots_word_is_the_requests(dispatch, first_step):
    cases = [dict(r=r, b=b, first_step=first_step, bias=True) for r in range(R) for b in range(B)]
    for c, g in zip(cases, dispatch(cases)):
        want = [CANARY] * B
        want[c["b"]] = WORDS[c["r"]]                    # set 5, NONE, set 0, set 5 again: the word as it is, NONE included
        assert g["bias_set"] == want, c                 # ... and the other slots' words are untouched
        assert g["requests_kept"] is True, c            # the requests' words are only read
        assert g["wipe"] is False, c                    # no window in this call
        for k, v in rest_of_the_world(c["r"], c["b"], first_step).items():
            assert g[k] == v, (c, k)


def test_without_the_arrays_nothing_is_touched(dispatch):
    """Both pointers NULL: nothing of them is dereferenced -- the sanitizers decide -- and every other word is what it is with them."""
    on = [dict(r=r, b=2 - r % 3, first_step=3, bias=True) for r in range(R)]
    off = [dict(c, bias=False) for c in on]
    for c, a, b_ in zip(on, dispatch(on), dispatch(off)):
        assert b_["bias_set"] == [CANARY] * B, c
        assert b_["requests_kept"] is True, c
        for k in ("tokens", "slots", "log", "sample", "gram_state", "wipe"):
            assert a[k] == b_[k], (c, k)
        for k, v in rest_of_the_world(c["r"], c["b"], 3).items():
            assert b_[k] == v, (c, k)
