"""The cut words of the request queue's dispatch rule (web-rwkv-gguf_amd/csrc/wrk_queue_dispatch.h queue_dispatch), on the CPU.

tests/host/queue_dispatch_cut_main.cpp includes that HIP-free header alone, runs one dispatch per case over host arrays pre-filled with
a canary and prints every word the arrays then hold.  It is built with the host compiler under the address and undefined-behaviour
sanitizers, linked into the program: a stand-alone executable that runs the same whatever the environment preloads.

The one function serves the host's step 0 (first_step 0, over host mirrors) and the device's refill (first_step > 0); the expectations
are worked from the contract of wrk_queue_cuts in include/wrk_hip.h, never read off the function:
  - "the values are written into the slot's row by the dispatch, at step 0 on the host and at a refill on the device": after request r
    goes to slot b the slot's five words are request r's, whatever the slot held, at either first_step;
  - a dispatch writes its own slot: the other slots' rows stay;
  - "with all five arrays NULL the call replays exactly the programs of the selected call": without the rows nothing of them is written
    and every other word is what it is with them.
The world of the program: request i has a prompt of i + 1 tokens 100 + 10 i .., seed 1000 + i, temperature 0.5 + 0.25 i, top_p 0.5,
top_k 3 + i, ln_min_p -1 - i and the cut words (1 + i, -2 - i, -3 - i, 0.125 (1 + i), -4 - i)."""
import json
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5A5A5A5
PROMPT, REPLY = 1, 2
B, R = 3, 4


def f32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def cut_words(r):
    return [f32(1.0 + r), f32(-2.0 - r), f32(-3.0 - r), f32(0.125 * (1 + r)), f32(-4.0 - r)]


@pytest.fixture(scope="module")
def dispatch(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host compiler g++ is required"
    exe = str(tmp_path_factory.mktemp("queue_dispatch_cut") / "queue_dispatch_cut")
    cmd = [cxx, "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "web-rwkv-gguf_amd", "csrc"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-g",
           os.path.join(ROOT, "tests", "host", "queue_dispatch_cut_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(cases):
        """cases: [dict(r, b, first_step, cut)] -> one dump per case"""
        lines = [f"case c{i} {B} {R} {c['r']} {c['b']} {c['first_step']} {int(c['cut'])}" for i, c in enumerate(cases)]
        ran = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert ran.returncode == 0, ran.stdout + ran.stderr
        out = [json.loads(line) for line in ran.stdout.splitlines()]
        assert len(out) == len(cases), ran.stdout + ran.stderr
        return out
    return run


def rest_of_the_world(r, b, first_step):
    """what the dispatch leaves in the arrays that are not the cuts', clause by clause from the queue's contract"""
    n = r + 1
    w = dict(tokens=[CANARY] * B, slots=[CANARY] * (4 * B), log=[CANARY] * (4 * R), sample=[CANARY] * (4 * B), filter=[CANARY] * (2 * B))
    w["tokens"][b] = 100 + 10 * r
    w["slots"][4 * b:4 * b + 4] = [r, 0, 0, REPLY if n == 1 else PROMPT]
    w["log"][4 * r:4 * r + 4] = [0, 3, b, first_step]
    w["sample"][4 * b:4 * b + 4] = [f32(0.5 + 0.25 * r), f32(0.5), 1000 + r, first_step + n - 1]
    w["filter"][2 * b:2 * b + 2] = [3 + r, f32(-1.0 - r)]
    return w


@pytest.mark.parametrize("first_step", [0, 6])      # the host's step 0 / a refill on the device
def test_the_slots_five_words_are_the_requests(dispatch, first_step):
    cases = [dict(r=r, b=b, first_step=first_step, cut=True) for r in range(R) for b in range(B)]
    for c, g in zip(cases, dispatch(cases)):
        want = [CANARY] * (5 * B)
        want[5 * c["b"]:5 * c["b"] + 5] = cut_words(c["r"])
        assert g["cut"] == want, c                      # ... and the other slots' rows are untouched
        assert g["requests_kept"] is True, c
        assert g["wipe"] is False, c
        for k, v in rest_of_the_world(c["r"], c["b"], first_step).items():
            assert g[k] == v, (c, k)


def test_without_the_rows_nothing_is_touched(dispatch):
    """cut_par NULL: nothing is written through it -- the sanitizers decide -- and every other word is what it is with the rows."""
    on = [dict(r=r, b=2 - r % 3, first_step=3, cut=True) for r in range(R)]
    off = [dict(c, cut=False) for c in on]
    for c, a, b_ in zip(on, dispatch(on), dispatch(off)):
        assert b_["cut"] == [CANARY] * (5 * B), c
        assert b_["requests_kept"] is True, c
        for k in ("tokens", "slots", "log", "sample", "filter", "wipe"):
            assert a[k] == b_[k], (c, k)
        for k, v in rest_of_the_world(c["r"], c["b"], 3).items():
            assert b_[k] == v, (c, k)
