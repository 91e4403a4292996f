"""Beam search's pure rule (web-rwkv-gguf_amd/csrc/wrk_beam_select.h beam_select_group), on the CPU.

tests/host/beam_select_main.cpp includes that HIP-free header alone, runs one step per group over output arrays of exactly W entries
pre-filled with a canary and prints every word they then hold.  It is built with the host compiler under the address and
undefined-behaviour sanitizers, linked into the program: a stand-alone executable that runs the same whatever the environment preloads.

The dumps are compared word for word -- score and key bits, length, status, token, parent, ended -- with the hand-worked groups of
tests/beam_cases.py and, on 200 random groups, with tests/beam_ref.py (the rule in NumPy, written from the header's contract).  The random
groups: W in {1, 2, 3, 4, 16}; scores and log-probs from nine values, all multiples of 1/4, so equal keys are common and every sum is
exact; statuses mixed; rows of a LIVE slot sorted as the sampler sorts them, some with a -inf or NaN tail; length_penalty 0 or 1."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import beam_cases as bc
import beam_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5A5A5A5
VALUES = np.array([0.0, -0.25, -0.5, -0.75, -1.0, -1.5, -2.0, -3.0, -5.25], np.float32)


def bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "the host compiler g++ is required"
    exe = str(tmp_path_factory.mktemp("beam_select") / "beam_select")
    cmd = [cxx, "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "web-rwkv-gguf_amd", "csrc"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-g",
           os.path.join(ROOT, "tests", "host", "beam_select_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(groups):
        """groups: [(W, inv_norm, stop, score, key, length, status, ids [W][W], lp [W][W])] -> one dump per group"""
        lines = []
        for i, (W, inv, stop, score, key, length, status, ids, lp) in enumerate(groups):
            lines.append(f"case g{i} {W}")
            lines.append(f"inv {len(inv)} " + " ".join(str(bits(x)) for x in inv))
            lines.append(f"stop {len(stop)} " + " ".join(str(int(s)) for s in sorted(stop)))          # the rule searches a sorted set
            lines += [f"slot {bits(score[b])} {bits(key[b])} {int(length[b])} {int(status[b])}" for b in range(W)]
            lines += ["row " + " ".join(f"{int(ids[b][j])} {bits(lp[b][j])}" for j in range(W)) for b in range(W)]
        ran = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert ran.returncode == 0, ran.stdout + ran.stderr
        out = [json.loads(line) for line in ran.stdout.splitlines()]
        assert len(out) == len(groups), ran.stdout + ran.stderr
        return out
    return run


def check(got, want, what):
    assert got["inputs_kept"] is True, what
    for k in ("slots", "token", "parent", "ended"):
        assert CANARY not in got[k] or CANARY in want[k], (what, k)     # every word of every slot is written
        assert got[k] == want[k], (what, k)


def test_hand_worked_groups(rule):
    names = sorted(bc.CASES)
    groups = []
    for n in names:
        c = bc.CASES[n]
        score, key, length, status, ids, lp = bc.arrays(c)
        groups.append((c["W"], br.inv_norm_table(c["alpha"], int(length.max()) + 1), c["stop"], score, key, length, status, ids, lp))
    for n, got in zip(names, rule(groups)):
        check(got, bc.want_words(bc.CASES[n]), n)


def random_group(rng, W):
    alpha = float(rng.integers(0, 2))
    length = rng.integers(0, 7, W).astype(np.uint32)
    status = rng.choice([br.DEAD, br.LIVE, br.LIVE, br.DONE], W).astype(np.uint32)
    score = rng.choice(VALUES, W).astype(np.float32)
    inv = br.inv_norm_table(alpha, 8)
    key = np.array([np.float32(score[b] * inv[max(int(length[b]), 1)]) for b in range(W)], np.float32)
    for b in range(W):
        if status[b] == br.DEAD:
            score[b] = key[b] = -np.inf
    ids = rng.integers(0, 32, (W, W)).astype(np.uint32)
    lp = -np.sort(-rng.choice(VALUES, (W, W)).astype(np.float32), axis=1)      # descending, as the sampler's order gives them
    for b in range(W):
        cut = int(rng.integers(0, 2 * W + 1))       # the candidates at or past `cut` have no finite logit
        if cut < W:
            lp[b, cut:] = np.nan if rng.integers(0, 4) == 0 else -np.inf
    stop = [int(x) for x in rng.choice(32, int(rng.integers(0, 5)), replace=False)]
    return W, inv, stop, score, key, length, status, ids, lp


def test_random_groups(rule):
    rng = np.random.default_rng(20240611)
    groups = [random_group(rng, [1, 2, 3, 4, 16][i % 5]) for i in range(200)]
    seen = dict(ties=0, done_out=0, dead=0)
    for i, (g, got) in enumerate(zip(groups, rule(groups))):
        W, inv, stop, score, key, length, status, ids, lp = g
        want = br.select_group(score, key, length, status, ids, lp, inv, stop)
        check(got, bc.got_words(want), (i, W))
        keys = want["key"][want["status"] != br.DEAD]
        seen["ties"] += len(set(keys.tolist())) < len(keys)
        seen["done_out"] += int(((status == br.DONE) & (want["status"] != br.DONE)).any())
        seen["dead"] += int((want["status"] == br.DEAD).any())
    assert min(seen.values()) >= 20, seen       # the set is not vacuous: equal keys, pushed-out DONE slots and DEAD slots all occur
