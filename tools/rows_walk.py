"""Walks the blocking functions on rows of f32 logits once and prints SHA-256 digests of everything they return: the check that a
change under them (csrc/wrk_sample.hip, wrk_score.hip, wrk_logprob.hip, wrk_penalty.hip, the shared row layer) computes bit for bit what
the build before it computed.  The sibling of tools/decode_walk.py, which walks the decode loops.

Shapes: V on each side of every register-copy step of the sampler, of the 2048-logit minimum slice and of the 4096-logit tile; row
stride V and V + 3 (the second takes the scalar loads); one row and three.  Rows: seeded normal logits x 4 (`plain`); the same with a
NaN, a +inf, several -inf, a -0.0 next to a +0.0 and a run of exact ties across index 1024 (`edges`); and `edges` without the +inf,
which would turn every log-prob of the row into NaN (`ties`).  A vocabulary of at most 5 tokens holds what fits.

Per shape and row set, one digest each for: the sampler in its four modes (Mirostat with the returned mu) and at temperature 0;
`score_logits`; `top_logprobs` with 0, 1 and 20 alternatives; `penalize_logits` followed by `Occurrence.back`; `Occurrence.add` with
decay 1 and 0.9 and a repeated token.  These are folded into one digest per vocabulary and row set: prints one JSON object
{"V/rows": digest}; --detail prints {"V/stride/rows/function": digest} instead.  NaN results are digested with the bits they have.

    python tools/rows_walk.py [--detail] [--out FILE]

Two builds are compared by running this under each (WRK_LIB_DIR selects the library directory) and comparing the objects key for key.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "web-rwkv-gguf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from decode_walk import digest, fold  # noqa: E402

VOCABS = (1, 5, 1023, 1024, 1025, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 65536)
PAD = 3


def make_rows(V, seed):
    """{name: [rows]} of f32 [V] each."""
    rng = np.random.default_rng(seed)
    plain, other = ((rng.standard_normal(V) * 4).astype(np.float32) for _ in range(2))
    edges = other.copy()
    if V <= 5:
        edges[:] = [np.nan, -0.0, 0.0, -np.inf, np.inf][:V] if V > 1 else [-0.0]
    else:
        edges[2], edges[3] = np.nan, np.inf
        edges[5], edges[6] = -0.0, 0.0
        edges[[7, 9, V - 1]] = -np.inf
        lo = 1020 if V >= 1030 else V // 2 - 2
        edges[lo:lo + 10 if V >= 1030 else lo + 4] = 2.5
    ties = edges.copy()
    ties[np.isposinf(ties)] = 0.0
    return {"plain": [plain], "edges": [edges], "ties": [ties], "three": [plain, edges, ties]}


def fold_rows(out):
    """{"V/rows": digest over both strides and the five functions}"""
    return fold(out, lambda k: "/".join(k.split("/")[::2]))


def sample(wrk, ctx, buf, V, stride, n, family, temperature):
    """Context.sample_logits on rows `stride` floats apart (it takes stride == V only): tokens, and mu for Mirostat."""
    C, hip, f32p, u32p, ptr, per_row = wrk.C, wrk.hip, wrk._f32p, wrk._u32p, wrk._ptr, wrk._per_row
    t, p = per_row(temperature, n, np.float32), per_row([0.9, 0.5, 1.0][:n], n, np.float32)
    sd, out = per_row([21, 22, 23][:n], n, np.uint32), np.zeros(n, np.uint32)
    head = (ctx.h, buf.h, V, stride, n, ptr(t, f32p), ptr(p, f32p))
    tail = (ptr(sd, u32p), 3, ptr(out, u32p))
    if family == "plain":
        ctx.check(hip.wrk_sample_logits(*head, *tail))
    elif family == "filtered":
        tk, mp = per_row(40, n, np.uint32), per_row(0.02, n, np.float32)
        ctx.check(hip.wrk_sample_logits_filtered(*head, ptr(tk, u32p), ptr(mp, f32p), *tail))
    elif family == "mirostat":
        tau, eta, mu = wrk._mirostat_rows(([5.0, 3.0, 4.0][:n], 0.1), None, n)
        ctx.check(hip.wrk_sample_logits_mirostat(*head, ptr(tau, f32p), ptr(eta, f32p), ptr(mu, f32p), *tail))
        return [out, mu]
    else:
        ty = per_row([0.9, 0.5, 0.2][:n], n, np.float32)
        ctx.check(hip.wrk_sample_logits_typical(*head, ptr(ty, f32p), *tail))
    return [out]


def walk(wrk, ctx, V, stride, name, rows, out):
    n = len(rows)
    a = np.full((n, stride), 7.0, np.float32)       # the padding beats every logit: a read past V would show
    for r, x in enumerate(rows):
        a[r, :V] = x
    flat = a.reshape(-1)[: (n - 1) * stride + V]
    buf = ctx.buffer(flat)
    key = f"V{V}/stride+{stride - V}/{name}/"
    targets = np.array([V // 3, min(5, V - 1), V - 1][:n], np.uint32)
    parts = []
    for family in ("plain", "filtered", "mirostat", "typical"):
        parts += sample(wrk, ctx, buf, V, stride, n, family, [1.0, 0.7, 1.3][:n])
    parts += sample(wrk, ctx, buf, V, stride, n, "plain", 0.0)
    out[key + "sample"] = digest(parts)
    out[key + "score"] = digest(ctx.score_logits(buf, targets, num_vocab=V, row_stride=stride))
    out[key + "top"] = digest([x for k in (0, 1, 20) for x in ctx.top_logprobs(buf, targets, k, num_vocab=V, row_stride=stride)])
    occ = wrk.Occurrence(ctx, n, V)
    parts = []
    for b in range(n):
        occ.add(b, [1 % V, 3 % V, 1 % V], 1.0)
        parts += list(occ.back(b))
        occ.add(b, [int(targets[b]), 1 % V, 1 % V], 0.9)
        parts += list(occ.back(b))
    out[key + "occ"] = digest(parts)
    if V > 1:
        occ.ban(0, [V - 1])
    ctx.penalize_logits(buf, occ, 0.4, [0.3, 0.0, 1.5][:n], num_vocab=V, row_stride=stride)
    parts = [buf.read(np.float32, flat.size)]
    for b in range(n):
        parts += list(occ.back(b))
    out[key + "pen"] = digest(parts)
    occ.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--detail", action="store_true", help="one digest per stride and function")
    ap.add_argument("--out", help="also write the JSON object to this file")
    args = ap.parse_args()
    import wrk

    ctx = wrk.Context(0)
    out = {}
    for V in VOCABS:
        for name, rows in make_rows(V, 1000 + V).items():
            for stride in (V, V + PAD):
                walk(wrk, ctx, V, stride, name, rows, out)
    ctx.close()
    if not args.detail:
        out = fold_rows(out)
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
