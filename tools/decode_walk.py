"""Walks every decode loop of both runners once and prints SHA-256 digests of everything the calls leave behind: the check that a
change to the loop driver (csrc/wrk_runner.hip) computes bit for bit what the build before it computed.

Configurations: RWKV-7 `small` at B = 1 and at B = 4, RWKV-7 `small` at B = 4 over two concurrent pipelines (groups = 2: the plain and
the stop tail only -- a queue has one lane -- and not with --eager, which the lanes refuse), RWKV-6 `small` at B = 4; each in modes 0 and
1.  In each, {greedy, sampled, sampled + filtered, penalised, penalised + filtered, Mirostat, typical, penalised + Mirostat, sampled
with log-probs and 3 alternatives} x {plain, stop, queue, queue + pool} once with fixed seeds, every call from zeroed state slots and occurrence rows (one token banned per row).  The stop id of a pick is what sequence 0
draws second in the plain call, so the stop and queue calls end sequences early, freeze their slots and leave the polled loop before
max steps; the queue serves B + 2 requests, so slots are refilled, and with a pool every other request starts from a preloaded entry.

Per call one digest over the raw bytes of tokens, lengths, steps run, last logits, the queue's log, the saved flags, `state_back` of
every slot, the occurrence rows, the pool's entries, the Mirostat mu read back and the log-prob arrays.  Prints one JSON object {"config/mode/pick/tail": digest}.

    python tools/decode_walk.py [--eager] [--per-pick] [--out FILE]

--per-pick folds the digests of a pick's tails into one, {"config/mode/pick": digest}: a quarter of the lines to keep in the tree.

Two builds are compared by running this under each (WRK_LIB_DIR selects the library directory) and comparing the objects key for key.
--eager sets WRK_NO_GRAPH=1: every step is enqueued instead of replayed from a captured program.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "web-rwkv-gguf_amd"))

PICKS = ("greedy", "sample", "sample+filter", "pen", "pen+filter", "mirostat", "typical", "pen+mirostat", "sample+logprobs")
TAILS = ("plain", "stop", "queue", "pool")
STEPS = 6
FIRST = [7, 100, 33, 250]
BANNED = 5


def digest(parts):
    h = hashlib.sha256()
    for p in parts:
        a = np.ascontiguousarray(p)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def fold(out, group=lambda k: k.rsplit("/", 1)[0]):
    """{group(key): one digest over the group's (key, digest) pairs in key order}."""
    groups = {}
    for k in sorted(out):
        groups.setdefault(group(k), hashlib.sha256()).update(f"{k}={out[k]};".encode())
    return {g: h.hexdigest() for g, h in groups.items()}


def walk(wrk, ctx, name, data, B, groups, out):
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    V = rt.info.num_vocab
    R = B + 2
    occ = wrk.Occurrence(ctx, B, V)
    pool = wrk.StatePool(ctx, rt, R + 1)
    zero = np.zeros_like(rt.state_back(0))
    preload = (np.random.default_rng(11).standard_normal(zero.shape) * 0.01).astype(np.float32)
    first = FIRST[:B]
    skw = dict(temperature=np.linspace(0.8, 1.2, R).tolist(), top_p=np.linspace(0.95, 0.85, R).tolist(), seed=list(range(21, 21 + R)))
    fkw = dict(skw, top_k=[3 + r for r in range(R)], min_p=0.02)
    pkw = dict(presence=0.4, frequency=0.3, decay=0.99)
    mkw = dict(skw, mirostat=(np.linspace(3.0, 5.0, R).tolist(), 0.1))
    picks = {"greedy": {}, "sample": skw, "sample+filter": fkw, "pen": dict(skw, **pkw), "pen+filter": dict(fkw, **pkw), "mirostat": mkw,
             "typical": dict(skw, typical_p=np.linspace(0.9, 0.5, R).tolist()), "pen+mirostat": dict(mkw, **pkw),
             "sample+logprobs": dict(skw, logprobs=3)}
    requests = [[first[r % B] + r, 3 + r, 9][: 1 + r % 3] for r in range(R)]

    def rows(kw, n):        # the per-sequence / per-request lists cut to n rows
        def cut(v):
            return tuple(cut(x) for x in v) if isinstance(v, tuple) else v[:n] if isinstance(v, list) else v
        return {k: cut(v) for k, v in kw.items()}

    def call(mode, pick, tail, stop_id):
        for b in range(B):
            rt.state_load(zero, b)
            occ.load(b)
            occ.ban(b, [BANNED])
        pen = pick.startswith("pen")
        if tail in ("plain", "stop"):
            kw = dict(rows(picks[pick], B), mode=mode, groups=groups, want_logits=True)
            if tail == "stop":
                got = rt.generate_stop(first, STEPS, [stop_id], occurrence=occ if pen else None, poll_steps=2, **kw)
            elif pick == "greedy":
                got = rt.generate_greedy(first, STEPS, **kw)
            elif pen:
                got = rt.generate_penalized(first, STEPS, occ, **kw)
            else:
                got = rt.generate_sample(first, STEPS, **kw)
            parts = [got[0], got[1] if tail == "stop" else np.zeros(0), got[2]]
        else:
            pk = {}
            if tail == "pool":
                for k in range(R):
                    pool.load(k, zero)
                pool.load(R, preload)
                pk = dict(pool=pool, save_state=list(range(R)), start_state=[R if r % 2 else None for r in range(R)])
            res, ran = rt.generate_queue(requests, stop=[stop_id], max_new=[2 + r % 3 for r in range(R)], occurrence=occ if pen else None,
                                         poll_steps=2, mode=mode, **rows(picks[pick], R), **pk)
            parts = [np.array([ran], np.uint32)] + [t for t, *_ in res] + [np.array([r[1:] for r in res], np.uint32)]
            if tail == "pool":
                parts += [np.array(rt.last_queue_saved, np.uint32)] + [pool.back(k) for k in range(R + 1)]
        if "mirostat" in pick:
            parts.append(rt.last_mirostat_mu)
        if "logprobs" in pick:
            lp = rt.last_logprobs
            parts += [a for r in lp for a in r] if isinstance(lp, list) else list(lp)
        parts += [rt.state_back(b) for b in range(B)]
        for b in range(B):
            parts += list(occ.back(b))
        return parts

    for mode in (0, 1):
        for pick in PICKS:
            stop_id = 0
            for tail in TAILS:
                if groups > 1 and tail in ("queue", "pool"):
                    continue
                parts = call(mode, pick, tail, stop_id)
                if tail == "plain":
                    stop_id = int(parts[0][1, 0])
                out[f"{name}/mode{mode}/{pick}/{tail}"] = digest(parts)
    rt.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--eager", action="store_true", help="WRK_NO_GRAPH=1: enqueue every step")
    ap.add_argument("--per-pick", action="store_true", help="one digest per pick, over its tails")
    ap.add_argument("--out", help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.eager:
        os.environ["WRK_NO_GRAPH"] = "1"
    import wrk
    from oracle import synth

    v7 = synth.make_v7_gguf(synth.CONFIGS["small"], 42)
    v6 = synth.make_v6_gguf(synth.V6_CONFIGS["small"], 42)
    ctx = wrk.Context(0)
    out = {}
    walk(wrk, ctx, "v7-small-B1", v7, 1, 1, out)
    walk(wrk, ctx, "v7-small-B4", v7, 4, 1, out)
    if not args.eager:
        walk(wrk, ctx, "v7-small-B4-groups2", v7, 4, 2, out)
    walk(wrk, ctx, "v6-small-B4", v6, 4, 1, out)
    ctx.close()
    if args.per_pick:
        out = fold(out)
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
