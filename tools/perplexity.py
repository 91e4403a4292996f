"""Score token sequences on the device: mean negative log-likelihood, perplexity and greedy-hit rate of a model on given or synthetic
token ids (`Runtime.score_sequences`: per-token log-probs and greedy ranks computed by wrk_score.hip, only NH floats + NH u32 read back).

    python tools/perplexity.py [--gguf FILE | --model 1.5B] [--tokens FILE] [--length 512] [--batch 1] [--chunk 128]
    python tools/perplexity.py --ab [--model 1.5B]                 # score against infer(Full) + host log-softmax, per chunk
    python tools/perplexity.py --kernel-rows 1,128 [--reps 50]      # the kernel alone on rows of V logits (for a kernel trace)

--tokens: a JSON list of ids (one sequence) or of lists (several), or whitespace-separated ids.  Without it, --batch sequences of
--length seeded random ids.  The synthetic bench models (bench.make_model_gguf) have random weights: their perplexity is only a
number to compare builds by.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "web-rwkv-gguf_amd"))


def load_tokens(path):
    text = open(path).read().strip()
    if text.startswith("["):
        v = json.loads(text)
        return [list(map(int, s)) for s in v] if v and isinstance(v[0], list) else [list(map(int, v))]
    return [[int(t) for t in text.split()]]


def zero_state(rt):
    z = np.zeros_like(rt.state_back(0))
    for b in range(rt.num_batch):
        rt.state_load(z, b)


def host_log_softmax_at(logits, targets):
    """What a caller does without device scoring: the full rows (already read back) through an f32 log-softmax."""
    m = logits.max(axis=1, keepdims=True)
    ls = logits - m - np.log(np.exp(logits - m).sum(axis=1, keepdims=True))
    return ls[np.arange(logits.shape[0]), targets]


def ab(rt, reps, mode):
    """Per chunk of B sequences x T tokens, every position scored: score_raw against infer_raw (Full: every row's logits back) + the
    host log-softmax.  Medians of `reps` alternating runs of each, wall time of the whole call."""
    import oracle.rnn as orn

    V = rt.info.num_vocab
    rng = np.random.default_rng(0)
    out = []
    for B, T in ((1, 128), (16, 128), (1, 1), (16, 1)):
        lens = [T] * B
        cursors = orn.stack_cursors(lens)
        tokens = rng.integers(0, V, B * T).tolist()
        headers = list(range(B * T))
        targets = rng.integers(0, V, B * T)
        zero_state(rt)
        lp, _ = rt.score_raw(tokens, cursors, headers, targets, mode=mode)
        zero_state(rt)
        want = host_log_softmax_at(rt.infer_raw(tokens, cursors, headers, mode=mode), targets)
        agree = float(np.abs(lp.astype(np.float64) - want).max())
        s, f = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            rt.score_raw(tokens, cursors, headers, targets, mode=mode)
            s.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            host_log_softmax_at(rt.infer_raw(tokens, cursors, headers, mode=mode), targets)
            f.append((time.perf_counter() - t0) * 1e3)
        sm, fm = float(np.median(s)), float(np.median(f))
        out.append({"batch": B, "tokens_per_sequence": T, "rows": B * T, "score_ms": round(sm, 4), "full_infer_plus_host_ms": round(fm, 4),
                    "saved_ms": round(fm - sm, 4), "bytes_back_score": B * T * 8, "bytes_back_full": B * T * V * 4,
                    "max_abs_dlogprob_vs_host": agree, "score_ms_all": [round(x, 4) for x in s], "full_ms_all": [round(x, 4) for x in f]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gguf", default=None, help="a GGUF model file (default: the bench's synthetic --model)")
    ap.add_argument("--model", default="1.5B")
    ap.add_argument("--weights", type=int, default=0, help="WEIGHTS_INLINE (0), WEIGHTS_INLINE_F16 (1), WEIGHTS_REFERENCE (2)")
    ap.add_argument("--tokens", default=None)
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--mode", type=int, default=1)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--kernel-rows", default=None, help="comma-separated row counts: time the kernel alone on rows of V logits")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import wrk

    ctx = wrk.Context(0)
    if args.kernel_rows:
        V = 65536
        res = {"kernel_rows": [], "num_vocab": V, "reps": args.reps}
        for n in [int(x) for x in args.kernel_rows.split(",")]:
            x = np.random.default_rng(n).normal(0.0, 2.0, (n, V)).astype(np.float32)
            buf = ctx.buffer(x)
            tg = np.arange(n, dtype=np.uint32) % V
            ctx.score_logits(buf, tg, num_vocab=V)
            ms = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                ctx.score_logits(buf, tg, num_vocab=V)
                ms.append((time.perf_counter() - t0) * 1e3)
            res["kernel_rows"].append({"rows": n, "call_ms": round(float(np.median(ms)), 4)})
        ctx.close()
        print(json.dumps(res))
        return

    if args.gguf:
        reader, name = wrk.GgufReader(path=args.gguf), os.path.basename(args.gguf)
    else:
        import bench
        reader, name = wrk.GgufReader(bench.make_model_gguf(args.model, seed=42)), f"RWKV-{args.model} (synthetic, bench.make_model_gguf)"
    seqs = load_tokens(args.tokens) if args.tokens else None
    nb = 16 if args.ab else (len(seqs) if seqs else args.batch)
    rt = wrk.Runtime(ctx, reader, num_batch=nb, weights=args.weights)
    V = rt.info.num_vocab
    if args.ab:
        res = {"model": name, "mode": args.mode, "num_vocab": V, "reps": args.reps, "chunks": ab(rt, args.reps, args.mode)}
    else:
        if seqs is None:
            rng = np.random.default_rng(1)
            seqs = [rng.integers(0, V, args.length).tolist() for _ in range(nb)]
        for s in seqs:
            assert all(0 <= t < V for t in s), "token id out of the vocabulary"
        zero_state(rt)
        t0 = time.perf_counter()
        got = rt.score_sequences(seqs, token_chunk_size=args.chunk, mode=args.mode)
        dt = time.perf_counter() - t0
        lp = np.concatenate([g[0] for g in got]).astype(np.float64)
        rk = np.concatenate([g[1] for g in got])
        nll = float(-lp.mean()) if lp.size else float("nan")
        res = {"model": name, "sequences": len(seqs), "tokens": int(sum(len(s) for s in seqs)), "scored_positions": int(lp.size),
               "token_chunk_size": args.chunk, "mode": args.mode, "mean_nll": nll, "perplexity": float(np.exp(nll)),
               "greedy_hit_rate": float((rk == 0).mean()) if rk.size else float("nan"),
               "tokens_per_s": float(sum(len(s) for s in seqs) / dt)}
    rt.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
