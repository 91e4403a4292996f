"""Cost of on-device sampling in the decode loop: generate_greedy against generate_sample (T = 1, top_p = 0.9) on the bench's synthetic
RWKV-7 1.5B Q4_K_M model, alternating the two, medians of the per-step time (HIP events around the replays).  Also prints, as context,
what the host alternative would cost per step: reading the logits back and a NumPy restatement of chat.rs's sampler per row.
A third leg, alternating with the other two, is generate_penalized with the same sampler parameters and ChatRWKV-style repetition
penalties (presence = frequency = 0.2, decay = 0.996, 16 banned tokens per sequence; --no-penalized skips it).

A fourth leg (--stop) is generate_stop with the same sampler parameters: the per-step cost of a stop program that never stops (16 stop
ids per sequence that are not drawn) against the sampled leg, for every --poll block size and with polling off, and the wall time of a
call with --stop-steps steps whose sequences all end by about step 32 against the same call without stops.

A fifth pair of legs (--top-k K and / or --min-p M), alternating with the others: generate_sample with the top-k / min-p cuts next to
the same top_p (the filtered kernel's fused boundary descent), and with --top-k also top_k alone at top_p = 1 (its count-only descent),
each against the plain sampled leg, with the run-to-run spread of both.

A sixth leg (--logprobs N[,N...]): the decode loop with log-probs and N alternatives per token against the same loop
without them -- both through the options entry point without stop sets, so the step programs differ by the log-prob launches alone --
for the greedy and the sampled pick, alternating, with the run-to-run spread of both; and, as context, the host route: leaving the
loop after every step to read back last_logits (wall time per step of one-step calls).

A seventh pair of legs (--mirostat TAU,ETA and / or --typical P): the decode loop with the Mirostat v2 / the locally typical pick
 against the plain sampler loop of the same run -- all through the options entry point without stop sets, so the step
programs differ by the sampler launch alone -- alternating, with the run-to-run spread of each.  Every call starts from the same state.

Cut legs (--xtc P,T, --top-n-sigma N, --eta E): generate_sample with each cut added to the filtered sampler's parameters
(--top-k / --min-p, else top_k = 40 and min_p = 0.05, at the same top_p), and all given cuts together, alternating with that filtered
step, medians and each leg's run-to-run spread: the step programs differ by the sampler kernel's instantiation alone.

An eighth leg (--grammar): the decode loop constrained by a two-state automaton that allows about half of the vocabulary in either state
 against the same loop without a grammar -- both through the options entry point without stop sets, so the step programs
differ by the mask launch and the advance launch alone -- for the greedy and the plain-sampler pick, alternating, with the run-to-run
spread of each.  Every call starts from the same state; the unconstrained tokens are recorded (as a hash) so that the same leg on another
build can be compared with them.

A ninth leg (--stop-seq): the stop-sequence step program with 8 sequences of 8 ids per sequence that never match against
the stop program with 16 ids that never match and against the plain sampled step, alternating, with the run-to-run spread of each; at the
runtime's full batch the same for a queue whose requests never end.  The stop-sequence program has the launch count of the stop program.

A tenth leg (--dry): the decode loop with a token window and DRY at text-generation-webui's defaults (multiplier 0.8, base 1.75,
allowed_length 2) against the same loop without a window -- both through the options entry point without stop sets, so
the step programs differ by the row copy, dry_rows and window_push alone -- for the greedy and the plain-sampler pick, alternating, with
the run-to-run spread of each; and the kernel's worst case: one-step calls whose windows hold 4096 equal tokens (4095 candidates that
all reach the cap and meet at one token) against one-step calls whose windows hold one token.

An eleventh leg (--logit-bias N): the decode loop with a logit bias of N entries per sequence (every sequence its own set,
a quarter of the entries bans, the rest uniform in [-4, 4]) against the same loop without a bias -- both through the options entry point
without stop sets, so the step programs differ by the bias_rows launch alone -- for the greedy and the plain-sampler pick, alternating,
with the run-to-run spread of each.  Every call starts from the same state.

A twelfth leg (--beam W): generate_beam with W beams per group on the B slots (B / W groups, --beam-length-penalty, no stop set, so every
step runs) against generate_greedy on the same B slots, alternating, with the run-to-run spread of each, and next to them
the bytes the slot permutation may move per step and moved on average.  Every call starts from the same states.  With --beam-ngram N,
--beam-penalty P,F or --beam-grammar each of those contexts per hypothesis is timed too, the context loop against the
same beam loop without a context, alternating, with the spread of each.

A thirteenth leg (--guidance S): generate_guided of B sequences with scale S and the plain-sampler pick (B conditional
slots and B partner slots, so the runtime gets 2B slots) against the plain sampled loop of the options entry point on the same 2B slots,
alternating, with the run-to-run spread of each: the step programs differ by guide_rows and guide_follow and by the pick, which runs on
B rows instead of 2B.  Every call starts from the same states.  With --guidance the one runtime of the process has 2 * max(batches) slots,
so the other legs of that invocation run on a larger state than in an invocation without the flag: compare those legs between
invocations of the same kind only.

    python tools/sample_bench.py [--batches 1,16,32] [--steps 64] [--reps 7] [--no-penalized] [--stop] [--poll 4,8,16,32,64]
                                 [--top-k 40] [--min-p 0.05] [--logprobs 0,5,20] [--mirostat 5,0.1] [--typical 0.9] [--grammar] [--stop-seq]
                                 [--dry] [--logit-bias 64] [--beam 4 [--beam-ngram 3] [--beam-penalty 0.5,0.5] [--beam-grammar]]
                                 [--guidance 1.5]

Prints one JSON object.
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

import bench  # noqa: E402  (the bench's model writer; bench.py itself is not changed)


def chat_rs_sample(probs, top_p, temp, u):
    """examples/chat.rs:150-190 in NumPy f32: sort, scan to top_p, p^(1/T), normalise, find_or_first."""
    order = np.argsort(-probs, kind="stable")
    sp = probs[order]
    cum = np.cumsum(sp, dtype=np.float32)
    n = int(np.count_nonzero((cum - sp) <= top_p))
    w = sp[:n] ** np.float32(1.0 / temp)
    c = np.cumsum(w / w.sum(), dtype=np.float32)
    hit = np.flatnonzero(u <= c)
    return int(order[hit[0] if hit.size else 0])


POLL_OFF = 0xffffffff       # one block: the live count is copied once, after the last step


def stop_leg(rt, first, B, V, args):
    """Every call starts from the same state (device snapshots), so the sampled run and the stopped runs draw the same tokens."""
    skw = dict(temperature=args.temperature, top_p=args.top_p)
    start = [rt.state_read(b) for b in range(B)]

    def reset():
        for b in range(B):
            rt.state_write(start[b], b)

    def wall(fn):
        reset()
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r
    reset()
    drawn, _ = rt.generate_sample(first, args.steps, **skw)
    used = set(drawn.reshape(-1).tolist())
    never = [i for i in range(V - 1, -1, -1) if i not in used][:16]
    polls = [int(x) for x in args.poll.split(",")] + [POLL_OFF]
    per = {p: [] for p in polls}
    samp, never_stopped = [], True
    for p in polls:                                                      # capture and warm up
        reset()
        rt.generate_stop(first, 4, never, poll_steps=p, **skw)
    for _ in range(args.reps):
        reset()
        samp.append(rt.generate_sample(first, args.steps, **skw)[1] / args.steps)
        for p in polls:
            reset()
            tok, lens = rt.generate_stop(first, args.steps, never, poll_steps=p, **skw)
            never_stopped &= bool((lens == args.steps).all()) and np.array_equal(tok, drawn)
            per[p].append(rt.last_stop_ms / args.steps)
    sm = float(np.median(samp))
    res = {"never_stops": never_stopped, "sample_ms_per_step": round(sm, 5), "sample_ms_all": [round(x, 5) for x in samp],
           "sample_spread_us": round((max(samp) - min(samp)) * 1e3, 2), "poll": []}
    for p in polls:
        m = float(np.median(per[p]))
        res["poll"].append({"poll_steps": "off" if p == POLL_OFF else p, "stop_ms_per_step": round(m, 5),
                            "stop_minus_sample_us": round((m - sm) * 1e3, 2), "stop_ms_all": [round(x, 5) for x in per[p]]})
    # early exit: every sequence ends by about step 32 of a long call
    reset()
    head, _ = rt.generate_sample(first, 40, **skw)
    stops = []
    for b in range(B):
        col = head[:, b].tolist()
        j = next((j for j in range(24, 40) if col[j] not in col[:j]), None)
        stops.append([col[j]] if j is not None else [])
    long_plain, long_stop, runs = [], [], []
    for _ in range(3):
        long_plain.append(wall(lambda: rt.generate_sample(first, args.stop_steps, **skw))[0])
        ms, (tok, lens) = wall(lambda: rt.generate_stop(first, args.stop_steps, stops, **skw))
        long_stop.append(ms)
        runs.append(int(tok.shape[0]))
    res["early_exit"] = {"steps": args.stop_steps, "lengths_max": int(lens.max()), "steps_run": runs, "poll_steps": "default",
                         "plain_wall_ms": [round(x, 3) for x in long_plain], "stop_wall_ms": [round(x, 3) for x in long_stop]}
    reset()
    return res


def stopseq_leg(rt, first, B, V, args):
    """Medians of the per-step time, alternating in one process and every call from the same state: the plain sampled step, the stop
    program with 16 stop ids per sequence that are never drawn (the --stop leg at polling off), and the stop-sequence program with 8
    stop sequences of 8 ids per sequence that never match.  At the runtime's full batch also the queue: one request per slot that never
    ends, with the 16 ids against with the 8 x 8 sequences."""
    skw = dict(temperature=args.temperature, top_p=args.top_p)
    start = [rt.state_read(b) for b in range(B)]

    def reset():
        for b in range(B):
            rt.state_write(start[b], b)
    reset()
    drawn, _ = rt.generate_sample(first, args.steps, **skw)
    used = set(drawn.reshape(-1).tolist())
    never = [i for i in range(V - 1, -1, -1) if i not in used][:16]
    seqs = [[never[(k + j) % 16] for j in range(8)] for k in range(8)]      # 8 x 8 of ids that are never drawn: one compare per sequence
    legs = {"sample": lambda: rt.generate_sample(first, args.steps, **skw)[1],
            "stop": lambda: (rt.generate_stop(first, args.steps, never, poll_steps=POLL_OFF, **skw), rt.last_stop_ms)[1],
            "stop_seq": lambda: (rt.generate_stop(first, args.steps, [], poll_steps=POLL_OFF, stop_sequences=seqs, **skw), rt.last_stop_ms)[1]}
    queue = B == rt.num_batch
    if queue:
        qkw = dict(max_new=args.steps, max_steps=args.steps, poll_steps=POLL_OFF, **skw)
        legs["queue_stop"] = lambda: (rt.generate_queue([[t] for t in first], stop=never, **qkw), rt.last_queue_ms)[1]
        legs["queue_stop_seq"] = lambda: (rt.generate_queue([[t] for t in first], stop_sequences=seqs, **qkw), rt.last_queue_ms)[1]
    reset()
    tok, lens = rt.generate_stop(first, args.steps, [], poll_steps=POLL_OFF, stop_sequences=seqs, **skw)
    never_stopped = bool((lens == args.steps).all()) and np.array_equal(tok, drawn) and bool((rt.last_stop_match == 0xFFFFFFFF).all())
    per = {k: [] for k in legs}
    for k, fn in legs.items():                                          # capture and warm up
        reset()
        fn()
    for _ in range(args.reps):
        for k, fn in legs.items():
            reset()
            per[k].append(fn() / args.steps)
    med = {k: float(np.median(v)) for k, v in per.items()}
    res = {"never_stops": never_stopped, "sequences": "8 x 8 ids, never drawn", "stop_ids": 16, "poll_steps": "off", "queue_slots": rt.num_batch if queue else None}
    for k, v in per.items():
        res[k] = {"ms_per_step": round(med[k], 5), "spread_us": round((max(v) - min(v)) * 1e3, 2), "ms_all": [round(x, 5) for x in v]}
    res["stop_seq_minus_stop_us"] = round((med["stop_seq"] - med["stop"]) * 1e3, 2)
    res["stop_seq_minus_sample_us"] = round((med["stop_seq"] - med["sample"]) * 1e3, 2)
    if queue:
        res["queue_stop_seq_minus_queue_stop_us"] = round((med["queue_stop_seq"] - med["queue_stop"]) * 1e3, 2)
    reset()
    return res


def logprob_leg(rt, first, args):
    """Per pick (greedy, sampled) and per N: medians of the per-step time of generate_stop without stop sets, with logprobs=N against
    without, alternating in one process; every call starts from the same state, so both draw the same tokens."""
    B = len(first)
    ns = [int(x) for x in args.logprobs.split(",")]
    start = [rt.state_read(b) for b in range(B)]

    def run(pick, **kw):
        for b in range(B):
            rt.state_write(start[b], b)
        tok, _ = rt.generate_stop(first, args.steps, [], poll_steps=POLL_OFF, **pick, **kw)
        return tok, rt.last_stop_ms / args.steps
    res = {}
    for name, pick in (("greedy", {}), ("sample", dict(temperature=args.temperature, top_p=args.top_p))):
        want, _ = run(pick)
        for n in ns:                                                       # capture and warm up
            run(pick, logprobs=n)
        base, per, same = [], {n: [] for n in ns}, True
        for _ in range(args.reps):
            base.append(run(pick)[1])
            for n in ns:
                tok, ms = run(pick, logprobs=n)
                same &= bool(np.array_equal(tok, want))
                per[n].append(ms)
        bm = float(np.median(base))
        # the host route: one-step calls, the logits read back after each
        for b in range(B):
            rt.state_write(start[b], b)
        cur, t0 = list(first), time.perf_counter()
        for _ in range(args.steps):
            tok, _, _ = rt.generate_stop(cur, 1, [], want_logits=True, **pick)
            cur = tok[0].tolist()
        host = (time.perf_counter() - t0) * 1e3 / args.steps
        res[name] = {"same_tokens": same, "without_ms_per_step": round(bm, 5), "without_ms_all": [round(x, 5) for x in base],
                     "without_spread_us": round((max(base) - min(base)) * 1e3, 2), "host_route_wall_ms_per_step": round(host, 4), "num_top": []}
        for n in ns:
            m = float(np.median(per[n]))
            res[name]["num_top"].append({"n": n, "with_ms_per_step": round(m, 5), "with_minus_without_us": round((m - bm) * 1e3, 2),
                                         "with_spread_us": round((max(per[n]) - min(per[n])) * 1e3, 2), "with_ms_all": [round(x, 5) for x in per[n]]})
    for b in range(B):
        rt.state_write(start[b], b)
    return res


def alt_leg(rt, first, args):
    """Medians of the per-step time of generate_stop without stop sets with the plain sampler, and with mirostat= / typical_p=,
    alternating in one process; every call starts from the same state."""
    B = len(first)
    start = [rt.state_read(b) for b in range(B)]
    skw = dict(temperature=args.temperature, top_p=args.top_p)
    legs = {"sample": {}}
    if args.mirostat:
        tau, eta = (float(x) for x in args.mirostat.split(","))
        legs["mirostat"] = dict(mirostat=(tau, eta))
    if args.typical is not None:
        legs["typical"] = dict(typical_p=args.typical)

    def run(kw):
        for b in range(B):
            rt.state_write(start[b], b)
        tok, _ = rt.generate_stop(first, args.steps, [], poll_steps=POLL_OFF, **skw, **kw)
        return tok, rt.last_stop_ms / args.steps
    per = {name: [] for name in legs}
    distinct = {name: len(np.unique(run(kw)[0])) for name, kw in legs.items()}       # capture and warm up
    for _ in range(args.reps):
        for name, kw in legs.items():
            per[name].append(run(kw)[1])
    for b in range(B):
        rt.state_write(start[b], b)
    bm = float(np.median(per["sample"]))
    res = {}
    for name in legs:
        m = float(np.median(per[name]))
        res[name] = {"ms_per_step": round(m, 5), "spread_us": round((max(per[name]) - min(per[name])) * 1e3, 2),
                     "ms_all": [round(x, 5) for x in per[name]], "distinct_tokens": distinct[name]}
        if name != "sample":
            res[name]["minus_sample_us"] = round((m - bm) * 1e3, 2)
    return res


def cut_leg(rt, first, args):
    """Medians of the per-step time of generate_sample with the filtered sampler (--top-k / --min-p, else top_k = 40, min_p = 0.05) and
    with each of --xtc P,T / --top-n-sigma N / --eta E added to it, and all of them together, alternating in one process."""
    fkw = dict(temperature=args.temperature, top_p=args.top_p, top_k=40 if args.top_k is None else args.top_k,
               min_p=0.05 if args.min_p is None else args.min_p)
    legs = {"filtered": {}}
    if args.xtc:
        legs["xtc"] = dict(xtc=tuple(float(x) for x in args.xtc.split(",")))
    if args.top_n_sigma is not None:
        legs["top_n_sigma"] = dict(top_n_sigma=args.top_n_sigma)
    if args.eta is not None:
        legs["eta"] = dict(eta_cutoff=args.eta)
    if len(legs) > 2:
        legs["all"] = {k: v for name, kw in legs.items() for k, v in kw.items()}

    def run(kw):
        tok, ms = rt.generate_sample(first, args.steps, **fkw, **kw)
        return tok, ms / args.steps
    per = {name: [] for name in legs}
    distinct = {name: len(np.unique(run(kw)[0])) for name, kw in legs.items()}       # capture and warm up
    for _ in range(args.reps):
        for name, kw in legs.items():
            per[name].append(run(kw)[1])
    bm = float(np.median(per["filtered"]))
    res = {"filters": {k: fkw[k] for k in ("top_k", "min_p")}}
    for name in legs:
        m = float(np.median(per[name]))
        res[name] = {"ms_per_step": round(m, 5), "spread_us": round((max(per[name]) - min(per[name])) * 1e3, 2),
                     "ms_all": [round(x, 5) for x in per[name]], "distinct_tokens": distinct[name]}
        if name != "filtered":
            res[name]["minus_filtered_us"] = round((m - bm) * 1e3, 2)
    return res


def half_vocabulary_automaton(V):
    """Two states over four token classes (id mod 4): state 0 allows classes 0 and 1, state 1 classes 1 and 2; class 1 changes the state."""
    token_class = np.arange(V, dtype=np.uint16) % 4
    rej = 0xFFFF
    return token_class, np.array([[0, 1, rej, rej], [rej, 0, 1, rej]], np.uint16)


def grammar_leg(rt, ctx, first, V, args):
    """Per pick (greedy, sampled): medians of the per-step time of generate_stop without stop sets, with the automaton against without,
    alternating in one process; every call starts from the same state."""
    import hashlib
    import wrk
    B = len(first)
    cls, trans = half_vocabulary_automaton(V)
    g = wrk.Grammar(ctx, V, cls, trans)
    start = [rt.state_read(b) for b in range(B)]

    def run(pick, **kw):
        for b in range(B):
            rt.state_write(start[b], b)
        tok, _ = rt.generate_stop(first, args.steps, [], poll_steps=POLL_OFF, **pick, **kw)
        return tok, rt.last_stop_ms / args.steps
    res = {}
    for name, pick in (("greedy", {}), ("sample", dict(temperature=args.temperature, top_p=args.top_p))):
        want, _ = run(pick)
        con, _ = run(pick, grammar=g, grammar_state=0)                     # capture and warm up
        for b in range(B):
            g.walk(0, con[:, b])                                           # raises at a disallowed token
        accepted = True
        base, with_, same = [], [], True
        for _ in range(args.reps):
            tok, ms = run(pick)
            same &= bool(np.array_equal(tok, want))
            base.append(ms)
            tok, ms = run(pick, grammar=g, grammar_state=0)
            same &= bool(np.array_equal(tok, con))
            with_.append(ms)
        bm, wm = float(np.median(base)), float(np.median(with_))
        res[name] = {"same_tokens_every_rep": same, "constrained_tokens_accepted": accepted,
                     "constrained_differs_from_plain": bool(not np.array_equal(want, con)),
                     "without_tokens_sha1": hashlib.sha1(np.ascontiguousarray(want).tobytes()).hexdigest(),
                     "without_ms_per_step": round(bm, 5), "without_spread_us": round((max(base) - min(base)) * 1e3, 2),
                     "without_ms_all": [round(x, 5) for x in base],
                     "with_ms_per_step": round(wm, 5), "with_spread_us": round((max(with_) - min(with_)) * 1e3, 2),
                     "with_ms_all": [round(x, 5) for x in with_], "with_minus_without_us": round((wm - bm) * 1e3, 2)}
    for b in range(B):
        rt.state_write(start[b], b)
    g.close()
    return res


def dry_leg(rt, ctx, first, V, args):
    """Per pick (greedy, sampled): medians of the per-step time of generate_stop without stop sets, with a token window and DRY against
    without, alternating in one process; every call starts from the same state and from empty windows.  Then the worst case."""
    import hashlib
    import wrk
    B = len(first)
    win = wrk.TokenWindow(ctx, B, V, 1024)
    big = wrk.TokenWindow(ctx, B, V, wrk.MAX_TOKEN_WINDOW)
    start = [rt.state_read(b) for b in range(B)]
    dkw = dict(dry=(0.8, 1.75, 2))

    def run(pick, steps=args.steps, **kw):
        for b in range(B):
            rt.state_write(start[b], b)
        tok, _ = rt.generate_stop(first, steps, [], poll_steps=POLL_OFF, **pick, **kw)
        return tok, rt.last_stop_ms / steps

    def with_dry(pick):
        for b in range(B):
            win.load(b)
        return run(pick, window=win, **dkw)
    res = {}
    for name, pick in (("greedy", {}), ("sample", dict(temperature=args.temperature, top_p=args.top_p))):
        want, _ = run(pick)
        con, _ = with_dry(pick)                                            # capture and warm up
        base, with_, same = [], [], True
        for _ in range(args.reps):
            tok, ms = run(pick)
            same &= bool(np.array_equal(tok, want))
            base.append(ms)
            tok, ms = with_dry(pick)
            same &= bool(np.array_equal(tok, con))
            with_.append(ms)
        bm, wm = float(np.median(base)), float(np.median(with_))
        res[name] = {"same_tokens_every_rep": same, "dry_differs_from_plain": bool(not np.array_equal(want, con)),
                     "without_tokens_sha1": hashlib.sha1(np.ascontiguousarray(want).tobytes()).hexdigest(),
                     "without_ms_per_step": round(bm, 5), "without_spread_us": round((max(base) - min(base)) * 1e3, 2),
                     "without_ms_all": [round(x, 5) for x in base],
                     "with_ms_per_step": round(wm, 5), "with_spread_us": round((max(with_) - min(with_)) * 1e3, 2),
                     "with_ms_all": [round(x, 5) for x in with_], "with_minus_without_us": round((wm - bm) * 1e3, 2)}
    # the worst case: every window holds 4096 times one token, so 4095 candidates walk to the cap and meet at that token's scratch word
    full, one = [], []
    for _ in range(args.reps + 1):
        for b in range(B):
            big.load(b, [7] * wrk.MAX_TOKEN_WINDOW)
        full.append(run({}, steps=1, window=big, **dkw)[1])
        for b in range(B):
            big.load(b, [7])
        one.append(run({}, steps=1, window=big, **dkw)[1])
    full, one = full[1:], one[1:]                                          # the first pair captures the one-step program
    res["worst_case_one_step"] = {"window": "4096 equal tokens", "full_ms": round(float(np.median(full)), 5), "one_token_ms": round(float(np.median(one)), 5),
                                  "full_minus_one_token_us": round((float(np.median(full)) - float(np.median(one))) * 1e3, 2),
                                  "full_ms_all": [round(x, 5) for x in full], "one_token_ms_all": [round(x, 5) for x in one]}
    for b in range(B):
        rt.state_write(start[b], b)
    win.close()
    big.close()
    return res


def bias_leg(rt, ctx, first, V, args):
    """Per pick (greedy, sampled): medians of the per-step time of generate_stop without stop sets, with a bias of args.logit_bias entries
    per sequence against without, alternating in one process; every call starts from the same state."""
    import hashlib
    import wrk
    B = len(first)
    rng = np.random.default_rng(args.logit_bias)
    sets = []
    for _ in range(B):
        vals = rng.uniform(-4, 4, args.logit_bias).astype(np.float32)
        vals[rng.random(args.logit_bias) < 0.25] = -np.inf
        sets.append((rng.choice(V, args.logit_bias, replace=False), vals))
    lb = wrk.LogitBias(ctx, V, sets)
    start = [rt.state_read(b) for b in range(B)]

    def run(pick, **kw):
        for b in range(B):
            rt.state_write(start[b], b)
        tok, _ = rt.generate_stop(first, args.steps, [], poll_steps=POLL_OFF, **pick, **kw)
        return tok, rt.last_stop_ms / args.steps
    bkw = dict(logit_bias=lb, bias_set=list(range(B)))
    res = {}
    for name, pick in (("greedy", {}), ("sample", dict(temperature=args.temperature, top_p=args.top_p))):
        want, _ = run(pick)
        con, _ = run(pick, **bkw)                                          # capture and warm up
        banned = any(v == -np.inf and t in set(con[:, b].tolist()) for b in range(B) for t, v in zip(*sets[b]))
        base, with_, same = [], [], True
        for _ in range(args.reps):
            tok, ms = run(pick)
            same &= bool(np.array_equal(tok, want))
            base.append(ms)
            tok, ms = run(pick, **bkw)
            same &= bool(np.array_equal(tok, con))
            with_.append(ms)
        bm, wm = float(np.median(base)), float(np.median(with_))
        res[name] = {"same_tokens_every_rep": same, "banned_token_drawn": bool(banned), "biased_differs_from_plain": bool(not np.array_equal(want, con)),
                     "without_tokens_sha1": hashlib.sha1(np.ascontiguousarray(want).tobytes()).hexdigest(),
                     "without_ms_per_step": round(bm, 5), "without_spread_us": round((max(base) - min(base)) * 1e3, 2),
                     "without_ms_all": [round(x, 5) for x in base],
                     "with_ms_per_step": round(wm, 5), "with_spread_us": round((max(with_) - min(with_)) * 1e3, 2),
                     "with_ms_all": [round(x, 5) for x in with_], "with_minus_without_us": round((wm - bm) * 1e3, 2)}
    for b in range(B):
        rt.state_write(start[b], b)
    lb.close()
    return res


def beam_leg(rt, first, B, V, args):
    """Medians of the per-step time of generate_beam with args.beam beams per group on B slots (B / beams groups, no stop set, so every
    step runs) against generate_greedy on the same B slots, alternating in one process; every call starts from the same states.  Next to
    them the bytes a step's permutation may move: a gather into the scratch and a scatter back, each at most B slots."""
    W = args.beam
    if B % W:
        return {"skipped": f"{B} slots are not groups of {W} beams"}
    G = B // W
    start = [rt.state_read(b) for b in range(B)]
    slot_bytes = rt.info.num_layer * (rt.info.num_emb // rt.info.num_head + 2) * rt.info.num_emb * 4

    def reset():
        for b in range(B):
            rt.state_write(start[b], b)

    def beam():
        reset()
        res, run = rt.generate_beam(first[:G], args.steps, W, length_penalty=args.beam_length_penalty)
        return res, rt.last_beam_ms / max(run, 1)

    def greedy():
        reset()
        return rt.generate_greedy(first, args.steps)[1] / args.steps
    want, _ = beam()                                                       # capture and warm up
    greedy()
    moved = int((rt.last_beam_steps[1] != np.arange(B)[None, :]).sum())    # slots whose parent is another slot, over the call
    bm, gm, same = [], [], True
    for _ in range(args.reps):
        gm.append(greedy())
        res, ms = beam()
        same &= all(a[0].tolist() == b[0].tolist() and a[1:] == b[1:] for x, y in zip(res, want) for a, b in zip(x, y))
        bm.append(ms)
    reset()
    b_med, g_med = float(np.median(bm)), float(np.median(gm))
    return {"num_beams": W, "groups": G, "length_penalty": args.beam_length_penalty, "same_hypotheses_every_rep": bool(same),
            "beam_ms_per_step": round(b_med, 5), "beam_spread_us": round((max(bm) - min(bm)) * 1e3, 2), "beam_ms_all": [round(x, 5) for x in bm],
            "greedy_ms_per_step": round(g_med, 5), "greedy_spread_us": round((max(gm) - min(gm)) * 1e3, 2),
            "greedy_ms_all": [round(x, 5) for x in gm], "beam_over_greedy": round(b_med / g_med, 4),
            "beam_minus_greedy_us": round((b_med - g_med) * 1e3, 2), "state_slot_bytes": slot_bytes,
            "permute_bytes_read_and_written_per_step_max": 2 * 2 * B * slot_bytes, "slots_moved_per_step_mean": round(moved / args.steps, 3),
            "permute_bytes_read_and_written_per_step_mean": round(2 * 2 * slot_bytes * moved / args.steps)}


def beam_context_legs(rt, ctx, first, B, V, args):
    """Medians of the per-step time of generate_beam with a context per hypothesis -- --beam-ngram N: a token window and
    no_repeat_ngram = N; --beam-penalty P,F: an occurrence table with presence P, frequency F, decay 0.99; --beam-grammar: the two-state
    automaton of the grammar leg -- each against the same beam loop without a context, alternating in one process; every call starts
    from the same states, empty windows and zero counts."""
    import wrk
    W = args.beam
    if B % W:
        return {"skipped": f"{B} slots are not groups of {W} beams"}
    G = B // W
    start = [rt.state_read(b) for b in range(B)]
    legs = {}
    if args.beam_ngram:
        win = wrk.TokenWindow(ctx, B, V, 1024)
        legs[f"ngram_{args.beam_ngram}"] = (dict(window=win, no_repeat_ngram=args.beam_ngram), win)
    if args.beam_penalty:
        p, f = (float(x) for x in args.beam_penalty.split(","))
        occ = wrk.Occurrence(ctx, B, V)
        legs[f"penalty_{p}_{f}"] = (dict(occurrence=occ, presence=p, frequency=f, decay=0.99), occ)
    if args.beam_grammar:
        trans = np.array([[0, 1, wrk.GRAMMAR_REJECT, wrk.GRAMMAR_REJECT], [wrk.GRAMMAR_REJECT, wrk.GRAMMAR_REJECT, 0, 1]], np.uint16)
        g = wrk.Grammar(ctx, V, (np.arange(V) % 4).astype(np.uint16), trans)
        legs["grammar"] = (dict(grammar=g, grammar_state=0), g)

    def run(kw, table):
        for b in range(B):
            rt.state_write(start[b], b)
            if isinstance(table, (wrk.TokenWindow, wrk.Occurrence)):
                table.load(b)
        res, steps = rt.generate_beam(first[:G], args.steps, W, length_penalty=args.beam_length_penalty, **kw)
        return rt.last_beam_ms / max(steps, 1)
    out = {}
    for name, (kw, table) in legs.items():
        run(kw, table)                                                      # capture and warm up
        run({}, None)
        cm, bm = [], []
        for _ in range(args.reps):
            bm.append(run({}, None))
            cm.append(run(kw, table))
        c_med, b_med = float(np.median(cm)), float(np.median(bm))
        out[name] = {"context_ms_per_step": round(c_med, 5), "context_spread_us": round((max(cm) - min(cm)) * 1e3, 2),
                     "context_ms_all": [round(x, 5) for x in cm], "beam_ms_per_step": round(b_med, 5),
                     "beam_spread_us": round((max(bm) - min(bm)) * 1e3, 2), "beam_ms_all": [round(x, 5) for x in bm],
                     "context_minus_beam_us": round((c_med - b_med) * 1e3, 2), "context_over_beam": round(c_med / b_med, 4)}
        table.close()
    for b in range(B):
        rt.state_write(start[b], b)
    out["context_bytes_per_slot"] = V * 5 + 1024 * 4 + 12
    return out


def guide_leg(rt, first, B, V, args):
    """Medians of the per-step time of generate_guided with B guided sequences (scale args.guidance, sampled pick) against the plain sampled
    loop of generate_stop on the same 2B slots, alternating in one process; every call starts from the same states and feeds the same
    first tokens, the partners' being other tokens than the conditional ones'."""
    start = [rt.state_read(b) for b in range(2 * B)]
    neg = [(t + 7) % (V - 1) for t in first]
    pick = dict(temperature=args.temperature, top_p=args.top_p)

    def reset():
        for b in range(2 * B):
            rt.state_write(start[b], b)

    def guided():
        reset()
        tok, _ = rt.generate_guided(first, args.steps, args.guidance, negative_first_tokens=neg, poll_steps=POLL_OFF, **pick)
        return tok, rt.last_stop_ms / args.steps

    def plain():
        reset()
        tok, _ = rt.generate_stop(first + neg, args.steps, [], poll_steps=POLL_OFF, **pick)
        return tok, rt.last_stop_ms / args.steps
    want, _ = guided()                                                     # capture and warm up
    base, _ = plain()
    gm, pm, same = [], [], True
    for _ in range(args.reps):
        tok, ms = plain()
        same &= bool(np.array_equal(tok, base))
        pm.append(ms)
        tok, ms = guided()
        same &= bool(np.array_equal(tok, want))
        gm.append(ms)
    reset()
    g_med, p_med = float(np.median(gm)), float(np.median(pm))
    return {"scale": args.guidance, "guided_sequences": B, "slots": 2 * B, "same_tokens_every_rep": bool(same),
            "guided_differs_from_plain": bool(not np.array_equal(want, base[:, :B])),
            "guided_ms_per_step": round(g_med, 5), "guided_spread_us": round((max(gm) - min(gm)) * 1e3, 2), "guided_ms_all": [round(x, 5) for x in gm],
            "plain_2b_ms_per_step": round(p_med, 5), "plain_2b_spread_us": round((max(pm) - min(pm)) * 1e3, 2),
            "plain_2b_ms_all": [round(x, 5) for x in pm], "guided_over_plain_2b": round(g_med / p_med, 4),
            "guided_minus_plain_2b_us": round((g_med - p_med) * 1e3, 2), "guide_rows_bytes_per_step": 3 * B * V * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="1.5B")
    ap.add_argument("--batches", default="1,16,32")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-p", type=float, default=0.9)
    ap.add_argument("--no-penalized", action="store_true")
    ap.add_argument("--stop", action="store_true")
    ap.add_argument("--poll", default="4,8,16,32,64")
    ap.add_argument("--stop-steps", type=int, default=1024)
    ap.add_argument("--top-k", type=int, default=None)
    ap.add_argument("--min-p", type=float, default=None)
    ap.add_argument("--logprobs", default=None, help="comma-separated numbers of alternatives, e.g. 0,5,20")
    ap.add_argument("--mirostat", default=None, help="TAU,ETA, e.g. 5,0.1")
    ap.add_argument("--typical", type=float, default=None, help="typical_p, e.g. 0.9")
    ap.add_argument("--xtc", default=None, help="PROBABILITY,THRESHOLD, e.g. 0.5,0.1: the cut step against the filtered step")
    ap.add_argument("--top-n-sigma", type=float, default=None, help="e.g. 1.0: the cut step against the filtered step")
    ap.add_argument("--eta", type=float, default=None, help="eta_cutoff, e.g. 0.0003: the cut step against the filtered step")
    ap.add_argument("--grammar", action="store_true", help="the constrained loop against the same loop without a grammar")
    ap.add_argument("--stop-seq", action="store_true", help="the stop-sequence programs against the stop programs and the sampled step")
    ap.add_argument("--dry", action="store_true", help="the loop with a token window and DRY against the same loop without")
    ap.add_argument("--logit-bias", type=int, default=None, help="entries per set: the loop with a logit bias against the same loop without")
    ap.add_argument("--beam", type=int, default=None, help="beams per group: generate_beam against generate_greedy on the same slots")
    ap.add_argument("--beam-length-penalty", type=float, default=1.0)
    ap.add_argument("--beam-ngram", type=int, default=None, help="with --beam: the beam loop with no_repeat_ngram = N against the loop without")
    ap.add_argument("--beam-penalty", default=None, help="with --beam: P,F -- presence and frequency per hypothesis (decay 0.99)")
    ap.add_argument("--beam-grammar", action="store_true", help="with --beam: a two-state automaton per hypothesis")
    ap.add_argument("--guidance", type=float, default=None,
                    help="scale: generate_guided of B sequences against the plain sampled loop on the same 2B slots")
    args = ap.parse_args()
    import wrk

    batches = [int(b) for b in args.batches.split(",")]
    ctx = wrk.Context(0)
    rt = wrk.Runtime(ctx, wrk.GgufReader(bench.make_model_gguf(args.model, seed=42)), num_batch=max(batches) * (2 if args.guidance is not None else 1))
    V = rt.info.num_vocab
    out = {"model": f"RWKV-7 {args.model} Q4_K_M (synthetic)", "temperature": args.temperature, "top_p": args.top_p, "steps": args.steps,
           "reps": args.reps, "batches": []}
    pen = not args.no_penalized
    occ = wrk.Occurrence(ctx, max(batches), V) if pen else None
    pkw = dict(temperature=args.temperature, top_p=args.top_p, presence=0.2, frequency=0.2, decay=0.996)
    if pen:
        out["penalties"] = {"presence": 0.2, "frequency": 0.2, "decay": 0.996, "banned_per_sequence": 16}
        for b in range(max(batches)):
            occ.ban(b, [(1000 + 997 * i + 31 * b) % V for i in range(16)])
    filt = args.top_k is not None or args.min_p is not None
    fkw = dict(temperature=args.temperature, top_p=args.top_p, top_k=args.top_k, min_p=args.min_p)
    kkw = dict(temperature=args.temperature, top_p=1.0, top_k=args.top_k)
    if filt:
        out["filters"] = {"top_k": args.top_k, "min_p": args.min_p}
    if args.mirostat or args.typical is not None:
        out["mirostat"], out["typical_p"] = args.mirostat, args.typical
    for B in batches:
        first = [(17 + 101 * b) % (V - 1) for b in range(B)]
        engine = rt.engine_status()[0] if B == 1 else False
        rt.generate_greedy(first, 4)
        rt.generate_sample(first, 4, temperature=args.temperature, top_p=args.top_p)
        if pen:
            rt.generate_penalized(first, 4, occ, **pkw)
        if filt:
            rt.generate_sample(first, 4, **fkw)
        g, s, p, f, k = [], [], [], [], []
        for _ in range(args.reps):
            g.append(rt.generate_greedy(first, args.steps)[1] / args.steps)
            s.append(rt.generate_sample(first, args.steps, temperature=args.temperature, top_p=args.top_p)[1] / args.steps)
            if pen:
                p.append(rt.generate_penalized(first, args.steps, occ, **pkw)[1] / args.steps)
            if filt:
                f.append(rt.generate_sample(first, args.steps, **fkw)[1] / args.steps)
            if args.top_k is not None:
                k.append(rt.generate_sample(first, args.steps, **kkw)[1] / args.steps)
        gm, sm = float(np.median(g)), float(np.median(s))
        # host alternative: logits back over PCIe + a CPU sort per row (what a caller of wrk_v7_infer has to do today)
        _, _, logits = rt.generate_greedy(first, 1, want_logits=True)
        buf = ctx.buffer(logits)
        rd = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            buf.read(np.float32, B * V)
            rd.append((time.perf_counter() - t0) * 1e3)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            for b in range(B):
                z = np.exp(logits[b] - logits[b].max())
                chat_rs_sample((z / z.sum()).astype(np.float32), args.top_p, args.temperature, np.float32(0.5))
            host.append((time.perf_counter() - t0) * 1e3)
        out["batches"].append({
            "batch": B, "decode_engine": bool(engine),
            "greedy_ms_per_step": round(gm, 5), "sample_ms_per_step": round(sm, 5), "sample_minus_greedy_us": round((sm - gm) * 1e3, 2),
            "greedy_ms_all": [round(x, 5) for x in g], "sample_ms_all": [round(x, 5) for x in s],
            "host_alternative_ms_per_step": {"logits_readback": round(float(np.median(rd)), 4), "numpy_chat_rs_sampler": round(float(np.median(host)), 4)},
        })
        if pen:
            pm = float(np.median(p))
            out["batches"][-1].update({"penalized_ms_per_step": round(pm, 5), "penalized_minus_sample_us": round((pm - sm) * 1e3, 2),
                                       "penalized_ms_all": [round(x, 5) for x in p]})
        if filt:
            fm = float(np.median(f))
            out["batches"][-1].update({"filtered_ms_per_step": round(fm, 5), "filtered_minus_sample_us": round((fm - sm) * 1e3, 2),
                                       "sample_spread_us": round((max(s) - min(s)) * 1e3, 2),
                                       "filtered_spread_us": round((max(f) - min(f)) * 1e3, 2), "filtered_ms_all": [round(x, 5) for x in f]})
        if k:
            km = float(np.median(k))
            out["batches"][-1].update({"top_k_only_ms_per_step": round(km, 5), "top_k_only_minus_sample_us": round((km - sm) * 1e3, 2),
                                       "top_k_only_spread_us": round((max(k) - min(k)) * 1e3, 2), "top_k_only_ms_all": [round(x, 5) for x in k]})
        if args.stop:
            out["batches"][-1]["stop"] = stop_leg(rt, first, B, V, args)
        if args.stop_seq:
            out["batches"][-1]["stop_seq"] = stopseq_leg(rt, first, B, V, args)
        if args.logprobs:
            out["batches"][-1]["logprobs"] = logprob_leg(rt, first, args)
        if args.mirostat or args.typical is not None:
            out["batches"][-1]["mirostat_typical"] = alt_leg(rt, first, args)
        if args.xtc or args.top_n_sigma is not None or args.eta is not None:
            out["cut_note"] = ("a cut step runs sample_rows_kernel<NPT, SAMPLE_CUT> in the place of the filtered kernel, the same launch count: "
                               "XTC / eta add the moments pass, top-n-sigma the integer-moments pass, XTC (when its coin falls) the count / min-key pass")
            out["batches"][-1]["cut"] = cut_leg(rt, first, args)
        if args.grammar:
            out["grammar_note"] = ("two states, four token classes (id mod 4), two classes allowed per state; a constrained step adds two "
                                   "launches to the step program: constrain_rows before the pick and grammar_advance in the tail")
            out["batches"][-1]["grammar"] = grammar_leg(rt, ctx, first, V, args)
        if args.dry:
            out["dry_note"] = ("multiplier 0.8, base 1.75, allowed_length 2, no breakers, windows of 1024 tokens that start empty; a DRY step "
                               "adds three launches to the step program: copy_rows and dry_rows before the pick, window_push in the tail")
            out["batches"][-1]["dry"] = dry_leg(rt, ctx, first, V, args)
        if args.logit_bias:
            out["logit_bias_note"] = (f"{args.logit_bias} entries per sequence, every sequence its own set, a quarter bans, the rest uniform in "
                                      "[-4, 4]; a biased step adds one launch to the step program: bias_rows before everything else")
            out["batches"][-1]["logit_bias"] = bias_leg(rt, ctx, first, V, args)
        if args.beam:
            out["beam_note"] = ("no stop set: every step runs; a beam step replaces the pick and the advance of a greedy step with five "
                                "launches: the two of the candidate front (wrk_top_logprobs' kernels), beam_select, and the gather and the "
                                "scatter of the slot permutation; the snapshot launch returns at once when no slot ended")
            out["batches"][-1]["beam"] = beam_leg(rt, first, B, V, args)
            if args.beam_ngram or args.beam_penalty or args.beam_grammar:
                out["beam_context_note"] = ("a context step adds to the beam step the row launches of its stages in front of the candidate "
                                            "front, the gather and the scatter of the context permutation, and one gated update launch "
                                            "per stage")
                out["batches"][-1]["beam_context"] = beam_context_legs(rt, ctx, first, B, V, args)
        if args.guidance is not None:
            out["guidance_note"] = ("B guided sequences on 2B slots against the plain sampled loop of 2B sequences; a guided step adds two "
                                    "launches to that step: guide_rows in front of the pick and guide_follow in front of the advance, and "
                                    "its pick runs on B rows instead of 2B; the runtime of this whole invocation has 2 * max(batches) state slots, "
                                    "also under the legs that are not guided")
            out["batches"][-1]["guidance"] = guide_leg(rt, first, B, V, args)
    if occ is not None:
        occ.close()
    rt.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
