"""Throughput of the request queue on the bench's synthetic RWKV-7 1.5B Q4_K_M model: R = 8 * B requests with prompts of
8 tokens and reply lengths drawn uniformly from [32, 256] with a fixed seed, enforced through max_new so that both sides do the same
useful work.  Every B gets a runtime (and state) of its own with num_batch = B, so the queue's slot count and the waves' batch are the
same number; the tool asserts that the queue used exactly the slots 0 .. B - 1.

  (a) generate_queue: one call, the slots refilled on the device
  (b) the way without it: waves of B requests; a wave takes its prompts in, then runs generate_stop from p_{n-1} for the longest reply
      of the wave.  Two intakes are timed: `steps` (n - 1 one-step generate_sample calls, decode rate as in the queue) and `infer` (the
      first n - 1 tokens of every prompt through Runtime.infer, the prefill path).  The faster one is the baseline and the JSON says
      which.  A wave resets no state and stops nothing early (no stop ids; replies shorter than the wave's longest are cut by the host,
      as a caller of generate_stop would cut them): neither changes the time of a step.
  (c) the added cost per step of a queue program whose requests never end (one request per slot, max_new = steps) against generate_sample

The legs alternate; medians of the wall time of whole calls (a, b) and of the HIP-event time per step (c).

    python tools/queue_bench.py [--batches 16,32] [--reps 5] [--steps 64]

--pool measures the state pool under the queue instead:

  (a) the per-step cost of a pool program whose requests never end (one request per slot, each in place on its own entry) next to the
      plain queue program's, same B, alternating.  The plain program's launch list is what it was before the pool existed; the figure
      of the commit before it comes from running this tool without --pool there ("queue_never_ending_ms_per_step").
  (b) `--turns` turns of R = 8 * B conversations.  Pool side: one generate_queue call per turn, every conversation in place on its own
      entry (turn 0 starts cold).  The host way: per wave of B conversations state_write x B, the prompt intake (both intakes timed, the
      faster one is the baseline), generate_stop for the wave's longest reply, state_read x B -- entry points this feature does not touch.
      As in the waves above, a wave stops nothing early, so the states it reads back are not the ones a caller wants: it is timed only.

    python tools/queue_bench.py --pool [--batches 1,16,32] [--turn-batches 16,32] [--turns 4] [--reps 3] [--steps 64]

--history measures prompt intake and the history pool: one runtime of --history-batch slots, a penalised + DRY sampled
queue with a state pool, R = --requests-per-slot * B requests with prompts of --history-prompt tokens -- several times their replies,
uniform in [8, 16] -- every request in place on its own entry.

  (a) the call without the new arguments: the whole workload (wall time) and the per-step time of a program whose requests never end
  (c) the same two with `history` and `count_prompt`, alternating with (a)

--baseline runs (a) alone and names nothing this feature added, so the same file also runs on the commit before it: that run is leg
(b), taken in the same job, the two commits alternating.

    python tools/queue_bench.py --history [--baseline] [--history-batch 16] [--history-prompt 48] [--reps 5] [--steps 64]

--guidance S measures the guided queue: per B of --batches a runtime of 2B state slots, R = 8 * B requests with prompts
and negative prompts of --prompt tokens each, scale S, the same reply lengths.

  (a) generate_queue_guided: one call, the pairs refilled on the device
  (b) waves of B requests through generate_guided on the same 2B slots; a wave takes both prompts of its requests in by Runtime.infer and
      runs for the longest reply of the wave
  (c) the per-step time of a guided queue program whose requests never end, next to the guided stop program (generate_guided) of the
      same B and the plain queue program on the same 2B slots, alternating

    python tools/queue_bench.py --guidance 1.5 [--batches 8,16] [--reps 5] [--steps 64]

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


def pool_bench(args, wrk, ctx, data, skw):
    out = {"model": f"RWKV-7 {args.model} Q4_K_M (synthetic)", "prompt_tokens": args.prompt, "turns": args.turns,
           "reply_lengths": "uniform [32, 256], seed 7 + turn", "reps": args.reps, **skw,
           "host_way_note": "state_write x B, prompt intake, generate_stop for the wave's longest reply, state_read x B per wave; timed only",
           "per_step": [], "sessions": []}
    med = lambda runs: float(np.median(runs))                       # noqa: E731
    for B in [int(b) for b in args.batches.split(",") if b]:       # (a)
        rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
        V = rt.info.num_vocab
        pool = wrk.StatePool(ctx, rt, B)
        own = list(range(B))
        reqs = [[(17 + 101 * b) % (V - 1)] for b in range(B)]
        kw = dict(max_new=args.steps, max_steps=args.steps, poll_steps=0xffffffff, **skw)

        def step_ms(**pk):
            res, run = rt.generate_queue(reqs, **kw, **pk)
            assert run == args.steps and [len(t) for t, *_ in res] == [args.steps] * B
            return rt.last_queue_ms / args.steps
        step_ms(), step_ms(pool=pool, start_state=own, save_state=own)          # capture and warm up
        plain, pooled = [], []
        for _ in range(args.reps):
            plain.append(step_ms())
            pooled.append(step_ms(pool=pool, start_state=own, save_state=own))
        out["per_step"].append({"batch": B, "steps": args.steps, "queue_ms_per_step": round(med(plain), 5),
                                "pool_queue_ms_per_step": round(med(pooled), 5),
                                "pool_minus_queue_us": round((med(pooled) - med(plain)) * 1e3, 2),
                                "queue_ms_per_step_all": [round(x, 5) for x in plain], "pool_queue_ms_per_step_all": [round(x, 5) for x in pooled]})
        pool.close()
        rt.close()
    for B in [int(b) for b in args.turn_batches.split(",") if b]:   # (b)
        rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
        V = rt.info.num_vocab
        R, T = args.requests_per_slot * B, args.turns
        lens = [np.random.default_rng(7 + t).integers(32, 257, R).tolist() for t in range(T)]
        prompts = [[[(17 + 101 * r + 7 * i + 31 * t) % (V - 1) for i in range(args.prompt)] for r in range(R)] for t in range(T)]
        useful = int(sum(sum(x) for x in lens))
        pool = wrk.StatePool(ctx, rt, R)
        own = list(range(R))
        snaps = [pool.get(r) for r in range(R)]                     # the host way's sessions: one zero snapshot per conversation

        def pool_turns():
            t0 = time.perf_counter()
            for t in range(T):
                res, _ = rt.generate_queue(prompts[t], max_new=lens[t], pool=pool, start_state=own if t else None, save_state=own, **skw)
                assert [len(x) for x, *_ in res] == lens[t] and all(rt.last_queue_saved)
            return (time.perf_counter() - t0) * 1e3

        def host_turns(intake):
            t0 = time.perf_counter()
            for t in range(T):
                for w in range(0, R, B):
                    wave = prompts[t][w:w + B]
                    for b in range(B):
                        rt.state_write(snaps[w + b], b)
                    if intake == "infer" and args.prompt > 1:
                        inp = wrk.RnnInput([p[:-1] for p in wave], 256)
                        while sum(inp.remaining(b) for b in range(B)) > 0:
                            rt.infer(inp)
                    else:
                        for i in range(args.prompt - 1):
                            rt.generate_sample([p[i] for p in wave], 1, **skw)
                    n = max(lens[t][w:w + B])
                    tok, _ = rt.generate_stop([p[-1] for p in wave], n, [], **skw)
                    assert tok.shape == (n, B)
                    for b in range(B):                              # into the conversation's own snapshot: no allocation in the loop
                        ctx.check(wrk.hip.wrk_v7_state_read(ctx.h, rt.state, b, snaps[w + b].h))
            return (time.perf_counter() - t0) * 1e3
        rt.generate_queue(prompts[0][:B], max_new=4, pool=pool, save_state=own[:B], **skw)     # capture and warm up
        rt.generate_sample([p[0] for p in prompts[0][:B]], 1, **skw)
        rt.generate_stop([p[0] for p in prompts[0][:B]], 4, [], **skw)
        rt.infer(wrk.RnnInput([p[:-1] for p in prompts[0][:B]], 256))
        pa, hs, hi = [], [], []
        for _ in range(args.reps):
            pa.append(pool_turns())
            hs.append(host_turns("steps"))
            hi.append(host_turns("infer"))
        pm, hsm, him = med(pa), med(hs), med(hi)
        hm, intake = (hsm, "one-step generate_sample calls") if hsm <= him else (him, "Runtime.infer of the first n - 1 prompt tokens")
        out["sessions"].append({"batch": B, "conversations": R, "turns": T, "reply_tokens": useful,
                                "pool_ms": round(pm, 2), "pool_reply_tokens_per_s": round(useful / pm * 1e3, 1),
                                "host_ms": round(hm, 2), "host_reply_tokens_per_s": round(useful / hm * 1e3, 1), "host_prompt_intake": intake,
                                "pool_ms_all": [round(x, 2) for x in pa], "host_steps_ms_all": [round(x, 2) for x in hs],
                                "host_infer_ms_all": [round(x, 2) for x in hi]})
        pool.close()
        rt.close()
    return out


def history_bench(args, wrk, ctx, data, skw):
    B, W = args.history_batch, args.history_window
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    V = rt.info.num_vocab
    R = args.requests_per_slot * B
    lens = np.random.default_rng(7).integers(8, 17, R).tolist()
    prompts = [[(17 + 101 * r + 7 * i) % (V - 1) for i in range(args.history_prompt)] for r in range(R)]
    occ, win, pool = wrk.Occurrence(ctx, B, V), wrk.TokenWindow(ctx, B, V, W), wrk.StatePool(ctx, rt, R)
    pick = dict(occurrence=occ, presence=0.3, frequency=0.2, decay=0.996, window=win, dry=(0.8, 1.75, 2), **skw)
    own = list(range(R))
    new = {} if args.baseline else dict(history=wrk.HistoryPool(ctx, R, V, W), count_prompt=True)

    def workload(**extra):
        t0 = time.perf_counter()
        res, run = rt.generate_queue(prompts, max_new=lens, pool=pool, start_state=own, save_state=own, **pick, **extra)
        ms = (time.perf_counter() - t0) * 1e3
        assert [len(t) for t, *_ in res] == lens and all(rt.last_queue_saved)
        return ms, run

    def step_ms(**extra):
        res, run = rt.generate_queue([[(17 + 101 * b) % (V - 1)] for b in range(B)], max_new=args.steps, max_steps=args.steps, poll_steps=0xffffffff,
                                     pool=pool, start_state=own[:B], save_state=own[:B], **pick, **extra)
        assert run == args.steps and [len(t) for t, *_ in res] == [args.steps] * B
        return rt.last_queue_ms / args.steps
    legs = [("plain", {})] + ([] if args.baseline else [("history", new)])
    for _, extra in legs:                           # capture and warm up
        workload(**extra), step_ms(**extra)
    wall, steps, per_step = {k: [] for k, _ in legs}, {}, {k: [] for k, _ in legs}
    for _ in range(args.reps):
        for k, extra in legs:
            ms, steps[k] = workload(**extra)
            wall[k].append(ms)
            per_step[k].append(step_ms(**extra))
    med = lambda runs: float(np.median(runs))       # noqa: E731
    out = {"model": f"RWKV-7 {args.model} Q4_K_M (synthetic)", "batch": B, "requests": R, "prompt_tokens": args.history_prompt,
           "reply_lengths": "uniform [8, 16], seed 7", "reply_tokens": int(sum(lens)), "window_capacity": W, "reps": args.reps,
           "pick": "sampled, presence 0.3 frequency 0.2 decay 0.996, DRY 0.8 / 1.75 / 2", "baseline_only": bool(args.baseline), **skw}
    for k, _ in legs:
        out[k] = {"workload_ms": round(med(wall[k]), 2), "workload_steps": steps[k], "never_ending_ms_per_step": round(med(per_step[k]), 5),
                  "workload_ms_all": [round(x, 2) for x in wall[k]], "never_ending_ms_per_step_all": [round(x, 5) for x in per_step[k]]}
    if not args.baseline:
        d_step = (med(per_step["history"]) - med(per_step["plain"])) * 1e3
        d_wall = (med(wall["history"]) - med(wall["plain"])) * 1e3
        out["history_minus_plain_us_per_step"] = round(d_step, 2)
        out["history_minus_plain_workload_us"] = round(d_wall, 1)
        # what of the workload's difference the per-step difference does not explain, over its R turnovers: a residual, which also
        # holds whatever the sampler and DRY spend on rows and windows that now have a context
        out["per_turnover_us"] = round((d_wall - d_step * steps["history"]) / R, 2)
        new["history"].close()
    for h in (occ, win, pool, rt):
        h.close()
    return out


def guided_bench(args, wrk, ctx, data, skw):
    scale = args.guidance
    out = {"model": f"RWKV-7 {args.model} Q4_K_M (synthetic)", "prompt_tokens": args.prompt, "negative_prompt_tokens": args.prompt,
           "guidance_scale": scale, "reply_lengths": "uniform [32, 256], seed 7", "reps": args.reps, **skw,
           "waves_note": "waves of B requests through generate_guided on the same 2B slots; both prompts of a wave go in by Runtime.infer; "
                         "a wave runs the longest reply of the wave, the host cuts the rest", "batches": []}
    med = lambda runs: float(np.median(runs))                       # noqa: E731
    for B in [int(b) for b in args.batches.split(",") if b]:
        rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2 * B)        # B request slots on 2B state slots
        V = rt.info.num_vocab
        R = args.requests_per_slot * B
        lens = np.random.default_rng(7).integers(32, 257, R).tolist()
        prompts = [[(17 + 101 * r + 7 * i) % (V - 1) for i in range(args.prompt)] for r in range(R)]
        negs = [[(23 + 89 * r + 11 * i) % (V - 1) for i in range(args.prompt)] for r in range(R)]
        useful = int(sum(lens))

        def queue():
            t0 = time.perf_counter()
            res, run = rt.generate_queue_guided(prompts, negs, scale, max_new=lens, **skw)
            ms = (time.perf_counter() - t0) * 1e3
            assert [len(t) for t, *_ in res] == lens
            assert sorted({slot for _, _, slot, _ in res}) == list(range(B)), "the guided queue must serve on exactly B pairs"
            return ms

        def waves():
            t0 = time.perf_counter()
            for w in range(0, R, B):
                wave, nwave = prompts[w:w + B], negs[w:w + B]
                if args.prompt > 1:
                    inp = wrk.RnnInput([p[:-1] for p in wave + nwave], 256)
                    while sum(inp.remaining(b) for b in range(2 * B)) > 0:
                        rt.infer(inp)
                n = max(lens[w:w + B])
                tok, _ = rt.generate_guided([p[-1] for p in wave], n, scale, negative_first_tokens=[q[-1] for q in nwave], **skw)
                assert tok.shape == (n, B)
            return (time.perf_counter() - t0) * 1e3

        first, nfirst = [p[0] for p in prompts[:B]], [q[0] for q in negs[:B]]
        never = dict(max_new=args.steps, max_steps=args.steps, poll_steps=0xffffffff, **skw)

        def guided_queue_step():
            res, run = rt.generate_queue_guided([[t] for t in first], [[t] for t in nfirst], scale, **never)
            assert run == args.steps and [len(t) for t, *_ in res] == [args.steps] * B
            return rt.last_queue_ms / args.steps

        def guided_stop_step():
            tok, _ = rt.generate_guided(first, args.steps, scale, negative_first_tokens=nfirst, poll_steps=0xffffffff, **skw)
            assert tok.shape == (args.steps, B)
            return rt.last_stop_ms / args.steps

        def plain_queue_step():                 # the plain queue on the same 2B slots
            res, run = rt.generate_queue([[t] for t in first + nfirst], **never)
            assert run == args.steps and [len(t) for t, *_ in res] == [args.steps] * (2 * B)
            return rt.last_queue_ms / args.steps
        queue(), waves(), guided_queue_step(), guided_stop_step(), plain_queue_step()      # capture and warm up
        qa, wa, gq, gs, pq = [], [], [], [], []
        for _ in range(args.reps):
            qa.append(queue())
            wa.append(waves())
            gq.append(guided_queue_step())
            gs.append(guided_stop_step())
            pq.append(plain_queue_step())
        out["batches"].append({
            "request_slots": B, "state_slots": 2 * B, "requests": R, "reply_tokens": useful,
            "guided_queue_ms": round(med(qa), 2), "guided_queue_reply_tokens_per_s": round(useful / med(qa) * 1e3, 1),
            "waves_ms": round(med(wa), 2), "waves_reply_tokens_per_s": round(useful / med(wa) * 1e3, 1),
            "guided_queue_ms_all": [round(x, 2) for x in qa], "waves_ms_all": [round(x, 2) for x in wa],
            "guided_queue_never_ending_ms_per_step": round(med(gq), 5), "guided_stop_ms_per_step": round(med(gs), 5),
            "plain_queue_2b_never_ending_ms_per_step": round(med(pq), 5),
            "guided_queue_minus_guided_stop_us": round((med(gq) - med(gs)) * 1e3, 2),
            "guided_queue_minus_plain_queue_us": round((med(gq) - med(pq)) * 1e3, 2),
            "guided_queue_ms_per_step_all": [round(x, 5) for x in gq], "guided_stop_ms_per_step_all": [round(x, 5) for x in gs],
            "plain_queue_ms_per_step_all": [round(x, 5) for x in pq]})
        rt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="1.5B")
    ap.add_argument("--batches", default="16,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=8)
    ap.add_argument("--requests-per-slot", type=int, default=8)
    ap.add_argument("--pool", action="store_true", help="the state-pool legs (DESIGN.md §7g) in the place of the queue's")
    ap.add_argument("--turns", type=int, default=4)
    ap.add_argument("--turn-batches", default="16,32")
    ap.add_argument("--history", action="store_true", help="prompt intake and the history pool (DESIGN.md §7o) in the place of the queue's legs")
    ap.add_argument("--baseline", action="store_true", help="with --history: leg (a) alone, with no argument this feature added")
    ap.add_argument("--history-batch", type=int, default=16)
    ap.add_argument("--history-prompt", type=int, default=48)
    ap.add_argument("--history-window", type=int, default=256)
    ap.add_argument("--guidance", type=float, default=None, help="the guided queue (DESIGN.md §7s) with this scale in the place of the queue's legs")
    args = ap.parse_args()
    import wrk

    batches = [int(b) for b in args.batches.split(",") if b]
    ctx = wrk.Context(0)
    data = bench.make_model_gguf(args.model, seed=42)
    skw = dict(temperature=1.0, top_p=0.9)
    if args.guidance is not None:
        print(json.dumps(guided_bench(args, wrk, ctx, data, skw)))
        ctx.close()
        return
    if args.history:
        print(json.dumps(history_bench(args, wrk, ctx, data, skw)))
        ctx.close()
        return
    if args.pool:
        print(json.dumps(pool_bench(args, wrk, ctx, data, skw)))
        ctx.close()
        return
    out = {"model": f"RWKV-7 {args.model} Q4_K_M (synthetic)", "prompt_tokens": args.prompt, "reply_lengths": "uniform [32, 256], seed 7",
           "reps": args.reps, **skw,
           "waves_note": "a wave resets no state and gives no per-request max_new: it runs the longest reply of the wave, the host cuts the rest",
           "batches": []}
    for B in batches:
        rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)           # one runtime per B: the queue serves on rt.num_batch slots
        V = rt.info.num_vocab
        R = args.requests_per_slot * B
        lens = np.random.default_rng(7).integers(32, 257, R).tolist()
        prompts = [[(17 + 101 * r + 7 * i) % (V - 1) for i in range(args.prompt)] for r in range(R)]
        useful = int(sum(lens))

        def queue():
            t0 = time.perf_counter()
            res, run = rt.generate_queue(prompts, max_new=lens, **skw)
            ms = (time.perf_counter() - t0) * 1e3
            assert [len(t) for t, *_ in res] == lens
            assert sorted({slot for _, _, slot, _ in res}) == list(range(B)), "the queue must serve on exactly B slots"
            return ms, run

        def waves(intake):
            t0 = time.perf_counter()
            run = 0
            for w in range(0, R, B):
                wave = prompts[w:w + B]
                if intake == "infer" and args.prompt > 1:
                    inp = wrk.RnnInput([p[:-1] for p in wave], 256)
                    while sum(inp.remaining(b) for b in range(B)) > 0:
                        rt.infer(inp)
                else:
                    for i in range(args.prompt - 1):
                        rt.generate_sample([p[i] for p in wave], 1, **skw)
                n = max(lens[w:w + B])
                tok, _ = rt.generate_stop([p[-1] for p in wave], n, [], **skw)
                assert tok.shape == (n, B)
                run += args.prompt - 1 + n
            return (time.perf_counter() - t0) * 1e3, run

        first = [p[0] for p in prompts[:B]]
        queue(), waves("steps"), waves("infer")                     # capture and warm up
        rt.generate_sample(first, 4, **skw)
        rt.generate_queue([[t] for t in first], max_new=4, **skw)
        qa, ws, wi, ss, qs = [], [], [], [], []
        for _ in range(args.reps):
            qa.append(queue())
            ws.append(waves("steps"))
            wi.append(waves("infer"))
            ss.append(rt.generate_sample(first, args.steps, **skw)[1] / args.steps)
            res, run = rt.generate_queue([[t] for t in first], max_new=args.steps, max_steps=args.steps, poll_steps=0xffffffff, **skw)
            assert run == args.steps and [len(t) for t, *_ in res] == [args.steps] * B
            qs.append(rt.last_queue_ms / args.steps)
        med = lambda runs: float(np.median([m for m, _ in runs]))   # noqa: E731
        qm, wsm, wim = med(qa), med(ws), med(wi)
        wm, intake = (wsm, "one-step generate_sample calls") if wsm <= wim else (wim, "Runtime.infer of the first n - 1 prompt tokens")
        out["batches"].append({
            "batch": B, "slots": B, "requests": R, "reply_tokens": useful,
            "queue_ms": round(qm, 2), "queue_steps": qa[0][1], "queue_reply_tokens_per_s": round(useful / qm * 1e3, 1),
            "waves_ms": round(wm, 2), "waves_steps": ws[0][1], "waves_reply_tokens_per_s": round(useful / wm * 1e3, 1),
            "waves_prompt_intake": intake, "waves_ms_intake_steps": round(wsm, 2), "waves_ms_intake_infer": round(wim, 2),
            "queue_ms_all": [round(m, 2) for m, _ in qa], "waves_steps_ms_all": [round(m, 2) for m, _ in ws],
            "waves_infer_ms_all": [round(m, 2) for m, _ in wi],
            "sample_ms_per_step": round(float(np.median(ss)), 5), "queue_never_ending_ms_per_step": round(float(np.median(qs)), 5),
            "queue_minus_sample_us": round((float(np.median(qs)) - float(np.median(ss))) * 1e3, 2),
        })
        rt.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
