"""NumPy restatement of the guided request queue's contract (wrk_v7_generate_queue_guided in include/wrk_hip.h): the
scheduling and token rules only.  The guided row itself is tests/guide_ref.py's.

R requests are served on B request slots; slot b is the pair of state slots (b, B + b): the conditional half and its partner.  Request r
has a prompt of n >= 1 tokens, a negative prompt of m >= 0 tokens (m == 0: an unguided request, its partner idles) and draws at most
max_new[r] reply tokens.  L = max(n, m).  Requests are dispatched in index order: at step 0 request b goes to pair b (b < min(B, R));
pairs that end in the same step take the next requests in ascending slot order.  A pair given request r at step f feeds p_0 at step
f + L - n and q_0 at step f + L - m; both halves feed their last prompt token at step f + L - 1, whose draw (from the guided row) is
y_0, and y_j is drawn by step f + L - 1 + j with sampler step j.  The state slot of a half is set to its start state directly in front
of the step that feeds the half's first token: its reset step.  The conditional half decides the end as in tests/queue_ref.py; the step
after the one that ends a request is the pair's next f.  A request whose p_0 was not fed within max_steps steps has reason 0.
Not a test module: tests/test_guided_queue_ref.py checks it by hand-worked cases, tests/test_gpu_guided_queue.py holds the device to it.
"""
import numpy as np

from queue_ref import CAP, NEVER, reply_length, steps_run, steps_run_bound  # noqa: F401  (the polled loop and the end rule are the queue's)

MAX_PAIRS = 128


def schedule(prompt_lens, neg_lens, lengths, B: int, max_steps=None):
    """The schedule as a pure function of (n, m, uncut reply lengths).  Returns (rows, steps_needed); rows[r] = dict(slot, dispatch_step,
    start_step, neg_start_step, step_base, length, cut).  dispatch_step: f.  start_step / neg_start_step: the steps that feed p_0 / q_0,
    which are the halves' reset steps (neg_start_step None when m == 0: the partner is neither reset nor fed).  step_base: the step that
    draws y_0.  A request never dispatched has None everywhere and length 0."""
    R = len(prompt_lens)
    assert R == len(neg_lens) == len(lengths) and 1 <= B <= MAX_PAIRS
    assert all(n >= 1 for n in prompt_lens) and all(m >= 0 for m in neg_lens) and all(k >= 1 for k in lengths)
    none = dict(slot=None, dispatch_step=None, start_step=None, neg_start_step=None, step_base=None, length=0, cut=False)
    rows = [dict(none) for _ in range(R)]
    free_at = [0] * B               # the first step the pair runs for its next request
    nxt, needed = 0, 0
    while nxt < R:
        f = min(free_at)
        for b in range(B):          # every pair free at this step, in ascending slot order
            if free_at[b] == f and nxt < R:
                n, m = prompt_lens[nxt], neg_lens[nxt]
                L = max(n, m)
                end = f + L - 1 + lengths[nxt] - 1          # the step that draws the request's last token
                rows[nxt].update(slot=b, dispatch_step=f, start_step=f + L - n, neg_start_step=f + L - m if m else None, step_base=f + L - 1,
                                 length=lengths[nxt])
                free_at[b] = end + 1
                needed = max(needed, end + 1)
                nxt += 1
    if max_steps is not None:
        for r, row in enumerate(rows):
            if row["start_step"] is None:
                continue
            if row["start_step"] >= max_steps:              # p_0 was never fed
                rows[r] = dict(none)
                continue
            drawn = min(max(max_steps - row["step_base"], 0), row["length"])
            if drawn < row["length"]:
                row.update(length=drawn, cut=True)
    return rows, needed


def run(prompts, negatives, replies, stops, max_new, B: int, max_steps=None, ends=None):
    """prompts / negatives: R token lists (a negative may be empty); replies[r]: what request r draws freely (>= max_new[r] tokens, or up
    to a stop).  ends: the (length, reason) of every request when something else than a stop id may end a reply (a stop sequence);
    None: queue_ref.reply_length of the stop ids.  Returns ([(tokens, reason, slot, start_step)] per request, steps_needed), as
    Runtime.generate_queue_guided reports them (slot and start_step 0 for a request never dispatched)."""
    if ends is None:
        ends = [reply_length(replies[r], stops[r], max_new[r]) for r in range(len(prompts))]
    rows, needed = schedule([len(p) for p in prompts], [len(q) for q in negatives], [n for n, _ in ends], B, max_steps)
    out = []
    for r, row in enumerate(rows):
        if row["start_step"] is None:
            out.append((np.zeros(0, np.uint32), NEVER, 0, 0))
            continue
        reason = CAP if row["cut"] else ends[r][1]
        out.append((np.asarray(replies[r][:row["length"]], np.uint32), reason, row["slot"], row["start_step"]))
    return out, needed


def check_request(n: int, m: int, scale: float):
    """The contract's conditions on one request: WRK_E_ARG otherwise."""
    return n >= 1 and m >= 0 and np.isfinite(scale) and scale >= 0 and (m > 0 or scale == 1.0)
