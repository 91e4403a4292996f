"""NumPy restatement of the request-queue contract of the decode loops (web-rwkv-gguf_amd/csrc/wrk_queue.hip): the
scheduling and token rules only.

R requests are served on B slots.  Request r has a prompt of n_r >= 1 tokens and draws at most max_new[r] reply tokens.  Requests are
dispatched in index order: at step 0 request b goes to slot b (b < min(B, R)); slots that end in the same step take the next requests in
ascending slot order, and a slot with no request left idles.  A slot that holds request r from step s on feeds p_0 .. p_{n-1} on steps
s .. s + n - 1; the draws of the first n - 1 of them are discarded, the draw of step s + n - 1 is reply token y_0, and y_j is drawn by
step s + n - 1 + j.  The request ends at the first j with y_j in its stop set (reason 1, the stop token is part of the reply), else at
j + 1 == max_new[r] (reason 2); the step after the one that ends it feeds the slot's next request.  A request still running after
max_steps steps has reason 3 and the tokens drawn so far; one never dispatched has reason 0 and length 0.  The sampler step of y_j is j.
Not a test module: tests/test_queue_ref.py checks it by hand-worked cases, tests/test_gpu_queue.py holds the device to it.
"""
import numpy as np

MAX_STOP_TOKENS = 16
NEVER, STOP, MAX_NEW, CAP = 0, 1, 2, 3


def reply_length(draws, stop, max_new: int):
    """(length, reason) of a request whose reply, drawn freely, would be `draws` (at least max_new tokens unless a stop comes first)."""
    assert max_new >= 1 and len(stop) <= MAX_STOP_TOKENS
    for j in range(max_new):
        if int(draws[j]) in set(int(s) for s in stop):
            return j + 1, STOP
    return max_new, MAX_NEW


def schedule(prompt_lens, lengths, B: int, max_steps=None):
    """The schedule as a pure function of the prompt lengths and the (uncut) reply lengths.  Returns (rows, steps_needed): rows[r] =
    dict(slot, start_step, length, cut) -- cut: the request was still running when max_steps steps had run, length is what it drew by
    then; a request never dispatched has slot = start_step = None and length 0.  steps_needed: the step count after which every request
    has ended (without a cap)."""
    R = len(prompt_lens)
    assert R == len(lengths) and B >= 1 and all(n >= 1 for n in prompt_lens) and all(m >= 1 for m in lengths)
    rows = [dict(slot=None, start_step=None, length=0, cut=False) for _ in range(R)]
    free_at = [0] * B              # the step at which the slot feeds the p_0 of its next request
    nxt, needed = 0, 0
    while nxt < R:
        step = min(free_at)
        for b in range(B):         # every slot free at this step, in ascending slot order
            if free_at[b] == step and nxt < R:
                end = step + prompt_lens[nxt] - 1 + lengths[nxt] - 1     # the step that draws the request's last token
                rows[nxt].update(slot=b, start_step=step, length=lengths[nxt])
                free_at[b] = end + 1
                needed = max(needed, end + 1)
                nxt += 1
    if max_steps is not None:
        for r, row in enumerate(rows):
            if row["start_step"] is None:
                continue
            if row["start_step"] >= max_steps:
                row.update(slot=None, start_step=None, length=0)
                continue
            first = row["start_step"] + prompt_lens[r] - 1               # the step that draws y_0
            drawn = min(max(max_steps - first, 0), row["length"])
            if drawn < row["length"]:
                row.update(length=drawn, cut=True)
    return rows, needed


def run(prompts, replies, stops, max_new, B: int, max_steps=None):
    """prompts: R token lists; replies[r]: what request r draws freely (>= max_new[r] tokens, or up to a stop).  Returns
    ([(tokens, reason, slot, start_step)] per request, steps_needed), as Runtime.generate_queue reports them (slot and start_step 0 for a
    request never dispatched)."""
    ends = [reply_length(replies[r], stops[r], max_new[r]) for r in range(len(prompts))]
    rows, needed = schedule([len(p) for p in prompts], [n for n, _ in ends], B, max_steps)
    out = []
    for r, row in enumerate(rows):
        if row["start_step"] is None:
            out.append((np.zeros(0, np.uint32), NEVER, 0, 0))
            continue
        reason = CAP if row["cut"] else ends[r][1]
        out.append((np.asarray(replies[r][:row["length"]], np.uint32), reason, row["slot"], row["start_step"]))
    return out, needed


def steps_run(needed: int, poll_steps: int, max_steps: int) -> int:
    """What the polled loop runs: the host waits for the live count of block k before it submits block k + 2, so exactly one block
    goes out after the block in which the last request ends, and never more than max_steps steps."""
    return min(max_steps, (-(-needed // poll_steps) + 1) * poll_steps)


def steps_run_bound(needed: int, poll_steps: int, max_steps: int) -> int:
    """What the polled loop may run at most once every request has ended: the host sees block k's live count before it submits
    block k + 2."""
    return min(max_steps, (-(-needed // poll_steps) + 2) * poll_steps)
