"""NumPy restatement of what the request queue does with the penalty context of a slot (web-rwkv-gguf_amd/csrc/wrk_queue.hip, DESIGN.md
§7o): prompt intake (`count_prompt`) and the history pool beside the state pool.

The context of a slot is its occurrence row (counts f32 [V], flags u32 [V]: bit 0 present, bit 1 banned) and its token window (the last
`capacity` tokens that counted, oldest first).  A history entry is (counts, present, window): no banned bits.  The context of request r,
with the prompt p_0 .. p_{n-1}, f = count_prompt[r] and the reply y_0 .. y_{m-1}, sees exactly these events, in this order:

  1. begin    with a start entry k: counts = entry.counts, flags = (slot flags & BANNED) | entry.present, window = entry.window;
              without one: counts = 0, flags = slot flags & BANNED, window empty;
  2. intake   p_f, .., p_{n-1}, one at a time (none when count_prompt is off or f >= n);
  3. draws    y_0, .., y_{m-1}, one at a time; the row y_j is picked from has seen 1, 2 and y_0 .. y_{j-1}.

Every event of 2 and 3 is penalty_ref.update with the request's decay (counts *= decay; counts[t] += w[t]; present[t] = 1) and
dry_ref.push.  A request that ends with reason 1 or 2 and names a save entry writes (counts, flags & PRESENT, window) there, after its
last draw; reasons 3 and 0 write nothing, and every entry that no such request names keeps its bits.  Which slot serves a request --
whose banned bits it sees -- is queue_ref's schedule; which tables are a call is queue_pool_ref's validation plus the rules of
`validate` below.  Not a test module: tests/test_history_ref.py checks it by hand-worked cases, tests/test_gpu_history.py holds the
device to it."""
import numpy as np

import dry_ref as D
import penalty_ref as P
import queue_pool_ref as PR
import queue_ref as Q

PRESENT, BANNED = P.PRESENT, P.BANNED


def empty_entry(V: int):
    return np.zeros(V, np.float32), np.zeros(V, np.uint32), []


def begin(slot_flags, entry):
    """The slot's context at a dispatch: (counts, flags, window).  entry None: the reset."""
    bans = np.asarray(slot_flags).astype(np.uint32) & BANNED
    if entry is None:
        return np.zeros(bans.size, np.float32), bans, []
    counts, present, window = entry
    return np.array(counts, np.float32), bans | (np.asarray(present).astype(np.uint32) & PRESENT), [int(t) for t in window]


def take(ctx, token: int, w, decay, capacity: int):
    """One token enters the context: a prompt token of the intake or a counted draw, the same rule.  capacity 0: no window."""
    counts, flags, window = ctx
    counts, flags = P.update(counts, flags, int(token), w, decay)
    return counts, flags, D.push(window, token, capacity) if capacity else []


def events(prompt, f, reply):
    """The tokens that enter a request's context after its begin, in order: [('prompt', p_i) for i >= f] + [('draw', y_j)]."""
    n = len(prompt)
    first = n if f is None else min(int(f), n)
    return [("prompt", int(t)) for t in prompt[first:]] + [("draw", int(y)) for y in reply]


def context_before_draw(slot_flags, entry, prompt, f, reply, j: int, w, decay, capacity: int):
    """What the row of y_j is penalised with."""
    ctx = begin(slot_flags, entry)
    for _, t in events(prompt, f, reply[:j]):
        ctx = take(ctx, t, w, decay, capacity)
    return ctx


def entry_of(ctx):
    """What a save writes: the present bit only."""
    counts, flags, window = ctx
    return np.array(counts, np.float32), np.asarray(flags).astype(np.uint32) & PRESENT, list(window)


def validate(start, save, state_entries: int, history_entries, history_capacity, has_pool: bool, has_occ: bool, window_capacity,
             count_prompt):
    """Raises ValueError unless the call is one the contract accepts.  history_entries None: no history pool (history_capacity is not
    read); window_capacity None: no token window; count_prompt None: off."""
    if count_prompt is not None and not has_occ and window_capacity is None:
        raise ValueError("count_prompt needs an occurrence table or a token window")
    if history_entries is None:
        return
    if not has_pool:
        raise ValueError("a history pool without a state pool")
    PR.validate(start, save, state_entries)
    if not has_occ and window_capacity is None:
        raise ValueError("a history pool needs an occurrence table or a token window")
    if history_entries != state_entries:
        raise ValueError(f"history pool of {history_entries} entries, state pool of {state_entries}")
    if window_capacity is not None and history_capacity == 0:
        raise ValueError("a token window with a history pool created without windows")
    if window_capacity is None and history_capacity != 0:
        raise ValueError("a history pool with windows and no token window")
    if window_capacity is not None and history_capacity != window_capacity:
        raise ValueError(f"history pool windows of capacity {history_capacity}, token window of {window_capacity}")


def run(prompts, replies, stops, max_new, B: int, start, save, entries, slot_flags, count_prompt, w, decay, capacity: int, max_steps=None):
    """A pool call with a history pool, given what every request draws freely (`replies`, as queue_ref.run).  entries: the history
    pool before the call, a list of (counts, present, window); slot_flags [B][V]: the slots' flags before the call (only the banned
    bits matter); count_prompt: None or one offset per request; decay: one value per request.  Returns (queue_ref.run's results, the
    entries after the call, {entry: the request that wrote it}).  A request reads its start entry as it was BEFORE the call: the
    validation lets nobody but the request itself save to it, and it saves after it has read."""
    R = len(prompts)
    PR.validate(start, save, len(entries))
    got, needed = Q.run(prompts, replies, stops, max_new, B, max_steps)
    after = [entry_of(e) for e in entries]
    written = PR.written(save, [why for _, why, *_ in got])
    for k, r in written.items():
        tokens, _, slot, _ = got[r]
        ctx = begin(slot_flags[slot], None if start[r] is None else entries[start[r]])
        for _, t in events(prompts[r], None if count_prompt is None else count_prompt[r], tokens):
            ctx = take(ctx, t, w, decay[r], capacity)
        after[k] = entry_of(ctx)
    assert all(0 <= k < len(entries) for k in written) and len(written) <= R
    return got, after, written
