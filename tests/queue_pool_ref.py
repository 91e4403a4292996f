"""Restatement of the state-pool contract of the request queue (web-rwkv-gguf_amd/csrc/wrk_queue.hip): which index
tables a call accepts and which pool entries it writes.  The schedule itself is tests/queue_ref.py's, unchanged by a pool.

The pool is one device buffer of P states, entry k at float offset k * L * (S+2) * D in `state_read`'s layout.  Request r may name a start
entry and a save entry (None: none).  A request with a start entry begins from a copy of it -- at step 0 or at a refill -- and one without
begins as without a pool, from zeros or `init_state`.  When request r ends with reason 1 (stop id) or 2 (max_new) and save[r] = k, entry k
receives the slot's state at that step: the prompt and y_0 .. y_{j-1} consumed, the last reply token y_j not fed, which is the state
`generate_stop` freezes for a sequence that ends there.  Reasons 3 (cut by max_steps) and 0 (never dispatched) write nothing, the entry
keeps its bits, and saved[r] is 1 if and only if the entry was written.

No races, by validation (ValueError here, WRK_E_ARG on the device side, before any launch): an index >= P, two requests saving to one
entry, a request reading an entry that ANOTHER request of the call saves to.  start[r] == save[r] is allowed (the read at r's start
precedes the write at r's end), and so is any number of requests reading an entry that nobody saves.  Hence the entries read and the
entries written within one step are disjoint and the result does not depend on the schedule.
Not a test module: tests/test_queue_pool_ref.py checks it by hand-worked cases, tests/test_gpu_queue_pool.py holds the device to it.
"""
NEVER, STOP, MAX_NEW, CAP = 0, 1, 2, 3
NO_ENTRY = 0xFFFFFFFF          # WRK_QUEUE_NO_ENTRY: what None is on the C side


def validate(start, save, num_entries: int):
    """Raises ValueError unless the tables are a call the contract accepts.  start, save: one entry index or None per request."""
    if len(start) != len(save):
        raise ValueError(f"{len(start)} start entries, {len(save)} save entries")
    if num_entries < 1:
        raise ValueError("an empty pool")
    saver = {}
    for r, k in enumerate(save):
        if k is None:
            continue
        if not 0 <= k < num_entries:
            raise ValueError(f"request {r}: save entry {k} of {num_entries}")
        if k in saver:
            raise ValueError(f"requests {saver[k]} and {r} both save to entry {k}")
        saver[k] = r
    for r, k in enumerate(start):
        if k is None:
            continue
        if not 0 <= k < num_entries:
            raise ValueError(f"request {r}: start entry {k} of {num_entries}")
        if saver.get(k, r) != r:
            raise ValueError(f"request {r} starts from entry {k}, which request {saver[k]} saves to")


def saved(save, reasons):
    """saved[r]: request r's entry was written -- it names one and ended by a stop id or by max_new."""
    assert len(save) == len(reasons)
    return [k is not None and why in (STOP, MAX_NEW) for k, why in zip(save, reasons)]


def written(save, reasons):
    """{entry: the request whose final state it holds after the call}; every other entry keeps its bits."""
    return {k: r for r, (k, ok) in enumerate(zip(save, saved(save, reasons))) if ok}
