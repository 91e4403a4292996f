"""NumPy restatement of the stop-token contract of the decode loops (web-rwkv-gguf_amd/csrc/wrk_stop.hip).

Step i feeds x_i (x_0 = the first token) and draws y_i.  A sequence that has not ended and whose y_i is in its stop set ends at step i:
its length is i + 1 (the stop token is part of the output).  A sequence that never ends has the length of the run.  Below its length a
sequence's tokens are those the call without stop sets draws; from its length on, every row repeats the stop token that ended it.
Not a test module: tests/test_stop_ref.py checks it by hand-worked cases, tests/test_gpu_stop.py holds the device to it.
"""
import numpy as np

MAX_STOP_TOKENS = 16


def lengths(tokens, stops) -> np.ndarray:
    """tokens [steps, B] drawn without stops, stops: B sets of ids -> length of every sequence, [B]."""
    tokens = np.asarray(tokens)
    steps, B = tokens.shape
    assert len(stops) == B
    out = np.full(B, steps, np.uint32)
    for b in range(B):
        assert len(stops[b]) <= MAX_STOP_TOKENS
        hit = np.flatnonzero(np.isin(tokens[:, b], np.asarray(list(stops[b]), tokens.dtype)))
        if hit.size:
            out[b] = hit[0] + 1
    return out


def apply(tokens, stops, steps_run=None):
    """(padded tokens [steps_run, B], lengths [B]) of the stopped call; steps_run: rows the loop ran (default: all)."""
    tokens = np.asarray(tokens, np.uint32)
    n = lengths(tokens, stops)
    run = tokens.shape[0] if steps_run is None else steps_run
    assert run >= (int(n.max()) if n.size else 0) or run == tokens.shape[0]
    out = tokens[:run].copy()
    for b in range(tokens.shape[1]):
        if n[b] < run:
            out[n[b]:, b] = tokens[n[b] - 1, b]
    n = np.minimum(n, run).astype(np.uint32)
    return out, n


def steps_run_bound(lens, poll_steps: int, steps: int) -> int:
    """What the polled loop may run at most once every sequence has ended: the host sees block k's live count before it submits
    block k + 2."""
    return min(steps, (-(-int(max(lens)) // poll_steps) + 2) * poll_steps)
