"""NumPy restatement of the stop-sequence contract of the decode loops (web-rwkv-gguf_amd/csrc/wrk_stopseq_dev.h).

An owner -- a sequence of generate_stop, a request of generate_queue -- has, next to its stop set of ids, 0 .. MAX_STOP_SEQUENCES stop
sequences of 1 .. MAX_STOP_SEQUENCE_LEN ids, and a tail: its last TAIL_LEN draws that counted, oldest first, right aligned, EMPTY where
there is none.  At a counted draw y, sequence k of length l matches when (tail ++ [y])[-l:] == seq_k; EMPTY equals no id, so nothing
matches across the start of the tail.  The owner ends at that draw if a sequence matches or y is in its stop set.  The match word is
NONE, TOKEN (an id of the stop set) or the index of the matching sequence: the longest match wins, at equal length the stop-set id beats
a sequence, and between sequences of equal length the lower index wins.  The tail takes every counted draw in, the one that ends the
owner included, and is frozen from then on.  x_0, prompt tokens and the discarded draws of prompt steps are not counted draws.
Not a test module: tests/test_stopseq_ref.py checks it against a brute force and by hand-worked cases, tests/test_gpu_stopseq.py holds
the device to it.
"""
import numpy as np

MAX_STOP_SEQUENCES = 8
MAX_STOP_SEQUENCE_LEN = 8
TAIL_LEN = 7
EMPTY = 0xFFFFFFFF
NONE = 0xFFFFFFFF
TOKEN = 0xFFFFFFFE


def empty_tail() -> list:
    return [EMPTY] * TAIL_LEN


def check(seqs, ids=()):
    assert len(seqs) <= MAX_STOP_SEQUENCES
    assert all(1 <= len(q) <= MAX_STOP_SEQUENCE_LEN for q in seqs)
    assert EMPTY not in [t for q in seqs for t in q] and EMPTY not in list(ids)


def step(tail, y, seqs, ids=()):
    """One counted draw: (match word, new tail)."""
    check(seqs, ids)
    assert len(tail) == TAIL_LEN and y != EMPTY
    window = [int(t) for t in tail] + [int(y)]
    match, best = NONE, 0
    if int(y) in [int(t) for t in ids]:
        match, best = TOKEN, 1
    for k, q in enumerate(seqs):
        l = len(q)
        if l > best and window[-l:] == [int(t) for t in q]:
            match, best = k, l
    return match, window[1:]


def run(stream, seqs, ids=(), tail=None):
    """A stream of draws from `tail` (None: empty): (length, match word, tail).  The owner ends at the first draw with a match; one that
    never ends has the length of the stream and NONE."""
    tail = empty_tail() if tail is None else [int(t) for t in tail]
    for i, y in enumerate(stream):
        match, tail = step(tail, y, seqs, ids)
        if match != NONE:
            return i + 1, match, tail
    return len(stream), NONE, tail


def lengths(tokens, seqs, ids=None, tails=None):
    """tokens [steps, B] drawn without stops, seqs: B lists of stop sequences, ids: B stop sets (None: none), tails: B tails (None:
    empty) -> (lengths [B], match words [B], tails [B, TAIL_LEN])."""
    tokens = np.asarray(tokens)
    steps, B = tokens.shape
    assert len(seqs) == B
    n, m, t = np.zeros(B, np.uint32), np.zeros(B, np.uint32), np.zeros((B, TAIL_LEN), np.uint32)
    for b in range(B):
        n[b], m[b], t[b] = run(tokens[:, b].tolist(), seqs[b], () if ids is None else ids[b], None if tails is None else tails[b])
    return n, m, t


def apply(tokens, seqs, ids=None, tails=None, steps_run=None):
    """(padded tokens [steps_run, B], lengths, match words, tails) of the stopped call: from its length on a sequence repeats the token
    that ended it, as tests/stop_ref.py's."""
    tokens = np.asarray(tokens, np.uint32)
    n, m, t = lengths(tokens, seqs, ids, tails)
    run_ = tokens.shape[0] if steps_run is None else steps_run
    out = tokens[:run_].copy()
    for b in range(tokens.shape[1]):
        if m[b] != NONE and n[b] < run_:
            out[n[b]:, b] = tokens[n[b] - 1, b]
    return out, n, m, t


def reply(stream, seqs, ids, max_new):
    """A request's reply of the queue, whose draws are `stream` while it runs: (length, reason, match word) -- reason 1 with the match
    word at the first draw with a match, else reason 2 and NONE at max_new (tests/queue_ref.py's reasons)."""
    n, m, _ = run(list(stream)[:max_new], seqs, ids)
    assert m != NONE or n == max_new, "the stream ends before the reply does"
    return (n, 1, m) if m != NONE else (n, 2, NONE)
