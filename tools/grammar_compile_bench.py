"""Time of wrk_grammar_compile: regex x vocabulary -> token automaton, on the device, against the NumPy walk of the tests.

The vocabulary is seeded and synthetic: 65 536 byte strings, all 256 single bytes first, the rest 2 to 16 bytes long -- half of them
over the printable ASCII that structured output is made of (digits, letters, JSON punctuation), half over all bytes.  Three inputs:

  datetime   an ISO date-time regex
  json       a JSON object with three typed fields (a string, an integer, a boolean)
  choices    1 000 random 8-byte choices (wrk.regex_of_choices)

For each: the byte-DFA states S and the time of the host regex compile, the token automaton's states and classes C, the device compile
time (median of --repeat runs, every phase of wrk_grammar_compile_last_ms separately, and the wall time of the call), and the time of
the NumPy reference on the same input: tests/grammar_compile_ref.py's vectorised walk in blocks of --block states (so that its
[states][V] temporaries stay bounded), and the merge of equal columns (wrk.grammar_from_dense on the trimmed table) where the dense
table has at most --merge-limit entries.  The device result is compared with the reference wherever the reference is complete.
One JSON line per input, and all of them in --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "web-rwkv-gguf_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import grammar_compile_ref as R  # noqa: E402
import wrk  # noqa: E402

DATETIME = r"[0-9]{4}-(0[1-9]|1[0-2])-(0[1-9]|[12][0-9]|3[01])T([01][0-9]|2[0-3]):[0-5][0-9]:[0-5][0-9](\.[0-9]{1,6})?(Z|[+\-][01][0-9]:[0-5][0-9])"
JSON_OBJECT = (r'\{\s?"name":\s?"([^"\\\x00-\x1f]|\\["\\/bfnrt]){0,32}",\s?"age":\s?(0|[1-9][0-9]{0,2}),\s?"member":\s?(true|false)\s?\}')
PRINTABLE = b"0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ {}[]\":,.-+_:\\/TZ\n"


def vocabulary(seed: int, V: int):
    rng = np.random.default_rng(seed)
    vocab = [bytes([b]) for b in range(256)]
    seen = set(vocab)
    alpha = np.frombuffer(PRINTABLE, np.uint8)
    while len(vocab) < V:
        n = int(rng.integers(2, 17))
        tok = bytes((alpha[rng.integers(0, alpha.size, n)] if len(vocab) % 2 else rng.integers(0, 256, n)).astype(np.uint8).tolist())
        if tok not in seen:
            seen.add(tok)
            vocab.append(tok)
    return vocab


def numpy_reference(dfa, vocab, end, block, merge_limit):
    S, V = dfa.num_states, len(vocab)
    full = (S + 1) * V <= merge_limit
    table = np.empty((S + 1, V), np.int64) if full else None
    t0 = time.perf_counter()
    for s0 in range(0, S, block):
        rows = R.walk_rows_numpy(dfa.next, vocab, s0, min(S, s0 + block))
        if full:
            table[s0:s0 + rows.shape[0]] = rows
    walk_s = time.perf_counter() - t0
    if not full:
        return dict(numpy_walk_s=walk_s, numpy_merge_s=None), None
    table[:S, end] = np.where(dfa.accepting != 0, S, -1)
    table[S] = -1
    table[S, end] = S
    t0 = time.perf_counter()
    trimmed, starts, fin = R.token_trim(table, dfa.starts.tolist())
    cls, trans = wrk.grammar_from_dense(trimmed)
    return dict(numpy_walk_s=walk_s, numpy_merge_s=time.perf_counter() - t0), (cls, trans, starts, fin)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=65536)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--merge-limit", type=int, default=1 << 27)
    ap.add_argument("--no-numpy", action="store_true", help="device times only (for a profiler run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    vocab = vocabulary(2024, args.vocab)
    end = 0
    rng = np.random.default_rng(77)
    inputs = [("datetime", DATETIME), ("json", JSON_OBJECT),
              ("choices", wrk.regex_of_choices([bytes(rng.integers(0, 256, 8).tolist()) for _ in range(1000)]))]
    ctx = wrk.Context(0)
    results = []
    for name, pattern in inputs:
        t0 = time.perf_counter()
        dfa = wrk.ByteDfa.from_regex(pattern)
        regex_ms = (time.perf_counter() - t0) * 1e3
        wrk.Grammar.compile(ctx, vocab, dfa, end).close()          # warm-up: code objects, allocator
        phases, wall = [], []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            g = wrk.Grammar.compile(ctx, vocab, dfa, end)
            wall.append((time.perf_counter() - t0) * 1e3)
            phases.append(g.compile_ms)
            tables = (g.token_class.copy(), g.transitions.copy(), g.start_states.tolist(), g.final_state)
            g.close()
        res = dict(input=name, vocab=len(vocab), vocab_bytes=sum(map(len, vocab)), byte_dfa_states=dfa.num_states, regex_compile_ms=round(regex_ms, 3),
                   states=int(tables[1].shape[0]), classes=int(tables[1].shape[1]), device_wall_ms=round(float(np.median(wall)), 3),
                   device_phase_ms={k: round(float(np.median([p[k] for p in phases])), 3) for k in wrk.GRAMMAR_COMPILE_PHASES},
                   repeat=args.repeat)
        if not args.no_numpy:
            ref, want = numpy_reference(dfa, vocab, end, args.block, args.merge_limit)
            res.update({k: (None if v is None else round(v, 3)) for k, v in ref.items()})
            if want is not None:
                same = (np.array_equal(tables[0], want[0]) and np.array_equal(tables[1], want[1]) and tables[2] == want[2] and tables[3] == want[3])
                res["equals_numpy"] = bool(same)
                assert same, name
            res["numpy_walk_over_device_wall"] = round(ref["numpy_walk_s"] * 1e3 / res["device_wall_ms"], 1)
        results.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
