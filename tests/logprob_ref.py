"""f64 restatement of the log-probs of chosen tokens and their top-N alternatives (web-rwkv-gguf_amd/csrc/wrk_logprob.hip,
`wrk_top_logprobs`), an f32 restatement of the kernel's sliced arithmetic, and the rows the tests share, for NumPy.

Per row x of V logits, chosen token y and n alternatives:
  logprob         = (x_y - m) - log sum_i exp(x_i - m), m = max_i x_i
  top_ids[j]      = the j-th token by logit descending, ties by index ascending (the sampler's order), j < n
  top_logprobs[j] = the same expression at top_ids[j]
A logit of -inf has log-prob -inf and sorts after every finite logit, by index; entries j >= V are id NO_ID and -inf; a NaN anywhere
gives NaN in logprob and in every top_logprobs entry (the ids are then unspecified: the restatement returns NO_ID)."""
import numpy as np

NO_ID = 0xFFFFFFFF
MAX_TOP = 20                # WRK_MAX_TOP_LOGPROBS
MIN_SLICE, MAX_SLICES = 2048, 32        # wrk_score.hip's SCORE_MIN_SLICE / SCORE_MAX_SLICES


def log_softmax(x):
    """f64 log-probs of a whole row without NaN."""
    x = np.asarray(x, np.float64)
    m = x.max()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lse = np.log(np.exp(x - m).sum())
        out = (x - m) - lse
    out[x == -np.inf] = -np.inf
    return out


def top_row(x, y: int, n: int):
    """(logprob f64, top_ids int64 [n], top_logprobs f64 [n]) of one row."""
    x = np.asarray(x, np.float64)
    V = x.size
    ids = np.full(n, NO_ID, np.int64)
    if np.isnan(x).any():
        return float("nan"), ids, np.full(n, np.nan)
    ls = log_softmax(x)
    # logit descending, then index ascending: a stable sort of the negated logits (-0 == +0: a tie)
    order = np.argsort(-x, kind="stable")[:n]
    ids[:order.size] = order
    tlp = np.full(n, -np.inf)
    tlp[:order.size] = ls[order]
    return float(ls[y]), ids, tlp


def top_rows(logits, tokens, n: int):
    """(logprob f64 [rows], top_ids int64 [rows, n], top_logprobs f64 [rows, n]) of rows [rows, V]."""
    out = [top_row(r, int(t), n) for r, t in zip(np.atleast_2d(logits), np.asarray(tokens).reshape(-1))]
    return (np.array([o[0] for o in out], np.float64), np.array([o[1] for o in out], np.int64).reshape(len(out), n),
            np.array([o[2] for o in out], np.float64).reshape(len(out), n))


# ------------------------------------------------------------------ the kernel's arithmetic in f32
def slices(rows: int, V: int, num_cu: int = 256):
    """wrk_score.hip's score_slices: the workgroups one row is split over."""
    want = (4 * max(num_cu, 1) + rows - 1) // rows
    most = (V + MIN_SLICE - 1) // MIN_SLICE
    return max(1, min(want, most, MAX_SLICES))


def keys(x32, descending_index: bool = False):
    """The sampler's unique order key per token: monotone(logit) << 20 | ~index (NaN counts as -inf, -0 as +0).
    descending_index: the mutant that breaks ties by index descending."""
    x = np.asarray(x32, np.float32).copy()
    x[np.isnan(x)] = -np.inf
    x = x + np.float32(0.0)
    b = x.view(np.uint32).astype(np.uint64)
    b = np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)
    idx = np.arange(x.size, dtype=np.uint64)
    return (b << np.uint64(20)) | (idx if descending_index else np.uint64(0xFFFFF) - idx)


def merge32(m, s, m2, s2, rescale: bool = True):
    """The kernel's (max, sum) merge in f32.  rescale=False: the mutant that forgets to rescale the smaller-max partial."""
    f = np.float32
    mn = max(m, m2)
    with np.errstate(invalid="ignore", over="ignore"):
        a = f(0) if s == 0 else (s if (m == mn or not rescale) else f(s * np.exp(f(m - mn))))
        b = f(0) if s2 == 0 else (s2 if (m2 == mn or not rescale) else f(s2 * np.exp(f(m2 - mn))))
    return f(mn), f(a + b)


def top_row_sliced(x32, y: int, n: int, S: int, rescale: bool = True, descending_index: bool = False):
    """The kernel's route in f32: S slices of ceil(V / S) rounded up to 4 logits, a (max, sum) partial and the n best keys per slice,
    the partials merged in slice order, the n best of the S * n candidates, the log-probs from the merged pair.
    Returns (logprob f32, top_ids int64 [n], top_logprobs f32 [n])."""
    f = np.float32
    x = np.asarray(x32, np.float32)
    V = x.size
    ln = ((V + S - 1) // S + 3) & ~3
    k = keys(x, descending_index)
    m, s, cand = f(-np.inf), f(0), []
    for a in range(0, V, ln):
        part = x[a:a + ln]
        pm = f(np.fmax.reduce(part, initial=f(-np.inf)))       # fmaxf drops NaN
        with np.errstate(invalid="ignore", over="ignore"):
            e = np.exp((part - pm).astype(f))
        ps = f(e[part != -np.inf].sum(dtype=f))
        m, s = merge32(m, s, pm, ps, rescale)
        cand.append(np.sort(k[a:a + ln])[::-1][:n])
    best = np.sort(np.concatenate(cand))[::-1][:n] if n else np.zeros(0, np.uint64)

    def finish(v):
        if s != s:
            return s
        with np.errstate(divide="ignore", invalid="ignore"):
            return f(-np.inf) if v == -np.inf else f(f(v - m) - f(np.log(s)))
    ids = np.full(n, NO_ID, np.int64)
    tlp = np.full(n, -np.inf, f)
    for j, key in enumerate(best):
        low = int(key) & 0xFFFFF
        ids[j] = low if descending_index else 0xFFFFF - low
        tlp[j] = finish(x[ids[j]])
    return finish(x[y]), ids, tlp


# ------------------------------------------------------------------ the rows the tests share
def kernel_rows(V: int, rows: int, seed: int):
    """`rows` rows of the kinds of tests/test_gpu_score.py's kernel_rows -- flat / peaked / half -inf / duplicated / tied maximum -- and
    a chosen token per row that alternates between the arg-max, a random token and a token on a tie (where the row has one)."""
    rng = np.random.default_rng(seed)
    out, tok = np.empty((rows, V), np.float32), np.empty(rows, np.uint32)
    for r in range(rows):
        kind = r % 5
        if kind == 0:
            x = rng.normal(0.0, 0.5, V)
        elif kind == 1:
            x = rng.normal(0.0, 3.0, V)
            x[rng.integers(V)] += 12.0
        elif kind == 2:
            x = rng.normal(0.0, 2.0, V)
            x[rng.random(V) < 0.5] = -np.inf
        else:
            x = np.round(rng.normal(0.0, 2.0, V) * 2.0) / 2.0
        if kind == 4:                                   # the maximum at several places
            ties = rng.choice(V, min(V, 4), replace=False)
            x[ties] = x.max() + 1.0
        x = x.astype(np.float32)
        choice = (r // 5 + r) % 3
        t = int(rng.integers(V))
        if choice == 0 and x.max() > -np.inf:
            t = int(x.argmax())
        elif choice == 2:
            vals, first, cnt = np.unique(x, return_index=True, return_counts=True)
            tied = np.nonzero(cnt > 1)[0]
            if tied.size:                               # the last token holding the largest repeated value
                t = int(np.nonzero(x == vals[tied[-1]])[0][-1])
        out[r], tok[r] = x, t
    return out, tok
