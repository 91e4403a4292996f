"""f64 restatement of sequence scoring (web-rwkv-gguf_amd/csrc/wrk_score.hip, `wrk_score_logits`) and of the
host's scoring plan (`wrk_rnn_score_plan`), for NumPy.

Per row x of logits and target token t:
  logprob = x_t - (m + log sum_i exp(x_i - m)), m = max_i x_i      (NaN anywhere: NaN; else x_t == -inf: -inf)
  rank    = #{i : x_i > x_t} + #{i < t : x_i == x_t}                (0 exactly when t is the first index of the maximum)
"""
import numpy as np


def score_row(x, t: int):
    """(logprob f64, rank int) of one row."""
    x = np.asarray(x, np.float64)
    xt = x[t]
    if np.isnan(x).any():
        lp = float("nan")
    elif xt == -np.inf:
        lp = -np.inf
    else:
        m = x.max()
        with np.errstate(invalid="ignore", over="ignore"):
            lp = float((xt - m) - np.log(np.exp(x - m).sum()))
    rank = int((x > xt).sum() + (x[:t] == xt).sum())
    return lp, rank


def score_rows(logits, targets):
    """(logprob f64 [n], rank int64 [n]) of rows [n, V]."""
    out = [score_row(r, int(t)) for r, t in zip(np.atleast_2d(logits), np.asarray(targets).reshape(-1))]
    return np.array([o[0] for o in out], np.float64), np.array([o[1] for o in out], np.int64)


def log_softmax_at(logits, targets):
    """The host-side route the device kernel replaces: an f64 log-softmax of full logit rows, read at the targets."""
    x = np.atleast_2d(np.asarray(logits, np.float64))
    m = x.max(axis=1, keepdims=True)
    ls = x - m - np.log(np.exp(x - m).sum(axis=1, keepdims=True))
    return ls[np.arange(x.shape[0]), np.asarray(targets, np.int64)]


def plan(remaining, lens):
    """wrk_rnn_score_plan: `remaining[b]` = batch b's tokens still in the input (this chunk included), `lens` = the chunk.
    Position i < lens[b] is scored iff token i + 1 of b exists; target = that token, header = its stacked row."""
    headers, targets, rows, p = [], [], [], 0
    for toks, n in zip(remaining, lens):
        k = 0
        for i in range(n):
            if i + 1 < len(toks):
                headers.append(p + i)
                targets.append(int(toks[i + 1]))
                k += 1
        rows.append(k)
        p += n
    return headers, targets, rows


def within_bar(got, want):
    """The kernel bar: |lp - lp64| <= 1e-5 + 1e-6 |lp64| (equal infinities and NaN pass)."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore"):
        close = np.abs(got - want) <= 1e-5 + 1e-6 * np.abs(want)
    return same | close
