"""NumPy (f64) restatement of the reference's sampler, `Sampler::sample` in examples/chat.rs:150-190, as the device sampler
(wrk_sample_logits / *_generate_sample) is specified:

  * T == 0 or P == 0: the first index of the maximum (argmax_rows: 0 when no logit exceeds -3e38);
  * p = softmax(l) at temperature 1 (-inf logits give p = 0, NaN counts as -inf);
  * order: p descending, ties by index ascending;
  * nucleus: the token at rank r is in iff the mass before it is <= P (the token that crosses P is in); P >= 1: every token;
  * weights w = p^(1/T) inside the nucleus, W = sum(w);
  * draw: the first rank r with u * W <= cumsum(w)[r], else rank 0 (find_or_first);
  * u = (SplitMix64((seed << 32) | step) >> 40) * 2^-24.

Not a test module: tests/test_sampling_ref.py checks it by hand-worked cases, tests/test_gpu_sampling.py holds the kernel to it.
"""
import numpy as np

_MASK = (1 << 64) - 1
PREFIX_SLACK = 1e-4     # a prefix mass this close to P makes the nucleus boundary ambiguous
EDGE_SLACK = 1e-5       # u this close to an interval edge makes the draw ambiguous


def splitmix(seed: int, step: int) -> int:
    z = ((((seed & 0xFFFFFFFF) << 32) | (step & 0xFFFFFFFF)) + 0x9E3779B97F4A7C15) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def uniform(seed: int, step: int) -> float:
    return float(splitmix(seed, step) >> 40) * 2.0 ** -24


def greedy(logits) -> int:
    l = np.asarray(logits, np.float64)
    ok = l > -3.0e38
    if not ok.any():
        return 0
    return int(np.flatnonzero(l == l[ok].max())[0])


def nucleus(logits, temperature: float, top_p: float):
    """(tokens of the nucleus in rank order, their normalised weights, masses before every rank in the full order)."""
    l = np.asarray(logits, np.float64)
    l = np.where(np.isnan(l), -np.inf, l)
    mx = l.max()
    p = np.exp(l - mx)
    p /= p.sum()
    order = np.lexsort((np.arange(l.size), -l))          # l descending, index ascending
    ps = p[order]
    before = np.cumsum(ps) - ps
    n = l.size if top_p >= 1.0 else int(np.count_nonzero(before <= top_p))
    w = np.exp((l[order[:n]] - mx) / temperature)        # p^(1/T) up to the normalisation
    return order[:n], w / w.sum(), before


def sample(logits, temperature: float, top_p: float, seed: int = 0, step: int = 0, u=None) -> int:
    if temperature == 0.0 or top_p == 0.0:
        return greedy(logits)
    l = np.asarray(logits, np.float64)
    if not (np.where(np.isnan(l), -np.inf, l) > -np.inf).any():
        return 0
    toks, w, _ = nucleus(l, temperature, top_p)
    u = uniform(seed, step) if u is None else u
    hit = np.flatnonzero(u <= np.cumsum(w))
    return int(toks[hit[0]] if hit.size else toks[0])


def ambiguous(logits, temperature: float, top_p: float, seed: int = 0, step: int = 0) -> bool:
    """True when f32 rounding on the device may legitimately pick another token: some prefix mass within PREFIX_SLACK of P, or u within
    EDGE_SLACK of an interval edge of the draw."""
    if temperature == 0.0 or top_p == 0.0:
        return False
    _, w, before = nucleus(logits, temperature, top_p)
    if top_p < 1.0 and np.any(np.abs(before - top_p) < PREFIX_SLACK):
        return True
    edges = np.concatenate([[0.0], np.cumsum(w)])
    return bool(np.min(np.abs(edges - uniform(seed, step))) < EDGE_SLACK)
