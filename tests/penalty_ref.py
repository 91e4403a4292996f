"""NumPy f32 restatement of the repetition penalties (ChatRWKV's PIPELINE.generate: alpha_presence, alpha_frequency, alpha_decay,
token_ban) as the device implements them (web-rwkv-gguf_amd/csrc/wrk_penalty.hip).  Every operation rounds to f32 once,
with no fused multiply-add, so the device matches it bit for bit:

  * penalize: x'[n] = -inf if banned[n]; x[n] - (ap + count[n] * af) if present[n] (t = count * af; t = ap + t; x - t); else x[n];
  * update after the draw of y: count *= decay (every entry), then count[y] += w[y], then present[y] = 1.

flags: bit 0 present, bit 1 banned.  The draw itself is tests/sampling_ref.py's `sample` on the penalised row.
Not a test module: tests/test_penalty_ref.py checks it by hand-worked cases, tests/test_gpu_penalty.py holds the device to it.
"""
import numpy as np

PRESENT, BANNED = 1, 2


def penalize(x, counts, flags, ap, af) -> np.ndarray:
    x = np.asarray(x, np.float32)
    c = np.asarray(counts, np.float32)
    f = np.asarray(flags).astype(np.uint32)
    with np.errstate(all="ignore"):
        t = c * np.float32(af)
        t = np.float32(ap) + t
        y = np.where(f & PRESENT, x - t, x)
    return np.where(f & BANNED, np.float32(-np.inf), y).astype(np.float32)


def update(counts, flags, y: int, w, decay):
    """(counts, flags) after drawing y; the inputs are not modified."""
    c = np.asarray(counts, np.float32) * np.float32(decay)
    f = np.asarray(flags).astype(np.uint32).copy()
    c[y] = c[y] + np.asarray(w, np.float32)[y]
    f[y] |= PRESENT
    return c.astype(np.float32), f


def update_all(counts, flags, tokens, w, decay):
    for y in tokens:
        counts, flags = update(counts, flags, int(y), w, decay)
    return counts, flags
