"""NumPy restatement of the logit bias (web-rwkv-gguf_amd/csrc/wrk_bias.hip): per-row sparse additive biases and bans.

  * a bias set is pairs (id, value); a value of -inf bans the token, a finite one is added to its logit;
  * apply: a banned token gets the bits of -inf whatever its logit is (not x + (-inf), which is NaN for x = +inf); a token with a finite
    value v gets x + v, one f32 addition; every other token keeps its bits (NaN payloads and -0 included);
  * a biased pick is the existing pick on the row after apply, then penalty_ref, then dry_ref, then grammar_ref.mask: bias first;
  * check_sets: what wrk_logit_bias_create accepts.

Not a test module: tests/test_bias_ref.py checks it, tests/test_gpu_bias.py holds the kernel and the decode loops to it.
"""
import numpy as np

NONE = 0xFFFFFFFF           # WRK_BIAS_NONE
MAX_SETS = 65536            # WRK_MAX_BIAS_SETS
MAX_VOCAB = 1 << 20         # the sampler's limit
NEG_INF_BITS = np.uint32(0xFF800000)


def apply(row, ids, values) -> np.ndarray:
    """The row as the rest of the step sees it with the set (ids, values); ids None: WRK_BIAS_NONE, the row bit for bit."""
    out = np.array(row, np.float32, copy=True)
    if ids is None:
        return out
    ids = np.asarray(ids, np.int64).reshape(-1)
    values = np.asarray(values, np.float32).reshape(-1)
    assert ids.size == values.size and len(set(ids.tolist())) == ids.size
    bits = out.view(np.uint32)
    ban = values == -np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        out[ids[~ban]] = out[ids[~ban]] + values[~ban]       # every id once: one f32 addition per entry
    bits[ids[ban]] = NEG_INF_BITS
    return out


def check_sets(num_vocab, offsets, ids, values) -> str:
    """"ok", "arg" (WRK_E_ARG) or "unsupported" (WRK_E_UNSUPPORTED): what wrk_logit_bias_create answers."""
    if num_vocab < 1:
        return "arg"
    if num_vocab > MAX_VOCAB:
        return "unsupported"
    if offsets is None or ids is None or values is None:
        return "arg"
    offsets = [int(x) for x in offsets]
    S = len(offsets) - 1
    if S < 1 or S > MAX_SETS or offsets[0] != 0 or any(b < a for a, b in zip(offsets, offsets[1:])):
        return "arg"
    for s in range(S):
        i = [int(x) for x in ids[offsets[s]:offsets[s + 1]]]
        v = np.asarray(values[offsets[s]:offsets[s + 1]], np.float32)
        if any(t < 0 or t >= num_vocab for t in i) or len(set(i)) != len(i):
            return "arg"
        if np.isnan(v).any() or (v == np.inf).any():
            return "arg"
        if int((v == -np.inf).sum()) >= num_vocab:
            return "arg"
    return "ok"


def check_set_words(num_sets, words) -> bool:
    """True iff every set word of a call is < num_sets or NONE."""
    return all(int(w) < num_sets or int(w) == NONE for w in words)
