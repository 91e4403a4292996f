"""The measure and the fixed bars of the per-layer, teacher-forced parity tests (tests/test_gpu_layer_parity.py for RWKV-7,
tests/test_gpu_v6_layer_parity.py and tests/test_v6_layer_ref.py for RWKV-6).  NumPy only: the CPU tests import it too."""
import numpy as np


def ulps(got, want):
    """|got - want| in units of the f16 spacing at max(|want|, rms(want)): an element that is small against its buffer (a
    cancelling sum) is measured with the spacing of a typical element -- the f32 accumulation error of a dot product scales
    with sum|w||x|, not with its result."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    rms = float(np.sqrt(np.mean(np.square(want, dtype=np.float64)))) + 1e-30
    mag = np.maximum(np.maximum(np.abs(want), rms), 2.0 ** -14)
    return np.abs(got - want) / 2.0 ** (np.floor(np.log2(mag)) - 10)


# FIXED bars.  RWKV-7, measured on MI355X over every case of test_gpu_layer_parity.py (profiles/r02_layer_parity.json, summary in DESIGN.md
# section 2): direct buffers <= 1 ulp everywhere (93-100 % bit-identical); downstream buffers <= 5 ulp, >= 84.7 % of the elements within 1 ulp.
# RWKV-6 takes the same bars (measured values: tests/test_gpu_v6_layer_parity.py).
DIRECT_MAX_ULP, DOWNSTREAM_MAX_ULP, DOWNSTREAM_FRAC_LE1 = 1.0, 6.0, 0.80
STATE_REL = 2.0 ** -9           # state (f32): max |delta| <= STATE_REL * max|state of the layer and sequence|

STATS = {}                      # RWKV-7's cases; the RWKV-6 files pass dicts of their own


def check(case, name, got, want, direct, downstream_max_ulp=None, stats=None):
    stats = STATS if stats is None else stats
    u = ulps(got.reshape(want.shape), want)
    s = stats.setdefault(case, {}).setdefault(name, {"max_ulp": 0.0, "min_frac_le1": 1.0, "min_frac_exact": 1.0, "n": 0, "max_strict_ulp": 0.0,
                                                     "min_frac_strict_le1": 1.0})
    # strict measure: the f16 spacing at |want| itself, no floor at the buffer's rms -- reported beside the graded one
    w32 = np.asarray(want, np.float32)
    su = np.abs(np.asarray(got, np.float32).reshape(w32.shape) - w32) / 2.0 ** (np.floor(np.log2(np.maximum(np.abs(w32), 2.0 ** -14))) - 10)
    s["max_strict_ulp"] = max(s["max_strict_ulp"], float(su.max()))
    s["min_frac_strict_le1"] = min(s["min_frac_strict_le1"], float((su <= 1.0).mean()))
    s["max_ulp"] = max(s["max_ulp"], float(u.max()))
    s["min_frac_le1"] = min(s["min_frac_le1"], float((u <= 1.0).mean()))
    s["min_frac_exact"] = min(s["min_frac_exact"], float((u == 0).mean()))
    s["n"] += 1
    max_ulp, frac1 = (DIRECT_MAX_ULP, 1.0) if direct else (downstream_max_ulp or DOWNSTREAM_MAX_ULP, DOWNSTREAM_FRAC_LE1)
    assert u.max() <= max_ulp, f"{case} {name}: {u.max():.2f} ulp (limit {max_ulp}); {int((u > 1).sum())} of {u.size} elements beyond 1 ulp"
    assert (u <= 1.0).mean() >= frac1, f"{case} {name}: only {(u <= 1.0).mean():.5f} of the elements within 1 ulp"


def aggregate(stats):
    """Worst max_ulp / min share within 1 ulp per buffer over all cases."""
    agg = {}
    for bufs in stats.values():
        for b, s in bufs.items():
            a = agg.setdefault(b, {"max_ulp": 0.0, "min_frac_le1": 1.0})
            a["max_ulp"] = max(a["max_ulp"], s["max_ulp"])
            a["min_frac_le1"] = min(a["min_frac_le1"], s["min_frac_le1"])
    return agg
