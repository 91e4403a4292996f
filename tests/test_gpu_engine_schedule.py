"""The row schedule of the decode engine's one-wave-per-row stages (eng_wave_rows in web-rwkv-gguf_amd/csrc/wrk_v7_engine.h) and the
unpadded last batch of eng_rows, on the smallest models that reach every branch of it on a 256-CU device.

Only WHICH wave computes a row, and in a batch of how many, differs from the launches' mapping; every row keeps its arithmetic.  So,
as in tests/test_gpu_engine.py, the comparison with the five-launch layer (one workgroup per head: WRK_SPLIT_HEAD=0) is EXACT: the
logits of six forced tokens on sequence slot 1 of 2 and both state slots are bit-identical.

Rows per workgroup on 256 CUs (the host partition of wrk_v7_engine_create):

    model                 K1 r / k / v   K5    what it reaches
    1.5B-3L (D = 2048)    36             32    a batch of four, then an unpadded batch of two; waves with three and with two pairs;
                                               layer 0 without and layers 1 - 2 with the value LoRA
    D = 1024, F = 4096    20             16    waves with two pairs and with one; K5 with one pair per wave: the two-row body alone
    D = 768, F = 3072     14             16    seven pairs on eight waves: one wave without rows; D not a power of two
"""
import functools

import numpy as np
import pytest

import wrk
from oracle import synth

pytestmark = pytest.mark.gpu

MODELS = {
    "1.5B-3L": synth.CONFIGS["1.5B-3L"],
    "d1024": synth.V7Config(2, 1024, 4096, 512, 64, 64, 64, 32, 128),
    "d768": synth.V7Config(2, 768, 3072, 512, 64, 64, 64, 32, 128),
}


@functools.lru_cache(maxsize=None)
def model_bytes(name):
    return synth.make_v7_gguf(MODELS[name], 42)


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def forced(rt, toks, batch):
    return np.stack([rt.infer_raw([t], [batch | (0 << 8) | (1 << 24)], [0], mode=1)[0] for t in toks])


def engine_equals_launches(ctx, monkeypatch, name, weights, waves=8):
    rt = wrk.Runtime(ctx, wrk.GgufReader(model_bytes(name)), num_batch=2, weights=weights)
    rt.num_batch = 2
    try:
        monkeypatch.setenv("WRK_ENGINE", "1")
        ok, why = rt.engine_status()
        assert ok, why
        assert why == f"{waves} compute waves", why      # the kernel the tokens below run on
        V = rt.info.num_vocab
        toks = [(5 + 37 * i) % (V - 1) for i in range(6)]
        res = []
        for engine in ("1", "0"):
            monkeypatch.setenv("WRK_ENGINE", engine)
            monkeypatch.setenv("WRK_SPLIT_HEAD", "0")
            z = np.zeros_like(rt.state_back(0))
            for b in range(2):
                rt.state_load(z, b)
            res.append((forced(rt, toks, 1), rt.state_back(1), rt.state_back(0)))
        (a, sa, s0a), (b, sb, s0b) = res
        assert np.isfinite(a).all() and a.std() > 0
        assert np.array_equal(a, b), float(np.abs(a - b).max())
        assert np.array_equal(sa, sb) and np.abs(sa).max() > 0
        assert np.array_equal(s0a, s0b) and not s0a.any()       # the other slot is untouched
    finally:
        rt.close()


@pytest.mark.parametrize("name,weights", [("1.5B-3L", wrk.WEIGHTS_INLINE), ("1.5B-3L", wrk.WEIGHTS_INLINE_F16), ("d1024", wrk.WEIGHTS_INLINE),
                                          ("d768", wrk.WEIGHTS_INLINE)])
def test_schedule_equals_launches(ctx, monkeypatch, name, weights):
    engine_equals_launches(ctx, monkeypatch, name, weights)


def test_schedule_equals_launches_14_compute_waves(ctx, monkeypatch):
    """WRK_ENGINE_WAVES=14 is read when the engine is built, i.e. at the runtime's first engine_status(), which then reports
    "14 compute waves": 18 row pairs on 14 waves."""
    monkeypatch.setenv("WRK_ENGINE_WAVES", "14")
    engine_equals_launches(ctx, monkeypatch, "1.5B-3L", wrk.WEIGHTS_INLINE, waves=14)
