"""The decode engine's head workgroups read the LoRA up-projections from a packed per-head image and run a 64-channel LN1
(web-rwkv-gguf_amd/csrc/wrk_lora2_pack.h, wrk_v7_engine.hip), on the ranks at which the pack can go wrong.

Only where a weight is fetched from changed, and how much of LN1 a head workgroup computes; every product and every rounding point is
what it was.  So, as in tests/test_gpu_engine_schedule.py, the comparison with the five-launch layer (one workgroup per head:
WRK_SPLIT_HEAD=0) is EXACT: the logits of six forced tokens on sequence slot 1 of 2 and both state slots -- the att shift state, which
the head workgroup's LN writes, among them -- are bit-identical.

    ranks (w, a, v, g)      pieces per unit    what it reaches
    40, 24, 8, 72           2, 1, 1, 3         partial last pieces (40, 72), a matrix below 32 columns (24: one piece, one lane in four
                                               beyond the rank), the minimum rank (8); three layers: layer 0 without the value LoRA
                                               (its pieces are zeros and its dots dropped), layers 1 - 2 with it
    128, 128, 128, 256      4, 4, 4, 8         the maximum ranks: every register of a lane holds a piece

The tests/test_gpu_engine*.py cases on 1.5B-3L cover whole pieces at the headline ranks (96, 96, 64, 256)."""
import numpy as np
import pytest

import wrk
from oracle import synth

pytestmark = pytest.mark.gpu

MODELS = {
    "partial": synth.V7Config(3, 256, 1024, 512, 64, 40, 24, 8, 72),
    "maximum": synth.V7Config(2, 512, 2048, 512, 64, 128, 128, 128, 256),
}


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def forced(rt, toks, batch):
    return np.stack([rt.infer_raw([t], [batch | (0 << 8) | (1 << 24)], [0], mode=1)[0] for t in toks])


@pytest.mark.parametrize("name", sorted(MODELS))
def test_packed_lora2_equals_launches(ctx, monkeypatch, name):
    rt = wrk.Runtime(ctx, wrk.GgufReader(synth.make_v7_gguf(MODELS[name], 42)), num_batch=2, weights=wrk.WEIGHTS_INLINE)
    rt.num_batch = 2
    try:
        monkeypatch.setenv("WRK_ENGINE", "1")
        ok, why = rt.engine_status()
        assert ok, why
        assert why == "8 compute waves", why      # the kernel the tokens below run on
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
