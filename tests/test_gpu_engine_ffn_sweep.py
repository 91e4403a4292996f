"""K6's fetch of the ffn vector in the decode engine (web-rwkv-gguf_amd/csrc/wrk_v7_engine.hip, eng_sweep_half): of the two waves of
a K quarter the one of row group 0 polls the `lo` halves of the quarter's chunks, the one of row group 1 the `hi` halves, both into an
exchange area in LDS that lies over the stage-input block, and every K6 wave reads its chunks back from there.

Only where a wave's inputs come from differs; the bits that reach the dot products do not.  So, as in
tests/test_gpu_engine_schedule.py, the comparison with the five-launch layer (one workgroup per head: WRK_SPLIT_HEAD=0) is EXACT:
logits of six forced tokens on sequence slot 1 of 2, both state slots, the other slot untouched.

K6 on 256 CUs (the host partition of wrk_v7_engine_create):

    model                 waves   rows per workgroup and row group   what it reaches
    1.5B-3L (F = 8192)    8       8 = 4 + 4                          the headline's layout: 256 chunks on 4 x 64 lanes, the exchange area
                                                                     over the stage-input block AND the tail behind it (16 KB over 11 KB)
    1.5B-3L               14      8 = 3 + 3 + 2                      a third row group, which polls nothing and only reads
    D = 768, F = 3072     8       4 = 2 + 2; 64 workgroups without   workgroups that neither poll nor read; 96 chunks on 256 lanes: lanes
                                  rows                               clamped to the last chunk write it again, and read it back as zeros
    D = 1024, F = 4096    8       4 = 2 + 2                          two rows per group, 128 chunks: K quarters 2 and 3 all clamped

The greedy run (32 tokens x 3 layers on one engine, against the launches) is there for a stale exchange area: the area is rewritten in
every layer of every token, over the block that the LN of the next layer overwrites in between.

An XD = 2 instantiation of K6 (D > 2048) cannot be reached: the smallest such shape the engine takes, D = 2304 / F = 9216, needs more
than 200 KB of LDS for the weights of a layer on 256 CUs (2.9B-2L: 242 KB), so engine_status() reports it off before any K6 runs.
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


def both(monkeypatch, rt, fn):
    """fn(rt) with the engine, then with the launches (one workgroup per head), each from zeroed state slots."""
    res = []
    for engine in ("1", "0"):
        monkeypatch.setenv("WRK_ENGINE", engine)
        monkeypatch.setenv("WRK_SPLIT_HEAD", "0")
        z = np.zeros_like(rt.state_back(0))
        for b in range(rt.num_batch):
            rt.state_load(z, b)
        res.append(fn(rt))
    return res


def open_runtime(ctx, monkeypatch, name, num_batch, waves):
    rt = wrk.Runtime(ctx, wrk.GgufReader(model_bytes(name)), num_batch=num_batch, weights=wrk.WEIGHTS_INLINE)
    rt.num_batch = num_batch
    monkeypatch.setenv("WRK_ENGINE", "1")
    ok, why = rt.engine_status()
    if not (ok and why == f"{waves} compute waves"):      # the kernel the tokens below run on
        rt.close()
        raise AssertionError(why)
    return rt


def sweep_equals_launches(ctx, monkeypatch, name, waves=8):
    rt = open_runtime(ctx, monkeypatch, name, 2, waves)
    try:
        V = rt.info.num_vocab
        toks = [(5 + 37 * i) % (V - 1) for i in range(6)]
        (a, sa, s0a), (b, sb, s0b) = both(monkeypatch, rt, lambda r: (forced(r, toks, 1), r.state_back(1), r.state_back(0)))
        assert np.isfinite(a).all() and a.std() > 0
        assert np.array_equal(a, b), float(np.abs(a - b).max())
        assert np.array_equal(sa, sb) and np.abs(sa).max() > 0
        assert np.array_equal(s0a, s0b) and not s0a.any()       # the other slot is untouched
    finally:
        rt.close()


@pytest.mark.parametrize("name", ["1.5B-3L", "d768", "d1024"])
def test_ffn_sweep_equals_launches(ctx, monkeypatch, name):
    sweep_equals_launches(ctx, monkeypatch, name)


def test_ffn_sweep_equals_launches_14_compute_waves(ctx, monkeypatch):
    """WRK_ENGINE_WAVES=14 is read when the engine is built, at the runtime's first engine_status()."""
    monkeypatch.setenv("WRK_ENGINE_WAVES", "14")
    sweep_equals_launches(ctx, monkeypatch, "1.5B-3L", waves=14)


def test_ffn_sweep_greedy_32_steps(ctx, monkeypatch):
    rt = open_runtime(ctx, monkeypatch, "1.5B-3L", 1, 8)
    try:
        (ta, la), (tb, lb) = both(monkeypatch, rt, lambda r: (lambda o: (o[0], o[2]))(r.generate_greedy([3], 32, mode=1, want_logits=True)))
        assert ta.shape[0] == 32
        assert np.array_equal(ta, tb)
        assert np.array_equal(la, lb)
    finally:
        rt.close()
