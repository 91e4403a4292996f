"""The decode engine's K5 -> K6 hand-off in four-value granules (web-rwkv-gguf_amd/csrc/wrk_ffn_granule.h, wrk_v7_engine.hip; DESIGN.md
section 4.8): the ffn vector travels as four f16 per 64-bit granule with the tag (layer % 15) + 1 in their sign bits.

No product and no rounding point changed: the payload is masked where its sign bits are provably 0.  So, as in
tests/test_gpu_engine.py, the comparison with the five-launch layer (one workgroup per head: WRK_SPLIT_HEAD=0) is EXACT.  Every case
runs 6 greedy tokens on a fresh runtime per side and compares the tokens, the last logits and every state slot (att shift rows, WKV
state, ffn shift rows) bit for bit.

    case        layers  D     F      what it reaches
    wrap        17      512   2048   the 4-bit tag wraps (layers 15, 16 carry the tags of layers 0, 1); on 256 CUs every workgroup
                                     publishes 8 ffn rows = 2 granules
    half        17      256   1024   on 256 CUs only the first 128 workgroups have ffn key rows: the others publish nothing and still
                                     sweep the whole vector
    layer0      2       512   2048   starts at layer 0, which has no value LoRA: some workgroups have no K1 rows there and are waited
                                     for by no head
    second      3       512   2048   generate_greedy twice on one runtime: the state that launch n leaves (the att shift rows among
                                     it) is what launch n + 1 starts from

The engine's host keeps a workgroup's ffn key rows a multiple of 8 for every shape it accepts (F is a multiple of 1024), so the ffn
vector leaves in four-value granules always: there is no shape with 2 rows per workgroup, and no pair form of this vector left to
select.  `half` stands where such a case would: the other way a workgroup's share of the vector can differ.  `layer0` and `second`
guard the att shift state's writer, whichever workgroup that is (a build that moved it to workgroups without a head was measured and
not kept: profiles/handoff_ab.txt).  On a device where engine_status() refuses a shape the case skips with the reason; on a 256-CU
MI355X all four run."""
import numpy as np
import pytest

import wrk
from oracle import synth

pytestmark = pytest.mark.gpu

CASES = {
    "wrap": (synth.V7Config(17, 512, 2048, 1000, 64, 32, 32, 32, 64), 1),
    "half": (synth.V7Config(17, 256, 1024, 512, 64, 32, 32, 32, 64), 1),
    "layer0": (synth.V7Config(2, 512, 2048, 1000, 64, 32, 32, 32, 64), 1),
    "second": (synth.CONFIGS["small"], 2),
}
STEPS = 6


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def run(ctx, monkeypatch, data, engine, calls):
    """`calls` greedy runs of STEPS tokens, each fed the last token of the one before, on a fresh runtime; the last run's results"""
    monkeypatch.setenv("WRK_ENGINE", engine)
    monkeypatch.setenv("WRK_SPLIT_HEAD", "0")
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=1, weights=wrk.WEIGHTS_INLINE)
    rt.num_batch = 1
    try:
        if engine == "1":
            ok, why = rt.engine_status()
            if not ok:
                pytest.skip(f"decode engine off for this shape: {why}")
        rt.state_load(np.zeros_like(rt.state_back(0)), 0)
        first = [3]
        for _ in range(calls):
            tok, _, logits = rt.generate_greedy(first, STEPS, mode=1, want_logits=True)
            first = [int(np.asarray(tok)[-1, 0])]
        return np.asarray(tok).copy(), np.asarray(logits).copy(), rt.state_back(0).copy()
    finally:
        rt.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_handoff_equals_launches(ctx, monkeypatch, name):
    cfg, calls = CASES[name]
    data = synth.make_v7_gguf(cfg, 42)
    tok_e, lg_e, st_e = run(ctx, monkeypatch, data, "1", calls)
    tok_l, lg_l, st_l = run(ctx, monkeypatch, data, "0", calls)
    assert np.isfinite(lg_e).all() and lg_e.std() > 0
    assert np.array_equal(tok_e, tok_l)
    assert np.array_equal(lg_e.view(np.uint32), lg_l.view(np.uint32)), float(np.abs(lg_e - lg_l).max())
    # every slot of the state: row 0 of a layer is the att shift state, rows 1 .. 64 the WKV state, the last row the ffn shift state
    se, sl = st_e.view(np.uint32), st_l.view(np.uint32)
    assert se.shape == sl.shape
    diff = np.argwhere(se != sl)
    assert diff.size == 0, diff[:8].tolist()
    assert np.abs(st_e).max() > 0
