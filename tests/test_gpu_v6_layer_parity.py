"""RWKV-6: per-layer, teacher-forced parity of every stored buffer (the RWKV-7 file is tests/test_gpu_layer_parity.py).

For every token the ORACLE (oracle/rwkv6.py) runs the whole model with its trace on.  The HIP path then runs each layer ALONE
(`wrk_v6_infer_layer`) on the oracle's own layer input and pre-token state, and every buffer the layer stores (`wrk_v6_frame_read`) is
compared with the oracle's buffer of that stage.  Differences can only come from inside ONE layer.  Cases, measure and bars are shared with
tests/test_v6_layer_ref.py, which runs the reference itself (in two other summation orders) and ten wrong layers through them on the CPU.

Bars (tests/layer_parity.py; "ulp" = the f16 spacing at max(|value|, rms of the buffer); the CPU column is the reference against itself in
another summation order, the GPU column what an MI355X measured over every case below, profiles/v6_layer_parity.json):

  | buffers                                                            | bar                                  | CPU                | GPU                  |
  |--------------------------------------------------------------------|--------------------------------------|--------------------|----------------------|
  | DIRECT: LN1(x) (att_x of the fused layer); att_xx in decode        | every element <= 1 ulp               | 0 ulp              | 1 ulp, 99.2 % exact  |
  | DOWNSTREAM f16: every other f16 buffer but att_sx                  | <= 6 ulp, >= 80 % <= 1 ulp           | 5 ulp, 92.2 %      | 5 ulp, 91.0 %        |
  | att_sx (v6_layer_ref.BUFFER_MAX_ULP: CPU worst 5 ulp, times 2)     | <= 10 ulp, >= 80 % <= 1 ulp          | 5 ulp, 99.7 %      | 7 ulp, 99.4 %        |
  | f32 (att_k, att_v, att_r, time_decay), same measure, as downstream | <= 6 ulp, >= 80 % <= 1 ulp           | 1.6 ulp, 99.6 %    | 1.6 ulp, 99.8 %      |
  | state (f32)                                                        | <= 2^-9 max|state|                   | 9.8e-4             | 5.5e-4               |
  | stage-local tm (op list) / att_sx (fused), from the stored tmx     | >= 95 % bit-identical; <= 1 / 10 ulp | 99.92 %; 1 / 4 ulp | 99.92 %; 1 / 4 ulp   |
  | stage-local time_decay (op list), from the stored att_w            | <= 1/8 ulp                           | 4e-4 ulp           | 2e-4 ulp             |

Which stage each buffer holds when the layer ends (several are overwritten on the way):

  | path                                         | buffers                                                                                          |
  |----------------------------------------------|--------------------------------------------------------------------------------------------------|
  | op list (mode 0; mode 1 where the fused      | att_xx, tmx, tmt (tmx transposed), tm, att_sx, att_k, att_v, att_r, att_g, att_w, time_decay,    |
  | layer declines)                              | aux_x = group-norm output, att_x = gated output (LN1(x) is overwritten), att_o, ffn_kx, ffn_rx,  |
  |                                              | ffn_k, ffn_v, ffn_r, ffn_x = gated ffn (LN2(x) is overwritten), x = layer output (halved)        |
  | merged op list (mode 1, chunks)              | the same without att_o (W_o's add is the GEMM's epilogue)                                        |
  | fused layer, one token (T == 1)              | att_x = LN1(x), tmx, att_sx, att_k, att_v, att_r, att_g, att_w, aux_x = gated output,            |
  |                                              | ffn_x = LN2(x), ffn_k, ffn_r, x                                                                  |
  | fused layer, several sequences               | the same + att_xx, ffn_kx, ffn_rx, ffn_v; ffn_x = gated ffn                                      |

`tm` and `att_o` are written by the op list only: on a fresh runtime they are still the zeros of the allocation after a fused layer, and
every fused case asserts that (the fallback case the opposite).  time_decay and the WKV output before the group norm never leave the
fused head kernel, and the op list normalises the WKV output in place: no table can hold them.
"""
import json
import os

import numpy as np
import pytest

import v6_layer_ref as R
import wrk
from layer_parity import aggregate, check
from oracle.rnn import stack_cursors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


STATS = {}

# (frame buffer, oracle trace key)
_COMMON = [("tmx", "tmx"), ("att_sx", "att_sx"), ("att_k", "k"), ("att_v", "v"), ("att_r", "r"), ("att_g", "g"), ("att_w", "att_w")]
MERGED = [("att_xx", "att_xx"), ("tmt", "tmt"), ("tm", "tm"), ("time_decay", "time_decay"), ("aux_x", "gn"), ("att_x", "att_x"), ("ffn_kx", "ffn_kx"),
          ("ffn_rx", "ffn_rx"), ("ffn_k", "ffn_k"), ("ffn_v", "ffn_v"), ("ffn_r", "ffn_r"), ("ffn_x", "ffn_x"), ("x", "x")] + _COMMON
OPS = MERGED + [("att_o", "att_o")]
FUSED_ONE = [("att_x", "att_x_ln"), ("aux_x", "att_x"), ("ffn_x", "ffn_x_ln"), ("ffn_k", "ffn_k"), ("ffn_r", "ffn_r"), ("x", "x")] + _COMMON
FUSED_MANY = [("att_x", "att_x_ln"), ("att_xx", "att_xx"), ("aux_x", "att_x"), ("ffn_kx", "ffn_kx"), ("ffn_rx", "ffn_rx"), ("ffn_k", "ffn_k"),
              ("ffn_v", "ffn_v"), ("ffn_r", "ffn_r"), ("ffn_x", "ffn_x"), ("x", "x")] + _COMMON


def path_of(model, lens, mode):
    """Which launches wrk_v6_infer (and so wrk_v6_infer_layer) picks: (table, fused?)."""
    decode, T = all(n <= 1 for n in lens), sum(lens)
    if mode == 0:
        return OPS, False
    if not decode:
        return MERGED, False
    if model.info.custom["time_mix"] > 128 or model.info.custom["time_decay"] > 128:
        return OPS, False                       # the fused layer declines: the plain op list
    return (FUSED_ONE if T == 1 else FUSED_MANY), True


def want_of(trace, li, key):
    if key == "tmt":                            # transpose [R, 5, T] -> [R, T, 5]
        tmx = trace[f"{li}_tmx"]
        return np.ascontiguousarray(tmx.reshape(len(tmx), 5, -1).transpose(1, 0, 2))
    return trace[f"{li}_{key}"]


def layers_of(ctx, case, mode):
    """Per (step, layer) of a case: the runtime after `infer_layer` of that layer alone on the oracle's input and pre-token state."""
    c = R.CASES[case]
    data, model = R.fixture(case)
    lens = c["lens"]
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=len(lens), weights=wrk.WEIGHTS_INLINE_F16 if c["f16"] else wrk.WEIGHTS_INLINE)
    try:
        assert rt.info.version == 6 and rt.info.num_layer == model.info.num_layer
        cursors = stack_cursors(lens)
        for before, trace, after in R.replay(model, lens, c["steps"], c["warm"]):
            for b in range(len(lens)):
                rt.state_load(before[:, b], b)                    # teacher-forced state: a layer's run touches its own slice only
            for li in range(model.info.num_layer):
                rt.infer_layer(li, R.layer_input(trace, li), None, cursors, mode=mode)
                yield rt, model, li, before[li], trace, after[li]
    finally:
        rt.close()


def run_case(ctx, case, mode):
    lens = R.CASES[case]["lens"]
    T, live = sum(lens), [b for b, n in enumerate(lens) if n]
    cid = f"{case}/mode{mode}"
    for rt, model, li, before, trace, after in layers_of(ctx, case, mode):
        table, fused = path_of(model, lens, mode)
        p = model.layers[li]
        got = {buf: rt.frame(buf, T).astype(np.float32) for buf in {b for b, _ in table} | {"tm", "att_o"}}
        op_list_ran = bool(np.any(got["tm"]) and (table is MERGED or np.any(got["att_o"])))
        if fused:
            assert not np.any(got["tm"]) and not np.any(got["att_o"]), f"{cid}: the op list ran, not the fused layer"
        else:
            assert op_list_ran, f"{cid}: the op list did not run"
        for buf, key in table:
            check(cid, buf, got[buf], want_of(trace, li, key), R.is_direct(key, lens), R.BUFFER_MAX_ULP.get(key), stats=STATS)
        state = np.stack([rt.state_back(b)[li] for b in range(len(lens))])
        R.grade_state(cid, li, state, after, lens, STATS)
        for b in set(range(len(lens))) - set(live):
            assert np.array_equal(state[b], before[b]), f"{cid} layer {li}: the state of idle slot {b} changed"
        # stage-local: recomputed from what this layer stored itself (v6_layer_ref.py)
        if fused:
            prev = np.stack([before[b, 0] for b in live])
            R.grade_local(cid, "local_att_sx", got["att_sx"], R.local_att_sx(p, got["tmx"], got["att_x"], prev), True, STATS,
                         max_ulp=R.BUFFER_MAX_ULP["att_sx"])
        else:
            R.grade_local(cid, "local_tm", got["tm"], R.local_tm(p, got["tmx"]), True, STATS)
            R.grade_local(cid, "local_time_decay", got["time_decay"], R.local_time_decay(p, got["att_w"]), False, STATS)


def _ids(prefix):
    return [(c, m) for c, v in R.CASES.items() if c.startswith(prefix) for m in v["modes"]]


@pytest.mark.parametrize("case,mode", _ids("decode-"))
def test_decode_layer_by_layer(ctx, case, mode):
    """The basic op-list and fused layers; `small`: layer 6 (halved output) and layer 7 (discounted w_o / ffn value), each in isolation."""
    run_case(ctx, case, mode)


@pytest.mark.parametrize("case,mode", _ids("cold-"))
def test_first_tokens_of_a_sequence_layer_by_layer(ctx, case, mode):
    """No warm-up: WKV outputs of variance 1e-3 .. 3e-2, where the group norm's eps decides the value."""
    run_case(ctx, case, mode)


@pytest.mark.parametrize("case,mode", _ids("batch-"))
def test_batch_addressing_of_the_fused_layer(ctx, case, mode):
    """T = 1 with batch0 = 2; cursor-indexed with batch != token index; multi-token matvec; MFMA; 9 tokens over 11 slots."""
    run_case(ctx, case, mode)


@pytest.mark.parametrize("case,mode", _ids("ks-"))
def test_decode_batches_on_the_k_sliced_gemm(ctx, case, mode, monkeypatch):
    monkeypatch.setenv("WRK_GEMM_KS", R.CASES[case]["ks"])
    run_case(ctx, case, mode)


@pytest.mark.parametrize("case,mode", _ids("rank-"))
def test_lora_ranks(ctx, case, mode):
    """Ranks 8 / 8, 40 / 72, 96 / 104, 128 / 128: the masked 8-wide loads of v6_mix_kernel and v6_head_kernel (mode 1), the op list on the
    same odd ranks (mode 0); 136 / 64: the fused layer declines and the op list gives the oracle's values."""
    run_case(ctx, case, mode)


@pytest.mark.parametrize("case,mode", _ids("chunk-"))
def test_prefill_chunk_layer_by_layer(ctx, case, mode):
    run_case(ctx, case, mode)


def test_merged_chunk_gives_the_bits_of_the_op_list(ctx):
    """Above 64 stacked tokens the merged launches of mode 1 sum in the op list's order: every buffer both store, and the state, bit for bit."""
    case = "chunk-small-70"
    lens = R.CASES[case]["lens"]
    T = sum(lens)
    frames = []
    for mode in (0, 1):
        frames.append([{**{buf: rt.frame(buf, T).copy() for buf, _ in MERGED}, "state": rt.state_back(0)[li].copy()}
                       for rt, _, li, _, _, _ in layers_of(ctx, case, mode)])
    assert len(frames[0]) == len(frames[1]) > 0
    for li, (a, b) in enumerate(zip(*frames)):
        for buf in a:
            assert np.array_equal(a[buf].view(np.uint8), b[buf].view(np.uint8)), (li, buf)


def test_entry_points_check_their_arguments(ctx):
    data, model = R.fixture("decode-tiny-q5k")
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2, weights=wrk.WEIGHTS_INLINE)
    other = wrk.Runtime(ctx, wrk.GgufReader(R.fixture("decode-small-q4k")[0]), num_batch=1, weights=wrk.WEIGHTS_INLINE)
    D = model.info.num_emb
    x, cur = np.zeros((1, D), np.float16), np.array(stack_cursors([1]), np.uint32)
    call = lambda m, st, layer, c: wrk.hip.wrk_v6_infer_layer(ctx.h, m, st, layer, x.ctypes.data_as(wrk._P), wrk._ptr(c, wrk._u32p), 1, 1)   # noqa: E731
    try:
        assert call(rt.model6, rt.state, model.info.num_layer, cur) == wrk.E_ARG            # layer out of range
        assert call(rt.model6, other.state, 0, cur) == wrk.E_ARG                            # the state of another model
        assert call(rt.model6, rt.state, 0, np.array([2 | 1 << 24], np.uint32)) == wrk.E_ARG   # batch 2 of 2
        with pytest.raises(Exception):
            rt.frame("no_such_buffer", 1)
        rt.infer_layer(0, x, None, cur, mode=1)
        assert rt.frame("att_k", 1).dtype == np.float32 and rt.frame("att_sx", 1).shape == (5, 1, D) and rt.frame("x", 1).dtype == np.float16
    finally:
        rt.close(); other.close()


def test_zz_write_layer_parity_stats():
    """Not a check: prints what the cases above measured (worst over steps and layers, per buffer) for DESIGN.md, and with WRK_PARITY_OUT=<dir>
    writes the per-case figures to <dir>/v6_layer_parity.json (profiles/v6_layer_parity.json is such a file)."""
    out_dir = os.environ.get("WRK_PARITY_OUT")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "v6_layer_parity.json"), "w") as f:
            json.dump(STATS, f, indent=1, sort_keys=True)
    agg = aggregate({c: {b: s for b, s in bufs.items() if "min_frac_le1" in s} for c, bufs in STATS.items()})
    for name in ("state", "local_tm", "local_att_sx", "local_time_decay"):
        rows = [bufs[name] for bufs in STATS.values() if name in bufs]
        if rows:
            agg[name] = {k: (max if k.startswith("max") else min)(r[k] for r in rows) for k in rows[0] if k != "n"}
    print(json.dumps(agg, indent=1, sort_keys=True))
