"""RWKV-6 layer parity, proven on the CPU before the GPU sees the bars (tests/test_gpu_v6_layer_parity.py uses the same cases, tables,
measure and bars; the shared code is tests/v6_layer_ref.py).

  1. The seam is sound: replaying every layer with V6Runtime.infer_layer on the traced layer inputs and the pre-token state reproduces the
     whole-model trace and state bit for bit, and the restatement that carries the mutants is the oracle.
  2. The bars are met by the reference alone: the oracle with its matmuls accumulated in f64, and in a second f32 order (K reversed, in
     chunks of 32), teacher-forced per layer against the plain oracle, stays inside the GPU's bars on every buffer of every GPU case.
     Measured worst over both orders and all cases (the GPU's order is one more draw from the same distribution):

       | measure                                             | worst | bar    |
       |-----------------------------------------------------|-------|--------|
       | direct buffers (LN1(x); att_xx in decode), max      | 0 ulp | 1 ulp  |
       | downstream f16 buffers, max (att_sx, ffn_k, ffn_x)  | 5 ulp | 6 ulp (att_sx: 10, v6_layer_ref.BUFFER_MAX_ULP) |
       | downstream, smallest share within 1 ulp (ffn_x)     | 92.2 %| 80 %   |
       | f32 buffers k / v / r, max                          | 1.6 ulp | 6 ulp |
       | f32 buffer time_decay, max                          | 0.19 ulp | 6 ulp |
       | state, relative to max|state|                       | 9.8e-4 | 2^-9 (1.95e-3) |
       | stage-local tm / att_sx, share bit-identical; max   | 99.92 %; 1 / 4 ulp | 95 %; 1 / 10 ulp |
       | stage-local time_decay, max                         | 4e-4 ulp | 1/8 ulp |

  3. The bars have teeth: each of ten wrong layers breaks a bar on a named buffer or the state.  Seven do at the fixed layer bars.  Three
     cannot, and the measurement says why:
       * group-norm eps 1e-5 instead of 64e-5 moves no buffer by more than 1 ulp once a sequence is 8 tokens old (every head's WKV output
         has a variance above 2): it is caught in the cold-start cases (no warm-up), where it is 20 .. 3800 ulp off;
       * the f16 store of the time_mix_w2 product dropped before the add, and time_decay rounded to f16, are faults of at most 1 and 1/2 ulp
         per element, below the layer's own flips (5 ulp): they are caught by the stage-local checks (v6_layer_ref.py), which recompute
         tm / att_sx and time_decay from the buffers the layer under test stored itself.
"""
import numpy as np
import pytest

import v6_layer_ref as R
from layer_parity import STATE_REL
from oracle import rwkv6 as O6

REPLAY_CASES = ["decode-tiny-q5k", "decode-small-q4k", "batch-tiny-10110111111", "chunk-tiny-9-0-23"]


@pytest.mark.parametrize("case", REPLAY_CASES)
def test_layer_replay_reproduces_the_whole_model_trace_and_state(case):
    """tiny, small (7 layers: the halving after layer 6 stays inside that layer's run), decode over idle slots and a ragged chunk."""
    c = R.CASES[case]
    _, model = R.fixture(case)
    lens, L = c["lens"], model.info.num_layer
    single = O6.V6Runtime(model, len(lens), act_f16=True)
    for before, trace, after in R.replay(model, lens, 2):
        assert sorted(trace) == sorted(["emb_x"] + [f"{li}_{k}" for li in range(L) for k in R.KEYS])
        single.state[:] = before
        single.trace = {}
        for li in range(L):
            out = single.infer_layer(li, R.layer_input(trace, li), lens)
            assert np.array_equal(out, trace[f"{li}_x"])
        for key, want in single.trace.items():
            assert want.dtype == np.float32 and np.array_equal(want, trace[key]), key
        assert np.array_equal(single.state, after)


def test_restatement_is_the_oracle():
    """RefRuntime with NumPy's order and no mutant: the same bits as oracle/rwkv6.py, trace and state (7 layers, a ragged chunk)."""
    for case in ("decode-small-q4k", "chunk-tiny-9-0-23"):
        c = R.CASES[case]
        _, model = R.fixture(case)
        lens, L = c["lens"], model.info.num_layer
        ref = R.RefRuntime(model, len(lens))
        for before, trace, after in R.replay(model, lens, 1):
            for li in range(L):
                got, state = R.run_layer(ref, li, R.layer_input(trace, li), before, lens)
                for key in R.KEYS:
                    assert np.array_equal(got[f"{li}_{key}"], trace[f"{li}_{key}"]), (li, key)
                assert np.array_equal(state, after[li])


def teacher_forced(case, order=None, mutant=None):
    """Per (step, layer): the plain oracle's trace and states beside the layer of a RefRuntime run alone on the oracle's inputs."""
    c = R.CASES[case]
    _, model = R.fixture(case)
    lens = c["lens"]
    ref = R.RefRuntime(model, len(lens), order or "numpy", mutant)
    for before, trace, after in R.replay(model, lens, c["steps"], c["warm"]):
        for li in range(model.info.num_layer):
            got, state = R.run_layer(ref, li, R.layer_input(trace, li), before, lens)
            yield model.layers[li], li, lens, before[li], trace, after[li], got, state


STATS = {}


@pytest.mark.parametrize("order", ["f64", "rev32"])
@pytest.mark.parametrize("case", list(R.CASES))
def test_reference_in_another_summation_order_is_inside_the_gpu_bars(case, order):
    cid = f"{case}/{order}"
    for p, li, lens, before, trace, after, got, state in teacher_forced(case, order):
        R.grade(cid, li, trace, got, lens, STATS)
        R.grade_state(cid, li, state, after, lens, STATS)
        R.grade_local(cid, "local_tm", got[f"{li}_tm"], R.local_tm(p, got[f"{li}_tmx"]), True, STATS)
        R.grade_local(cid, "local_time_decay", got[f"{li}_time_decay"], R.local_time_decay(p, got[f"{li}_att_w"]), False, STATS)
        if all(n <= 1 for n in lens):
            prev = np.stack([before[b, 0] for b, n in enumerate(lens) if n])
            R.grade_local(cid, "local_att_sx", got[f"{li}_att_sx"], R.local_att_sx(p, got[f"{li}_tmx"], got[f"{li}_att_x_ln"], prev), True, STATS,
                         max_ulp=R.BUFFER_MAX_ULP["att_sx"])


# mutant -> (case, layer index or None for any, what must break: layer-bar buffers, "state", or stage-local checks "local_*")
MUTANT_EVIDENCE = {
    "u_on_state": ("decode-tiny-q5k", None, ["att_x", "x"]),
    "decay_before_read": ("decode-tiny-q5k", None, ["att_x", "x"]),
    "gn_eps_1e-5": ("cold-tiny-q5k", None, ["att_x", "x"]),
    "gate_sigmoid": ("decode-tiny-q5k", None, ["att_x", "x"]),
    "shift_state_from_x": ("decode-tiny-q5k", None, ["state"]),
    "w2_product_not_stored": ("decode-tiny-q5k", None, ["local_tm", "local_att_sx"]),
    "mix_swapped": ("decode-tiny-q5k", None, ["att_sx", "k", "ffn_k", "x"]),
    "no_halving": ("decode-small-q4k", 5, ["x"]),
    "w_o_not_discounted": ("decode-small-q4k", 6, ["att_o", "x"]),
    "time_decay_f16": ("decode-tiny-q5k", None, ["local_time_decay"]),
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_a_wrong_layer_breaks_a_bar(mutant):
    """Every named buffer is one the GPU tables read (att_x = the gated output, aux_x of the fused layer); local_time_decay exists on the op
    list only: the fused layer never stores time_decay."""
    case, layer, names = MUTANT_EVIDENCE[mutant]
    broken = {n: False for n in names}
    for p, li, lens, before, trace, after, got, state in teacher_forced(case, mutant=mutant):
        if layer is not None and li != layer:
            continue
        prev = np.stack([before[b, 0] for b, n in enumerate(lens) if n])
        for n in names:
            if n == "state":
                hit = any(R.state_error(state[b], after[b]) > STATE_REL for b, ln in enumerate(lens) if ln)
            elif n == "local_tm":
                hit = R.local_breaks_exact(got[f"{li}_tm"], R.local_tm(p, got[f"{li}_tmx"]))
            elif n == "local_att_sx":
                hit = R.local_breaks_exact(got[f"{li}_att_sx"], R.local_att_sx(p, got[f"{li}_tmx"], got[f"{li}_att_x_ln"], prev), R.BUFFER_MAX_ULP["att_sx"])
            elif n == "local_time_decay":
                hit = R.local_breaks_f32(got[f"{li}_time_decay"], R.local_time_decay(p, got[f"{li}_att_w"]))
            else:
                hit = R.breaks(got[f"{li}_{n}"], trace[f"{li}_{n}"], R.is_direct(n, lens), R.BUFFER_MAX_ULP.get(n))
            broken[n] = broken[n] or hit
    assert all(broken.values()), f"{mutant} passes the bars on {[n for n, b in broken.items() if not b]}"


def test_zz_print_reference_stats():
    """Not a check: the worst figures of the reference runs above, per buffer (the table in this file's docstring and DESIGN.md section 2)."""
    import json
    agg = {}
    for bufs in STATS.values():
        for b, s in bufs.items():
            a = agg.setdefault(b, {})
            for k, v in s.items():
                if k.startswith("max"):
                    a[k] = max(a.get(k, 0.0), v)
                elif k.startswith("min"):
                    a[k] = min(a.get(k, 1.0), v)
    print(json.dumps(agg, indent=1, sort_keys=True))
