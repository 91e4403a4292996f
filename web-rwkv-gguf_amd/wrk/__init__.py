"""ctypes binding of libwrk_hip.so (include/wrk_hip.h) and libwrk_runtime.so (include/wrk_runtime.h).

This is the harness-side mirror of the reference's public API for the hot path
(`Context`, `TensorOp::*`, `Matrix`, `GgufReader`, `Loader::info`, `ModelBuilder::build_v7`,
`v7::Bundle`, `RnnInput`, `runtime.infer`).  All compute happens in the HIP library; there is NO
CPU fallback: importing this module raises if the libraries are not built, and creating a `Context`
raises if no HIP device is present.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBDIR = os.environ.get("WRK_LIB_DIR") or os.path.join(os.path.dirname(_HERE), "lib")   # WRK_LIB_DIR: e.g. the `make TIMING=1` build
LIB_HIP = os.path.join(_LIBDIR, "libwrk_hip.so")
LIB_RT = os.path.join(_LIBDIR, "libwrk_runtime.so")


class WrkError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[{STATUS.get(code, code)}] {msg}")
        self.code = code


OK, E_ARG, E_OOM, E_HIP, E_UNSUPPORTED = 0, 1, 2, 3, 4
STATUS = {0: "WRK_OK", 1: "WRK_E_ARG", 2: "WRK_E_OOM", 3: "WRK_E_HIP", 4: "WRK_E_UNSUPPORTED"}
F16, F32, U8, U32 = 0, 1, 2, 3
ACT = {"none": 0, "squared_relu": 1, "tanh": 2, "stable_exp": 3, "opposite_exp": 4, "softplus": 5, "sigmoid": 6, "silu": 7}
MAT = {"F32": 0, "F16": 1, "Q8_0": 8, "Q4_K": 12, "Q5_K": 13, "Q6_K": 14, "INT8": 100, "NF4": 101}
MATRIX_EXACT, MATRIX_ROUND_F16 = 0, 1
WEIGHTS_INLINE, WEIGHTS_INLINE_F16, WEIGHTS_REFERENCE = 0, 1, 2
RNN_NONE, RNN_LAST, RNN_FULL = -1, 0, 1
QUANT_NONE, QUANT_INT8, QUANT_NF4 = 0, 1, 2

if not (os.path.exists(LIB_HIP) and os.path.exists(LIB_RT)):
    raise ImportError(
        f"{LIB_HIP} / {LIB_RT} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
        "(there is no CPU fallback for the HIP path)")

hip = C.CDLL(LIB_HIP, mode=C.RTLD_GLOBAL)
rt = C.CDLL(LIB_RT, mode=C.RTLD_GLOBAL)


class View(C.Structure):
    _fields_ = [("shape", C.c_uint32 * 4), ("stride", C.c_uint32 * 4), ("offset", C.c_uint32 * 4)]


class TensorDesc(C.Structure):
    _fields_ = [("buf", C.c_void_p), ("dtype", C.c_uint32), ("view", View)]


class ModelInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("version", "num_layer", "num_emb", "num_hidden", "num_vocab", "num_head",
                                           "lora_w", "lora_a", "lora_g", "lora_v")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BuildOptions(C.Structure):
    _fields_ = [("rescale", C.c_uint32), ("weights", C.c_uint32), ("quant", C.POINTER(C.c_uint8)), ("num_quant", C.c_uint32)]


_P = C.c_void_p
_u32p = C.POINTER(C.c_uint32)
_i32p = C.POINTER(C.c_int32)
_f32p = C.POINTER(C.c_float)


class GenerateOptions(C.Structure):
    """wrk_generate_options: the pick (sampler arrays all NULL: arg-max; occ NULL: no penalties), the stop sets (CSR) and the log-prob
    outputs (out_logprob NULL: off) of wrk_v*_generate_stop."""
    _fields_ = [("temperature", _f32p), ("top_p", _f32p), ("seed", _u32p), ("presence", _f32p), ("frequency", _f32p), ("decay", _f32p),
                ("occ", _P), ("bias", _P), ("bias_set", _u32p), ("guidance_scale", _f32p), ("guidance_first_tokens", _u32p),
                ("stop_tokens", _u32p), ("stop_offsets", _u32p), ("poll_steps", C.c_uint32),
                ("top_n_sigma", _f32p), ("epsilon_cutoff", _f32p), ("eta_cutoff", _f32p), ("xtc_probability", _f32p), ("xtc_threshold", _f32p),
                ("num_top", C.c_uint32), ("out_logprob", _f32p), ("out_top_ids", _u32p), ("out_top_logprobs", _f32p),
                ("window", _P), ("dry_multiplier", _f32p), ("dry_base", _f32p), ("dry_allowed_length", _u32p), ("no_repeat_ngram", _u32p),
                ("dry_breakers", _u32p), ("num_dry_breakers", C.c_uint32),
                ("grammar", _P), ("grammar_state", _u32p),
                ("stop_seq_tokens", _u32p), ("stop_seq_offsets", _u32p), ("stop_seq_owners", _u32p), ("out_stop_match", _u32p),
                ("stop_tail", _u32p),
                ("mirostat_tau", _f32p), ("mirostat_eta", _f32p), ("mirostat_mu", _f32p), ("typical_p", _f32p),
                ("top_k", _u32p), ("min_p", _f32p)]


class QueueOptions(C.Structure):
    """wrk_queue_options: the requests (CSR prompts, max_new, CSR stop sets), the pick arrays [R] as in GenerateOptions, the shared
    prefix state, the polled loop's block size and step cap and the log-prob outputs (out_logprob NULL: off) of wrk_v*_generate_queue."""
    _fields_ = [("num_requests", C.c_uint32), ("prompt_tokens", _u32p), ("prompt_offsets", _u32p), ("max_new", _u32p),
                ("stop_tokens", _u32p), ("stop_offsets", _u32p), ("temperature", _f32p), ("top_p", _f32p), ("seed", _u32p),
                ("presence", _f32p), ("frequency", _f32p), ("decay", _f32p), ("occ", _P), ("bias", _P), ("bias_set", _u32p), ("guidance_scale", _f32p),
                ("init_state", _P),
                ("poll_steps", C.c_uint32), ("max_steps", C.c_uint32), ("prompt_context_from", _u32p),
                ("history", _P),
                ("num_top", C.c_uint32), ("out_logprob", _f32p), ("out_top_ids", _u32p), ("out_top_logprobs", _f32p),
                ("window", _P), ("dry_multiplier", _f32p), ("dry_base", _f32p), ("dry_allowed_length", _u32p), ("no_repeat_ngram", _u32p),
                ("dry_breakers", _u32p), ("num_dry_breakers", C.c_uint32),
                ("grammar", _P), ("grammar_state", _u32p),
                ("stop_seq_tokens", _u32p), ("stop_seq_offsets", _u32p), ("stop_seq_owners", _u32p), ("out_stop_match", _u32p),
                ("mirostat_tau", _f32p), ("mirostat_eta", _f32p), ("mirostat_mu", _f32p), ("typical_p", _f32p),
                ("top_k", _u32p), ("min_p", _f32p)]


class QueueResult(C.Structure):
    """wrk_queue_result: host arrays [R] (out_tokens: [sum of max_new]) and the steps the call ran."""
    _fields_ = [("lengths", _u32p), ("reasons", _u32p), ("slots", _u32p), ("start_steps", _u32p), ("out_tokens", _u32p),
                ("steps_run", _u32p)]


class QueuePool(C.Structure):
    """wrk_queue_pool: the state pool of wrk_v*_generate_queue_pool and the start / save entries [R] of the requests."""
    _fields_ = [("states", _P), ("num_entries", C.c_uint32), ("start", _u32p), ("save", _u32p), ("saved", _u32p)]


class QueueGuidance(C.Structure):
    """wrk_queue_guidance: the scales [R], the CSR negative prompts and the partners' shared prefix state of wrk_v*_generate_queue_guided."""
    _fields_ = [("scale", _f32p), ("negative_tokens", _u32p), ("negative_offsets", _u32p), ("negative_init_state", _P)]


class QueueCuts(C.Structure):
    """wrk_queue_cuts: the cut sampler's arrays [R] of wrk_v*_generate_queue_cut and the pool or the guidance of the call (both NULL: the
    plain queue)."""
    _fields_ = [("top_n_sigma", _f32p), ("epsilon_cutoff", _f32p), ("eta_cutoff", _f32p), ("xtc_probability", _f32p), ("xtc_threshold", _f32p),
                ("pool", C.POINTER(QueuePool)), ("guide", C.POINTER(QueueGuidance))]


class BeamOptions(C.Structure):
    """wrk_beam_options: num_beams, length_penalty and the GenerateOptions a beam call shares (stop sets, bias, poll_steps)."""
    _fields_ = [("num_beams", C.c_uint32), ("length_penalty", C.c_float), ("gen", C.POINTER(GenerateOptions))]


class BeamResult(C.Structure):
    """wrk_beam_result: host arrays per group and rank [G * W] (tokens: [G][W][steps]), num_hyps [G], the steps the call ran and the
    optional per-step arrays [steps][B]."""
    _fields_ = [("tokens", _u32p), ("lengths", _u32p), ("scores", _f32p), ("finished", _u32p), ("slots", _u32p), ("num_hyps", _u32p),
                ("steps_run", _u32p), ("step_tokens", _u32p), ("step_parents", _u32p), ("step_scores", _f32p)]


class BeamContext(C.Structure):
    """wrk_beam_context: what every hypothesis of wrk_v*_generate_beam_context carries beside its state -- an occurrence table, a token
    window and a grammar (each may be NULL) with one value per group in every array, and the per-slot automaton states that come back."""
    _fields_ = [("occ", _P), ("presence", _f32p), ("frequency", _f32p), ("decay", _f32p),
                ("window", _P), ("dry_multiplier", _f32p), ("dry_base", _f32p), ("dry_allowed_length", _u32p), ("no_repeat_ngram", _u32p),
                ("dry_breakers", _u32p), ("num_dry_breakers", C.c_uint32),
                ("grammar", _P), ("grammar_state", _u32p), ("out_grammar_state", _u32p)]


MAX_BEAMS = 16              # WRK_MAX_BEAMS
MAX_BEAM_STOP_TOKENS = 128  # WRK_MAX_BEAM_STOP_TOKENS
BEAM_NO_TOKEN = 0xFFFFFFFF  # WRK_BEAM_NO_TOKEN
BEAM_NO_COPY = 0xFFFFFFFF   # WRK_BEAM_NO_COPY
BEAM_DEAD, BEAM_LIVE, BEAM_DONE = 0, 1, 2   # WRK_BEAM_DEAD / _LIVE / _DONE
MAX_STOP_TOKENS = 16        # WRK_MAX_STOP_TOKENS
MAX_TOP_LOGPROBS = 20       # WRK_MAX_TOP_LOGPROBS
MAX_STOP_SEQUENCES = 8      # WRK_MAX_STOP_SEQUENCES
MAX_STOP_SEQUENCE_LEN = 8   # WRK_MAX_STOP_SEQUENCE_LEN
STOP_TAIL_LEN = 7           # WRK_STOP_TAIL_LEN
STOP_TAIL_EMPTY = 0xFFFFFFFF    # WRK_STOP_TAIL_EMPTY
STOP_MATCH_NONE = 0xFFFFFFFF    # WRK_STOP_MATCH_NONE
STOP_MATCH_TOKEN = 0xFFFFFFFE   # WRK_STOP_MATCH_TOKEN
QUEUE_NO_ENTRY = 0xFFFFFFFF     # WRK_QUEUE_NO_ENTRY
GRAMMAR_REJECT = 0xFFFF         # WRK_GRAMMAR_REJECT
MAX_TOKEN_CLASSES = 8192        # WRK_MAX_TOKEN_CLASSES
BIAS_NONE = 0xFFFFFFFF          # WRK_BIAS_NONE
MAX_BIAS_SETS = 65536           # WRK_MAX_BIAS_SETS
MAX_TOKEN_WINDOW = 4096         # WRK_MAX_TOKEN_WINDOW
MAX_DRY_BREAKERS = 16           # WRK_MAX_DRY_BREAKERS
DRY_MAX_MATCH = 50              # WRK_DRY_MAX_MATCH
_u16p = C.POINTER(C.c_uint16)
_u8p = C.POINTER(C.c_uint8)
_u64p = C.POINTER(C.c_uint64)
GRAMMAR_COMPILE_PHASES = ("map", "hash", "fill", "verify", "trim", "create")     # wrk_grammar_compile_last_ms, in order
_TP = C.POINTER(TensorDesc)

# name -> (restype, argtypes); every symbol declared in include/*.h
HIP_SYMBOLS = {
    "wrk_abi_version": (C.c_int32, []),
    "wrk_ctx_create": (C.c_int32, [C.c_int32, C.POINTER(_P)]),
    "wrk_ctx_destroy": (C.c_int32, [_P]),
    "wrk_last_error": (C.c_char_p, [_P]),
    "wrk_ctx_sync": (C.c_int32, [_P]),
    "wrk_ctx_stream": (_P, [_P]),
    "wrk_buf_create": (C.c_int32, [_P, C.c_size_t, _P, C.POINTER(_P)]),
    "wrk_buf_retain": (C.c_int32, [_P]),
    "wrk_buf_release": (C.c_int32, [_P]),
    "wrk_buf_size": (C.c_size_t, [_P]),
    "wrk_buf_device_ptr": (_P, [_P]),
    "wrk_buf_write": (C.c_int32, [_P, _P, C.c_size_t, _P, C.c_size_t]),
    "wrk_buf_read": (C.c_int32, [_P, _P, C.c_size_t, _P, C.c_size_t]),
    "wrk_buf_copy": (C.c_int32, [_P, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t]),
    "wrk_capture_begin": (C.c_int32, [_P]),
    "wrk_capture_end": (C.c_int32, [_P, C.POINTER(_P)]),
    "wrk_program_launch": (C.c_int32, [_P, _P]),
    "wrk_program_destroy": (C.c_int32, [_P]),
    "wrk_matrix_create": (C.c_int32, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_size_t, C.c_uint32, C.POINTER(_P)]),
    "wrk_matrix_quantize": (C.c_int32, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.POINTER(C.c_float), C.POINTER(_P)]),
    "wrk_matrix_export": (C.c_int32, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "wrk_matrix_set_scale": (C.c_int32, [_P, C.c_float]),
    "wrk_matrix_release": (C.c_int32, [_P]),
    "wrk_matrix_stream_bytes": (C.c_size_t, [_P]),
    "wrk_op_matmul": (C.c_int32, [_P, _P, _TP, _TP, C.c_uint32, C.c_int32, C.c_int32]),
    "wrk_op_layer_norm": (C.c_int32, [_P, _P, _P, _TP, C.c_float]),
    "wrk_op_group_norm": (C.c_int32, [_P, _P, _P, _TP, C.c_float]),
    "wrk_op_l2_norm": (C.c_int32, [_P, _TP, C.c_float]),
    "wrk_op_token_shift": (C.c_int32, [_P, _P, _TP, _TP, _TP, _TP, C.c_int32]),
    "wrk_op_add": (C.c_int32, [_P, _TP, _TP, C.c_uint32, C.c_uint32, C.c_uint32]),
    "wrk_op_mul": (C.c_int32, [_P, _TP, _TP, C.c_uint32, C.c_uint32, C.c_uint32]),
    "wrk_op_lerp": (C.c_int32, [_P, _TP, _TP, _TP, C.c_int32]),
    "wrk_op_blit": (C.c_int32, [_P, _TP, _TP]),
    "wrk_op_affine": (C.c_int32, [_P, _TP, C.c_float, C.c_float]),
    "wrk_op_activate": (C.c_int32, [_P, _TP, C.c_uint32]),
    "wrk_op_control_k_v7": (C.c_int32, [_P, _P, _TP, _TP]),
    "wrk_op_time_mix_v7": (C.c_int32, [_P, _P, _TP, _TP, _TP, _TP, _TP]),
    "wrk_op_time_first_v7": (C.c_int32, [_P, _P, _TP, _TP, _TP]),
    "wrk_op_channel_mix_v7": (C.c_int32, [_P, _P, _TP, _TP, _TP]),
    "wrk_op_softmax": (C.c_int32, [_P, _TP]),
    "wrk_v7_model_create": (C.c_int32, [_P, _P, C.POINTER(_P)]),
    "wrk_v7_model_destroy": (C.c_int32, [_P]),
    "wrk_v7_model_token_bytes": (C.c_size_t, [_P, C.c_uint32]),
    "wrk_v7_state_create": (C.c_int32, [_P, _P, C.c_uint32, C.POINTER(_P)]),
    "wrk_v7_state_destroy": (C.c_int32, [_P]),
    "wrk_v7_state_load": (C.c_int32, [_P, _P, C.c_uint32, _f32p]),
    "wrk_v7_state_read": (C.c_int32, [_P, _P, C.c_uint32, _P]),
    "wrk_v7_state_write": (C.c_int32, [_P, _P, C.c_uint32, _P]),
    "wrk_v7_state_back": (C.c_int32, [_P, _P, C.c_uint32, _f32p]),
    "wrk_v7_infer": (C.c_int32, [_P, _P, _P, _u32p, C.POINTER(C.c_uint16), _u32p, C.c_uint32, _u32p, C.c_uint32, _f32p, _u32p, C.c_uint32]),
    "wrk_v7_model_set_frame_dtype": (C.c_int32, [_P, _P, C.c_uint32]),
    "wrk_v7_model_engine_status": (C.c_int32, [_P, _P, C.c_char_p, C.c_size_t]),
    "wrk_v7_infer_layer": (C.c_int32, [_P, _P, _P, C.c_uint32, _P, _P, _u32p, C.c_uint32, C.c_uint32]),
    "wrk_v7_frame_read": (C.c_int32, [_P, _P, C.c_char_p, C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "wrk_v7_generate_greedy": (C.c_int32, [_P, _P, _P, _u32p, C.c_uint32, C.c_uint32, _u32p, _f32p, _f32p, C.c_uint32]),
    "wrk_op_transpose": (C.c_int32, [_P, _TP, _TP]),
    "wrk_op_time_mix_v6": (C.c_int32, [_P, _P, _TP, _P, _TP, _TP, _TP, _TP, _TP]),
    "wrk_op_channel_mix": (C.c_int32, [_P, _P, _TP, _TP, _TP, _TP]),
    "wrk_v6_model_create": (C.c_int32, [_P, _P, C.POINTER(_P)]),
    "wrk_v6_model_destroy": (C.c_int32, [_P]),
    "wrk_v6_model_token_bytes": (C.c_size_t, [_P, C.c_uint32]),
    "wrk_v6_state_create": (C.c_int32, [_P, _P, C.c_uint32, C.POINTER(_P)]),
    "wrk_v6_infer_layer": (C.c_int32, [_P, _P, _P, C.c_uint32, _P, _u32p, C.c_uint32, C.c_uint32]),
    "wrk_v6_frame_read": (C.c_int32, [_P, _P, C.c_char_p, C.c_uint32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "wrk_v6_infer": (C.c_int32, [_P, _P, _P, _u32p, C.POINTER(C.c_uint16), _u32p, C.c_uint32, _u32p, C.c_uint32, _f32p, _u32p, C.c_uint32]),
    "wrk_v6_generate_greedy": (C.c_int32, [_P, _P, _P, _u32p, C.c_uint32, C.c_uint32, _u32p, _f32p, _f32p, C.c_uint32]),
    "wrk_sample_logits": (C.c_int32, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _f32p, _f32p, _u32p, C.c_uint32, _u32p]),
    "wrk_sample_logits_cut": (C.c_int32, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _f32p, _f32p, _u32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p,
                                          _u32p, C.c_uint32, _u32p]),
    "wrk_sample_logits_filtered": (C.c_int32, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _f32p, _f32p, _u32p, _f32p, _u32p, C.c_uint32,
                                               _u32p]),
    "wrk_sample_logits_mirostat": (C.c_int32, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _f32p, _f32p, _f32p, _f32p, _f32p, _u32p, C.c_uint32,
                                               _u32p]),
    "wrk_sample_logits_typical": (C.c_int32, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _f32p, _f32p, _f32p, _u32p, C.c_uint32, _u32p]),
    "wrk_v7_generate_sample": (C.c_int32, [_P, _P, _P, _u32p, C.c_uint32, C.c_uint32, _f32p, _f32p, _u32p, _u32p, _f32p, _f32p,
                                           C.c_uint32]),
    "wrk_v6_generate_sample": (C.c_int32, [_P, _P, _P, _u32p, C.c_uint32, C.c_uint32, _f32p, _f32p, _u32p, _u32p, _f32p, _f32p,
                                           C.c_uint32]),
    "wrk_score_logits": (C.c_int32, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _f32p, _u32p]),
    "wrk_top_logprobs": (C.c_int32, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, C.c_uint32, _f32p, _u32p, _f32p]),
    "wrk_v7_score": (C.c_int32, [_P, _P, _P, _u32p, C.POINTER(C.c_uint16), _u32p, C.c_uint32, _u32p, C.c_uint32, _u32p, _f32p, _u32p,
                                 C.c_uint32]),
    "wrk_v6_score": (C.c_int32, [_P, _P, _P, _u32p, C.POINTER(C.c_uint16), _u32p, C.c_uint32, _u32p, C.c_uint32, _u32p, _f32p, _u32p,
                                 C.c_uint32]),
    "wrk_occurrence_create": (C.c_int32, [_P, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "wrk_occurrence_destroy": (C.c_int32, [_P]),
    "wrk_occurrence_set_weights": (C.c_int32, [_P, _P, _f32p]),
    "wrk_occurrence_ban": (C.c_int32, [_P, _P, C.c_uint32, _u32p, C.c_uint32, C.c_int32]),
    "wrk_occurrence_add": (C.c_int32, [_P, _P, C.c_uint32, _u32p, C.c_uint32, C.c_float]),
    "wrk_occurrence_back": (C.c_int32, [_P, _P, C.c_uint32, _f32p, _u32p]),
    "wrk_occurrence_load": (C.c_int32, [_P, _P, C.c_uint32, _f32p, _u32p]),
    "wrk_penalize_logits": (C.c_int32, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint32, _f32p, _f32p]),
    "wrk_v7_generate_penalized": (C.c_int32, [_P, _P, _P, _u32p, C.c_uint32, C.c_uint32, _f32p, _f32p, _u32p, _f32p, _f32p, _f32p, _P,
                                              _u32p, _f32p, _f32p, C.c_uint32]),
    "wrk_v6_generate_penalized": (C.c_int32, [_P, _P, _P, _u32p, C.c_uint32, C.c_uint32, _f32p, _f32p, _u32p, _f32p, _f32p, _f32p, _P,
                                              _u32p, _f32p, _f32p, C.c_uint32]),
    "wrk_grammar_create": (C.c_int32, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _u16p, _u16p, C.POINTER(_P)]),
    "wrk_grammar_destroy": (C.c_int32, [_P]),
    "wrk_constrain_logits": (C.c_int32, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _u32p]),
    "wrk_grammar_advance": (C.c_int32, [_P, _P, _u32p, _u32p, C.c_uint32]),
    "wrk_regex_compile": (C.c_int32, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_uint32, C.POINTER(_P), C.c_char_p, C.c_size_t]),
    "wrk_byte_dfa_from_arrays": (C.c_int32, [C.c_uint32, _u16p, _u8p, _u32p, C.c_uint32, C.POINTER(_P)]),
    "wrk_byte_dfa_export": (C.c_int32, [_P, _u32p, _u32p, _u16p, _u8p, _u32p]),
    "wrk_byte_dfa_destroy": (None, [_P]),
    "wrk_grammar_compile": (C.c_int32, [_P, _P, C.c_uint32, _u8p, _u64p, C.c_uint32, C.POINTER(_P), _u32p, _u32p]),
    "wrk_grammar_compile_last_ms": (C.c_int32, [_f32p]),
    "wrk_grammar_export": (C.c_int32, [_P, _u32p, _u32p, _u16p, _u16p]),
    "wrk_logit_bias_create": (C.c_int32, [_P, C.c_uint32, C.c_uint32, _u32p, _u32p, _f32p, C.POINTER(_P)]),
    "wrk_logit_bias_destroy": (C.c_int32, [_P]),
    "wrk_bias_logits": (C.c_int32, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _u32p]),
    "wrk_guide_logits": (C.c_int32, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _f32p, _P, C.c_uint32]),
    "wrk_token_window_create": (C.c_int32, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "wrk_token_window_destroy": (C.c_int32, [_P]),
    "wrk_token_window_add": (C.c_int32, [_P, _P, C.c_uint32, _u32p, C.c_uint32]),
    "wrk_token_window_back": (C.c_int32, [_P, _P, C.c_uint32, _u32p, _u32p]),
    "wrk_token_window_load": (C.c_int32, [_P, _P, C.c_uint32, _u32p, C.c_uint32]),
    "wrk_dry_logits": (C.c_int32, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint32, _f32p, _f32p, _u32p, _u32p, _u32p, C.c_uint32]),
    "wrk_stop_sequences_advance": (C.c_int32, [_P, C.c_uint32, C.c_uint32, _u32p, _u32p, _u32p, _u32p, _u32p, _u32p, _u32p, _u32p]),
    "wrk_v7_generate_stop": (C.c_int32, [_P, _P, _P, _u32p, C.c_uint32, C.c_uint32, C.POINTER(GenerateOptions), _u32p, _u32p, _f32p, _u32p,
                                         _f32p, C.c_uint32]),
    "wrk_v6_generate_stop": (C.c_int32, [_P, _P, _P, _u32p, C.c_uint32, C.c_uint32, C.POINTER(GenerateOptions), _u32p, _u32p, _f32p, _u32p,
                                         _f32p, C.c_uint32]),
    "wrk_v7_generate_queue": (C.c_int32, [_P, _P, _P, C.c_uint32, C.POINTER(QueueOptions), C.POINTER(QueueResult), _f32p, C.c_uint32]),
    "wrk_v6_generate_queue": (C.c_int32, [_P, _P, _P, C.c_uint32, C.POINTER(QueueOptions), C.POINTER(QueueResult), _f32p, C.c_uint32]),
    "wrk_history_pool_create": (C.c_int32, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "wrk_history_pool_destroy": (C.c_int32, [_P]),
    "wrk_history_pool_load": (C.c_int32, [_P, _P, C.c_uint32, _f32p, _u32p, _u32p, C.c_uint32]),
    "wrk_history_pool_back": (C.c_int32, [_P, _P, C.c_uint32, _f32p, _u32p, _u32p, _u32p]),
    "wrk_history_pool_put": (C.c_int32, [_P, _P, C.c_uint32, _P, C.c_uint32, _P]),
    "wrk_history_pool_get": (C.c_int32, [_P, _P, C.c_uint32, _P, C.c_uint32, _P]),
    "wrk_v7_generate_queue_pool": (C.c_int32, [_P, _P, _P, C.c_uint32, C.POINTER(QueueOptions), C.POINTER(QueueResult), _f32p, C.c_uint32,
                                               C.POINTER(QueuePool)]),
    "wrk_v6_generate_queue_pool": (C.c_int32, [_P, _P, _P, C.c_uint32, C.POINTER(QueueOptions), C.POINTER(QueueResult), _f32p, C.c_uint32,
                                               C.POINTER(QueuePool)]),
    "wrk_v7_generate_queue_guided": (C.c_int32, [_P, _P, _P, C.c_uint32, C.POINTER(QueueOptions), C.POINTER(QueueResult), _f32p, C.c_uint32,
                                                 C.POINTER(QueueGuidance)]),
    "wrk_v6_generate_queue_guided": (C.c_int32, [_P, _P, _P, C.c_uint32, C.POINTER(QueueOptions), C.POINTER(QueueResult), _f32p, C.c_uint32,
                                                 C.POINTER(QueueGuidance)]),
    "wrk_v7_generate_queue_cut": (C.c_int32, [_P, _P, _P, C.c_uint32, C.POINTER(QueueOptions), C.POINTER(QueueResult), _f32p, C.c_uint32,
                                              C.POINTER(QueueCuts)]),
    "wrk_v6_generate_queue_cut": (C.c_int32, [_P, _P, _P, C.c_uint32, C.POINTER(QueueOptions), C.POINTER(QueueResult), _f32p, C.c_uint32,
                                              C.POINTER(QueueCuts)]),
    "wrk_v7_generate_beam": (C.c_int32, [_P, _P, _P, _u32p, C.c_uint32, C.c_uint32, C.POINTER(BeamOptions), C.POINTER(BeamResult), _f32p,
                                         C.c_uint32]),
    "wrk_v6_generate_beam": (C.c_int32, [_P, _P, _P, _u32p, C.c_uint32, C.c_uint32, C.POINTER(BeamOptions), C.POINTER(BeamResult), _f32p,
                                         C.c_uint32]),
    "wrk_beam_step": (C.c_int32, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, _u32p, _u32p, _f32p, _f32p, _u32p, _u32p,
                                  _u32p, _u32p, _u32p]),
    "wrk_v7_state_permute": (C.c_int32, [_P, _P, _u32p, C.c_uint32]),
    "wrk_v7_generate_beam_context": (C.c_int32, [_P, _P, _P, _u32p, C.c_uint32, C.c_uint32, C.POINTER(BeamOptions), C.POINTER(BeamResult), _f32p,
                                                 C.c_uint32, C.POINTER(BeamContext)]),
    "wrk_v6_generate_beam_context": (C.c_int32, [_P, _P, _P, _u32p, C.c_uint32, C.c_uint32, C.POINTER(BeamOptions), C.POINTER(BeamResult), _f32p,
                                                 C.c_uint32, C.POINTER(BeamContext)]),
    "wrk_occurrence_permute": (C.c_int32, [_P, _P, _u32p, C.c_uint32]),
    "wrk_token_window_permute": (C.c_int32, [_P, _P, _u32p, C.c_uint32]),
}
RT_SYMBOLS = {
    "wrk_host_last_error": (C.c_char_p, []),
    "wrk_gguf_open": (C.c_int32, [C.c_char_p, C.POINTER(_P)]),
    "wrk_gguf_from_memory": (C.c_int32, [_P, C.c_size_t, C.POINTER(_P)]),
    "wrk_gguf_close": (C.c_int32, [_P]),
    "wrk_gguf_version": (C.c_uint32, [_P]),
    "wrk_gguf_tensor_data_offset": (C.c_uint64, [_P]),
    "wrk_gguf_contains": (C.c_int32, [_P, C.c_char_p]),
    "wrk_gguf_shape": (C.c_int32, [_P, C.c_char_p, C.c_uint32 * 4, _u32p]),
    "wrk_gguf_tensor_f16": (C.c_int32, [_P, C.c_char_p, C.POINTER(C.c_uint16), C.c_size_t, C.POINTER(C.c_size_t)]),
    "wrk_gguf_raw": (C.c_int32, [_P, C.c_char_p, _u32p, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "wrk_gguf_meta_u64": (C.c_int32, [_P, C.c_char_p, C.POINTER(C.c_uint64)]),
    "wrk_gguf_read_state": (C.c_int32, [_P, _f32p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "wrk_gguf_info": (C.c_int32, [_P, C.POINTER(ModelInfo)]),
    "wrk_quantile_student": (C.c_int32, [C.c_double, _f32p]),
    "wrk_rnn_input_create": (C.c_int32, [C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "wrk_rnn_input_destroy": (C.c_int32, [_P]),
    "wrk_rnn_input_token_chunk_size": (C.c_uint32, [_P]),
    "wrk_rnn_input_append": (C.c_int32, [_P, C.c_uint32, _u32p, C.c_uint32]),
    "wrk_rnn_input_set_option": (C.c_int32, [_P, C.c_uint32, C.c_int32]),
    "wrk_rnn_input_remaining": (C.c_uint32, [_P, C.c_uint32]),
    "wrk_rnn_input_step": (C.c_int32, [_P]),
    "wrk_rnn_iter_create": (C.c_int32, [_P, C.POINTER(_P)]),
    "wrk_rnn_iter_destroy": (C.c_int32, [_P]),
    "wrk_rnn_iter_next": (C.c_int32, [_P, _u32p, _i32p]),
    "wrk_rnn_redirect": (C.c_int32, [_u32p, _i32p, C.c_uint32, _u32p, _u32p, _u32p, _u32p]),
    "wrk_runtime_create": (C.c_int32, [_P, _P, C.POINTER(BuildOptions), C.c_uint32, C.POINTER(_P)]),
    "wrk_runtime_destroy": (C.c_int32, [_P]),
    "wrk_runtime_info": (C.c_int32, [_P, C.POINTER(ModelInfo)]),
    "wrk_runtime_model": (_P, [_P]),
    "wrk_runtime_state": (_P, [_P]),
    "wrk_runtime_model_v6": (_P, [_P]),
    "wrk_runtime_infer": (C.c_int32, [_P, _P, _f32p, C.c_size_t, _u32p, C.c_uint32]),
    "wrk_rnn_score_plan": (C.c_int32, [_P, _u32p, _u32p, _u32p, _u32p, _u32p]),
    "wrk_runtime_score": (C.c_int32, [_P, _P, _f32p, _u32p, C.c_size_t, _u32p, C.c_uint32]),
}
for _lib, _tab in ((hip, HIP_SYMBOLS), (rt, RT_SYMBOLS)):
    for _name, (_res, _args) in _tab.items():
        _f = getattr(_lib, _name)      # AttributeError here == header/library mismatch
        _f.restype = _res
        _f.argtypes = _args


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32))


def _ptr(a: np.ndarray, ty):
    return a.ctypes.data_as(ty)


def _per_row(v, n: int, dtype) -> np.ndarray:
    """A scalar broadcast to n entries, or a length-n array."""
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (n,)))
    return a


def _filters(top_k, min_p, n: int, keep: list):
    """(top_k pointer, min_p pointer) of the filtered sampler's per-row arrays, None for a filter that is off; the arrays go into
    `keep`, which must outlive the call."""
    tk = mp = None
    if top_k is not None:
        keep.append(_per_row(top_k, n, np.uint32))
        tk = _ptr(keep[-1], _u32p)
    if min_p is not None:
        keep.append(_per_row(min_p, n, np.float32))
        mp = _ptr(keep[-1], _f32p)
    return tk, mp


def _cuts(cuts, n: int, keep: list):
    """The cut sampler's five per-row pointers (top_n_sigma, epsilon_cutoff, eta_cutoff, xtc_probability, xtc_threshold; None: off) of
    `cuts` = (top_n_sigma, epsilon_cutoff, eta_cutoff, xtc), each a scalar or one value per row, xtc = (probability, threshold); None when
    all four are None.  The arrays go into `keep`, which must outlive the call."""
    if cuts is None or all(v is None for v in cuts):
        return None
    ns, eps, eta, xtc = cuts
    def put(v):
        if v is None:
            return None
        keep.append(_per_row(v, n, np.float32))
        return _ptr(keep[-1], _f32p)
    if xtc is not None and len(xtc) != 2:
        raise ValueError("xtc = (probability, threshold)")
    return put(ns), put(eps), put(eta), put(None if xtc is None else xtc[0]), put(None if xtc is None else xtc[1])


def _mirostat_rows(mirostat, mirostat_mu, n: int):
    """(tau [n], eta [n], mu [n]) f32 of `mirostat` = (tau, eta), scalars or one value per row; mu: `mirostat_mu`, or 2 tau (a fresh
    sequence).  mu is a writable copy: the call returns the new values in it."""
    tau, eta = mirostat
    tau, eta = _per_row(tau, n, np.float32), _per_row(eta, n, np.float32)
    mu = (2.0 * tau).astype(np.float32) if mirostat_mu is None else np.array(_per_row(mirostat_mu, n, np.float32), np.float32)
    return tau, eta, mu


def _fill_pick(opt, n: int, keep: list, temperature, top_p, seed, occurrence, presence, frequency, decay, top_k, min_p,
               mirostat=None, mirostat_mu=None, typical_p=None, cuts=None):
    """The sampler / penalty / filter fields of a GenerateOptions or QueueOptions for n rows (scalars broadcast; seed None: seed[i] = i).
    All of temperature, top_p, seed, occurrence, top_k, min_p, mirostat, typical_p and cuts None: nothing is set, the arg-max.  The arrays
    go into `keep`, which must outlive the call.  mirostat = (tau, eta): returns the in/out mu array [n] (mirostat_mu, or 2 tau), else
    None.  cuts: `_cuts`' argument; a GenerateOptions takes the five arrays, a QueueOptions has no such fields (the queue passes them in
    a QueueCuts) and only becomes a sampled pick."""
    def put(v, dtype, ty):
        keep.append(_per_row(v, n, dtype))
        return _ptr(keep[-1], ty)
    if mirostat is None and mirostat_mu is not None:
        raise ValueError("mirostat_mu without mirostat")
    cut_ptrs = _cuts(cuts, n, keep)
    if all(v is None for v in (temperature, top_p, seed, occurrence, top_k, min_p, mirostat, typical_p, cut_ptrs)):
        return None
    if cut_ptrs is not None and isinstance(opt, GenerateOptions):
        opt.top_n_sigma, opt.epsilon_cutoff, opt.eta_cutoff, opt.xtc_probability, opt.xtc_threshold = cut_ptrs
    opt.temperature = put(1.0 if temperature is None else temperature, np.float32, _f32p)
    opt.top_p = put(0.5 if top_p is None else top_p, np.float32, _f32p)
    opt.seed = put(np.arange(n, dtype=np.uint32) if seed is None else seed, np.uint32, _u32p)
    if occurrence is not None:
        opt.presence, opt.frequency, opt.decay = (put(v, np.float32, _f32p) for v in (presence, frequency, decay))
        opt.occ = occurrence.h
    tk, mp = _filters(top_k, min_p, n, keep)
    if tk is not None:
        opt.top_k = tk
    if mp is not None:
        opt.min_p = mp
    if typical_p is not None:
        opt.typical_p = put(typical_p, np.float32, _f32p)
    if mirostat is None:
        return None
    tau, eta, mu = _mirostat_rows(mirostat, mirostat_mu, n)
    keep.extend([tau, eta, mu])
    opt.mirostat_tau, opt.mirostat_eta, opt.mirostat_mu = _ptr(tau, _f32p), _ptr(eta, _f32p), _ptr(mu, _f32p)
    return mu


def _logprob_arrays(logprobs, rows: int):
    """(logprob [rows], top_ids [rows, n], top_logprobs [rows, n]) host arrays for `logprobs` = n alternatives per row; the top arrays
    keep one element when empty so that their pointers are valid."""
    n = int(logprobs)
    if not 0 <= n <= MAX_TOP_LOGPROBS:
        raise ValueError(f"logprobs = {logprobs}: None, or 0..{MAX_TOP_LOGPROBS}")
    return np.zeros(max(rows, 1), np.float32), np.zeros(max(rows * n, 1), np.uint32), np.zeros(max(rows * n, 1), np.float32)


def _stop_csr(stop, n: int, owners: str):
    """Stop sets as (ids, offsets [n + 1]): one list of ids for all n owners, or one list per owner."""
    sets = [] if stop is None else list(stop)
    if not (sets and all(isinstance(x, (list, tuple, np.ndarray)) for x in sets)):
        sets = [sets] * n
    if len(sets) != n:
        raise ValueError(f"{len(sets)} stop sets for {n} {owners}")
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(x) for x in sets])
    ids = _u32(np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in sets]) if n else [])
    return (ids if ids.size else np.zeros(1, np.uint32)), off


def _stop_seq_csr(stop_sequences, n: int, owners: str):
    """Stop sequences as the ABI's CSR of a CSR, (ids, offsets [S + 1], owners [n + 1]): one list of id lists for all n owners, or one
    such list per owner.  Told apart by depth: a list whose entries hold ids is one owner's list.  ValueError on a wrong owner count, an
    empty sequence, one longer than MAX_STOP_SEQUENCE_LEN, or more than MAX_STOP_SEQUENCES for an owner; the ids are checked against
    the vocabulary by the call."""
    def is_seq(x):
        return isinstance(x, (list, tuple, np.ndarray))
    top = list(stop_sequences)
    if any(not is_seq(x) for x in top):
        raise ValueError("stop_sequences: a list of id lists, or one such list per " + owners[:-1])
    per_owner = any(is_seq(y) for x in top for y in x) or (len(top) == n and all(len(x) == 0 for x in top) and n > 0)
    lists = [list(x) for x in top] if per_owner else [top] * n
    if len(lists) != n:
        raise ValueError(f"{len(lists)} lists of stop sequences for {n} {owners}")
    seqs, own = [], np.zeros(n + 1, np.uint32)
    for b, lst in enumerate(lists):
        if len(lst) > MAX_STOP_SEQUENCES:
            raise ValueError(f"{len(lst)} stop sequences, at most {MAX_STOP_SEQUENCES}")
        for q in lst:
            q = np.asarray(q, np.int64).reshape(-1)
            if not 1 <= q.size <= MAX_STOP_SEQUENCE_LEN:
                raise ValueError(f"a stop sequence of {q.size} ids: 1 to {MAX_STOP_SEQUENCE_LEN}")
            if q.min() < 0 or q.max() > 0xFFFFFFFF:
                raise ValueError("stop sequence ids must fit 32 bits")
            seqs.append(q)
        own[b + 1] = len(seqs)
    off = np.zeros(len(seqs) + 1, np.uint32)
    off[1:] = np.cumsum([q.size for q in seqs])
    ids = _u32(np.concatenate(seqs)) if seqs else np.zeros(1, np.uint32)
    return ids, off, own


def _stop_tails(stop_tail, n: int) -> np.ndarray:
    """A writable [n, STOP_TAIL_LEN] u32 copy of `stop_tail` (None: all EMPTY); a shorter row is right aligned."""
    out = np.full((n, STOP_TAIL_LEN), STOP_TAIL_EMPTY, np.uint32)
    if stop_tail is None:
        return out
    rows = list(stop_tail)
    if len(rows) != n:
        raise ValueError(f"{len(rows)} tails for {n} sequences")
    for b, row in enumerate(rows):
        row = np.asarray(row, np.int64).reshape(-1)
        if row.size > STOP_TAIL_LEN:
            raise ValueError(f"a tail of {row.size} entries, at most {STOP_TAIL_LEN}")
        if row.size:
            out[b, STOP_TAIL_LEN - row.size:] = row.astype(np.uint32)
    return out


def _fill_stop_sequences(opt, n: int, keep: list, stop_sequences, owners: str):
    """The stop-sequence fields of a GenerateOptions or QueueOptions for n owners; returns the out_stop_match array [n], or None
    without stop sequences.  The arrays go into `keep`."""
    if stop_sequences is None:
        return None
    ids, off, own = _stop_seq_csr(stop_sequences, n, owners)
    match = np.full(max(n, 1), STOP_MATCH_NONE, np.uint32)
    keep.extend([ids, off, own, match])
    opt.stop_seq_tokens, opt.stop_seq_offsets, opt.stop_seq_owners = _ptr(ids, _u32p), _ptr(off, _u32p), _ptr(own, _u32p)
    opt.out_stop_match = _ptr(match, _u32p)
    return match


def _dry_rows(n: int, keep: list, dry, no_repeat_ngram, dry_breakers):
    """(multiplier, base, allowed_length, no_repeat_ngram, breakers) pointers and the breaker count for n rows: dry = (multiplier, base,
    allowed_length), scalars or one value per row (None: off); no_repeat_ngram a scalar or one value per row (None: off); dry_breakers a
    list of ids (None: none).  A part that is None stays a NULL pointer.  The arrays go into `keep`."""
    mult = base = allowed = nr = brk = None
    nb = 0
    if dry is not None:
        m, b, a = dry
        keep.extend((_per_row(m, n, np.float32), _per_row(b, n, np.float32), _per_row(a, n, np.uint32)))
        mult, base, allowed = _ptr(keep[-3], _f32p), _ptr(keep[-2], _f32p), _ptr(keep[-1], _u32p)
    if no_repeat_ngram is not None:
        keep.append(_per_row(no_repeat_ngram, n, np.uint32))
        nr = _ptr(keep[-1], _u32p)
    if dry_breakers is not None and len(dry_breakers):
        keep.append(_u32(dry_breakers).reshape(-1))
        brk, nb = _ptr(keep[-1], _u32p), int(keep[-1].size)
    return mult, base, allowed, nr, brk, nb


def _fill_dry(opt, n: int, keep: list, window, dry, no_repeat_ngram, dry_breakers):
    """The DRY fields of a GenerateOptions or QueueOptions for n rows; nothing is set without a window."""
    if window is None:
        if dry is not None or no_repeat_ngram is not None or dry_breakers is not None:
            raise ValueError("dry / no_repeat_ngram / dry_breakers without window")
        return
    opt.window = window.h
    (opt.dry_multiplier, opt.dry_base, opt.dry_allowed_length, opt.no_repeat_ngram, opt.dry_breakers,
     opt.num_dry_breakers) = _dry_rows(n, keep, dry, no_repeat_ngram, dry_breakers)


def _fill_grammar(opt, n: int, keep: list, grammar, grammar_state):
    """The grammar fields of a GenerateOptions or QueueOptions for n rows; returns the in/out state array [n] (grammar_state, a scalar
    or one value per row; None: every row starts in state 0), or None without a grammar.  The array goes into `keep`."""
    if grammar is None:
        if grammar_state is not None:
            raise ValueError("grammar_state without grammar")
        return None
    st = np.array(_per_row(0 if grammar_state is None else grammar_state, n, np.uint32), np.uint32)
    keep.append(st)
    opt.grammar, opt.grammar_state = grammar.h, _ptr(st, _u32p)
    return st


def _fill_bias(opt, n: int, keep: list, logit_bias, bias_set):
    """The bias fields of a GenerateOptions or QueueOptions for n rows: bias_set a scalar or one set index per row (BIAS_NONE: the row
    is left alone); None: set 0 for every row.  The array goes into `keep`."""
    if logit_bias is None:
        if bias_set is not None:
            raise ValueError("bias_set without logit_bias")
        return
    opt.bias = logit_bias.h
    if bias_set is not None:
        keep.append(_per_row(bias_set, n, np.uint32))
        opt.bias_set = _ptr(keep[-1], _u32p)


def _fill_guidance(opt, n: int, keep: list, guidance_scale, negative_first_tokens=None):
    """The guidance fields of a GenerateOptions or QueueOptions for n sequences: guidance_scale a scalar or one value per sequence."""
    if guidance_scale is None:
        if negative_first_tokens is not None:
            raise ValueError("negative_first_tokens without guidance_scale")
        return
    keep.append(_per_row(guidance_scale, n, np.float32))
    opt.guidance_scale = _ptr(keep[-1], _f32p)
    if negative_first_tokens is not None:
        keep.append(_per_row(negative_first_tokens, n, np.uint32))
        opt.guidance_first_tokens = _ptr(keep[-1], _u32p)


def _bias_csr(sets):
    """(offsets u32 [S + 1], ids u32 [E], values f32 [E]) of a list of bias sets, each a {token: value} dict or an (ids, values) pair;
    what `LogitBias` hands to the library, which validates it."""
    off, ids, vals = [0], [], []
    for st in sets:
        i, v = (list(st.keys()), list(st.values())) if isinstance(st, dict) else st
        i, v = np.asarray(i, np.int64).reshape(-1), np.asarray(v, np.float32).reshape(-1)
        if i.size != v.size:
            raise ValueError(f"a bias set of {i.size} ids and {v.size} values")
        if i.size and (i.min() < 0 or i.max() > 0xFFFFFFFF):
            raise ValueError("a bias id outside [0, 2^32)")
        ids.append(i.astype(np.uint32))
        vals.append(v)
        off.append(off[-1] + i.size)
    cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts) if parts else [], dt)
    return np.asarray(off, np.uint32), cat(ids, np.uint32), cat(vals, np.float32)


def _grammar_tables(num_vocab: int, token_class, transitions):
    """(token_class u16 [V], transitions u16 [S, C]) checked for range and shape (ValueError); what `Grammar` uploads."""
    tc = np.asarray(token_class, np.int64).reshape(-1)
    tr = np.asarray(transitions, np.int64)
    if tc.size != num_vocab:
        raise ValueError(f"token_class has {tc.size} entries for {num_vocab} tokens")
    if tr.ndim != 2 or tr.size == 0:
        raise ValueError("transitions: a non-empty [num_states, num_classes] table")
    if tc.min(initial=0) < 0 or tc.max(initial=0) > 0xFFFF or tr.min() < 0 or tr.max() > 0xFFFF:
        raise ValueError("token_class / transitions entries must fit 16 bits")
    return np.ascontiguousarray(tc.astype(np.uint16)), np.ascontiguousarray(tr.astype(np.uint16))


def grammar_walk(token_class, transitions, state: int, tokens) -> int:
    """The state after `tokens` from `state` on the host; ValueError at the first rejected token."""
    s = int(state)
    for i, t in enumerate(np.asarray(tokens, np.int64).reshape(-1)):
        nx = int(transitions[s][int(token_class[int(t)])])
        if nx == GRAMMAR_REJECT:
            raise ValueError(f"token {i} (id {int(t)}) is not allowed in state {s}")
        s = nx
    return s


def grammar_from_dense(table):
    """table [S][V] of next states (-1: the token is not allowed in the state) -> (token_class u16 [V], transitions u16 [S][C]):
    identical columns are merged into one class, classes numbered by first occurrence.  Bookkeeping only: no device is touched."""
    t = np.asarray(table, np.int64)
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("table: [num_states >= 1][num_vocab >= 1]")
    S, V = t.shape
    if S > 0xFFFF or t.min() < -1 or t.max() >= S:
        raise ValueError(f"table: at most 65535 states, entries -1 or < {S}")
    _, first, inv = np.unique(t, axis=1, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(first, kind="stable")            # unique column k -> its rank by first occurrence
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    if order.size > MAX_TOKEN_CLASSES:
        raise ValueError(f"{order.size} distinct columns, at most {MAX_TOKEN_CLASSES} classes")
    cols = t[:, first[order]]
    return rank[inv].astype(np.uint16), np.where(cols < 0, GRAMMAR_REJECT, cols).astype(np.uint16)


def grammar_from_choices(num_vocab: int, choices, end_token: int):
    """The trie automaton that accepts exactly one of the token sequences `choices` and then `end_token` forever (vLLM's
    guided_choice) -> (token_class, transitions, start_state).  A state per trie node, the root first, and one final state that
    allows only end_token and loops on it; a choice may be a prefix of another (its node then allows end_token beside its children)
    but may not contain end_token.  Bookkeeping only: no device is touched."""
    seqs = [[int(t) for t in c] for c in choices]
    end_token = int(end_token)
    if not seqs:
        raise ValueError("no choices")
    if not 0 <= end_token < num_vocab or any(not 0 <= t < num_vocab for c in seqs for t in c):
        raise ValueError(f"token ids must be < {num_vocab}")
    if any(end_token in c for c in seqs):
        raise ValueError("a choice contains end_token")
    used = {end_token: 0}                               # token -> column of the reduced table; the last column: every other token
    nodes, terminal = [{}], [False]                     # per trie node: column -> child, and whether a choice ends there
    for c in seqs:
        s = 0
        for t in c:
            k = used.setdefault(t, len(used))
            if k not in nodes[s]:
                nodes[s][k] = len(nodes)
                nodes.append({})
                terminal.append(False)
            s = nodes[s][k]
        terminal[s] = True
    final = len(nodes)
    small = np.full((final + 1, len(used) + 1), -1, np.int64)
    for s, kids in enumerate(nodes):
        for k, child in kids.items():
            small[s, k] = child
        if terminal[s]:
            small[s, 0] = final
    small[final, 0] = final
    cls, trans = grammar_from_dense(small)
    token_class = np.full(num_vocab, cls[-1], np.uint16)
    for t, k in used.items():
        token_class[t] = cls[k]
    return token_class, trans, 0


_REGEX_META = frozenset(b"\\.^$*+?()[]{}|")


def regex_of_choices(strings) -> str:
    """The regex that matches exactly one of `strings` (str or bytes): every choice escaped, joined by |.  Escaping only: ASCII
    metacharacters get a backslash, bytes outside printable ASCII become \\xHH (a str is taken as its UTF-8 bytes).  For
    `ByteDfa.from_regex` / `Grammar.compile`; bytes >= 0x80 written as \\xHH are raw bytes there, so a `bytes` pattern keeps them."""
    alts = []
    for c in strings:
        raw = c.encode("utf-8") if isinstance(c, str) else bytes(c)
        alts.append("".join("\\" + chr(b) if b in _REGEX_META else chr(b) if 0x20 <= b < 0x7F else f"\\x{b:02x}" for b in raw))
    if not alts:
        raise ValueError("no choices")
    return "|".join(alts)


class ByteDfa:
    """A deterministic automaton over bytes, on the host: next [num_states, 256] u16 (a state or GRAMMAR_REJECT),
    accepting [num_states] u8, starts [num_patterns] u32.  `from_regex` compiles one pattern or a list of patterns (str, taken as
    UTF-8, or bytes) into one automaton with a disjoint, minimal, trimmed state set per pattern; `from_arrays` wraps tables of a
    compiler of the caller's.  `Grammar.compile` turns it into the token automaton of a vocabulary."""

    def __init__(self, h):
        self.h = h
        ns, npat = C.c_uint32(), C.c_uint32()
        hip.wrk_byte_dfa_export(h, C.byref(ns), C.byref(npat), None, None, None)
        self.num_states, self.num_patterns = ns.value, npat.value
        self.next = np.empty((self.num_states, 256), np.uint16)
        self.accepting = np.empty(self.num_states, np.uint8)
        self.starts = np.empty(self.num_patterns, np.uint32)
        hip.wrk_byte_dfa_export(h, None, None, _ptr(self.next, _u16p), _ptr(self.accepting, _u8p), _ptr(self.starts, _u32p))

    @classmethod
    def from_regex(cls, patterns) -> "ByteDfa":
        if isinstance(patterns, (str, bytes)):
            patterns = [patterns]
        raw = [p.encode("utf-8") if isinstance(p, str) else bytes(p) for p in patterns]
        n = len(raw)
        arr = (C.c_char_p * max(n, 1))(*raw)
        lens = (C.c_size_t * max(n, 1))(*[len(r) for r in raw])
        err = C.create_string_buffer(512)
        h = _P()
        rc = hip.wrk_regex_compile(arr, lens, n, C.byref(h), err, len(err))
        if rc != OK:
            raise WrkError(rc, err.value.decode(errors="replace"))
        return cls(h)

    @classmethod
    def from_arrays(cls, next, accepting, starts) -> "ByteDfa":
        nx = np.ascontiguousarray(np.asarray(next, np.uint16))
        ac = np.ascontiguousarray(np.asarray(accepting, np.uint8)).reshape(-1)
        st = _u32(starts).reshape(-1)
        if nx.ndim != 2 or nx.shape[1] != 256 or ac.size != nx.shape[0]:
            raise ValueError("next: [num_states, 256], accepting: [num_states]")
        h = _P()
        rc = hip.wrk_byte_dfa_from_arrays(nx.shape[0], _ptr(nx, _u16p), _ptr(ac, _u8p), _ptr(st, _u32p), st.size, C.byref(h))
        if rc != OK:
            raise WrkError(rc, "byte DFA arrays: a next state, a start state or a count out of range")
        return cls(h)

    def close(self):
        if self.h:
            hip.wrk_byte_dfa_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------------------- backend objects
class Context:
    """`Context` (src/context.rs:51-64): one HIP device + submission stream."""

    def __init__(self, device: int = 0):
        h = _P()
        rc = hip.wrk_ctx_create(device, C.byref(h))
        if rc != OK:
            raise WrkError(rc, f"wrk_ctx_create(device={device}) failed: no usable HIP device (the HIP path has no CPU fallback)")
        self.h = h

    def check(self, rc: int):
        if rc != OK:
            raise WrkError(rc, (hip.wrk_last_error(self.h) or b"").decode())

    def sync(self):
        self.check(hip.wrk_ctx_sync(self.h))

    def close(self):
        if self.h:
            hip.wrk_ctx_destroy(self.h)
            self.h = None

    # -- programs
    def encode(self, build) -> "Program":
        """`Context::encode(&TensorOp)` (ops.rs:79-143): run `build()` (which calls `TensorOp.*` / `matmul_op`) with the ops
        recorded into a `Program` instead of executed.  Safe from several threads at once: a capture belongs to the calling
        thread and records on a private stream (runtime/mod.rs:139-167 encodes on spawn_blocking workers)."""
        self.check(hip.wrk_capture_begin(self.h))
        try:
            build()
        finally:
            h = _P()
            rc = hip.wrk_capture_end(self.h, C.byref(h))
        self.check(rc)
        return Program(self, h)

    # -- tensors
    def tensor(self, array: np.ndarray, shape: Optional[Sequence[int]] = None) -> "Tensor":
        """context.tensor_from_data: numpy float16/float32 array; `shape` is [x fastest, y, z, w]."""
        a = np.ascontiguousarray(array)
        dt = {np.dtype(np.float16): F16, np.dtype(np.float32): F32}[a.dtype]
        if shape is None:
            shape = list(reversed(a.shape))
        shape = list(shape) + [1] * (4 - len(shape))
        assert int(np.prod(shape)) == a.size
        return Tensor(self, Buffer(self, a.nbytes, a), dt, shape)

    def zeros(self, shape: Sequence[int], dtype=np.float16) -> "Tensor":
        shape = list(shape) + [1] * (4 - len(shape))
        return self.tensor(np.zeros(int(np.prod(shape)), dtype=dtype), shape)

    def buffer(self, array: np.ndarray) -> "Buffer":
        a = np.ascontiguousarray(array)
        return Buffer(self, a.nbytes, a)

    def sample_logits(self, logits, temperature=1.0, top_p=0.5, seed=0, step: int = 0, num_vocab: Optional[int] = None,
                      top_k=None, min_p=None, mirostat=None, typical_p=None, top_n_sigma=None, epsilon_cutoff=None, eta_cutoff=None, xtc=None,
                      row_stride: Optional[int] = None):
        """`Sampler::sample` (examples/chat.rs:150-190; defaults are its `--temp 1.0 --top-p 0.5`) on the device, one token per row.
        `logits`: an [n, V] f32 array, or a `Buffer` of n rows of `num_vocab` f32; temperature / top_p / seed: scalars or per-row arrays.
        A temperature must be finite and >= 0 (+inf or NaN: WrkError E_ARG, here and in every decode loop); a NaN logit counts as -inf,
        and a row with +inf logits draws among those alone.
        top_k (0: off) / min_p (0: off): scalars or per-row arrays; with either the candidates are also cut to the top_k highest logits
        and to the tokens whose probability is at least min_p times the largest.  Returns uint32 [n].
        mirostat=(tau, eta, mu): Mirostat v2 with the target surprise tau (bits; 0: a plain row), the learning rate eta
        and the running mu (None: 2 tau, a fresh sequence), scalars or per-row arrays; returns (tokens uint32 [n], mu float32 [n]), mu
        after the draw.  typical_p (>= 1: a plain row): locally typical sampling.  One family per call; top_p is not read by a Mirostat
        or typical row.
        top_n_sigma (0: off) / epsilon_cutoff (0: off) / eta_cutoff (0: off) / xtc=(probability, threshold): scalars or per-row arrays,
        the cuts of DESIGN.md §7t next to top_k / min_p -- the tokens within top_n_sigma standard deviations of the maximum logit, those
        of probability at least epsilon_cutoff or min(eta, sqrt(eta) exp(-entropy)), and XTC, which with the given probability drops
        every token at or above the threshold but the least likely of them.  They share the top_k / min_p family.
        row_stride: the floats between the rows of a `Buffer` (None: num_vocab); only the cut sampler's path takes it."""
        stride = None
        if isinstance(logits, Buffer):
            assert num_vocab, "a Buffer needs num_vocab"
            buf, V = logits, int(num_vocab)
            stride = V if row_stride is None else int(row_stride)
            n = buf.nbytes // (4 * stride)
        else:
            a = np.ascontiguousarray(logits, dtype=np.float32)
            a = a.reshape(1, -1) if a.ndim == 1 else a
            n, V = a.shape
            buf = self.buffer(a)
        t, p, sd = _per_row(temperature, n, np.float32), _per_row(top_p, n, np.float32), _per_row(seed, n, np.uint32)
        out = np.zeros(n, np.uint32)
        cut_keep = []
        cut_ptrs = _cuts((top_n_sigma, epsilon_cutoff, eta_cutoff, xtc), n, cut_keep)
        if sum(x is not None for x in (mirostat, typical_p)) + (top_k is not None or min_p is not None or cut_ptrs is not None) > 1:
            raise ValueError("one family per call: top_k / min_p and the cuts, mirostat or typical_p")
        if cut_ptrs is not None:
            tk, mp = _filters(top_k, min_p, n, cut_keep)
            self.check(hip.wrk_sample_logits_cut(self.h, buf.h, V, V if stride is None else stride, n, _ptr(t, _f32p), _ptr(p, _f32p), tk, mp,
                                                 *cut_ptrs, _ptr(sd, _u32p), step, _ptr(out, _u32p)))
            return out
        if stride not in (None, V):
            raise ValueError("row_stride: only with the cut sampler's parameters")
        if mirostat is not None:
            tau, eta, mu = _mirostat_rows(mirostat[:2], mirostat[2], n)
            self.check(hip.wrk_sample_logits_mirostat(self.h, buf.h, V, V, n, _ptr(t, _f32p), _ptr(p, _f32p), _ptr(tau, _f32p), _ptr(eta, _f32p),
                                                      _ptr(mu, _f32p), _ptr(sd, _u32p), step, _ptr(out, _u32p)))
            return out, mu
        if typical_p is not None:
            ty = _per_row(typical_p, n, np.float32)
            self.check(hip.wrk_sample_logits_typical(self.h, buf.h, V, V, n, _ptr(t, _f32p), _ptr(p, _f32p), _ptr(ty, _f32p), _ptr(sd, _u32p),
                                                     step, _ptr(out, _u32p)))
            return out
        if top_k is None and min_p is None:
            self.check(hip.wrk_sample_logits(self.h, buf.h, V, V, n, _ptr(t, _f32p), _ptr(p, _f32p), _ptr(sd, _u32p), step, _ptr(out, _u32p)))
            return out
        keep = []
        tk, mp = _filters(top_k, min_p, n, keep)
        self.check(hip.wrk_sample_logits_filtered(self.h, buf.h, V, V, n, _ptr(t, _f32p), _ptr(p, _f32p), tk, mp, _ptr(sd, _u32p), step,
                                                  _ptr(out, _u32p)))
        return out

    def score_logits(self, logits, targets, num_vocab: Optional[int] = None, row_stride: Optional[int] = None):
        """Per row of f32 logits and its target token t: (logprob = x_t - logsumexp(x), rank = #{x_i > x_t} + #{i < t : x_i == x_t}),
        computed on the device.  `logits`: an [n, V] f32 array, or a `Buffer` of n rows of `row_stride` f32 (first `num_vocab` used).
        Returns (float32 [n], uint32 [n])."""
        tg = _u32(targets).reshape(-1)
        n = tg.size
        if isinstance(logits, Buffer):
            assert num_vocab, "a Buffer needs num_vocab"
            buf, V = logits, int(num_vocab)
            stride = int(row_stride or V)
        else:
            a = np.ascontiguousarray(logits, dtype=np.float32)
            a = a.reshape(1, -1) if a.ndim == 1 else a
            assert a.shape[0] == n, "one target per row"
            V = stride = a.shape[1]
            buf = self.buffer(a)
        lp = np.zeros(n, np.float32)
        rk = np.zeros(n, np.uint32)
        self.check(hip.wrk_score_logits(self.h, buf.h, V, stride, n, _ptr(tg, _u32p), _ptr(lp, _f32p), _ptr(rk, _u32p)))
        return lp, rk

    def top_logprobs(self, logits, tokens, num_top: int, num_vocab: Optional[int] = None, row_stride: Optional[int] = None):
        """Per row of f32 logits and its chosen token y: (logprob = x_y - logsumexp(x), the ids of the `num_top` most likely tokens --
        logit descending, ties by index ascending, the sampler's order -- and their log-probs), computed on the device on the raw row
        (DESIGN.md §7h).  `logits`: an [n, V] f32 array, or a `Buffer` of n rows of `row_stride` f32 (first `num_vocab` used).  Returns
        (float32 [n], uint32 [n, num_top], float32 [n, num_top]); entries past the vocabulary are id 0xFFFFFFFF and -inf."""
        tk = _u32(tokens).reshape(-1)
        n = tk.size
        if isinstance(logits, Buffer):
            assert num_vocab, "a Buffer needs num_vocab"
            buf, V = logits, int(num_vocab)
            stride = int(row_stride or V)
        else:
            a = np.ascontiguousarray(logits, dtype=np.float32)
            a = a.reshape(1, -1) if a.ndim == 1 else a
            assert a.shape[0] == n, "one token per row"
            V = stride = a.shape[1]
            buf = self.buffer(a)
        num_top = int(num_top)
        lp = np.zeros(max(n, 1), np.float32)
        ids = np.zeros(max(n * num_top, 1), np.uint32)
        tlp = np.zeros(max(n * num_top, 1), np.float32)
        self.check(hip.wrk_top_logprobs(self.h, buf.h, V, stride, n, _ptr(tk, _u32p), num_top, _ptr(lp, _f32p), _ptr(ids, _u32p),
                                        _ptr(tlp, _f32p)))
        return lp[:n], ids[:n * num_top].reshape(n, num_top), tlp[:n * num_top].reshape(n, num_top)

    def penalize_logits(self, logits, occ: "Occurrence", presence, frequency, first_batch: int = 0, num_vocab: Optional[int] = None,
                        row_stride: Optional[int] = None):
        """ChatRWKV's repetition penalties on the device: row r of the logits penalised with slot first_batch + r of `occ` (banned:
        -inf; present: x - (presence + count * frequency)).  `logits`: an [n, V] f32 array (returns the penalised
        copy), or a `Buffer` of n rows of `row_stride` f32 (first `num_vocab` used), penalised in place (returns None).
        presence / frequency: scalars or per-row arrays."""
        if isinstance(logits, Buffer):
            assert num_vocab, "a Buffer needs num_vocab"
            buf, V = logits, int(num_vocab)
            stride = int(row_stride or V)
            n = (buf.nbytes // 4 - V) // stride + 1 if buf.nbytes >= 4 * V else 0
            a = None
        else:
            a = np.ascontiguousarray(logits, dtype=np.float32)
            a = a.reshape(1, -1) if a.ndim == 1 else a
            n, V = a.shape
            stride = V
            buf = self.buffer(a)
        ap, af = _per_row(presence, n, np.float32), _per_row(frequency, n, np.float32)
        self.check(hip.wrk_penalize_logits(self.h, buf.h, V, stride, n, occ.h, first_batch, _ptr(ap, _f32p), _ptr(af, _f32p)))
        return None if a is None else buf.read(np.float32, n * V).reshape(n, V)

    def constrain_logits(self, logits, grammar: "Grammar", states, num_vocab: Optional[int] = None, row_stride: Optional[int] = None):
        """Masks rows of logits with an automaton on the device: row r keeps the bits of every token that `grammar`
        allows in states[r] and gets -inf elsewhere.  `logits`: an [n, V] f32 array (returns the masked copy), or a `Buffer` of n rows
        of `row_stride` f32 (first `num_vocab` used), masked in place (returns None).  states: a scalar or one state per row."""
        if isinstance(logits, Buffer):
            assert num_vocab, "a Buffer needs num_vocab"
            buf, V = logits, int(num_vocab)
            stride = int(row_stride or V)
            n = (buf.nbytes // 4 - V) // stride + 1 if buf.nbytes >= 4 * V else 0
            a = None
        else:
            a = np.ascontiguousarray(logits, dtype=np.float32)
            a = a.reshape(1, -1) if a.ndim == 1 else a
            n, V = a.shape
            stride = V
            buf = self.buffer(a)
        st = _per_row(states, n, np.uint32)
        self.check(hip.wrk_constrain_logits(self.h, buf.h, V, stride, n, grammar.h, _ptr(st, _u32p)))
        return None if a is None else buf.read(np.float32, n * V).reshape(n, V)

    def bias_logits(self, logits, lb: "LogitBias", sets, num_vocab: Optional[int] = None, row_stride: Optional[int] = None):
        """Biases rows of logits on the device: row r gets -inf at every token its set bans (value -inf), x + v at every
        other token of the set and keeps the bits of the rest; a row with BIAS_NONE is left alone.  `logits`: an [n, V] f32 array
        (returns the biased copy), or a `Buffer` of n rows of `row_stride` f32 (first `num_vocab` used), biased in place (returns
        None).  sets: a scalar or one set index per row.  In a host loop it goes in front of `penalize_logits`."""
        if isinstance(logits, Buffer):
            assert num_vocab, "a Buffer needs num_vocab"
            buf, V = logits, int(num_vocab)
            stride = int(row_stride or V)
            n = (buf.nbytes // 4 - V) // stride + 1 if buf.nbytes >= 4 * V else 0
            a = None
        else:
            a = np.ascontiguousarray(logits, dtype=np.float32)
            a = a.reshape(1, -1) if a.ndim == 1 else a
            n, V = a.shape
            stride = V
            buf = self.buffer(a)
        st = _per_row(sets, n, np.uint32)
        self.check(hip.wrk_bias_logits(self.h, buf.h, V, stride, n, lb.h, _ptr(st, _u32p)))
        return None if a is None else buf.read(np.float32, n * V).reshape(n, V)

    def guide_logits(self, logits, scale, num_vocab: Optional[int] = None, row_stride: Optional[int] = None):
        """Classifier-free guidance on rows of logits on the device.  `logits` holds 2R rows, the R conditional ones
        first and row R + r the unconditional partner of row r: an [2R, V] f32 array, or a `Buffer` of 2R rows of `row_stride` f32
        (first `num_vocab` used).  scale: a scalar or one value per guided row, finite and >= 0; a row with scale 1 is its conditional
        row bit for bit.  The rows are mixed raw (u + s (c - u), three f32 roundings), not log-softmaxed: no pick sees the
        difference.  Returns the guided rows [R, V].  In a host loop it goes in front of `bias_logits`."""
        if isinstance(logits, Buffer):
            assert num_vocab, "a Buffer needs num_vocab"
            buf, V = logits, int(num_vocab)
            stride = int(row_stride or V)
            n2 = (buf.nbytes // 4 - V) // stride + 1 if buf.nbytes >= 4 * V else 0
        else:
            a = np.ascontiguousarray(logits, dtype=np.float32)
            a = a.reshape(2, -1) if a.ndim == 1 else a
            n2, V = a.shape
            stride = V
            buf = self.buffer(a)
        if n2 % 2:
            raise ValueError(f"{n2} rows: guidance takes the conditional rows and as many unconditional ones")
        n = n2 // 2
        sc = _per_row(scale, n, np.float32)
        out = self.buffer(np.zeros(max(n * V, 1), np.float32))
        self.check(hip.wrk_guide_logits(self.h, buf.h, V, stride, n, _ptr(sc, _f32p), out.h, V))
        return out.read(np.float32, n * V).reshape(n, V)

    def beam_step(self, logits, num_beams: int, scores, keys, lengths, status, stop=None, length_penalty: float = 0.0,
                  num_vocab: Optional[int] = None, row_stride: Optional[int] = None):
        """One beam-search step on the device (wrk_beam_step) for a host-driven loop: rows [G * num_beams, V] of logits --
        an f32 array, or a `Buffer` of rows of `row_stride` f32 (first `num_vocab` used) -- and the slot records scores / keys (f32) and
        lengths / status (BEAM_LIVE / BEAM_DONE / BEAM_DEAD), all [B].  stop: one list of ids for all groups, or one list per group.
        Returns (tokens [B], parents [B], copy_src [B], scores, keys, lengths, status): the token every slot feeds next (BEAM_NO_TOKEN:
        not filled in this step), the slot it descends from, the step's copy list (BEAM_NO_COPY: the slot moves no bytes) and the
        records after the step."""
        sc, ky = np.array(scores, np.float32).reshape(-1), np.array(keys, np.float32).reshape(-1)
        ln, stt = np.array(lengths, np.uint32).reshape(-1), np.array(status, np.uint32).reshape(-1)
        B, W = sc.size, int(num_beams)
        assert ky.size == B and ln.size == B and stt.size == B, "one record per slot"
        if W < 1 or B % W:
            raise ValueError(f"{B} slots are not groups of {W} beams")
        G = B // W
        if isinstance(logits, Buffer):
            assert num_vocab, "a Buffer needs num_vocab"
            buf, V = logits, int(num_vocab)
            stride = int(row_stride or V)
        else:
            a = np.ascontiguousarray(logits, dtype=np.float32)
            a = a.reshape(1, -1) if a.ndim == 1 else a
            assert a.shape[0] == B, "one row per slot"
            V = stride = a.shape[1]
            buf = self.buffer(a)
        ids, off = _stop_csr(stop, G, "groups")
        tok, par, cp = np.zeros(B, np.uint32), np.zeros(B, np.uint32), np.zeros(B, np.uint32)
        self.check(hip.wrk_beam_step(self.h, buf.h, V, stride, G, W, float(length_penalty), _ptr(ids, _u32p), _ptr(off, _u32p),
                                     _ptr(sc, _f32p), _ptr(ky, _f32p), _ptr(ln, _u32p), _ptr(stt, _u32p), _ptr(tok, _u32p), _ptr(par, _u32p),
                                     _ptr(cp, _u32p)))
        return tok, par, cp, sc, ky, ln, stt

    def stop_sequences_advance(self, tails, tokens, stop_sequences, stop=None, num_vocab: Optional[int] = None):
        """One counted draw of the stop-sequence matcher on the device (wrk_stop_sequences_advance) for n rows: row r has the
        tail tails[r] (STOP_TAIL_LEN entries, oldest first, STOP_TAIL_EMPTY where there is none), the drawn token tokens[r], the stop
        sequences `stop_sequences` (one list of id lists for all rows, or one per row) and optionally the stop ids `stop` (as
        `generate_stop`).  Returns (match [n], tails [n, STOP_TAIL_LEN]): STOP_MATCH_NONE, STOP_MATCH_TOKEN or the index of the matching
        sequence (the longest wins, then a stop id, then the lower index), and the tails with the token taken in.  num_vocab: the bound the
        ids are checked against (None: any id below STOP_TAIL_EMPTY)."""
        tk = _u32(tokens).reshape(-1)
        n = tk.size
        tl = _stop_tails(tails, n)
        ids, off, own = _stop_seq_csr(stop_sequences, n, "rows")
        sid, soff = (None, None) if stop is None else _stop_csr(stop, n, "rows")
        match = np.zeros(max(n, 1), np.uint32)
        self.check(hip.wrk_stop_sequences_advance(self.h, 0xFFFFFFFF if num_vocab is None else int(num_vocab), n, _ptr(ids, _u32p), _ptr(off, _u32p),
                                                  _ptr(own, _u32p), None if sid is None else _ptr(sid, _u32p),
                                                  None if soff is None else _ptr(soff, _u32p), _ptr(tl, _u32p), _ptr(tk, _u32p), _ptr(match, _u32p)))
        return match[:n], tl

    def dry_logits(self, logits, window: "TokenWindow", dry=None, no_repeat_ngram=None, dry_breakers=None, first_batch: int = 0,
                   num_vocab: Optional[int] = None, row_stride: Optional[int] = None):
        """DRY and the no-repeat-n-gram ban on rows of logits, on the device: row r is changed with slot first_batch + r
        of `window` -- the token that would extend a repeat of M tokens loses multiplier * base ** (M - allowed_length) once M >=
        allowed_length, and gets -inf once M >= no_repeat_ngram - 1; every other token keeps its bits.  dry = (multiplier, base,
        allowed_length), scalars or one value per row (None: off); no_repeat_ngram: a scalar or one value per row (None: off);
        dry_breakers: ids a match never crosses.  `logits`: an [n, V] f32 array (returns the changed copy), or a `Buffer` of n rows of
        `row_stride` f32 (first `num_vocab` used), changed in place (returns None).  In a host loop it goes between `penalize_logits`
        and `constrain_logits`.  The window is only read."""
        if isinstance(logits, Buffer):
            assert num_vocab, "a Buffer needs num_vocab"
            buf, V = logits, int(num_vocab)
            stride = int(row_stride or V)
            n = (buf.nbytes // 4 - V) // stride + 1 if buf.nbytes >= 4 * V else 0
            a = None
        else:
            a = np.ascontiguousarray(logits, dtype=np.float32)
            a = a.reshape(1, -1) if a.ndim == 1 else a
            n, V = a.shape
            stride = V
            buf = self.buffer(a)
        keep = []
        self.check(hip.wrk_dry_logits(self.h, buf.h, V, stride, n, window.h, first_batch, *_dry_rows(n, keep, dry, no_repeat_ngram, dry_breakers)))
        return None if a is None else buf.read(np.float32, n * V).reshape(n, V)


class TokenWindow:
    """The per-sequence window of recent tokens that DRY and the no-repeat-n-gram ban match on, on the device:
    `num_batch` slots (slot b belongs to state slot b) of the last `capacity` tokens that counted, oldest first.  The decode loops push
    every draw that counts when it is passed as `window=`; a prompt is pushed with `add`."""

    def __init__(self, ctx: "Context", num_batch: int, num_vocab: int, capacity: int):
        h = _P()
        ctx.check(hip.wrk_token_window_create(ctx.h, num_batch, num_vocab, capacity, C.byref(h)))
        self.ctx, self.h = ctx, h
        self.num_batch, self.num_vocab, self.capacity = int(num_batch), int(num_vocab), int(capacity)

    def add(self, batch: int, tokens):
        """Pushes `tokens` into slot `batch` in order."""
        t = _u32(tokens).reshape(-1)
        self.ctx.check(hip.wrk_token_window_add(self.ctx.h, self.h, batch, _ptr(t, _u32p) if t.size else None, t.size))

    def back(self, batch: int) -> np.ndarray:
        """The tokens of slot `batch`, oldest first (uint32 [length])."""
        out, n = np.zeros(self.capacity, np.uint32), C.c_uint32()
        self.ctx.check(hip.wrk_token_window_back(self.ctx.h, self.h, batch, _ptr(out, _u32p), C.byref(n)))
        return out[:n.value].copy()

    def permute(self, parents):
        """Slot q <- slot parents[q] for q < len(parents), ring and meta, on the device and correct under any aliasing; slots with
        parents[q] == q move no bytes and slots >= len(parents) are untouched (wrk_token_window_permute): `Runtime.state_permute`'s
        companion in a host-driven beam loop."""
        p = _u32(parents).reshape(-1)
        self.ctx.check(hip.wrk_token_window_permute(self.ctx.h, self.h, _ptr(p, _u32p), p.size))

    def load(self, batch: int, tokens=None):
        """Slot `batch` becomes `tokens` (at most `capacity`, oldest first); None: empty."""
        if tokens is None:
            self.ctx.check(hip.wrk_token_window_load(self.ctx.h, self.h, batch, None, 0))
            return
        t = _u32(tokens).reshape(-1)
        if t.size == 0:
            return self.load(batch, None)
        self.ctx.check(hip.wrk_token_window_load(self.ctx.h, self.h, batch, _ptr(t, _u32p), t.size))

    def close(self):
        if self.h and self.ctx.h:
            hip.wrk_token_window_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LogitBias:
    """Bias sets for the decode loops, on the device and immutable: `sets` is a list of {token: value} dicts or of
    (ids, values) pairs over one vocabulary; a value of -inf bans the token, a finite one is added to its logit, NaN and +inf are
    refused, as is a set that bans the whole vocabulary.  Pass it to the decode loops as `logit_bias=`, with `bias_set=` the index of
    the set each sequence or request uses (BIAS_NONE: none)."""

    NONE = BIAS_NONE

    def __init__(self, ctx: Context, num_vocab: int, sets):
        off, ids, vals = _bias_csr(sets)
        self.num_vocab, self.num_sets = int(num_vocab), int(off.size - 1)
        h = _P()
        if ids.size == 0:       # no entry at all: the arrays must still be there
            ids, vals = np.zeros(1, np.uint32), np.zeros(1, np.float32)
        ctx.check(hip.wrk_logit_bias_create(ctx.h, self.num_vocab, self.num_sets, _ptr(off, _u32p), _ptr(ids, _u32p), _ptr(vals, _f32p),
                                            C.byref(h)))
        self.ctx, self.h = ctx, h

    def close(self):
        if self.h and self.ctx.h:
            hip.wrk_logit_bias_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Grammar:
    """A deterministic automaton over token ids for constrained decoding, on the device: token_class [num_vocab] maps
    every token to a class and transitions [num_states, num_classes] holds the next state, or GRAMMAR_REJECT where the class is not
    allowed.  `grammar_from_dense` / `grammar_from_choices` build the two tables and `Grammar.compile` builds them on the device from
    regex patterns and a vocabulary; BNF or JSON-schema compilers sit above `ByteDfa.from_arrays`.
    Every state must allow at least one token.  Pass it to the decode loops as `grammar=`, with `grammar_state=` the state each
    sequence starts in."""

    REJECT = GRAMMAR_REJECT

    def __init__(self, ctx: Context, num_vocab: int, token_class, transitions):
        self.token_class, self.transitions = _grammar_tables(num_vocab, token_class, transitions)
        self.num_vocab = int(num_vocab)
        self.num_states, self.num_classes = self.transitions.shape
        h = _P()
        ctx.check(hip.wrk_grammar_create(ctx.h, self.num_vocab, self.num_states, self.num_classes, _ptr(self.token_class, _u16p),
                                         _ptr(self.transitions, _u16p), C.byref(h)))
        self.ctx, self.h = ctx, h

    @classmethod
    def compile(cls, ctx: Context, vocab, dfa_or_patterns, end_token: int) -> "Grammar":
        """The token automaton of regex patterns (or of a `ByteDfa`) over `vocab`, a list of `bytes`, one per token id (DESIGN.md
        §7v): the walk of every token through every state runs on the device.  A sequence that has matched may draw `end_token`,
        which leads to `final_state`, where only `end_token` is allowed.  The grammar carries `start_states` [num_patterns] (pass
        one as `grammar_state=`), `final_state` and `compile_ms` (milliseconds per phase of GRAMMAR_COMPILE_PHASES); its host tables
        are read back from the device object."""
        dfa = dfa_or_patterns if isinstance(dfa_or_patterns, ByteDfa) else ByteDfa.from_regex(dfa_or_patterns)
        toks = [bytes(t) for t in vocab]
        off = np.zeros(len(toks) + 1, np.uint64)
        off[1:] = np.cumsum([len(t) for t in toks], dtype=np.uint64)
        data = np.frombuffer(b"".join(toks) + b"\0", np.uint8)        # never empty: a pointer is required
        starts = np.zeros(dfa.num_patterns, np.uint32)
        final = C.c_uint32()
        h = _P()
        ctx.check(hip.wrk_grammar_compile(ctx.h, dfa.h, len(toks), _ptr(data, _u8p), _ptr(off, _u64p), int(end_token), C.byref(h),
                                          _ptr(starts, _u32p), C.byref(final)))
        g = cls.__new__(cls)
        g.ctx, g.h, g.num_vocab = ctx, h, len(toks)
        ns, nc = C.c_uint32(), C.c_uint32()
        ctx.check(hip.wrk_grammar_export(h, C.byref(ns), C.byref(nc), None, None))
        g.num_states, g.num_classes = ns.value, nc.value
        g.token_class = np.empty(g.num_vocab, np.uint16)
        g.transitions = np.empty((g.num_states, g.num_classes), np.uint16)
        ctx.check(hip.wrk_grammar_export(h, None, None, _ptr(g.token_class, _u16p), _ptr(g.transitions, _u16p)))
        g.start_states, g.final_state = starts, int(final.value)
        ms = np.zeros(len(GRAMMAR_COMPILE_PHASES), np.float32)
        hip.wrk_grammar_compile_last_ms(_ptr(ms, _f32p))
        g.compile_ms = dict(zip(GRAMMAR_COMPILE_PHASES, ms.tolist()))
        return g

    def walk(self, state: int, tokens) -> int:
        """The state after `tokens` from `state`, walked on the host; ValueError at the first rejected token."""
        return grammar_walk(self.token_class, self.transitions, state, tokens)

    def advance(self, states, tokens) -> np.ndarray:
        """One step per row on the device: the next state of states[r] on tokens[r]; a rejected token leaves the state as it was.
        Returns uint32 [n]."""
        tk = _u32(tokens).reshape(-1)
        st = np.array(_per_row(states, tk.size, np.uint32), np.uint32)
        self.ctx.check(hip.wrk_grammar_advance(self.ctx.h, self.h, _ptr(st, _u32p), _ptr(tk, _u32p), tk.size))
        return st

    def close(self):
        if self.h and self.ctx.h:
            hip.wrk_grammar_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Occurrence:
    """The per-sequence occurrence table of the repetition penalties (ChatRWKV's `occurrence` dict and `token_ban`, on the device):
    num_batch slots of num_vocab (count f32, flags: bit 0 present, bit 1 banned), slot b belonging to state slot b, and one weight vector
    (ChatRWKV's `www`, default 1).  Survives across calls, like the RNN state."""

    PRESENT, BANNED = 1, 2

    def __init__(self, ctx: Context, num_batch: int, num_vocab: int):
        h = _P()
        ctx.check(hip.wrk_occurrence_create(ctx.h, num_batch, num_vocab, C.byref(h)))
        self.ctx, self.h, self.num_batch, self.num_vocab = ctx, h, num_batch, num_vocab

    def set_weights(self, weights=None):
        """weights: f32 [num_vocab], finite and >= 0; None: all 1."""
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
        assert w is None or w.size == self.num_vocab
        self.ctx.check(hip.wrk_occurrence_set_weights(self.ctx.h, self.h, None if w is None else _ptr(w, _f32p)))

    def ban(self, b: int, tokens, banned: bool = True):
        t = _u32(tokens).reshape(-1)
        self.ctx.check(hip.wrk_occurrence_ban(self.ctx.h, self.h, b, _ptr(t, _u32p), t.size, 1 if banned else 0))

    def add(self, b: int, tokens, decay: float = 1.0):
        """Counts tokens in order as the decode loop counts drawn ones: count *= decay, then count[y] += w[y], present[y] = 1."""
        t = _u32(tokens).reshape(-1)
        self.ctx.check(hip.wrk_occurrence_add(self.ctx.h, self.h, b, _ptr(t, _u32p), t.size, decay))

    def back(self, b: int):
        """(counts f32 [num_vocab], flags u32 [num_vocab]) of slot b."""
        c = np.empty(self.num_vocab, np.float32)
        f = np.empty(self.num_vocab, np.uint32)
        self.ctx.check(hip.wrk_occurrence_back(self.ctx.h, self.h, b, _ptr(c, _f32p), _ptr(f, _u32p)))
        return c, f

    def permute(self, parents):
        """Slot q <- slot parents[q] for q < len(parents), counts and both flag bits, on the device and correct under any aliasing;
        slots with parents[q] == q move no bytes and slots >= len(parents) are untouched (wrk_occurrence_permute): `Runtime.state_permute`'s
        companion in a host-driven beam loop."""
        p = _u32(parents).reshape(-1)
        self.ctx.check(hip.wrk_occurrence_permute(self.ctx.h, self.h, _ptr(p, _u32p), p.size))

    def load(self, b: int, counts=None, flags=None):
        """Sets slot b; counts=None and flags=None reset it (zero counts, no flags)."""
        if counts is None and flags is None:
            self.ctx.check(hip.wrk_occurrence_load(self.ctx.h, self.h, b, None, None))
            return
        c = np.ascontiguousarray(counts, dtype=np.float32)
        f = _u32(flags)
        assert c.size == self.num_vocab and f.size == self.num_vocab
        self.ctx.check(hip.wrk_occurrence_load(self.ctx.h, self.h, b, _ptr(c, _f32p), _ptr(f, _u32p)))

    def close(self):
        if self.h and self.ctx.h:
            hip.wrk_occurrence_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Program:
    """The `Vec<CommandBuffer>` an `RnnJob` keeps (v7.rs:423-432): a captured hipGraph; `launch` == `queue.submit`."""

    def __init__(self, ctx: Context, h):
        self.ctx, self.h = ctx, h

    def launch(self):
        self.ctx.check(hip.wrk_program_launch(self.ctx.h, self.h))

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.ctx.sync()
                hip.wrk_program_destroy(self.h)
        except Exception:
            pass
        self.h = None


class Buffer:
    def __init__(self, ctx: Context, nbytes: int, init: Optional[np.ndarray] = None):
        self.ctx = ctx
        h = _P()
        p = init.ctypes.data_as(_P) if init is not None else None
        ctx.check(hip.wrk_buf_create(ctx.h, nbytes, p, C.byref(h)))
        self.h, self.nbytes = h, nbytes

    def write(self, array: np.ndarray, offset: int = 0):
        a = np.ascontiguousarray(array)
        self.ctx.check(hip.wrk_buf_write(self.ctx.h, self.h, offset, a.ctypes.data_as(_P), a.nbytes))

    def read(self, dtype, count: int, offset: int = 0) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        self.ctx.check(hip.wrk_buf_read(self.ctx.h, self.h, offset, out.ctypes.data_as(_P), out.nbytes))
        return out

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                hip.wrk_buf_release(self.h)
        except Exception:
            pass
        self.h = None


class Tensor:
    """TensorGpu / TensorGpuView: buffer + dtype + View{shape, stride, offset}."""

    def __init__(self, ctx, buf: Buffer, dtype: int, shape, stride=None, offset=None):
        self.ctx, self.buf, self.dtype = ctx, buf, dtype
        self.shape = list(shape)
        self.stride = list(stride) if stride is not None else list(shape)
        self.offset = list(offset) if offset is not None else [0, 0, 0, 0]

    def view(self, *slices) -> "Tensor":
        """tensor.view(.., a..b, .., ..): each arg is None (full), int, or (start, end)."""
        shape, off = list(self.shape), list(self.offset)
        for i, s in enumerate(slices):
            if s is None:
                continue
            a, b = (s, s + 1) if isinstance(s, int) else s
            assert 0 <= a <= b <= self.shape[i]
            shape[i], off[i] = b - a, self.offset[i] + a
        return Tensor(self.ctx, self.buf, self.dtype, shape, self.stride, off)

    def reshape(self, shape) -> "Tensor":
        shape = list(shape) + [1] * (4 - len(shape))
        assert int(np.prod(shape)) == int(np.prod(self.shape)) and self.offset == [0, 0, 0, 0] and self.stride == self.shape
        return Tensor(self.ctx, self.buf, self.dtype, shape)

    def desc(self) -> TensorDesc:
        d = TensorDesc()
        d.buf = self.buf.h
        d.dtype = self.dtype
        for i in range(4):
            d.view.shape[i], d.view.stride[i], d.view.offset[i] = self.shape[i], self.stride[i], self.offset[i]
        return d

    def back(self) -> np.ndarray:
        """TensorGpu::back -> numpy array of the PARENT tensor, numpy shape reversed ([w, z, y, x])."""
        n = int(np.prod(self.stride))
        dt = np.float16 if self.dtype == F16 else np.float32
        return self.buf.read(dt, n).reshape(list(reversed(self.stride)))


class Matrix:
    """`enum Matrix` (src/tensor/matrix.rs:82-131) created from raw GGUF blocks or f16/f32 values."""

    def __init__(self, ctx: Context, kind: str, k: int, m: int, data: np.ndarray, flags: int = MATRIX_EXACT):
        a = np.ascontiguousarray(data)
        h = _P()
        ctx.check(hip.wrk_matrix_create(ctx.h, MAT[kind], k, m, a.ctypes.data_as(_P), a.nbytes, flags, C.byref(h)))
        self.ctx, self.h, self.k, self.m, self.kind = ctx, h, k, m, kind

    @classmethod
    def _quant(cls, kind: str, matrix: "Buffer", k: int, m: int, levels=None) -> "Matrix":
        ctx = matrix.ctx
        h = _P()
        lv = None
        if levels is not None:
            lv = np.ascontiguousarray(levels, np.float32)
            assert lv.size == 16
            lv = lv.ctypes.data_as(C.POINTER(C.c_float))
        ctx.check(hip.wrk_matrix_quantize(ctx.h, MAT[kind], k, m, matrix.h, lv, C.byref(h)))
        self = cls.__new__(cls)
        self.ctx, self.h, self.k, self.m, self.kind = ctx, h, k, m, kind
        return self

    @classmethod
    def quant_u8(cls, matrix: "Buffer", k: int, m: int) -> "Matrix":
        """`Matrix::quant_u8` (matrix.rs:211-227): f16 [K, M] buffer -> Int8 matrix, quantised on the device."""
        return cls._quant("INT8", matrix, k, m)

    @classmethod
    def quant_nf4(cls, matrix: "Buffer", k: int, m: int) -> "Matrix":
        """`Matrix::quant_nf4` (matrix.rs:229-249)."""
        return cls._quant("NF4", matrix, k, m)

    @classmethod
    def quant_sf4(cls, matrix: "Buffer", k: int, m: int, levels) -> "Matrix":
        """`Matrix::quant_sf4` (matrix.rs:251-271) with the caller's 16 levels (`Float4Quant::new_student`)."""
        return cls._quant("NF4", matrix, k, m, levels)

    def export(self) -> np.ndarray:
        """Int8 / NF4 planes in `wrk_matrix_create`'s layout (codes ++ side table [++ levels])."""
        n = C.c_size_t()
        self.ctx.check(hip.wrk_matrix_export(self.h, None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint8)
        self.ctx.check(hip.wrk_matrix_export(self.h, out.ctypes.data_as(_P), out.nbytes, C.byref(n)))
        return out

    def set_scale(self, scale: float):
        """y = act(scale * (W . x)): `load_matrix_discount`'s 2^-k factor without leaving the quantised form."""
        self.ctx.check(hip.wrk_matrix_set_scale(self.h, scale))

    @property
    def stream_bytes(self) -> int:
        return hip.wrk_matrix_stream_bytes(self.h)

    def matmul_op(self, inp: Tensor, out: Tensor, act: str = "none", turbo: bool = False, sparse: bool = False):
        di, do = inp.desc(), out.desc()
        self.ctx.check(hip.wrk_op_matmul(self.ctx.h, self.h, C.byref(di), C.byref(do), ACT[act], int(turbo), int(sparse)))

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                hip.wrk_matrix_release(self.h)
        except Exception:
            pass
        self.h = None


class TensorOp:
    """Constructors named like `TensorOp::*` (src/tensor/ops.rs); each enqueues on the context."""

    @staticmethod
    def _c(t: Tensor):
        return t.ctx

    @staticmethod
    def layer_norm(w: Buffer, b: Buffer, x: Tensor, eps: float):
        d = x.desc(); x.ctx.check(hip.wrk_op_layer_norm(x.ctx.h, w.h, b.h, C.byref(d), eps))

    @staticmethod
    def group_norm(w: Buffer, b: Buffer, x: Tensor, eps: float):
        d = x.desc(); x.ctx.check(hip.wrk_op_group_norm(x.ctx.h, w.h, b.h, C.byref(d), eps))

    @staticmethod
    def l2_norm(x: Tensor, eps: float):
        d = x.desc(); x.ctx.check(hip.wrk_op_l2_norm(x.ctx.h, C.byref(d), eps))

    @staticmethod
    def token_shift(cursors: Buffer, time_mix: Tensor, state: Tensor, inp: Tensor, out: Tensor, reversed_: bool):
        m, s, i, o = time_mix.desc(), state.desc(), inp.desc(), out.desc()
        inp.ctx.check(hip.wrk_op_token_shift(inp.ctx.h, cursors.h, C.byref(m), C.byref(s), C.byref(i), C.byref(o), int(reversed_)))

    @staticmethod
    def transpose(inp: Tensor, out: Tensor):
        i, o = inp.desc(), out.desc()
        out.ctx.check(hip.wrk_op_transpose(out.ctx.h, C.byref(i), C.byref(o)))

    @staticmethod
    def time_mix_v6(cursors: Buffer, time_decay: Tensor, time_first: Buffer, state: Tensor, k: Tensor, v: Tensor, r: Tensor, x: Tensor):
        dd, ds, dk, dv, dr, dx = time_decay.desc(), state.desc(), k.desc(), v.desc(), r.desc(), x.desc()
        x.ctx.check(hip.wrk_op_time_mix_v6(x.ctx.h, cursors.h, C.byref(dd), time_first.h, C.byref(ds), C.byref(dk), C.byref(dv), C.byref(dr), C.byref(dx)))

    @staticmethod
    def channel_mix(cursors: Buffer, state: Tensor, r: Tensor, v: Tensor, x: Tensor):
        ds, dr, dv, dx = state.desc(), r.desc(), v.desc(), x.desc()
        x.ctx.check(hip.wrk_op_channel_mix(x.ctx.h, cursors.h, C.byref(ds), C.byref(dr), C.byref(dv), C.byref(dx)))

    @staticmethod
    def add_activate(inp: Tensor, out: Tensor, act_x="none", act_y="none", act_out="none"):
        i, o = inp.desc(), out.desc()
        out.ctx.check(hip.wrk_op_add(out.ctx.h, C.byref(i), C.byref(o), ACT[act_x], ACT[act_y], ACT[act_out]))

    add = add_activate

    @staticmethod
    def mul_activate(inp: Tensor, out: Tensor, act_x="none", act_y="none", act_out="none"):
        i, o = inp.desc(), out.desc()
        out.ctx.check(hip.wrk_op_mul(out.ctx.h, C.byref(i), C.byref(o), ACT[act_x], ACT[act_y], ACT[act_out]))

    mul = mul_activate

    @staticmethod
    def lerp(x: Tensor, y: Tensor, f: Tensor, reversed_: bool):
        a, b, c = x.desc(), y.desc(), f.desc()
        y.ctx.check(hip.wrk_op_lerp(y.ctx.h, C.byref(a), C.byref(b), C.byref(c), int(reversed_)))

    @staticmethod
    def blit(inp: Tensor, out: Tensor):
        i, o = inp.desc(), out.desc()
        out.ctx.check(hip.wrk_op_blit(out.ctx.h, C.byref(i), C.byref(o)))

    @staticmethod
    def affine(x: Tensor, scale: float, bias: float):
        d = x.desc(); x.ctx.check(hip.wrk_op_affine(x.ctx.h, C.byref(d), scale, bias))

    @staticmethod
    def activate(x: Tensor, act: str):
        d = x.desc(); x.ctx.check(hip.wrk_op_activate(x.ctx.h, C.byref(d), ACT[act]))

    @staticmethod
    def control_k_v7(p: Buffer, a: Tensor, k: Tensor):
        da, dk = a.desc(), k.desc()
        k.ctx.check(hip.wrk_op_control_k_v7(k.ctx.h, p.h, C.byref(da), C.byref(dk)))

    @staticmethod
    def time_mix_v7(cursors: Buffer, state: Tensor, r: Tensor, w: Tensor, n: Tensor, x: Tensor):
        ds, dr, dw, dn, dx = state.desc(), r.desc(), w.desc(), n.desc(), x.desc()
        x.ctx.check(hip.wrk_op_time_mix_v7(x.ctx.h, cursors.h, C.byref(ds), C.byref(dr), C.byref(dw), C.byref(dn), C.byref(dx)))

    @staticmethod
    def time_first_v7(u: Buffer, r: Tensor, n: Tensor, x: Tensor):
        dr, dn, dx = r.desc(), n.desc(), x.desc()
        x.ctx.check(hip.wrk_op_time_first_v7(x.ctx.h, u.h, C.byref(dr), C.byref(dn), C.byref(dx)))

    @staticmethod
    def channel_mix_v7(cursors: Buffer, state: Tensor, v: Tensor, x: Tensor):
        ds, dv, dx = state.desc(), v.desc(), x.desc()
        x.ctx.check(hip.wrk_op_channel_mix_v7(x.ctx.h, cursors.h, C.byref(ds), C.byref(dv), C.byref(dx)))

    @staticmethod
    def softmax(x: Tensor):
        d = x.desc(); x.ctx.check(hip.wrk_op_softmax(x.ctx.h, C.byref(d)))


# ----------------------------------------------------------------------------- host layer
def _host_check(rc: int):
    if rc != OK:
        raise WrkError(rc, (rt.wrk_host_last_error() or b"").decode())


def quantile_student(nu: float = 5.0) -> np.ndarray:
    """`quantile_student(nu)` (src/tensor/matrix.rs:29-44): the 16 f32 levels of `Float4Quant::new_student(nu)` (SF4)."""
    out = np.zeros(16, np.float32)
    _host_check(rt.wrk_quantile_student(float(nu), _ptr(out, _f32p)))
    return out


class GgufReader:
    """`GgufReader` + `Reader` trait (src/runtime/gguf.rs)."""

    def __init__(self, data=None, path: Optional[str] = None):
        h = _P()
        if path is not None:
            _host_check(rt.wrk_gguf_open(path.encode(), C.byref(h)))
            self._keep = None
        else:
            self._keep = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
            _host_check(rt.wrk_gguf_from_memory(self._keep.ctypes.data_as(_P), self._keep.nbytes, C.byref(h)))
        self.h = h

    @property
    def version(self) -> int:
        return rt.wrk_gguf_version(self.h)

    @property
    def tensor_data_offset(self) -> int:
        return rt.wrk_gguf_tensor_data_offset(self.h)

    def contains(self, name: str) -> bool:
        return bool(rt.wrk_gguf_contains(self.h, name.encode()))

    def shape(self, name: str) -> List[int]:
        dims = (C.c_uint32 * 4)()
        nd = C.c_uint32()
        _host_check(rt.wrk_gguf_shape(self.h, name.encode(), dims, C.byref(nd)))
        return [int(dims[i]) for i in range(nd.value)]

    def tensor_f16(self, name: str) -> np.ndarray:
        n = C.c_size_t()
        _host_check(rt.wrk_gguf_tensor_f16(self.h, name.encode(), None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.uint16)
        _host_check(rt.wrk_gguf_tensor_f16(self.h, name.encode(), out.ctypes.data_as(C.POINTER(C.c_uint16)), out.size, C.byref(n)))
        return out.view(np.float16)

    def raw(self, name: str):
        t, p, n = C.c_uint32(), _P(), C.c_size_t()
        _host_check(rt.wrk_gguf_raw(self.h, name.encode(), C.byref(t), C.byref(p), C.byref(n)))
        return t.value, np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,))

    def read_state(self) -> np.ndarray:
        """`read_state(context, info, reader)` (v7.rs:1229-1262): pre-trained initial state -> [L, S+2, D] f32."""
        n = C.c_size_t()
        _host_check(rt.wrk_gguf_read_state(self.h, None, 0, C.byref(n)))
        mi = self.info()
        out = np.empty(n.value, np.float32)
        _host_check(rt.wrk_gguf_read_state(self.h, _ptr(out, _f32p), out.size, C.byref(n)))
        S = mi.num_emb // mi.num_head
        return out.reshape(mi.num_layer, S + 2, mi.num_emb)

    def info(self) -> ModelInfo:
        """`Loader::info(&reader)`."""
        mi = ModelInfo()
        _host_check(rt.wrk_gguf_info(self.h, C.byref(mi)))
        return mi

    def close(self):
        if self.h:
            rt.wrk_gguf_close(self.h)
            self.h = None


class RnnInput:
    """`RnnInput::new(batches, token_chunk_size)` (src/runtime/infer/rnn.rs:204-253)."""

    def __init__(self, batches: Sequence[Sequence[int]], token_chunk_size: int = 128, options: Optional[Sequence[int]] = None):
        h = _P()
        _host_check(rt.wrk_rnn_input_create(len(batches), token_chunk_size, C.byref(h)))
        self.h, self.num_batch = h, len(batches)
        for b, toks in enumerate(batches):
            self.append(b, toks)
            if options is not None:
                _host_check(rt.wrk_rnn_input_set_option(self.h, b, options[b]))

    @property
    def token_chunk_size(self) -> int:
        return rt.wrk_rnn_input_token_chunk_size(self.h)

    def append(self, batch: int, tokens: Sequence[int]):
        a = _u32(tokens)
        _host_check(rt.wrk_rnn_input_append(self.h, batch, _ptr(a, _u32p), a.size))

    def remaining(self, batch: int) -> int:
        return rt.wrk_rnn_input_remaining(self.h, batch)

    def step(self):
        _host_check(rt.wrk_rnn_input_step(self.h))

    def iter(self):
        it = _P()
        _host_check(rt.wrk_rnn_iter_create(self.h, C.byref(it)))
        nb = self.num_batch
        try:
            while True:
                lens = np.zeros(nb, np.uint32)
                opts = np.zeros(nb, np.int32)
                _host_check(rt.wrk_rnn_iter_next(it, _ptr(lens, _u32p), _ptr(opts, _i32p)))
                yield [(int(l), int(o)) for l, o in zip(lens, opts)]
        finally:
            rt.wrk_rnn_iter_destroy(it)

    def __del__(self):
        try:
            if self.h:
                rt.wrk_rnn_input_destroy(self.h)
        except Exception:
            pass
        self.h = None


def score_plan(inp: RnnInput, lens):
    """`wrk_rnn_score_plan` of the chunk `lens` (RnnIter::next of `inp`, before `inp.step()`): (headers, targets, rows per batch)."""
    ln = _u32(lens)
    cap = max(int(ln.sum()), 1)
    headers = np.zeros(cap, np.uint32)
    targets = np.zeros(cap, np.uint32)
    nh = C.c_uint32()
    rows = np.zeros(inp.num_batch, np.uint32)
    _host_check(rt.wrk_rnn_score_plan(inp.h, _ptr(ln, _u32p), _ptr(headers, _u32p), _ptr(targets, _u32p), C.byref(nh), _ptr(rows, _u32p)))
    n = nh.value
    return headers[:n].tolist(), targets[:n].tolist(), rows.tolist()


def redirect(info):
    """`RnnInfo::redirect` -> (headers, inputs, outputs)."""
    nb = len(info)
    lens = _u32([l for l, _ in info])
    opts = np.ascontiguousarray(np.asarray([o for _, o in info], dtype=np.int32))
    headers = np.zeros(max(int(lens.sum()), 1), np.uint32)
    nh = C.c_uint32()
    inputs = np.zeros(2 * nb, np.uint32)
    outputs = np.zeros(2 * nb, np.uint32)
    _host_check(rt.wrk_rnn_redirect(_ptr(lens, _u32p), _ptr(opts, _i32p), nb, _ptr(headers, _u32p), C.byref(nh),
                                    _ptr(inputs, _u32p), _ptr(outputs, _u32p)))
    return ([int(x) for x in headers[: nh.value]], [tuple(int(v) for v in inputs[2 * b:2 * b + 2]) for b in range(nb)],
            [tuple(int(v) for v in outputs[2 * b:2 * b + 2]) for b in range(nb)])


class Runtime:
    """`ModelBuilder::new(&context, reader).build_v7()` -> `v7::Bundle::<f16>::new(model, num_batch)`
    -> `SimpleRuntime::new(bundle)`; `infer(input)` as src/runtime/mod.rs:238-263."""

    def __init__(self, ctx: Context, reader: GgufReader, num_batch: int = 1, weights: int = WEIGHTS_INLINE, rescale: int = 0,
                 quant: Optional[Dict[int, int]] = None):
        """`quant`: `ModelBuilder::quant`'s layer -> QUANT_* map."""
        opt = BuildOptions(rescale, weights, None, 0)
        if quant:
            q = np.zeros(max(quant) + 1, np.uint8)
            for l, v in quant.items():
                q[l] = v
            opt.quant, opt.num_quant = q.ctypes.data_as(C.POINTER(C.c_uint8)), q.size
        h = _P()
        _host_check(rt.wrk_runtime_create(ctx.h, reader.h, C.byref(opt), num_batch, C.byref(h)))
        self.ctx, self.h, self.num_batch = ctx, h, num_batch
        self.info = ModelInfo()
        rt.wrk_runtime_info(h, C.byref(self.info))
        self.model = rt.wrk_runtime_model(h)
        self.model6 = rt.wrk_runtime_model_v6(h)
        self.state = rt.wrk_runtime_state(h)
        # the log-probs of the last generate_* call with `logprobs`: (logprob [steps_run, B], top_ids [steps_run, B, n], top_logprobs
        # [steps_run, B, n]); after generate_queue one such triple per request ([len], [len, n], [len, n]); None after a call without
        self.last_logprobs = None
        # the mu of the last generate_* call with `mirostat`, per sequence (generate_queue: per request); None after a call without
        self.last_mirostat_mu = None
        # the automaton states after the last generate_* call with `grammar`, per sequence (generate_queue: per request); None after
        # a call without
        self.last_grammar_state = None
        # what ended each sequence (generate_queue: each request) of the last call with `stop_sequences`, and after generate_stop the
        # tails [B, STOP_TAIL_LEN] to pass to the next call of a session; None after a call without
        self.last_stop_match = None
        self.last_stop_tail = None
        # what every step of the last generate_beam call put in every slot: (tokens, parents, scores), each [steps_run, B]
        self.last_beam_steps = None

    def token_bytes(self, num_batch: int = 1) -> int:
        if self.model6:
            return hip.wrk_v6_model_token_bytes(self.model6, num_batch)
        return hip.wrk_v7_model_token_bytes(self.model, num_batch)

    def infer(self, inp: RnnInput, mode: int = 1) -> List[np.ndarray]:
        """(input, output) = runtime.infer(input): runs one chunk; returns per-batch logits [rows, V]."""
        V = self.info.num_vocab
        cap = inp.token_chunk_size + inp.num_batch
        logits = np.empty((cap, V), dtype=np.float32)
        rows = np.zeros(inp.num_batch, np.uint32)
        _host_check(rt.wrk_runtime_infer(self.h, inp.h, _ptr(logits, _f32p), cap, _ptr(rows, _u32p), mode))
        out, p = [], 0
        for b in range(inp.num_batch):
            out.append(logits[p:p + rows[b]].copy())
            p += int(rows[b])
        return out

    def score(self, inp: RnnInput, mode: int = 1):
        """The scoring analogue of `infer`: runs one chunk and returns per-batch (logprob, rank) of every position whose next token
        is still in `inp` (`score_plan`); the state advances as `infer`'s would."""
        cap = inp.token_chunk_size + inp.num_batch
        lp = np.empty(cap, np.float32)
        rk = np.empty(cap, np.uint32)
        rows = np.zeros(inp.num_batch, np.uint32)
        _host_check(rt.wrk_runtime_score(self.h, inp.h, _ptr(lp, _f32p), _ptr(rk, _u32p), cap, _ptr(rows, _u32p), mode))
        out, p = [], 0
        for b in range(inp.num_batch):
            out.append((lp[p:p + rows[b]].copy(), rk[p:p + rows[b]].copy()))
            p += int(rows[b])
        return out

    def score_sequences(self, seqs, token_chunk_size: int = 128, mode: int = 1):
        """Scores whole sequences, one per state slot (len(seqs) == num_batch): for each, (logprob[len-1], rank[len-1]) where entry i
        is `log p(seq[i+1] | seq[:i+1])` and that token's greedy rank.  Scoring continues from the runtime's current state slots, as
        `infer` does: reset them first (`state_load` / `state_write`) to score from an empty context."""
        inp = RnnInput(seqs, token_chunk_size)
        lps = [[] for _ in seqs]
        rks = [[] for _ in seqs]
        while any(inp.remaining(b) for b in range(inp.num_batch)):
            for b, (lp, rk) in enumerate(self.score(inp, mode)):
                lps[b].append(lp)
                rks[b].append(rk)
        return [(np.concatenate(l) if l else np.zeros(0, np.float32), np.concatenate(r) if r else np.zeros(0, np.uint32))
                for l, r in zip(lps, rks)]

    def score_raw(self, tokens, cursors, headers, targets, mode: int = 1):
        """One RnnJob on explicit stacked tokens / packed cursors / header rows, the header rows scored against `targets`:
        (logprob float32 [NH], rank uint32 [NH])."""
        t, c, h, tg = _u32(tokens), _u32(cursors), _u32(headers), _u32(targets)
        lp = np.zeros(max(h.size, 1), np.float32)
        rk = np.zeros(max(h.size, 1), np.uint32)
        fn, mdl = (hip.wrk_v6_score, self.model6) if self.model6 else (hip.wrk_v7_score, self.model)
        self.ctx.check(fn(self.ctx.h, mdl, self.state, _ptr(t, _u32p), None, _ptr(c, _u32p), t.size, _ptr(h, _u32p), h.size,
                          _ptr(tg, _u32p) if tg.size else None, _ptr(lp, _f32p), _ptr(rk, _u32p), mode))
        return lp[: h.size], rk[: h.size]

    def infer_raw(self, tokens, cursors, headers, mode: int = 1, want_argmax: bool = False):
        """One RnnJob on explicit stacked tokens / packed cursors / header rows."""
        t, c, h = _u32(tokens), _u32(cursors), _u32(headers)
        V = self.info.num_vocab
        logits = np.empty((max(h.size, 1), V), np.float32)
        am = np.zeros(max(h.size, 1), np.uint32)
        fn, mdl = (hip.wrk_v6_infer, self.model6) if self.model6 else (hip.wrk_v7_infer, self.model)
        self.ctx.check(fn(self.ctx.h, mdl, self.state, _ptr(t, _u32p), None, _ptr(c, _u32p), t.size,
                          _ptr(h, _u32p), h.size, _ptr(logits, _f32p), _ptr(am, _u32p) if want_argmax else None, mode))
        return (logits[: h.size], am[: h.size]) if want_argmax else logits[: h.size]

    def set_frame_dtype(self, dtype: int):
        """`Bundle::<f16>` (F16, default) or `Bundle::<f32>` (F32) -- v7.rs:281-364 is generic over the activation type."""
        self.ctx.check(hip.wrk_v7_model_set_frame_dtype(self.ctx.h, self.model, dtype))
        self.frame_dtype = dtype

    def engine_status(self):
        """(exists, note) of the persistent batch-1 decode engine of this model (RWKV-7): why there is none, or "<N> compute waves"."""
        buf = C.create_string_buffer(512)
        rc = hip.wrk_v7_model_engine_status(self.ctx.h, self.model, buf, 512)
        if rc < 0:
            self.ctx.check(rc)
        return rc == 1, buf.value.decode()

    def infer_layer(self, layer: int, x: np.ndarray, v_first: Optional[np.ndarray], cursors, mode: int = 0):
        """Teacher-forced run of one layer on the layer input `x` [T, D] (and the layer-0 value `v_first`; RWKV-6 has none: pass None)."""
        if self.model6:
            xa, c = np.ascontiguousarray(x, dtype=np.float16), _u32(cursors)
            self.ctx.check(hip.wrk_v6_infer_layer(self.ctx.h, self.model6, self.state, layer, xa.ctypes.data_as(_P), _ptr(c, _u32p), c.size, mode))
            return
        dt = np.float32 if getattr(self, "frame_dtype", F16) == F32 else np.float16
        xa = np.ascontiguousarray(x, dtype=dt)
        va = np.ascontiguousarray(v_first, dtype=dt) if v_first is not None else None
        c = _u32(cursors)
        self.ctx.check(hip.wrk_v7_infer_layer(self.ctx.h, self.model, self.state, layer, xa.ctypes.data_as(_P),
                                              va.ctypes.data_as(_P) if va is not None else None, _ptr(c, _u32p), c.size, mode))

    def frame(self, name: str, num_token: int) -> np.ndarray:
        """One `Runtime<F>` buffer of the last job, [T, C] (names: examples/inspect.rs:208-248).  RWKV-6: in the buffer's own dtype
        (att_k, att_v, att_r, time_decay are float32), the five-plane buffers att_sx and tm as [5, T, D]."""
        if self.model6:
            n = C.c_size_t()
            self.ctx.check(hip.wrk_v6_frame_read(self.ctx.h, self.model6, name.encode(), num_token, None, 0, C.byref(n)))
            out = np.empty(n.value // 4, np.float32) if name in ("att_k", "att_v", "att_r", "time_decay") else np.empty(n.value // 2, np.float16)
            self.ctx.check(hip.wrk_v6_frame_read(self.ctx.h, self.model6, name.encode(), num_token, out.ctypes.data_as(_P), out.nbytes, C.byref(n)))
            return out.reshape(5, num_token, -1) if name in ("att_sx", "tm") else out.reshape(num_token, -1)
        dt = np.float32 if getattr(self, "frame_dtype", F16) == F32 else np.float16
        n = C.c_size_t()
        self.ctx.check(hip.wrk_v7_frame_read(self.ctx.h, self.model, name.encode(), num_token, None, 0, C.byref(n)))
        out = np.empty(n.value // np.dtype(dt).itemsize, dt)
        self.ctx.check(hip.wrk_v7_frame_read(self.ctx.h, self.model, name.encode(), num_token, out.ctypes.data_as(_P), out.nbytes, C.byref(n)))
        return out.reshape(num_token, -1)

    def _entry(self, name: str):
        """(wrk_v6_<name>, the RWKV-6 model) or (wrk_v7_<name>, the RWKV-7 model)."""
        return (getattr(hip, "wrk_v6_" + name), self.model6) if self.model6 else (getattr(hip, "wrk_v7_" + name), self.model)

    def _mode(self, mode: int, groups: int) -> int:
        """The ABI's mode word: mode | concurrent pipelines << 8 (RWKV-7 only)."""
        return (mode & 0xff) | ((groups & 0xff) << 8 if groups > 1 and not self.model6 else 0)

    def _generate(self, name: str, first_tokens, steps, rows, mode, groups, want_logits):
        """wrk_v*_generate_<name> with `rows` (per-sequence arrays and handles) between steps and the outputs: (tokens [steps, B],
        elapsed ms[, last logits [B, V]])."""
        ft = _u32(first_tokens)
        B = ft.size
        out = np.zeros((steps, B), np.uint32)
        ms = C.c_float()
        logits = np.empty((B, self.info.num_vocab), np.float32) if want_logits else None
        fn, mdl = self._entry("generate_" + name)
        self.last_logprobs = None
        self.last_grammar_state = None
        self.last_stop_match = self.last_stop_tail = None
        self.ctx.check(fn(self.ctx.h, mdl, self.state, _ptr(ft, _u32p), B, steps, *rows, _ptr(out, _u32p),
                          _ptr(logits, _f32p) if want_logits else None, C.byref(ms), self._mode(mode, groups)))
        return (out, ms.value, logits) if want_logits else (out, ms.value)

    def generate_greedy(self, first_tokens, steps: int, mode: int = 1, want_logits: bool = False, groups: int = 1, logprobs=None,
                        grammar: "Grammar" = None, grammar_state=None, window: "TokenWindow" = None, dry=None, no_repeat_ngram=None, dry_breakers=None,
                        logit_bias: "LogitBias" = None, bias_set=None):
        """Device-resident greedy loop; returns (tokens [steps, B], elapsed_ms[, last logits [B, V]]).
        groups > 1 (RWKV-7): the B independent sequences are dealt over that many concurrent pipelines (each a contiguous block of
        sequences with its own frame, decode program and HIP stream) instead of one batched step.
        logprobs (None: off; 0..MAX_TOP_LOGPROBS): every step also leaves the log-prob of each picked token and the `logprobs` most
        likely alternatives at its position, computed on the device on the raw head output (`Context.top_logprobs`), in
        `last_logprobs`; such a call goes through the options entry point (wrk_v*_generate_stop without stop sets).  The return
        shapes do not change.
        grammar / grammar_state (a scalar or one state per sequence; None: 0): constrained decoding: every pick is made
        on the row masked by the `Grammar` in the sequence's automaton state, and every draw moves that state, on the device;
        afterwards `last_grammar_state` [B] holds the states to pass to the next call of a session.  Such a call goes through the
        options entry point and replays step programs of its own.
        window / dry=(multiplier, base, allowed_length) / no_repeat_ngram / dry_breakers: every pick sees its row as
        `Context.dry_logits` leaves it with the sequence's slot of the `TokenWindow` -- the token that would extend a verbatim repeat
        is penalised, or with no_repeat_ngram banned -- and every draw is pushed into that slot, on the device.  Scalars or one value
        per sequence; a window alone only records the draws.  Greedy with DRY is the deterministic "no loops" mode.  Such a call goes
        through the options entry point and replays step programs of its own.
        logit_bias / bias_set (a scalar or one set index per sequence; None: set 0; BIAS_NONE: none): every pick sees
        its row as `Context.bias_logits` leaves it with the sequence's set of the `LogitBias` -- banned tokens at -inf, the others of
        the set shifted -- before penalties, DRY and the grammar; log-probs and last logits stay raw.  Greedy with a bias bans and
        prefers tokens without a sampler.  Such a call goes through the options entry point and replays step programs of its own."""
        if any(v is not None for v in (logprobs, grammar, grammar_state, window, dry, no_repeat_ngram, dry_breakers, logit_bias, bias_set)):
            return self._generate_filtered(first_tokens, steps, None, None, None, None, 0.0, 0.0, 1.0, None, None, mode, want_logits, groups,
                                           logprobs, grammar=grammar, grammar_state=grammar_state,
                                           dry_args=(window, dry, no_repeat_ngram, dry_breakers), bias_args=(logit_bias, bias_set))
        return self._generate("greedy", first_tokens, steps, (), mode, groups, want_logits)

    def _generate_options(self, first_tokens, steps, opt, keep, mode, want_logits, logprobs=None):
        """wrk_v*_generate_stop on prepared options: (tokens [steps, B], lengths [B], steps_run, elapsed ms, last logits or None).
        logprobs: the alternatives per row, None for a call without log-probs; sets `last_logprobs`."""
        ft = _u32(first_tokens)
        B = ft.size
        out = np.zeros((steps, B), np.uint32)
        lengths = np.zeros(B, np.uint32)
        run, ms = C.c_uint32(), C.c_float()
        logits = np.empty((B, self.info.num_vocab), np.float32) if want_logits else None
        self.last_logprobs = None
        if logprobs is not None:
            lp, ids, tlp = _logprob_arrays(logprobs, steps * B)
            opt.num_top, opt.out_logprob, opt.out_top_ids, opt.out_top_logprobs = int(logprobs), _ptr(lp, _f32p), _ptr(ids, _u32p), _ptr(tlp, _f32p)
        fn, mdl = self._entry("generate_stop")
        self.ctx.check(fn(self.ctx.h, mdl, self.state, _ptr(ft, _u32p), B, steps, C.byref(opt), _ptr(out, _u32p), _ptr(lengths, _u32p),
                          _ptr(logits, _f32p) if want_logits else None, C.byref(run), C.byref(ms), mode))
        if logprobs is not None:
            n, rows = int(logprobs), run.value * B
            self.last_logprobs = (lp[:rows].reshape(run.value, B), ids[:rows * n].reshape(run.value, B, n),
                                  tlp[:rows * n].reshape(run.value, B, n))
        return out, lengths, run.value, ms.value, logits

    @staticmethod
    def _sampler_rows(B: int, temperature, top_p, seed):
        """(temperature, top_p, seed) [B] and their pointers, as wrk_v*_generate_sample takes them."""
        t, p = _per_row(temperature, B, np.float32), _per_row(top_p, B, np.float32)
        sd = np.arange(B, dtype=np.uint32) if seed is None else _per_row(seed, B, np.uint32)
        return (t, p, sd), (_ptr(t, _f32p), _ptr(p, _f32p), _ptr(sd, _u32p))

    def generate_sample(self, first_tokens, steps: int, temperature=1.0, top_p=0.5, seed=None, mode: int = 1, want_logits: bool = False,
                        groups: int = 1, top_k=None, min_p=None, logprobs=None, mirostat=None, mirostat_mu=None, typical_p=None,
                        grammar: "Grammar" = None, grammar_state=None, window: "TokenWindow" = None, dry=None, no_repeat_ngram=None, dry_breakers=None,
                        logit_bias: "LogitBias" = None, bias_set=None, top_n_sigma=None, epsilon_cutoff=None, eta_cutoff=None, xtc=None):
        """As `generate_greedy`, each sequence's next token drawn by `Sampler::sample` (examples/chat.rs:150-190) on the device with its
        own (temperature, top_p, seed) at step t = 0..steps-1 of this call.  Scalars broadcast; seed=None: seed[b] = b.
        top_k / min_p (a scalar or one value per sequence; None: off): the draw is `sample_logits(..., top_k, min_p)`'s; such a call goes
        through the options entry point (wrk_v*_generate_stop without stop sets) and replays step programs of its own.
        logprobs: as `generate_greedy`; the log-prob of a drawn token is its probability under the model, not under the sampler.
        mirostat=(tau, eta) (scalars or one pair of values per sequence): the draw is Mirostat v2's (`sample_logits(..., mirostat=)`,
        DESIGN.md §7i), mu carried on the device from step to step; mirostat_mu: the mu each sequence starts from (None: 2 tau);
        afterwards `last_mirostat_mu` [B] holds the values to pass to the next call of a session.  typical_p (a scalar or one value per
        sequence): locally typical sampling.  One family per call (top_k / min_p, mirostat, typical_p); such a call goes through the
        options entry point and replays step programs of its own.
        grammar / grammar_state: as `generate_greedy`; the draw is the same sampler's on the masked row.
        window / dry / no_repeat_ngram / dry_breakers: as `generate_greedy`; the draw is the same sampler's on the changed row.
        logit_bias / bias_set: as `generate_greedy`; the draw is the same sampler's on the biased row.
        top_n_sigma / epsilon_cutoff / eta_cutoff / xtc=(probability, threshold) (a scalar or one value per sequence; None: off): the
        cuts of `Context.sample_logits`, made next to top_k / min_p on the row the pick sees; they share that family
        and make the pick a sampled one."""
        if any(v is not None for v in (top_k, min_p, logprobs, mirostat, mirostat_mu, typical_p, grammar, grammar_state, window, dry,
                                       no_repeat_ngram, dry_breakers, logit_bias, bias_set, top_n_sigma, epsilon_cutoff, eta_cutoff, xtc)):
            return self._generate_filtered(first_tokens, steps, temperature, top_p, seed, None, 0.0, 0.0, 1.0, top_k, min_p, mode,
                                           want_logits, groups, logprobs, mirostat, mirostat_mu, typical_p, grammar, grammar_state,
                                           (window, dry, no_repeat_ngram, dry_breakers), (logit_bias, bias_set), (top_n_sigma, epsilon_cutoff, eta_cutoff, xtc))
        keep, rows = self._sampler_rows(_u32(first_tokens).size, temperature, top_p, seed)
        return self._generate("sample", first_tokens, steps, rows, mode, groups, want_logits)

    def _generate_filtered(self, first_tokens, steps, temperature, top_p, seed, occurrence, presence, frequency, decay, top_k, min_p, mode,
                           want_logits, groups, logprobs=None, mirostat=None, mirostat_mu=None, typical_p=None, grammar=None,
                           grammar_state=None, dry_args=(None, None, None, None), bias_args=(None, None), cuts=None):
        opt, keep = GenerateOptions(), []
        mu = _fill_pick(opt, _u32(first_tokens).size, keep, temperature, top_p, seed, occurrence, presence, frequency, decay, top_k, min_p,
                        mirostat, mirostat_mu, typical_p, cuts)
        gs = _fill_grammar(opt, _u32(first_tokens).size, keep, grammar, grammar_state)
        _fill_dry(opt, _u32(first_tokens).size, keep, *dry_args)
        _fill_bias(opt, _u32(first_tokens).size, keep, *bias_args)
        out, _, _, ms, logits = self._generate_options(first_tokens, steps, opt, keep, self._mode(mode, groups), want_logits, logprobs)
        self.last_mirostat_mu = mu
        self.last_grammar_state = gs
        self.last_stop_match = self.last_stop_tail = None
        return (out, ms, logits) if want_logits else (out, ms)

    def generate_penalized(self, first_tokens, steps: int, occurrence: "Occurrence", temperature=1.0, top_p=0.5, seed=None, presence=0.0,
                           frequency=0.0, decay=1.0, mode: int = 1, want_logits: bool = False, groups: int = 1, top_k=None, min_p=None,
                           logprobs=None, mirostat=None, mirostat_mu=None, typical_p=None, grammar: "Grammar" = None, grammar_state=None, window: "TokenWindow" = None, dry=None, no_repeat_ngram=None, dry_breakers=None,
                           logit_bias: "LogitBias" = None, bias_set=None, top_n_sigma=None, epsilon_cutoff=None, eta_cutoff=None, xtc=None):
        """As `generate_sample`, each draw made on the logits penalised with the sequence's slot of `occurrence` (ChatRWKV's
        alpha_presence / alpha_frequency / token_ban), and the slot updated after every draw (count *= decay, then the drawn token's
        weight added).  The first token of a call is not counted; the last drawn one is.  The table carries over between calls.
        Scalars broadcast; seed=None: seed[b] = b.  last logits: the head output before penalties.  top_k / min_p: as `generate_sample`,
        the cuts made on the penalised logits.  logprobs: as `generate_greedy`, on the head output before penalties and bans (a banned
        token may appear among the alternatives).  mirostat / mirostat_mu / typical_p: as `generate_sample`, the pick made on the
        penalised logits.  grammar / grammar_state: as `generate_greedy`, the mask applied to the penalised logits; bans belong in the
        grammar (a row that bans and automaton together leave empty draws an unspecified token, which the automaton rejects).
        window / dry / no_repeat_ngram / dry_breakers: as `generate_greedy`, applied to the penalised logits, before the grammar.
        logit_bias / bias_set: as `generate_greedy`; the penalties are applied to the biased logits: a token is (x + v) - penalty.
        top_n_sigma / epsilon_cutoff / eta_cutoff / xtc: as `generate_sample`, the cuts made on the penalised logits."""
        if any(v is not None for v in (top_k, min_p, logprobs, mirostat, mirostat_mu, typical_p, grammar, grammar_state, window, dry,
                                       no_repeat_ngram, dry_breakers, logit_bias, bias_set, top_n_sigma, epsilon_cutoff, eta_cutoff, xtc)):
            return self._generate_filtered(first_tokens, steps, temperature, top_p, seed, occurrence, presence, frequency, decay, top_k,
                                           min_p, mode, want_logits, groups, logprobs, mirostat, mirostat_mu, typical_p, grammar, grammar_state,
                                           (window, dry, no_repeat_ngram, dry_breakers), (logit_bias, bias_set), (top_n_sigma, epsilon_cutoff, eta_cutoff, xtc))
        B = _u32(first_tokens).size
        keep, rows = self._sampler_rows(B, temperature, top_p, seed)
        pen = [_per_row(v, B, np.float32) for v in (presence, frequency, decay)]
        rows += tuple(_ptr(a, _f32p) for a in pen) + (occurrence.h,)
        return self._generate("penalized", first_tokens, steps, rows, mode, groups, want_logits)

    def generate_stop(self, first_tokens, steps: int, stop, temperature=None, top_p=None, seed=None, occurrence: "Occurrence" = None,
                      presence=0.0, frequency=0.0, decay=1.0, mode: int = 1, want_logits: bool = False, groups: int = 1,
                      poll_steps: int = 0, top_k=None, min_p=None, logprobs=None, mirostat=None, mirostat_mu=None, typical_p=None,
                      grammar: "Grammar" = None, grammar_state=None, stop_sequences=None, stop_tail=None, window: "TokenWindow" = None, dry=None, no_repeat_ngram=None, dry_breakers=None,
                      logit_bias: "LogitBias" = None, bias_set=None, top_n_sigma=None, epsilon_cutoff=None, eta_cutoff=None, xtc=None):
        """`generate_greedy` (no temperature / top_p), `generate_sample`, or with `occurrence` `generate_penalized`, each sequence ending
        at the step that draws one of its stop ids.  stop: one list of ids for all sequences, or one list per sequence (at most
        MAX_STOP_TOKENS each; empty: never ends).  Returns (tokens [steps_run, B], lengths [B][, last logits [B, V]]): tokens[:lengths[b], b]
        are what the call without stops draws, the stop token last; later rows repeat it.  The state slot, the occurrence slot and the
        logits row of a finished sequence are those of a `lengths[b]`-step call.  steps_run < steps once every sequence has ended (the host
        looks every `poll_steps` steps; 0: the default).  top_k / min_p: as `generate_sample` (they make the pick a sampled one).
        logprobs: as `generate_greedy`; rows [:lengths[b], b] of `last_logprobs` are those of the call without stops, the stop token's
        own row included; later rows of a finished sequence are unspecified.
        mirostat / mirostat_mu / typical_p: as `generate_sample`; `last_mirostat_mu[b]` has seen exactly lengths[b] draws, the stop
        token's included.
        grammar / grammar_state: as `generate_greedy`; `last_grammar_state[b]` has seen exactly lengths[b] draws, the stop token's
        included: the state freezes with the sequence.
        stop_sequences (None: off): multi-token stops -- one list of id lists for all sequences, or one such list per
        sequence, at most MAX_STOP_SEQUENCES of 1 .. MAX_STOP_SEQUENCE_LEN ids each (a stop string: one entry per way it tokenizes).  A
        sequence also ends at the draw that completes one of them, with everything frozen as for a stop id; `last_stop_match[b]` is
        STOP_MATCH_NONE, STOP_MATCH_TOKEN or the index of the sequence that matched (the caller trims its length, or 1: the device trims
        nothing).  stop_tail ([B, STOP_TAIL_LEN] from an earlier call's `last_stop_tail`; None: empty): the last draws of the session so
        far, so that a stop sequence that straddles two calls still ends the reply; `last_stop_tail` holds the tails after this call.
        Both are None after a call without stop_sequences, which runs exactly the step programs it ran before.
        window / dry / no_repeat_ngram / dry_breakers: as `generate_greedy`; slot b of the window has taken exactly lengths[b] pushes,
        the stop token's included: the window freezes with the sequence.
        logit_bias / bias_set: as `generate_greedy`; the tokens are a prefix of those of the call without stops.
        top_n_sigma / epsilon_cutoff / eta_cutoff / xtc: as `generate_sample` (they make the pick a sampled one)."""
        ft = _u32(first_tokens)
        ids, off = _stop_csr(stop, ft.size, "sequences")
        opt, keep = GenerateOptions(), []
        if stop_sequences is None and stop_tail is not None:
            raise ValueError("stop_tail without stop_sequences")
        self.last_stop_match = _fill_stop_sequences(opt, ft.size, keep, stop_sequences, "sequences")
        self.last_stop_tail = None
        if stop_sequences is not None:
            self.last_stop_tail = _stop_tails(stop_tail, ft.size)
            opt.stop_tail = _ptr(self.last_stop_tail, _u32p)
        self.last_mirostat_mu = _fill_pick(opt, ft.size, keep, temperature, top_p, seed, occurrence, presence, frequency, decay, top_k, min_p,
                                           mirostat, mirostat_mu, typical_p, (top_n_sigma, epsilon_cutoff, eta_cutoff, xtc))
        self.last_grammar_state = _fill_grammar(opt, ft.size, keep, grammar, grammar_state)
        _fill_dry(opt, ft.size, keep, window, dry, no_repeat_ngram, dry_breakers)
        _fill_bias(opt, ft.size, keep, logit_bias, bias_set)
        opt.stop_tokens, opt.stop_offsets, opt.poll_steps = _ptr(ids, _u32p), _ptr(off, _u32p), poll_steps
        out, lengths, run, self.last_stop_ms, logits = self._generate_options(ft, steps, opt, keep, self._mode(mode, groups), want_logits,
                                                                              logprobs)
        out = out[:run]
        return (out, lengths, logits) if want_logits else (out, lengths)

    def generate_guided(self, first_tokens, steps: int, guidance_scale, negative_first_tokens=None, stop=None, temperature=None, top_p=None,
                        seed=None, occurrence: "Occurrence" = None, presence=0.0, frequency=0.0, decay=1.0, mode: int = 1,
                        want_logits: bool = False, poll_steps: int = 0, top_k=None, min_p=None, logprobs=None, mirostat=None,
                        mirostat_mu=None, typical_p=None, grammar: "Grammar" = None, grammar_state=None, stop_sequences=None, stop_tail=None,
                        window: "TokenWindow" = None, dry=None, no_repeat_ngram=None, dry_breakers=None, logit_bias: "LogitBias" = None,
                        bias_set=None, top_n_sigma=None, epsilon_cutoff=None, eta_cutoff=None, xtc=None):
        """`generate_stop` with classifier-free guidance (a negative prompt).  B = len(first_tokens) sequences run on state
        slots [0, B), and sequence b has a partner on slot B + b, which the caller has fed the negative prompt (`infer` on slots
        [B, 2B)): the state needs 2B slots.  Every step runs both, and the pick of b is made on `Context.guide_logits` of their two
        head rows with guidance_scale[b] (a scalar or one value per sequence, finite and >= 0; 1: the conditional row bit for bit, which
        makes the call the unguided `generate_stop` of the same 2B-sequence frame, columns [0, B) -- a `generate_stop` of B sequences runs
        a smaller frame whose matmuls round differently, so it agrees to rounding, not bit for bit; > 1:
        away from the negative prompt) -- in front of the bias, the penalties, DRY and the grammar, inside the step program.  The
        partner feeds negative_first_tokens[b] at step 0 (None: first_tokens[b]) and then b's draws; it ends and is frozen with b.
        stop (None: no stop ids) and every pick argument: as `generate_stop`, all B wide; log-probs and last logits stay on the raw
        conditional rows.  Returns what `generate_stop` returns.  One lane only."""
        ft = _u32(first_tokens)
        ids, off = _stop_csr(stop, ft.size, "sequences")
        opt, keep = GenerateOptions(), []
        if stop_sequences is None and stop_tail is not None:
            raise ValueError("stop_tail without stop_sequences")
        self.last_stop_match = _fill_stop_sequences(opt, ft.size, keep, stop_sequences, "sequences")
        self.last_stop_tail = None
        if stop_sequences is not None:
            self.last_stop_tail = _stop_tails(stop_tail, ft.size)
            opt.stop_tail = _ptr(self.last_stop_tail, _u32p)
        self.last_mirostat_mu = _fill_pick(opt, ft.size, keep, temperature, top_p, seed, occurrence, presence, frequency, decay, top_k, min_p,
                                           mirostat, mirostat_mu, typical_p, (top_n_sigma, epsilon_cutoff, eta_cutoff, xtc))
        self.last_grammar_state = _fill_grammar(opt, ft.size, keep, grammar, grammar_state)
        _fill_dry(opt, ft.size, keep, window, dry, no_repeat_ngram, dry_breakers)
        _fill_bias(opt, ft.size, keep, logit_bias, bias_set)
        _fill_guidance(opt, ft.size, keep, guidance_scale, negative_first_tokens)
        opt.stop_tokens, opt.stop_offsets, opt.poll_steps = _ptr(ids, _u32p), _ptr(off, _u32p), poll_steps
        out, lengths, run, self.last_stop_ms, logits = self._generate_options(ft, steps, opt, keep, mode, want_logits, logprobs)
        out = out[:run]
        return (out, lengths, logits) if want_logits else (out, lengths)

    def generate_queue(self, requests, stop=None, max_new=16, temperature=None, top_p=None, seed=None, occurrence: "Occurrence" = None,
                       presence=0.0, frequency=0.0, decay=1.0, init_state: "Buffer" = None, max_steps=None, poll_steps: int = 0,
                       mode: int = 1, top_k=None, min_p=None, pool: "StatePool" = None, start_state=None, save_state=None, logprobs=None,
                       mirostat=None, mirostat_mu=None, typical_p=None, grammar: "Grammar" = None, grammar_state=None, stop_sequences=None, window: "TokenWindow" = None, dry=None, no_repeat_ngram=None, dry_breakers=None,
                       count_prompt=None, history: "HistoryPool" = None, logit_bias: "LogitBias" = None, bias_set=None,
                       guidance_scale=None, top_n_sigma=None, epsilon_cutoff=None, eta_cutoff=None, xtc=None):
        """Serves `requests` (one non-empty list of prompt tokens each) on the state's slots in one call: a slot whose request ends is
        reset on the device (to zeros, or to the shared prefix state `init_state` from `state_read`) and takes the next request in the
        same step.  Request r feeds its prompt at decode rate, then draws at most max_new[r] reply tokens, ending at the first one in
        stop[r] (one list for all requests, or one per request).  The pick is one for the call, as in `generate_stop`; per-request
        parameters broadcast from scalars; seed=None: seed[r] = r.  The sampler step of a reply token is its index in the reply, so a
        reply does not depend on when its request was scheduled.  Returns ([(tokens, reason, slot, start_step)] per request, steps_run):
        reason 1 stop token (part of the reply), 2 max_new, 3 cut by max_steps, 0 never dispatched.  max_steps defaults to the sum of
        prompt and max_new lengths, enough even for one slot.  The state and the occurrence rows are unspecified afterwards.
        top_k / min_p: per request (scalars broadcast), as `generate_sample`.
        pool, start_state, save_state: request r begins from a copy of entry start_state[r] of the `StatePool` (None: zeros / init_state)
        and, ending with reason 1 or 2, leaves its final state -- the prompt and the reply but its last token consumed, what
        `generate_stop` freezes -- in entry save_state[r] (None: nowhere).  Each is one value for all requests or a list; the same entry
        for start and save continues a session in place.  `last_queue_saved[r]` tells whether request r's entry was written.  Two
        requests may not save to one entry, nor one read an entry another saves to.
        logprobs (None: off; 0..MAX_TOP_LOGPROBS): `last_logprobs[r]` = (logprob [len], top_ids [len, n], top_logprobs [len, n]) of
        request r's reply tokens, as `generate_greedy`'s; the rows of the steps that feed prompt tokens are discarded.
        mirostat=(tau, eta) / typical_p: per request (scalars broadcast), as `generate_sample`.  mirostat_mu[r] (None: 2 tau[r]) is what
        request r starts from when it is dispatched, whatever its slot held; `last_mirostat_mu[r]` is its mu after its reply draws
        (untouched for reason 0).  mu is not part of a pool entry: a session carries it through these arrays.
        grammar / grammar_state (a scalar or one state per request; None: 0): one `Grammar` for the call; request r starts in
        grammar_state[r] when it is dispatched, whatever its slot held, and only its reply draws move the state (the steps that feed
        prompt tokens do not); `last_grammar_state[r]` is its state after its reply draws (the start state for reason 0).  Requests
        that need different grammars use disjoint state sets of one automaton; the state is not part of a pool entry.
        stop_sequences (None: off): as `generate_stop`, one list of id lists for all requests or one such list per request.  Only reply
        draws are matched: a prompt that is, or ends in the beginning of, a stop sequence does not end its reply, and a refilled slot
        starts with an empty tail.  A match ends the request with reason 1; `last_stop_match[r]` says what ended request r
        (STOP_MATCH_NONE for reasons 0, 2 and 3).  None after a call without stop_sequences.
        window / dry / no_repeat_ngram / dry_breakers: as `generate_greedy`, dry and no_repeat_ngram per request (scalars broadcast), the
        breakers for the call.  Slot b of the window serves whatever request runs on state slot b: it is emptied when a request is
        dispatched to it and takes only that request's reply draws, never prompt tokens.  The window's rows are unspecified afterwards
        and are not part of a pool entry.
        count_prompt (None: off; True: 0 for every request; or one offset f per request): the prompt tokens p_f .. p_{n-1} of request r
        enter its slot's occurrence row (as `Occurrence.add` with decay[r]) and window (as `TokenWindow.add`), on the device, after
        the reset or restore its dispatch makes and before y_0 is picked.  f >= n: none.  A turn that continues a pool entry passes 1:
        its prompt opens with the last reply token, which the entry's history has already counted.  Needs `occurrence` or `window`.
        history: a `HistoryPool` beside `pool`, entry k of it belonging to entry k of the states: a request that starts from entry k
        begins with the entry's occurrence row (the slot's bans kept) and window instead of empty ones, and one that saves to entry k
        (reasons 1 and 2) leaves its slot's row and window there in the step that ends it, its last reply token counted.
        logit_bias / bias_set (a scalar or one set index per request; None: set 0; BIAS_NONE: none): one `LogitBias` for the call;
        request r's rows are biased with set bias_set[r] from the step it is dispatched, whatever its slot's previous request used, so
        two requests of one call may ban different tokens.  The bias is not part of a pool entry.
        guidance_scale: the queue's guidance_scale field; guidance is not built for the queue: anything but None is
        refused with WRK_E_UNSUPPORTED.  Guided requests go through `generate_queue_guided`, guided sequences through `generate_guided`.
        top_n_sigma / epsilon_cutoff / eta_cutoff / xtc=(probability, threshold): per request (scalars broadcast), as `generate_sample`;
        the dispatch writes request r's values into its slot's row, and XTC's coin for reply token j is a function of (seed[r], j) alone,
        so a reply does not depend on when or where its request ran.  Such a call goes through wrk_v*_generate_queue_cut, which takes
        the arrays beside the options, and replays step programs of its own."""
        args = dict(locals())
        del args["self"]
        return self._queue(None, **args)

    def generate_queue_guided(self, requests, negative_prompts, guidance_scale, negative_init_state: "Buffer" = None, stop=None, max_new=16,
                              temperature=None, top_p=None, seed=None, occurrence: "Occurrence" = None, presence=0.0, frequency=0.0,
                              decay=1.0, init_state: "Buffer" = None, max_steps=None, poll_steps: int = 0, mode: int = 1, top_k=None,
                              min_p=None, logprobs=None, mirostat=None, mirostat_mu=None, typical_p=None, grammar: "Grammar" = None,
                              grammar_state=None, stop_sequences=None, window: "TokenWindow" = None, dry=None, no_repeat_ngram=None,
                              dry_breakers=None, count_prompt=None, logit_bias: "LogitBias" = None, bias_set=None, num_slots=None, top_n_sigma=None, epsilon_cutoff=None, eta_cutoff=None, xtc=None):
        """`generate_queue` with classifier-free guidance per request: request r brings the negative prompt
        negative_prompts[r] (None or []: none, an unguided request, only with scale 1) and guidance_scale[r] (a scalar or one value per
        request, finite and >= 0).  The queue has B = num_slots request slots (None: half the state's slots), each a pair of state
        slots: b runs the request and B + b its partner, which takes the negative prompt in at decode rate beside it, both prompts
        ending in the same step; a half that starts late is reset on the device directly in front of its first token (to zeros, or to
        `init_state` / `negative_init_state`, shared prefix states from `state_read`).  Every reply token is picked on
        `Context.guide_logits` of the pair's two head rows with the request's scale, in front of the bias, the penalties, DRY and the
        grammar; log-probs stay on the raw conditional rows.  A refilled pair takes the next request's negative prompt the same way.
        Every other argument, the return value and the `last_*` attributes: as `generate_queue` without a pool; occurrence rows,
        windows and count_prompt see the conditional prompt only.  max_steps defaults to the sum over the requests of the longer of the
        two prompts plus max_new."""
        args = dict(locals())
        for name in ("self", "negative_prompts", "guidance_scale", "negative_init_state", "num_slots"):
            del args[name]
        return self._queue((negative_prompts, guidance_scale, negative_init_state, num_slots), pool=None, start_state=None, save_state=None,
                           history=None, guidance_scale=None, **args)

    def _queue(self, guide, requests, stop, max_new, temperature, top_p, seed, occurrence, presence, frequency, decay, init_state, max_steps,
               poll_steps, mode, top_k, min_p, pool, start_state, save_state, logprobs, mirostat, mirostat_mu, typical_p, grammar, grammar_state,
               stop_sequences, window, dry, no_repeat_ngram, dry_breakers, count_prompt, history, logit_bias, bias_set, guidance_scale,
               top_n_sigma=None, epsilon_cutoff=None, eta_cutoff=None, xtc=None):
        """wrk_v*_generate_queue / _queue_pool / _queue_guided on the arguments of `generate_queue`; guide: None, or (negative_prompts,
        guidance_scale, negative_init_state, num_slots) of `generate_queue_guided`.  With any of the cut arguments the same call goes
        through wrk_v*_generate_queue_cut with the pool or the guidance in its QueueCuts."""
        prompts = [np.asarray(x, np.int64).reshape(-1) for x in requests]
        R = len(prompts)
        B = self.num_batch
        poff = np.zeros(R + 1, np.uint32)
        poff[1:] = np.cumsum([x.size for x in prompts])
        ptok = _u32(np.concatenate(prompts) if R else [])
        ids, soff = _stop_csr(stop, R, "requests")
        if ptok.size == 0:
            ptok = np.zeros(1, np.uint32)
        mn = _per_row(max_new, R, np.uint32)
        opt = QueueOptions()
        opt.num_requests = R
        opt.prompt_tokens, opt.prompt_offsets, opt.max_new = _ptr(ptok, _u32p), _ptr(poff, _u32p), _ptr(mn, _u32p)
        opt.stop_tokens, opt.stop_offsets = _ptr(ids, _u32p), _ptr(soff, _u32p)
        keep = []
        self.last_mirostat_mu = _fill_pick(opt, R, keep, temperature, top_p, seed, occurrence, presence, frequency, decay, top_k, min_p,
                                           mirostat, mirostat_mu, typical_p, (top_n_sigma, epsilon_cutoff, eta_cutoff, xtc))
        cut_ptrs = _cuts((top_n_sigma, epsilon_cutoff, eta_cutoff, xtc), R, keep)
        self.last_grammar_state = _fill_grammar(opt, R, keep, grammar, grammar_state)
        _fill_dry(opt, R, keep, window, dry, no_repeat_ngram, dry_breakers)
        _fill_bias(opt, R, keep, logit_bias, bias_set)
        _fill_guidance(opt, R, keep, guidance_scale)
        match = _fill_stop_sequences(opt, R, keep, stop_sequences, "requests")
        self.last_stop_match = self.last_stop_tail = None
        if init_state is not None:
            opt.init_state = init_state.h
        if count_prompt is not None:
            frm = _per_row(0 if count_prompt is True else count_prompt, R, np.uint32)
            keep.append(frm)
            opt.prompt_context_from = _ptr(frm, _u32p)
        if history is not None:
            opt.history = history.h
        opt.poll_steps = poll_steps
        opt.max_steps = int(poff[-1]) + int(mn.sum()) if max_steps is None else max_steps
        if guide is not None:
            negs, scale, neg_init, num_slots = guide
            if len(negs) != R:
                raise ValueError(f"{len(negs)} negative prompts for {R} requests")
            negs = [np.asarray([] if x is None else x, np.int64).reshape(-1) for x in negs]
            noff = np.zeros(R + 1, np.uint32)
            noff[1:] = np.cumsum([x.size for x in negs])
            ntok = _u32(np.concatenate(negs) if noff[-1] else [0])
            sc = _per_row(scale, R, np.float32) if R else np.ones(1, np.float32)
            qg = QueueGuidance(_ptr(sc, _f32p), _ptr(ntok, _u32p), _ptr(noff, _u32p), neg_init.h if neg_init is not None else None)
            B = self.num_batch // 2 if num_slots is None else int(num_slots)
            if max_steps is None:       # a pair is busy for max(n, m) - 1 + reply steps
                opt.max_steps = int(sum(max(p.size, q.size) for p, q in zip(prompts, negs))) + int(mn.sum())
        lengths, reasons, slots, starts = (np.zeros(max(R, 1), np.uint32) for _ in range(4))
        out = np.zeros(max(int(mn.sum()), 1), np.uint32)
        run, ms = C.c_uint32(), C.c_float()
        res = QueueResult(_ptr(lengths, _u32p), _ptr(reasons, _u32p), _ptr(slots, _u32p), _ptr(starts, _u32p), _ptr(out, _u32p),
                          C.pointer(run))
        self.last_logprobs = None
        if logprobs is not None:
            lp, top_ids, tlp = _logprob_arrays(logprobs, int(mn.sum()))     # `ids` stays alive: opt.stop_tokens points into it
            opt.num_top, opt.out_logprob, opt.out_top_ids, opt.out_top_logprobs = int(logprobs), _ptr(lp, _f32p), _ptr(top_ids, _u32p), _ptr(tlp, _f32p)
        cut_fn = None
        if cut_ptrs is not None:
            cut_fn, mdl = self._entry("generate_queue_cut")
        if guide is not None:
            if cut_fn:
                qc = QueueCuts(*cut_ptrs, None, C.pointer(qg))
                self.ctx.check(cut_fn(self.ctx.h, mdl, self.state, B, C.byref(opt), C.byref(res), C.byref(ms), mode, C.byref(qc)))
            else:
                fn, mdl = self._entry("generate_queue_guided")
                self.ctx.check(fn(self.ctx.h, mdl, self.state, B, C.byref(opt), C.byref(res), C.byref(ms), mode, C.byref(qg)))
            self.last_queue_saved = None
        elif pool is None and cut_fn:
            if start_state is not None or save_state is not None:
                raise ValueError("start_state / save_state need a pool")
            qc = QueueCuts(*cut_ptrs, None, None)
            self.ctx.check(cut_fn(self.ctx.h, mdl, self.state, B, C.byref(opt), C.byref(res), C.byref(ms), mode, C.byref(qc)))
            self.last_queue_saved = None
        elif pool is None:
            if start_state is not None or save_state is not None:
                raise ValueError("start_state / save_state need a pool")
            fn, mdl = self._entry("generate_queue")
            self.ctx.check(fn(self.ctx.h, mdl, self.state, B, C.byref(opt), C.byref(res), C.byref(ms), mode))
            self.last_queue_saved = None
        else:
            def entries(v):
                if v is None or np.isscalar(v):
                    v = [v] * R
                if len(v) != R:
                    raise ValueError(f"{len(v)} pool entries for {R} requests")
                return _u32([QUEUE_NO_ENTRY if k is None else int(k) for k in v]) if R else np.zeros(1, np.uint32)
            st, sv, saved = entries(start_state), entries(save_state), np.zeros(max(R, 1), np.uint32)
            qp = QueuePool(pool.buf.h, pool.entries, _ptr(st, _u32p), _ptr(sv, _u32p), _ptr(saved, _u32p))
            if cut_fn:
                qc = QueueCuts(*cut_ptrs, C.pointer(qp), None)
                self.ctx.check(cut_fn(self.ctx.h, mdl, self.state, B, C.byref(opt), C.byref(res), C.byref(ms), mode, C.byref(qc)))
            else:
                fn, mdl = self._entry("generate_queue_pool")
                self.ctx.check(fn(self.ctx.h, mdl, self.state, B, C.byref(opt), C.byref(res), C.byref(ms), mode, C.byref(qp)))
            self.last_queue_saved = [bool(x) for x in saved[:R]]
        self.last_queue_ms = ms.value
        if match is not None:
            self.last_stop_match = match[:R]
        off = np.concatenate([[0], np.cumsum(mn)]).astype(np.int64)
        if logprobs is not None:
            n = int(logprobs)
            self.last_logprobs = [(lp[off[r]:off[r] + lengths[r]].copy(), top_ids[off[r] * n:(off[r] + lengths[r]) * n].reshape(-1, n).copy(),
                                   tlp[off[r] * n:(off[r] + lengths[r]) * n].reshape(-1, n).copy()) for r in range(R)]
        return [(out[off[r]:off[r] + lengths[r]].copy(), int(reasons[r]), int(slots[r]), int(starts[r])) for r in range(R)], run.value

    def generate_beam(self, first_tokens, steps: int, num_beams: int, stop=None, length_penalty: float = 0.0, logit_bias: "LogitBias" = None,
                      bias_set=None, mode: int = 1, poll_steps: int = 0, guidance_scale=None,
                      occurrence: "Occurrence" = None, presence=0.0, frequency=0.0, decay=1.0,
                      window: "TokenWindow" = None, dry=None, no_repeat_ngram=None, dry_breakers=None,
                      grammar: "Grammar" = None, grammar_state=None):
        """Beam search kept on the device (wrk_v*_generate_beam): G = len(first_tokens) groups of `num_beams` beams on
        state slots [0, G * num_beams); group g starts from the state in slot g * num_beams and feeds first_tokens[g].  Every step
        keeps, per group, the num_beams best of the live beams' continuations and the finished hypotheses, ordered by
        score / length ** length_penalty (score: the f32 sum of the tokens' log-probs), and moves the state slots accordingly, all
        inside the step program.  stop: one list of ids for all groups, or one list per group; a hypothesis that draws one is finished,
        the stop token its last.  logit_bias / bias_set (one set index per group; None: set 0): the beams see the biased row, so a
        banned token is in no hypothesis.  Returns (per group: [(tokens, score, finished, slot)] by rank, steps_run); afterwards state
        slot `slot` holds that hypothesis's state, having consumed everything but its last token.  `last_beam_steps` = (tokens,
        parents, scores), each [steps_run, B]: what every step put in every slot (BEAM_NO_TOKEN: not filled).
        guidance_scale: the `gen` options' guidance_scale field; guidance is not built for beam search: anything but
        None is refused with WRK_E_UNSUPPORTED.
        occurrence / presence / frequency / decay, window / dry / no_repeat_ngram / dry_breakers, grammar / grammar_state (DESIGN.md
        §7u): a context per hypothesis, each value a scalar or one per group.  Slot g * num_beams of the table and the window carries
        the group's context at the start (`occ.add` / `occ.ban` / `win.add`); every beam's row is penalised, DRY-penalised or n-gram
        banned and masked with its own hypothesis's occurrence row, window and automaton state, which move with the hypothesis and
        count the token it was given.  Afterwards slot `slot` of the table and the window holds that hypothesis's context, its last
        token counted, and `last_grammar_state` [B] the automaton state per slot.  With none of them given the call is
        wrk_v*_generate_beam, as before."""
        ft = _u32(first_tokens).reshape(-1)
        G, W, steps = ft.size, int(num_beams), int(steps)
        B = G * max(W, 0)
        ids, off = _stop_csr(stop, G, "groups")
        gen, keep = GenerateOptions(), []
        _fill_bias(gen, G, keep, logit_bias, bias_set)
        _fill_guidance(gen, G, keep, guidance_scale)
        gen.stop_tokens, gen.stop_offsets, gen.poll_steps = _ptr(ids, _u32p), _ptr(off, _u32p), poll_steps
        opt = BeamOptions(max(W, 0), float(length_penalty), C.pointer(gen))
        n = max(B, 1)
        tokens, lengths = np.zeros((n, max(steps, 1)), np.uint32), np.zeros(n, np.uint32)
        scores, finished, slots, hyps = np.zeros(n, np.float32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(max(G, 1), np.uint32)
        st, sp, ss = (np.zeros((max(steps, 1), n), np.uint32), np.zeros((max(steps, 1), n), np.uint32), np.zeros((max(steps, 1), n), np.float32))
        run, ms = C.c_uint32(), C.c_float()
        res = BeamResult(_ptr(tokens, _u32p), _ptr(lengths, _u32p), _ptr(scores, _f32p), _ptr(finished, _u32p), _ptr(slots, _u32p),
                         _ptr(hyps, _u32p), C.pointer(run), _ptr(st, _u32p), _ptr(sp, _u32p), _ptr(ss, _f32p))
        self.last_beam_steps = None
        self.last_grammar_state = None
        if occurrence is None and window is None and grammar is None:
            if dry is not None or no_repeat_ngram is not None or dry_breakers is not None:
                raise ValueError("dry / no_repeat_ngram / dry_breakers without window")
            if grammar_state is not None:
                raise ValueError("grammar_state without grammar")
            fn, mdl = self._entry("generate_beam")
            self.ctx.check(fn(self.ctx.h, mdl, self.state, _ptr(ft, _u32p), G, steps, C.byref(opt), C.byref(res), C.byref(ms), mode & 0xff))
        else:
            bc, gn = BeamContext(), max(G, 1)
            if occurrence is not None:
                keep.extend(_per_row(v, gn, np.float32) for v in (presence, frequency, decay))
                bc.occ, bc.presence, bc.frequency, bc.decay = occurrence.h, *(_ptr(a, _f32p) for a in keep[-3:])
            _fill_dry(bc, gn, keep, window, dry, no_repeat_ngram, dry_breakers)
            _fill_grammar(bc, gn, keep, grammar, grammar_state)
            gs = np.zeros(n, np.uint32)
            if grammar is not None:
                bc.out_grammar_state = _ptr(gs, _u32p)
            fn, mdl = self._entry("generate_beam_context")
            self.ctx.check(fn(self.ctx.h, mdl, self.state, _ptr(ft, _u32p), G, steps, C.byref(opt), C.byref(res), C.byref(ms), mode & 0xff,
                              C.byref(bc)))
            if grammar is not None:
                self.last_grammar_state = gs[:B].copy()
        self.last_beam_ms = ms.value
        r = run.value
        self.last_beam_steps = (st.reshape(-1)[:r * B].reshape(r, B).copy(), sp.reshape(-1)[:r * B].reshape(r, B).copy(),
                                ss.reshape(-1)[:r * B].reshape(r, B).copy())
        out = []
        for g in range(G):
            out.append([(tokens[g * W + k, :lengths[g * W + k]].copy(), float(scores[g * W + k]), bool(finished[g * W + k]), int(slots[g * W + k]))
                        for k in range(int(hyps[g]))])
        return out, r

    def state_permute(self, parents):
        """State slot q <- state slot parents[q] for q < len(parents), on the device and correct under any aliasing (swaps, chains,
        many-to-one); slots with parents[q] == q move no bytes and slots >= len(parents) are untouched (wrk_v7_state_permute)."""
        p = _u32(parents).reshape(-1)
        self.ctx.check(hip.wrk_v7_state_permute(self.ctx.h, self.state, _ptr(p, _u32p), p.size))

    def state_back(self, batch: int) -> np.ndarray:
        """`State::back(batch)` -> [L, S+2, D] f32."""
        L, D, S = self.info.num_layer, self.info.num_emb, self.info.num_emb // self.info.num_head
        out = np.empty((L, S + 2, D), np.float32)
        self.ctx.check(hip.wrk_v7_state_back(self.ctx.h, self.state, batch, _ptr(out, _f32p)))
        return out

    def state_read(self, batch: int) -> "Buffer":
        """`State::read(batch)` (v7.rs:246-262): a device-resident snapshot [L, S+2, D] f32 (no host round trip)."""
        L, D, S = self.info.num_layer, self.info.num_emb, self.info.num_emb // self.info.num_head
        buf = Buffer(self.ctx, L * (S + 2) * D * 4)
        self.ctx.check(hip.wrk_v7_state_read(self.ctx.h, self.state, batch, buf.h))
        return buf

    def state_write(self, snapshot: "Buffer", batch: int):
        """`State::write(tensor, batch)` (v7.rs:229-244)."""
        self.ctx.check(hip.wrk_v7_state_write(self.ctx.h, self.state, batch, snapshot.h))

    def state_load(self, tensor: np.ndarray, batch: int):
        a = np.ascontiguousarray(tensor, dtype=np.float32)
        L, D, S = self.info.num_layer, self.info.num_emb, self.info.num_emb // self.info.num_head
        assert a.shape == (L, S + 2, D)
        self.ctx.check(hip.wrk_v7_state_load(self.ctx.h, self.state, batch, _ptr(a, _f32p)))

    def close(self):
        if self.h:
            rt.wrk_runtime_destroy(self.h)
            self.h = None


class StatePool:
    """The state pool of `Runtime.generate_queue(pool=...)`: `entries` states of `runtime`'s model in one device buffer, entry k in
    `state_read`'s layout [L, S+2, D] f32 (multi-session serving keeps its snapshots in HBM, v7.rs:229-262).  Entries start as zeros."""

    def __init__(self, ctx: Context, runtime: Runtime, entries: int):
        L, D, S = runtime.info.num_layer, runtime.info.num_emb, runtime.info.num_emb // runtime.info.num_head
        self.ctx, self.entries, self.shape, self.entry_bytes = ctx, entries, (L, S + 2, D), L * (S + 2) * D * 4
        self.buf = Buffer(ctx, entries * self.entry_bytes, np.zeros(entries * L * (S + 2) * D, np.float32))

    def _at(self, k: int) -> int:
        if not 0 <= k < self.entries:
            raise IndexError(f"entry {k} of {self.entries}")
        return k * self.entry_bytes

    def put(self, k: int, snapshot: Buffer):
        """entry k <- a `state_read` snapshot (device to device)"""
        self.ctx.check(hip.wrk_buf_copy(self.ctx.h, snapshot.h, 0, self.buf.h, self._at(k), self.entry_bytes))

    def get(self, k: int) -> Buffer:
        """a snapshot of entry k for `state_write` / `init_state` (device to device)"""
        out = Buffer(self.ctx, self.entry_bytes)
        self.ctx.check(hip.wrk_buf_copy(self.ctx.h, self.buf.h, self._at(k), out.h, 0, self.entry_bytes))
        return out

    def load(self, k: int, tensor: np.ndarray):
        a = np.ascontiguousarray(tensor, dtype=np.float32)
        assert a.shape == self.shape
        self.buf.write(a, self._at(k))

    def back(self, k: int) -> np.ndarray:
        return self.buf.read(np.float32, self.entry_bytes // 4, self._at(k)).reshape(self.shape)

    def close(self):
        self.buf = None


class HistoryPool:
    """The history pool of `Runtime.generate_queue(pool=..., history=...)`: `entries` entries on the device, entry k beside entry k of
    the `StatePool`.  An entry holds what a slot of an `Occurrence` and of a `TokenWindow` hold -- counts, the present bit per token
    and, with window_capacity > 0, the last window_capacity tokens that counted -- but no banned bits: those stay the slot's.
    Entries start empty."""

    def __init__(self, ctx: Context, entries: int, num_vocab: int, window_capacity: int = 0):
        self.ctx, self.entries, self.num_vocab, self.capacity = ctx, entries, num_vocab, window_capacity
        h = _P()
        ctx.check(hip.wrk_history_pool_create(ctx.h, entries, num_vocab, window_capacity, C.byref(h)))
        self.h = h

    def load(self, k: int, counts=None, present=None, tokens=None):
        """entry k <- counts / present (both or neither: an empty row) and tokens, oldest first (None: an empty window)"""
        c = None if counts is None else np.ascontiguousarray(counts, np.float32)
        f = None if present is None else _u32(present)
        if (c is not None and c.size != self.num_vocab) or (f is not None and f.size != self.num_vocab):
            raise ValueError(f"counts / present of an entry hold {self.num_vocab} values")
        t = None if tokens is None else _u32(tokens).reshape(-1)
        self.ctx.check(hip.wrk_history_pool_load(self.ctx.h, self.h, k, None if c is None else _ptr(c, _f32p), None if f is None else _ptr(f, _u32p),
                                                 None if t is None or t.size == 0 else _ptr(t, _u32p), 0 if t is None else t.size))

    def back(self, k: int):
        """(counts f32 [V], present u32 [V], the window's tokens oldest first) of entry k"""
        c, f = np.empty(self.num_vocab, np.float32), np.empty(self.num_vocab, np.uint32)
        t, n = np.zeros(max(self.capacity, 1), np.uint32), C.c_uint32()
        self.ctx.check(hip.wrk_history_pool_back(self.ctx.h, self.h, k, _ptr(c, _f32p), _ptr(f, _u32p), _ptr(t, _u32p), C.byref(n)))
        return c, f, t[:n.value].copy()

    def put(self, k: int, occurrence: "Occurrence" = None, batch: int = 0, window: "TokenWindow" = None):
        """entry k <- slot `batch` of the occurrence table (the present bit only) and of the window, device to device"""
        self.ctx.check(hip.wrk_history_pool_put(self.ctx.h, self.h, k, occurrence.h if occurrence is not None else None, batch,
                                                window.h if window is not None else None))

    def get(self, k: int, occurrence: "Occurrence" = None, batch: int = 0, window: "TokenWindow" = None):
        """slot `batch` of the occurrence table and of the window <- entry k, device to device; the slot keeps its banned bits"""
        self.ctx.check(hip.wrk_history_pool_get(self.ctx.h, self.h, k, occurrence.h if occurrence is not None else None, batch,
                                                window.h if window is not None else None))

    def close(self):
        if self.h and self.ctx.h:
            hip.wrk_history_pool_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
