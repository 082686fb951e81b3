"""ctypes binding of include/mocr.h (libmocr_hip.so).  No fallback: if the library or a GPU is
missing, importing works but constructing an engine raises."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libmocr_hip.so")

MOCR_OK = 0
MOCR_F32, MOCR_BF16 = 0, 1
FLAG_SIMPLE_ATTENTION, FLAG_NO_GRAPH, FLAG_NO_EARLY_EXIT, FLAG_CLASSIC_ATTENTION = 1, 2, 4, 8
FLAG_NO_FUSED_ARGMAX, FLAG_NO_FUSED_QQT, FLAG_LATENT_ALWAYS, FLAG_FP8_ATTENTION = 16, 32, 64, 128
FLAG_NO_SMALL_BATCH_PATH = 256
FLAG_NO_LN_FOLD = 512
EPI_SLAB, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_PATCH, EPI_BIAS_F32 = range(6)


class MocrConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "struct_size", "device", "dtype", "max_batch", "max_len", "image_size", "patch_size", "hidden",
        "enc_layers", "dec_layers", "heads", "ffn", "vocab", "max_pos", "start_id", "eos_id", "pad_id")] + \
        [("ln_eps", C.c_float), ("flags", C.c_int32), ("lanes", C.c_int32)]


class MocrKernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("total_ms", C.c_double),
                ("flops", C.c_double), ("bytes", C.c_double)]


# every symbol include/mocr.h declares: name -> (restype, argtypes)
_P = C.c_void_p
class MocrImage(C.Structure):
    """include/mocr.h: mocr_image"""
    _fields_ = [("data", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32), ("row_stride", C.c_int64),
                ("channels", C.c_int32), ("rotate", C.c_int32)]


class MocrRegion(C.Structure):
    """include/mocr.h: mocr_region"""
    _fields_ = [(n, C.c_int32) for n in ("page", "x", "y", "width", "height")]


class MocrTokenArgs(C.Structure):
    """include/mocr.h: mocr_token_args"""
    _fields_ = [("struct_size", C.c_int32), ("first", C.c_int32), ("n", C.c_int32), ("nslab", C.c_int32),
                ("slabs", C.c_void_p), ("vbias", C.c_void_p), ("cand_val", C.c_void_p), ("cand_idx", C.c_void_p),
                ("ncand", C.c_int32), ("forced_T", C.c_int32), ("forced", C.c_void_p), ("ids", C.c_void_p),
                ("step", C.c_void_p), ("finished", C.c_void_p), ("len", C.c_void_p), ("n_unfinished", C.c_void_p),
                ("rowmap", C.c_void_p), ("ids_ld", C.c_int32), ("max_len", C.c_int32), ("n_real", C.c_int32),
                ("cache_fp8", C.c_int32), ("x_f32", C.c_void_p), ("x_t", C.c_void_p), ("cache", C.c_void_p),
                ("inv_sx", C.c_float)]


class MocrSmallmArgs(C.Structure):
    """include/mocr.h: mocr_smallm_args"""
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "pro", "epi", "rows", "K", "N", "ldo")] + \
        [(n, C.c_void_p) for n in ("a_bf16", "a_f32", "ln_g", "ln_b", "stats_out", "w", "bias", "resid", "resid_stats",
                                   "resid_g", "resid_b", "out")]


class MocrGemmArgs(C.Structure):
    """include/mocr.h: mocr_gemm_args"""
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "M", "N", "K", "epilogue", "tile", "split_k", "lda", "ldo", "group_n")] + \
        [("slab_stride", C.c_int64)] + [(n, C.c_void_p) for n in ("A", "W", "bias", "out", "resid")]


class MocrGemmPersArgs(C.Structure):
    """include/mocr.h: mocr_gemm_pers_args"""
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "M", "N", "K", "epilogue", "tile", "group_n")] + \
        [(n, C.c_void_p) for n in ("A", "W", "bias", "out", "resid", "ln_part", "csum", "xb")]


DECODE_PLAN_FIELDS = 25   # MOCR_DECODE_PLAN_FIELDS


class MocrLatentArgs(C.Structure):
    """include/mocr.h: mocr_latent_args"""
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "self", "n", "regime_rows", "fixed_len")] + \
        [(n, C.c_void_p) for n in ("x_in", "wq", "bq", "wkT", "wv", "bv", "keys")] + \
        [("key_stride", C.c_int64), ("step", C.c_void_p), ("rowmap", C.c_void_p), ("sx", C.c_float)] + \
        [(n, C.c_void_p) for n in ("q", "qt", "et", "ctx")]


class MocrBeamConfig(C.Structure):
    """include/mocr.h: mocr_beam_config"""
    _fields_ = [("num_beams", C.c_int32), ("length_penalty", C.c_float), ("early_stopping", C.c_int32),
                ("no_repeat_ngram_size", C.c_int32)]


class MocrAutomatonDesc(C.Structure):
    """include/mocr.h: mocr_automaton_desc"""
    _fields_ = [("struct_size", C.c_int32), ("n_states", C.c_int32), ("edge_begin", C.c_void_p), ("edge_token", C.c_void_p),
                ("edge_next", C.c_void_p), ("accepting", C.c_void_p)]


class MocrSoftAutomatonDesc(C.Structure):
    """include/mocr.h: mocr_automaton_desc with its two trailing fields (soft token automata); MocrAutomatonDesc is the
    struct as it was before it grew, which the library still takes"""
    _fields_ = MocrAutomatonDesc._fields_ + [("edge_weight", C.c_void_p), ("default_next", C.c_void_p)]


class MocrSoftTables(C.Structure):
    """include/mocr.h: mocr_soft_tables"""
    _fields_ = [("struct_size", C.c_int32), ("d_aut_state", C.c_void_p), ("d_edge_begin", C.c_void_p), ("d_edge_token", C.c_void_p),
                ("d_edge_weight", C.c_void_p)]


MAX_AUTOMATA = 256                    # MOCR_MAX_AUTOMATA
MAX_AUTOMATON_STATES = 1 << 20        # MOCR_MAX_AUTOMATON_STATES: over all automata of an engine
MAX_AUTOMATON_EDGES = 1 << 22         # MOCR_MAX_AUTOMATON_EDGES
AUTOMATON_NONE = 0                    # MOCR_AUTOMATON_NONE
STATE_NONE, STATE_DEAD = -1, -2       # MOCR_STATE_NONE, MOCR_STATE_DEAD
MAX_BEAMS = 4             # MOCR_MAX_BEAMS
CHANNELS_BGR = -3
MAX_TOKEN_SETS = 256      # MOCR_MAX_TOKEN_SETS: token sets per engine, set 0 included
TOKEN_SET_ALL = 0         # MOCR_TOKEN_SET_ALL: the whole vocabulary
ALTERNATIVES = 4          # MOCR_ALTERNATIVES: candidates per position of the *_alts entry points
POSITION_FIELDS = 5       # MOCR_POSITION_FIELDS: cx, cy, sx, sy, mass per position of the *_positions entry points
ROTATE_NONE, ROTATE_90_CW, ROTATE_90_CCW = 0, 1, 2

SYMBOLS = {
    "mocr_abi_version": (C.c_int, []),
    "mocr_create": (C.c_int, [C.POINTER(MocrConfig), C.POINTER(_P)]),
    "mocr_destroy": (None, [_P]),
    "mocr_last_error": (C.c_char_p, [_P]),
    "mocr_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int32]),
    "mocr_commit_weights": (C.c_int, [_P]),
    "mocr_recognize": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, _P, _P]),
    "mocr_recognize_images": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, _P, _P]),
    "mocr_recognize_regions": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrRegion), C.c_int32, _P, _P]),
    "mocr_recognize_images_scored": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, _P, _P, _P]),
    "mocr_recognize_regions_scored": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrRegion), C.c_int32, _P, _P, _P]),
    "mocr_recognize_device_scored": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P]),
    "mocr_recognize_gray_host_scored": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "mocr_recognize_images_alts": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, _P, _P, _P, _P, _P]),
    "mocr_recognize_regions_alts": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrRegion), C.c_int32, _P, _P, _P, _P, _P]),
    "mocr_recognize_device_alts": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, _P]),
    "mocr_recognize_gray_host_alts": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    "mocr_token_set_create": (C.c_int, [_P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    "mocr_token_set_count": (C.c_int, [_P]),
    "mocr_recognize_images_constrained": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_regions_constrained": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrRegion), C.c_int32, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_device_constrained": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_gray_host_constrained": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_images_norepeat": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_regions_norepeat": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrRegion), C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_device_norepeat": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_gray_host_norepeat": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_images_positions": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_regions_positions": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrRegion), C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_device_positions": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_gray_host_positions": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_images_prefix": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32]),
    "mocr_recognize_regions_prefix": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrRegion), C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P,
                                                _P, _P, C.c_int32]),
    "mocr_recognize_device_prefix": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32]),
    "mocr_recognize_gray_host_prefix": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32]),
    "mocr_recognize_images_shared": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                               C.c_int32]),
    "mocr_recognize_regions_shared": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrRegion), C.c_int32, C.c_int32, _P, _P, _P,
                                                _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32]),
    "mocr_recognize_device_shared": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32]),
    "mocr_recognize_gray_host_shared": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                                  C.c_int32]),
    "mocr_encoded_crops": (C.c_int64, [_P]),
    "mocr_automaton_create": (C.c_int, [_P, C.POINTER(MocrAutomatonDesc), C.POINTER(C.c_int32)]),
    "mocr_automaton_count": (C.c_int, [_P]),
    "mocr_automaton_state_bytes": (C.c_int64, [_P]),
    "mocr_recognize_images_automaton": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                                  C.c_int32, _P, _P]),
    "mocr_recognize_regions_automaton": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrRegion), C.c_int32, C.c_int32, _P, _P, _P,
                                                   _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P, _P]),
    "mocr_recognize_device_automaton": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P, _P]),
    "mocr_recognize_gray_host_automaton": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                                     C.c_int32, _P, _P]),
    "mocr_op_dec_token_automaton": (C.c_int, [_P, C.POINTER(MocrTokenArgs), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P,
                                              _P, _P, _P, _P, _P, _P]),
    "mocr_op_automaton_init": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, _P, _P, _P, _P]),
    "mocr_op_dec_token_soft": (C.c_int, [_P, C.POINTER(MocrTokenArgs), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P,
                                         _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_op_automaton_init_soft": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "mocr_op_gemm_argmax_soft": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P,
                                           C.c_int32, _P, _P, C.POINTER(MocrSoftTables)]),
    "mocr_recognize_images_penalty": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                                C.c_int32, _P, _P, _P]),
    "mocr_recognize_regions_penalty": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrRegion), C.c_int32, C.c_int32, _P, _P, _P,
                                                 _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P, _P, _P]),
    "mocr_recognize_device_penalty": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P, _P, _P]),
    "mocr_recognize_gray_host_penalty": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                                   C.c_int32, _P, _P, _P]),
    "mocr_op_dec_token_penalty": (C.c_int, [_P, C.POINTER(MocrTokenArgs), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P,
                                            _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_op_penalty_init": (C.c_int, [_P, _P, C.c_int32]),
    "mocr_op_gemm_argmax_penalty": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P,
                                              C.c_int32, _P, _P, C.POINTER(MocrSoftTables), _P, _P]),
    "mocr_op_enc_expand": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32]),
    "mocr_graph_count": (C.c_int, [_P]),
    "mocr_compaction_count": (C.c_int64, [_P]),
    "mocr_decode_slot_steps": (C.c_int64, [_P]),
    "mocr_ln_fold_state": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "mocr_device_memory": (C.c_int, [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mocr_preprocess": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, _P]),
    "mocr_recognize_device": (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    "mocr_set_generate_max_length": (C.c_int, [_P, C.c_int32]),
    "mocr_synchronize": (C.c_int, [_P]),
    "mocr_stream": (_P, [_P]),
    "mocr_encode": (C.c_int, [_P, _P, C.c_int32, _P]),
    "mocr_decode_logits": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P]),
    "mocr_recognize_gray_host": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    "mocr_op_gemm": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mocr_op_layernorm": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32]),
    "mocr_op_gemm_ln": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "mocr_op_ln_prep": (C.c_int, [_P, _P, _P, _P, C.c_int32]),
    "mocr_op_enc_attention": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32]),
    "mocr_op_embed": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    "mocr_op_layernorm_slab": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int64, _P, _P, _P, _P, C.c_int32]),
    "mocr_encoder_plan": (C.c_int, [_P, C.c_int32, _P]),
    "mocr_decode_plan": (C.c_int, [_P, C.c_int32, C.c_int32, _P]),
    "mocr_op_gemm_args": (C.c_int, [_P, C.POINTER(MocrGemmArgs)]),
    "mocr_last_tile_launch": (C.c_int, [_P, _P]),
    "mocr_encoder_groups": (C.c_int, [_P, C.c_int32, _P]),
    "mocr_op_gemm_pers": (C.c_int, [_P, C.POINTER(MocrGemmPersArgs)]),
    "mocr_last_pers_launch": (C.c_int, [_P, _P]),
    "mocr_op_latent_attention": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int64]),
    "mocr_op_quant_fp8": (C.c_int, [_P, _P, _P, C.c_int64, C.c_float]),
    "mocr_op_latent_attention_fp8": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int64, C.c_float]),
    "mocr_op_qqt": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32]),
    "mocr_op_dec_attn": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32]),
    "mocr_op_dec_add_ln": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P, C.c_int32, C.c_float, _P, _P]),
    "mocr_op_dec_bias_gelu": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32]),
    "mocr_op_dec_token": (C.c_int, [_P, C.POINTER(MocrTokenArgs)]),
    "mocr_op_gemm_argmax": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mocr_op_dec_token_scored": (C.c_int, [_P, C.POINTER(MocrTokenArgs), _P, _P]),
    "mocr_op_gemm_argmax_lse": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mocr_op_dec_token_topk": (C.c_int, [_P, C.POINTER(MocrTokenArgs), _P, _P, _P, _P, _P, _P]),
    "mocr_op_gemm_topk": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mocr_op_dec_token_masked": (C.c_int, [_P, C.POINTER(MocrTokenArgs), _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_op_dec_token_ngram": (C.c_int, [_P, C.POINTER(MocrTokenArgs), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_op_dec_token_prefix": (C.c_int, [_P, C.POINTER(MocrTokenArgs), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P]),
    "mocr_op_ngram_init": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32]),
    "mocr_op_attn_positions": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    "mocr_op_gemm_argmax_masked": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "mocr_op_gemm_argmax_target": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P,
                                             _P, _P, C.c_int32, _P, _P]),
    "mocr_op_smallm_gemm": (C.c_int, [_P, C.POINTER(MocrSmallmArgs)]),
    "mocr_op_latent_block": (C.c_int, [_P, C.POINTER(MocrLatentArgs)]),
    "mocr_recognize_images_beam": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrBeamConfig), _P, _P, _P]),
    "mocr_recognize_regions_beam": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrRegion), C.c_int32,
                                              C.POINTER(MocrBeamConfig), _P, _P, _P]),
    "mocr_recognize_gray_host_beam": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(MocrBeamConfig), _P, _P, _P]),
    "mocr_recognize_device_beam": (C.c_int, [_P, _P, C.c_int32, C.POINTER(MocrBeamConfig), _P, _P, _P]),
    "mocr_recognize_images_beam_tokens": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P]),
    "mocr_recognize_regions_beam_tokens": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrRegion), C.c_int32,
                                                     C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P]),
    "mocr_recognize_gray_host_beam_tokens": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P]),
    "mocr_recognize_device_beam_tokens": (C.c_int, [_P, _P, C.c_int32, C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P]),
    "mocr_recognize_images_beam_positions": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_regions_beam_positions": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrRegion), C.c_int32,
                                                        C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_gray_host_beam_positions": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_device_beam_positions": (C.c_int, [_P, _P, C.c_int32, C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_images_beam_automaton": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P,
                                                       _P, _P]),
    "mocr_recognize_regions_beam_automaton": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrRegion), C.c_int32,
                                                        C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_gray_host_beam_automaton": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P,
                                                          _P, _P]),
    "mocr_recognize_device_beam_automaton": (C.c_int, [_P, _P, C.c_int32, C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_op_beam_select_automaton": (C.c_int, [_P, C.POINTER(MocrTokenArgs), C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                                _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_images_beam_soft": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_regions_beam_soft": (C.c_int, [_P, C.POINTER(MocrImage), C.c_int32, C.POINTER(MocrRegion), C.c_int32,
                                                   C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_gray_host_beam_soft": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_recognize_device_beam_soft": (C.c_int, [_P, _P, C.c_int32, C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_op_beam_select_soft": (C.c_int, [_P, C.POINTER(MocrTokenArgs), C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                           _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_beam_state_bytes": (C.c_int64, [_P]),
    "mocr_beam_token_state_bytes": (C.c_int64, [_P]),
    "mocr_beam_position_state_bytes": (C.c_int64, [_P]),
    "mocr_op_beam_select_positions": (C.c_int, [_P, C.POINTER(MocrTokenArgs), C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                                _P, _P]),
    "mocr_op_attn_positions_gathered": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32]),
    "mocr_lane_rowmap": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "mocr_op_beam_select": (C.c_int, [_P, C.POINTER(MocrTokenArgs), C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P]),
    "mocr_op_beam_select_tokens": (C.c_int, [_P, C.POINTER(MocrTokenArgs), C.POINTER(MocrBeamConfig), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mocr_op_beam_permute": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P,
                                       C.c_int32, C.c_int32]),
    "mocr_profile_enable": (C.c_int, [_P, C.c_int32]),
    "mocr_profile_reset": (C.c_int, [_P]),
    "mocr_profile_get": (C.c_int, [_P, C.POINTER(MocrKernelStat), C.c_int32, C.POINTER(C.c_int32)]),
}

_lib: Optional[C.CDLL] = None


class MocrError(RuntimeError):
    pass


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen libmocr_hip.so and bind every declared symbol (raises if one is missing)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("MOCR_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise MocrError(f"{p} not found: build it with `python manga-ocr_amd/build.py` "
                        "(the Manga-OCR engine has no CPU fallback)")
    lib = C.CDLL(p)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)     # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.mocr_abi_version() != 2:
        raise MocrError("libmocr_hip.so ABI version mismatch")
    if path is None:
        _lib = lib
    return lib
