"""ctypes binding of libf5hip.so (C ABI: include/f5hip.h).  Fails loudly when the library or the GPU is missing."""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must be imported first: libf5hip resolves libamdhip64.so.7 to the runtime torch already loaded)

_HERE = os.path.dirname(os.path.abspath(__file__))
# (F5HIP_LIB: developer override, another in-tree build of the library for same-box A/B runs of two builds)
LIB_PATH = os.environ.get("F5HIP_LIB") or os.path.join(_HERE, "lib", "libf5hip.so")

F5_PREC_BF16, F5_PREC_FP32, F5_PREC_FP16 = 0, 1, 2
# precision names of DiT(precision=...) / F5TTSWrapper(precision=...) / F5HIP_PRECISION (include/f5hip.h: F5_PREC_*)
PRECISIONS = {"bf16": F5_PREC_BF16, "fp32": F5_PREC_FP32, "fp16": F5_PREC_FP16}
F5_ODE_EULER, F5_ODE_MIDPOINT, F5_ODE_RK4, F5_ODE_HEUN2, F5_ODE_HEUN3 = 0, 1, 2, 3, 4
# odeint_kwargs["method"] -> F5_ODE_* (torchdiffeq's fixed-grid names; f5_ode_evals_per_step gives the evaluations per step)
ODE_METHODS = {"euler": F5_ODE_EULER, "midpoint": F5_ODE_MIDPOINT, "rk4": F5_ODE_RK4, "heun2": F5_ODE_HEUN2, "heun3": F5_ODE_HEUN3}
F5_ROPE_ADJACENT, F5_ROPE_HALF_SPLIT = 0, 1
F5_BACKBONE_DIT, F5_BACKBONE_UNETT, F5_BACKBONE_MMDIT = 0, 1, 2
F5_SKIP = {"concat": 0, "add": 1, "none": 2}
SITES = ("qkv", "attention", "attn_out", "ff1", "ff2", "ln1", "ln2", "conv31", "input_proj")  # F5_SITE_* order
F5_MEL_VOCOS, F5_MEL_BIGVGAN = 0, 1
ACT = {"none": 0, "gelu_tanh": 1, "gelu_erf": 2, "mish": 3}


class F5HipError(RuntimeError):
    pass


class DitConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dim", "depth", "heads", "dim_head", "ff_inner", "mel_dim", "text_num_embeds", "text_dim",
                                         "conv_layers", "text_mask_padding", "pe_attn_head", "qk_norm", "long_skip", "precision", "rope_layout",
                                         "backbone", "skip_connect")]


class VocosConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_mels", "dim", "inter_dim", "layers", "n_fft", "hop")]


class BigVGANConfig(C.Structure):  # struct f5_bigvgan_config
    _fields_ = [("num_mels", C.c_int32), ("upsample_initial_channel", C.c_int32), ("num_upsamples", C.c_int32), ("upsample_rates", C.c_int32 * 8),
                ("upsample_kernel_sizes", C.c_int32 * 8), ("num_kernels", C.c_int32), ("resblock_kernel_sizes", C.c_int32 * 4),
                ("resblock_dilations", (C.c_int32 * 3) * 4), ("snake_logscale", C.c_int32), ("use_tanh_at_final", C.c_int32),
                ("use_bias_at_final", C.c_int32)]


class SpeakerConfig(C.Structure):  # struct f5_speaker_config
    _fields_ = [(n, C.c_int32) for n in ("feat_dim", "channels", "emb_dim", "layers", "cat_channels", "se_bottleneck", "attention_channels", "scale")]


class WavLMConfig(C.Structure):  # struct f5_wavlm_config
    _fields_ = [("num_conv_layers", C.c_int32), ("conv_dim", C.c_int32 * 8), ("conv_kernel", C.c_int32 * 8), ("conv_stride", C.c_int32 * 8)] + \
               [(n, C.c_int32) for n in ("conv_bias", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size",
                                         "num_conv_pos_embeddings", "num_conv_pos_embedding_groups", "num_buckets", "max_bucket_distance",
                                         "feat_extract_norm", "do_stable_layer_norm", "add_adapter", "normalize_input")] + [("layer_norm_eps", C.c_float)]


class MelConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_fft", "hop", "win", "n_mels", "sample_rate", "mel_type")]


class DurationWeights(C.Structure):  # struct f5_duration_weights
    _fields_ = [(n, C.c_void_p) for n in ("text_embed", "conv1_w", "conv1_b", "norm1_w", "norm1_b", "conv2_w", "conv2_b", "norm2_w", "norm2_b",
                                          "proj_w", "proj_b")] + [(n, C.c_int32) for n in ("vocab_rows", "in_channels", "filter_channels", "kernel_size")] + \
               [("cond_w", C.c_void_p), ("cond_b", C.c_void_p), ("gin_channels", C.c_int32)]


class TileGemm(C.Structure):  # struct f5_tile_gemm (f5_op_tile_gemm: the reference tile kernel, test hook)
    _fields_ = [(n, C.c_void_p) for n in ("A", "W", "bias", "gate", "rope", "addend", "rowmask", "out_t", "out_f")] + \
               [(n, C.c_int32) for n in ("precision", "mode", "epi", "M", "N", "K", "a_row_mod", "act", "gate_bstride", "rows_per_batch", "rope_heads",
                                         "ldadd", "add2_f16", "ldo", "ldof", "out_rows")]


class ReferenceRule(C.Structure):  # struct f5_reference_rule
    _fields_ = [(n, C.c_int32) for n in ("clip_short", "min_silence_len_1", "threshold_floor_1", "min_silence_len_2", "threshold_floor_2",
                                         "keep_silence", "seek_step", "soft_limit_ms", "hard_limit_ms", "r_lead", "r_trail", "lead_chunk_ms",
                                         "pad_ms")] + [("target_rms", C.c_float)]


# f5_reference_*: the words of counts_dev (include/f5hip.h: F5_REF_*)
REF_WORDS = ("kept", "parts", "clip", "lead_ms", "trail_ms", "sumsq", "boost", "gathered", "gathered_ms", "lead_frame", "edge_frames", "edge_ms",
             "out_frames", "rms_bits", "pass2")
F5_REF_WORDS = 16

_P, _I, _F = C.c_void_p, C.c_int, C.c_float
_PROTOS = {
    "f5_last_error": (C.c_char_p, []),
    "f5_version": (_I, []),
    "f5_device_count": (_I, [C.c_char_p]),
    "f5_model_create": (_I, [C.POINTER(DitConfig), C.POINTER(_P)]),
    "f5_model_set_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _I]),
    "f5_model_has_tensor": (_I, [_P, C.c_char_p, C.POINTER(C.c_int64)]),
    "f5_model_finalize": (_I, [_P]),
    "f5_model_destroy": (_I, [_P]),
    "f5_plan_create": (_I, [_P, _I, _I, _I, C.POINTER(_P)]),
    "f5_plan_destroy": (_I, [_P]),
    "f5_plan_workspace_bytes": (C.c_int64, [_P]),
    "f5_ode_evals_per_step": (_I, [_I]),
    "f5_sample": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _P, _P, _I, _F, _I, _P, _P, _I, _P]),
    "f5_sample_masked": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _P, _P, _I, _F, _I, _P, _P, _P, _I, _P]),
    "f5_sample_finish": (_I, [_P, _P]),
    "f5_text_embed": (_I, [_P, _I, _I, _P, _I, _I, _P, _P]),
    "f5_dit_forward": (_I, [_P, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    "f5_sample_ragged": (_I, [_P, _I, _P, _P, _P, _I, _P, _P, _P, _I, C.c_float, _I, _P, _P]),
    "f5_sample_ragged_ex": (_I, [_P, _I, _P, _P, _P, _I, _P, _P, _P, _P, _I, C.c_float, _P, _I, _P, _P]),
    "f5_mmdit_forward": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    "f5_cfm_noise": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "f5_cfm_loss_workspace": (C.c_int64, [_I, _I, _I]),
    "f5_cfm_loss": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "f5_distill_loss_workspace": (C.c_int64, [_I, _I, _I]),
    "f5_distill_loss": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "f5_plan_set_blocks": (_I, [_P, _P, _I]),
    "f5_plan_get_blocks": (_I, [_P, _P, _I]),
    "f5_align_similarity":(_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "f5_align_workspace": (C.c_int64, [_I, _I, _I]),
    "f5_align_viterbi": (_I, [_I, _I, _I, _P, _P, _P, _P, _P]),
    "f5_align_window": (_I, [_I, _I, _I, _P, _P, _P, _P, _P]),
    "f5_duration_loss": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "f5_plan_timing_begin": (_I, [_P, _I]),
    "f5_plan_timing_end": (_I, [_P, C.POINTER(C.c_float), C.POINTER(C.c_int), _P]),
    "f5_plan_timing_site": (_I, [_P, _I, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "f5_plan_set_tap": (_I, [_P, C.c_char_p, _P]),
    "f5_plan_set_probe": (_I, [_P, C.c_char_p, _P]),
    "f5_plan_set_option": (_I, [_P, C.c_char_p, _I]),
    "f5_plan_set_attn_dropout": (_I, [_P, _F, C.c_uint64]),
    "f5_plan_get_option": (_I, [_P, C.c_char_p, C.POINTER(C.c_int)]),
    "f5_duration_predict": (_I, [C.POINTER(DurationWeights), _I, _I, _P, _I, _P, _P, _P, _P]),
    "f5_duration_predict_g": (_I, [C.POINTER(DurationWeights), _I, _I, _P, _I, _P, _P, _I, _P, _P, _P]),
    "f5_op_linear": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P]),
    "f5_op_linear_fused": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _I, _I, _P, _P]),
    "f5_op_ln_fold": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _P, _P, _P]),
    "f5_op_linear_fused_p": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _I, _I, _P, _P]),
    "f5_op_ln_fold_p": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, _I, _P, _P, _P]),
    "f5_op_resid_stats_p": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "f5_op_layernorm_modulate": (_I, [_I, _I, _P, _P, _P, _P, _P]),
    "f5_op_attention": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "f5_op_attention_dropout": (_I, [_I, _I, _I, _I, _I, _P, _P, _F, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P]),
    "f5_op_attention_prescaled": (_I, [_I, _I, _I, _I, _P, _P, _P, _P]),
    "f5_op_fold_weights": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "f5_op_attention_ragged": (_I, [_I, _I, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int), _I, _I, _I, _I, _P, _P, _P]),
    "f5_op_conv_pos_embed": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "f5_op_conv31": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P]),
    "f5_op_tile_gemm": (_I, [C.POINTER(TileGemm), _P]),
    "f5_op_layernorm_res": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "f5_op_f32_to_f16": (_I, [C.c_int64, _P, _P, _P, _P]),
    "f5_op_qknorm_rope": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "f5_op_dwconv7_ln": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "f5_op_grn": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "f5_op_rmsnorm": (_I, [_I, _I, _I, _P, _P, _P, _P]),
    "f5_bench_gemm_site": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_float), _P]),
    "f5_bench_attention": (_I, [_I, _I, _I, _I, _I, C.POINTER(C.c_float), _P]),
    "f5_bench_mfma_rate": (_I, [_I, C.POINTER(C.c_float), _P]),
    "f5_tuning_set": (_I, [C.c_char_p, _I]),
    "f5_tuning_get": (_I, [C.c_char_p, C.POINTER(C.c_int)]),
    "f5_tuning_key": (C.c_char_p, [_I]),
    "f5_debug_gemm_clock": (_I, [_P]),
    "f5_debug_last_gemm": (_I, [C.POINTER(C.c_int)] * 5),
    "f5_debug_site_gemm": (_I, [_I] + [C.POINTER(C.c_int)] * 6),
    "f5_debug_eval_modes": (_I, [_P, _I, _I, _I, C.POINTER(C.c_int32)]),
    "f5_vocoder_create": (_I, [C.POINTER(VocosConfig), C.POINTER(_P)]),
    "f5_vocoder_set_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _I]),
    "f5_vocoder_has_tensor": (_I, [_P, C.c_char_p, C.POINTER(C.c_int64)]),
    "f5_vocoder_finalize": (_I, [_P]),
    "f5_vocoder_destroy": (_I, [_P]),
    "f5_vocoder_decode": (_I, [_P, _I, _I, _P, _P, _P]),
    "f5_vocoder_istft_head": (_I, [_P, _I, _I, _P, _P, _P]),
    "f5_vocoder_decode_ragged": (_I, [_P, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _I, _P, C.POINTER(C.c_int64), _P]),
    "f5_wave_finish": (_I, [_I, _P, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint8), _P, C.c_float, _I, _I, _P, _P, _P, _P, _P,
                            C.POINTER(C.c_int64), _P]),
    "f5_wave_finish_segments": (_I, [_I, _P, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_uint8), _P, _I,
                                     C.POINTER(C.c_int32), C.c_float, _I, _I, _P, _P, C.POINTER(C.c_uint8), _P, _P, _P, C.POINTER(C.c_int64), _P]),
    "f5_wave_stream_create_segments": (_I, [_I, C.POINTER(C.c_uint8), _I, _P, _P, _P, _I, C.POINTER(C.c_int32), C.c_float, _I, C.POINTER(C.c_uint8),
                                            C.POINTER(_P)]),
    "f5_wave_stream_create": (_I, [_I, _I, _P, _P, _P, C.c_float, _I, C.POINTER(_P)]),
    "f5_wave_stream_push": (_I, [_P, _I, _P, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint8), _P, _P, _P, C.POINTER(C.c_int64), _P]),
    "f5_wave_stream_destroy": (_I, [_P]),
    "f5_wave_remove_silence_workspace": (C.c_int64, [C.c_int64, _I, _I, _I]),
    "f5_wave_remove_silence": (_I, [_P, _I, C.c_int64, _I, C.c_int64, _I, _I, _I, _I, _P, _P, C.c_int64, _P, _P, _P, _P, _P]),
    "f5_op_silence_ranges": (_I, [_P, _I, C.c_int64, _I, C.c_int64, _I, _I, _I, _I, _P, C.c_int64, _P, _P, _P, _P]),
    "f5_op_g711_encode": (_I, [C.c_int64, _P, _I, _P, _P]),
    "f5_wave_convert": (_I, [_P, _I, C.c_int64, _I, _I, _P, _I, _P, _P, _P, C.POINTER(C.c_int64), _P]),
    "f5_wave_convert_stream_create": (_I, [_I, _I, _P, _I, _I, C.POINTER(_P)]),
    "f5_wave_convert_stream_push": (_I, [_P, _P, C.c_int64, _I, _P, _P, _P, C.POINTER(C.c_int64), _P]),
    "f5_wave_convert_stream_destroy": (_I, [_P]),
    "f5_reference_prepare_workspace": (C.c_int64, [C.c_int64, _I, _I, C.POINTER(ReferenceRule)]),
    "f5_reference_table_rows": (C.c_int64, [C.c_int64, _I, _I, C.POINTER(ReferenceRule)]),
    "f5_reference_prepare": (_I, [_P, C.c_int64, _I, _I, C.POINTER(ReferenceRule), _I, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, _P, _P, _P]),
    "f5_op_reference_plan": (_I, [_P, C.c_int64, _I, _I, C.POINTER(ReferenceRule), _P, C.c_int64, _P, _P, _P]),
    "f5_bigvgan_create": (_I, [C.POINTER(BigVGANConfig), C.POINTER(_P)]),
    "f5_bigvgan_set_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _I]),
    "f5_bigvgan_has_tensor": (_I, [_P, C.c_char_p, C.POINTER(C.c_int64)]),
    "f5_bigvgan_finalize": (_I, [_P]),
    "f5_bigvgan_destroy": (_I, [_P]),
    "f5_bigvgan_forward": (_I, [_P, _I, _I, _P, _P, _P]),
    "f5_bigvgan_decode_ragged": (_I, [_P, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _I, _P, C.POINTER(C.c_int64), _P]),
    "f5_op_bigvgan_snake": (_I, [_I, _I, _P, _P, _P, C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _P]),
    "f5_op_bigvgan_snake_ragged": (_I, [_I, C.POINTER(C.c_int32), _I, _I, _P, _P, _P, C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _P]),
    "f5_frontend_create": (_I, [C.POINTER(MelConfig), C.POINTER(_P)]),
    "f5_frontend_destroy": (_I, [_P]),
    "f5_frontend_mel": (_I, [_P, _I, _I, _P, _P, _P]),
    "f5_frontend_resample": (_I, [_P, _I, _I, _I, _I, _P, _P, _P]),
    "f5_speaker_create": (_I, [C.POINTER(SpeakerConfig), C.POINTER(_P)]),
    "f5_speaker_set_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _I]),
    "f5_speaker_has_tensor": (_I, [_P, C.c_char_p, C.POINTER(C.c_int64)]),
    "f5_speaker_finalize": (_I, [_P]),
    "f5_speaker_destroy": (_I, [_P]),
    "f5_speaker_embed_ragged": (_I, [_P, _I, C.POINTER(C.c_int32), _P, _P, _P]),
    "f5_speaker_set_tap": (_I, [_P, C.c_char_p, _P]),
    "f5_op_speaker_featnorm": (_I, [_I, C.POINTER(C.c_int32), _I, _I, _P, _P, _P, _P]),
    "f5_op_speaker_conv_relu_bn": (_I, [_I, C.POINTER(C.c_int32), _I, _I, _I, _I, _P, _P, _P, _P, _F, _P, _P]),
    "f5_op_speaker_res2": (_I, [_I, C.POINTER(C.c_int32), _I, _I, _I, _P, _P, _P, _P, _F, _P, _P]),
    "f5_op_speaker_se": (_I, [_I, C.POINTER(C.c_int32), _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "f5_op_speaker_pool": (_I, [_I, C.POINTER(C.c_int32), _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "f5_wavlm_create": (_I, [C.POINTER(WavLMConfig), C.POINTER(_P)]),
    "f5_wavlm_set_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _I]),
    "f5_wavlm_has_tensor": (_I, [_P, C.c_char_p, C.POINTER(C.c_int64)]),
    "f5_wavlm_finalize": (_I, [_P]),
    "f5_wavlm_destroy": (_I, [_P]),
    "f5_wavlm_frames": (_I, [_P, C.c_int64]),
    "f5_wavlm_set_buckets": (_I, [_P, _I, C.POINTER(C.c_int32)]),
    "f5_wavlm_extract_ragged": (_I, [_P, _I, C.POINTER(C.c_int32), _P, _I, _P, _P]),
    "f5_wavlm_set_tap": (_I, [_P, C.c_char_p, _P]),
    "f5_op_wavlm_attention": (_I, [_I, _I, _I, _P, _P, _P, _P, _P]),
    "f5_op_wavlm_pos_conv": (_I, [_I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "f5_op_wavlm_conv_ln_gelu": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
}
EXPORTS = tuple(_PROTOS)

_lib = None


def load(build_if_missing: bool = False):
    """Load libf5hip.so (no compute).  Raises F5HipError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        if build_if_missing:
            from . import build as _b
            _b.build(verbose=False)
        else:
            raise F5HipError(f"{LIB_PATH} not found: build it with `python -m eraxvif5tts_amd.build` (hipcc, gfx950). "
                             "There is no CPU / eager-PyTorch fallback for the hot path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _PROTOS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if not os.environ.get("F5HIP_LIB"):
                raise
            continue  # (an A/B run's other build may predate an entry point: calling it there raises AttributeError)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    # developer knobs for A/B runs: F5HIP_TUNING="gemm_variant=0,attn_variant=2" -> f5_tuning_set(key, value)
    for item in filter(None, os.environ.get("F5HIP_TUNING", "").split(",")):
        key, _, val = item.partition("=")
        if lib.f5_tuning_set(key.strip().encode(), int(val)) != 0:
            raise F5HipError(f"F5HIP_TUNING: {lib.f5_last_error().decode('utf-8', 'replace')}")
    return lib


def last_error() -> str:
    return load().f5_last_error().decode("utf-8", "replace")


F5_ENOTSUP = -5  # f5hip.h: a configuration the kernels do not implement (callers with a host route of their own test for it)


def check(rc: int, what: str = ""):
    if rc != 0:
        raise F5HipError(f"libf5hip {what} failed (code {rc}): {last_error()}")


def require_gpu():
    """The product path needs a real MI355X; anything else is an error, never a silent fallback."""
    lib = load()
    if not torch.cuda.is_available():
        raise F5HipError("no ROCm device visible to PyTorch: the HIP hot path cannot run (no CPU fallback)")
    name = C.create_string_buffer(64)
    if lib.f5_device_count(name) <= 0:
        raise F5HipError("no gfx950 (MI355X) device usable by libf5hip")
    return name.value.decode()


def ptr(t):
    """Device/host pointer of a contiguous tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), "libf5hip takes contiguous tensors"
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def set_tensors(handle, setter, has, state: dict):
    """Upload every tensor of `state` the native handle knows (strict=False semantics); returns the names used."""
    lib = load()
    used = []
    for name, t in state.items():
        if not getattr(lib, has)(handle, name.encode(), None):
            continue
        h = t.detach().to("cpu", torch.float32).contiguous()
        shape = (C.c_int64 * h.ndim)(*h.shape)
        check(getattr(lib, setter)(handle, name.encode(), C.c_void_p(h.data_ptr()), shape, h.ndim), f"set_tensor({name})")
        used.append(name)
    return used
