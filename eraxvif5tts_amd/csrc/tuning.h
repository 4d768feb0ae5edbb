// tuning.h -- the one list of the process-wide integer tuning knobs (f5_tuning_set / f5_tuning_get / f5_tuning_key; F5HIP_TUNING at load time).
// The launch code reads the variables directly; this header is the only place that declares them and tuning.hip the only place that defines them.
//
// A row is X(key, variable, default, kind, check):
//   kind   INT  = stored as given, BOOL = stored as value != 0
//   check  ANY  = every value is accepted, otherwise the name of a validator in tuning.hip (null = accepted, else the message of the refusal)
#pragma once

// clang-format off
#define F5_TUNING_KNOBS(X)                                                                                                                             \
    /* attention: 0 = by grid size, 2 = 64 queries per wave, 5 = software-pipelined 32 queries per wave (6, the persistent grid, was removed) */       \
    X("attn_variant", g_attn_variant, 0, INT, attn_variant_known)                                                                                      \
    /* pre-scaled q (plan_attn_prescale); the plan option of the same name overrides it */                                        \
    X("attn_prescale", g_attn_prescale, 1, BOOL, ANY)                                                                                                  \
    /* 1 = dedicated halo-tile kernel for the dim-1024 grouped conv, 0 = implicit GEMM (gemm_fast.hip) */                                              \
    X("conv31", g_conv31, 1, BOOL, ANY)                                                                                                                \
    /* conv31 tokens per workgroup, 0 = by grid size, 128 or 256 forced */                                                                             \
    X("conv31_tok", g_conv31_tok, 0, INT, ANY)                                                                                                         \
    /* f5_op_conv_pos_embed runs the tuned conv kernels (bf16) */                                                                                      \
    X("op_conv_kernel", g_op_conv_kernel, 0, BOOL, ANY)                                                                                                \
    /* Vocos ISTFT head by FFT (1) or by the dense inverse-DFT GEMM (0: the parity cross-check) */                                                     \
    X("vocos_fft", g_vocos_fft, 1, BOOL, ANY)                                                                                                          \
    /* BigVGAN frame budget of one launch set (bounds the im2col workspace; measured: profiles/r5_bigvgan_ragged_ab.md) */                             \
    X("bigvgan_group_frames", g_bigvgan_group_frames, 2048, INT, bigvgan_group_frames_positive)                                                        \
    /* tuned GEMM main loop: 0 = plain ring everywhere, 1 = staggered wave groups (+ persistent grid) */                                               \
    X("gemm_variant", g_gemm_variant, 1, INT, ANY)                                                                                                     \
    /* token tiles per L2 patch (0 = by shape, 1 = feature-tile-fastest order) */                                                                      \
    X("gemm_group", g_gemm_group, 0, INT, ANY)                                                                                                         \
    /* diagnostic: patch height per block call site, two decimal digits each: qkv|out|ff1|ff2 */                                                       \
    X("gemm_group_sites", g_gemm_group_sites, 0, INT, ANY)                                                                                             \
    /* bit mask of block call sites (bit 0 qkv, 1 out, 2 ff1, 3 ff2) that walk their tiles backwards; 8: FF2 272.5 -> 267.3 us in situ, C2 30 185 -> */ \
    /* 30 328 mel-frames/s (same-box A/B; the reason: apply_site_knobs, gemm_fast.hip).  Same values either way. */                                   \
    X("gemm_reverse_sites", g_gemm_reverse_sites, 8, INT, ANY)                                                                                         \
    /* 1 = whole-tile block linears run on the persistent grid */                                                                                      \
    X("gemm_persist", g_gemm_persist, 1, BOOL, ANY)                                                                                                    \
    /* workgroups of the persistent kernel (0 = one per CU of the device: gemm_persist_grid()) */                                                      \
    X("gemm_persist_grid", g_gemm_persist_grid, 0, INT, gemm_persist_grid_in_range)                                                                    \
    /* diagnostic: bm * 1000 + bn forces the tile of every tuned-GEMM launch that supports it (0 = by shape) */                                        \
    X("gemm_tile", g_gemm_tile, 0, INT, ANY)                                                                                                           \
    /* 128-row token tiles when the 256-row ones leave CUs without a workgroup (single-utterance launches) */                                          \
    X("gemm_bm128", g_gemm_bm128, 1, INT, ANY)                                                                                                         \
    /* 1 = lean epilogue on whole tiles, 0 = generic epilogue everywhere */                                                                            \
    X("gemm_lean", g_gemm_lean, 1, BOOL, ANY)                                                                                                          \
    /* the block GEMMs of a DiT evaluation run over the token rows rounded up to 256 (dit_eval) */                                                     \
    X("gemm_pad_rows", g_gemm_pad_rows, 1, BOOL, ANY)                                                                                                  \
    /* 1 = whole-tile block linears with enough tiles for the CUs (w4_tile_rows) run on the one-wave-per-SIMD kernel */                                \
    X("gemm_w4", g_gemm_w4, 1, BOOL, ANY)                                                                                                              \
    /* folded projections on the one-wave-per-SIMD kernel's 128-row tiles finish the row statistics themselves (no statistics launch) */               \
    X("gemm_w4_ink", g_gemm_w4_ink, 1, INT, ANY)                                                                                                       \
    /* diagnostic: token rows per tile of that kernel, 0 = by tile count, 128 / 256 forced where the shape allows */                                   \
    X("gemm_w4_bm", g_gemm_w4_bm, 0, INT, ANY)                                                                                                         \
    /* rows per wave of the read-only LayerNorm pass (1 = the one-row kernel; same-box A/B at C2, pair of passes: 96.4 us -> 90.8 with 2, 93.3 with 4) */ \
    X("ln_rows", g_ln_rows, 2, INT, ANY)                                                                                                               \
    /* smallest launch (token rows) that takes the multi-row LayerNorm kernel */                                                                       \
    X("ln_rows_min", g_ln_rows_min, 16384, INT, ANY)                                                                                                   \
    /* 16-byte form of the LayerNorm pass at its production shape */                                                                                   \
    X("ln_wide", g_ln_wide, 1, BOOL, ANY)                                                                                                              \
    /* write the residual stream once per DiT block (0 = after every LayerNorm pass) */                                                                \
    X("ln_defer", g_ln_defer, 1, BOOL, ANY)                                                                                                            \
    /* LayerNorm fold (dit_eval); 0 = the two LayerNorm passes per block of round 3 */                                                                 \
    X("ln_fold", g_ln_fold, 1, BOOL, ANY)                                                                                                              \
    /* 1 = folded projections on tiles narrower than 256 take their row statistics inside the kernel, no statistics launch.  Same bits (tested), */    \
    /* but slower where it applies: 1 x 1024 79.0 - 80.1 against 76.9 - 77.6 ms per sample(), 2 x 1024 107.8 - 108.6 against 105.5 - 105.9 ms: */ \
    /* the 16 partial loads per row sit in front of a latency-bound main loop and cost more than the 44 small launches they replace.  Off. */          \
    X("ln_fold_inkernel", g_ln_fold_inkernel, 0, BOOL, ANY)                                                                                            \
    /* in-place residual epilogues: see dit_eval */                                                                                                    \
    X("resid_rmw", g_resid_rmw, 1, BOOL, ANY)                                                                                                          \
    /* bf16 production mode keeps the residual stream in fp16 from the first block on (0 = fp32) */                                                    \
    X("residual_f16", g_res_f16, 1, BOOL, ANY)                                                                                                         \
    /* LayerNorm passes prefetch the following GEMMs' weights when the launch has at most this many token rows (0 = never).  M = 8192: +2.3 %, */      \
    /* M = 2048: +2.9 % mel-frames/s; M = 65536: no effect (each weight line serves 256 token tiles there) */                                          \
    X("w_prefetch", g_w_prefetch, 16384, INT, ANY)                                                                                                     \
    /* diagnostic: an eager sample() synchronises the stream after every network evaluation, which bounds the number of dispatches in flight */        \
    /* (profiles/r3_rocprof_pmc_sigsegv.md: rocprofv3 --pmc died under ~5 400 queued dispatches) */                                                    \
    X("sync_evals", g_sync_evals, 0, BOOL, ANY)                                                                                                        \
    /* f5_bench_gemm_site: leading-dimension padding (elements) of the activation / weight operand */                                                  \
    X("bench_pad_a", g_bench_pad_a, 0, INT, ANY)                                                                                                       \
    X("bench_pad_w", g_bench_pad_w, 0, INT, ANY)
// clang-format on

#define F5_KNOB_DECLARE(key, var, def, kind, check) extern int var;
F5_TUNING_KNOBS(F5_KNOB_DECLARE)
#undef F5_KNOB_DECLARE

extern int g_tuning_epoch;  // bumped by every f5_tuning_set: graphs captured under other knob values are dropped at their next use (model.hip)
