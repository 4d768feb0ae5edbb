/*
 * f5hip.h -- C ABI of libf5hip.so: the MI355X (gfx950) implementation of the F5-TTS flow-matching
 * inference hot path (CFM.sample -> DiT ODE loop -> Vocos), written from scratch in HIP.
 *
 * The reference (hungkq-1724/EraXviF5TTS) is 100 % Python and has no native ABI; the entry points below
 * are what a binding for the reference's two plug points would call:
 *
 *   plug point A  "backbone class"   f5_tts/infer/f5tts_wrapper.py:134,145  model_cls(**arch, ...)
 *                                    f5_tts/model/cfm.py:164-172            transformer(x, cond, text, time, ...)
 *   plug point B  "vocoder object"   f5_tts/infer/utils_infer.py:101-124    load_vocoder(...)
 *                                    f5_tts/infer/f5tts_wrapper.py:524      vocoder.decode(mel)
 *   sampler                          f5_tts/model/cfm.py:82-208             CFM.sample(...)
 *
 * Conventions
 *   - every function returns 0 on success, a negative F5_E* code on failure; f5_last_error() returns a
 *     thread-local human readable message.  Nothing throws across the boundary.
 *   - "dev" pointers are device (HBM) pointers owned by the caller (e.g. torch tensor data_ptr());
 *     "host" pointers are ordinary host memory.  The library never frees or reallocates caller memory.
 *   - all work is enqueued on the caller's hipStream_t (f5_stream_t); the library only synchronises
 *     inside f5_*_create / f5_model_finalize (uploads) and never on the hot path.
 *   - handles are not thread-safe; distinct handles may be used from distinct threads/processes.
 *   - there is NO CPU fallback: every entry point fails with F5_ENODEVICE when no gfx950 device is usable.
 */
#ifndef F5HIP_H
#define F5HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden: only the entry points declared here are exported */
#define F5_API __attribute__((visibility("default")))

#define F5HIP_VERSION 400 /* 0.4.0 (round 4; round 5 adds f5_vocoder_decode_ragged, f5_wave_finish and f5_bigvgan_decode_ragged (+ tuning key "bigvgan_group_frames") under the same number, which tests/test_host_logic.py pins: detect them by symbol -- as f5_plan_set_blocks, f5_plan_get_blocks and f5_distill_loss after them): + the BigVGAN entry points and mel front-end, f5_op_ln_fold, bounded timing ring; plan options "ln_fold_active", "gemm_w4"; tuning keys "ln_fold", "gemm_w4"; 0.3.2: + f5_sample_ragged, f5_mmdit_forward, f5_duration_predict_g */

/* error codes */
#define F5_OK 0
#define F5_EINVAL -1    /* bad argument / shape */
#define F5_ENODEVICE -2 /* no usable HIP device */
#define F5_EHIP -3      /* a HIP runtime call failed (message has the hipError string) */
#define F5_ESTATE -4    /* call out of order (e.g. forward before finalize) */
#define F5_ENOTSUP -5   /* configuration the kernels do not implement (qk_norm, long_skip_connection) */
#define F5_ENOMEM -6

/* arithmetic of the dense kernels */
#define F5_PREC_BF16 0 /* bf16 MFMA inputs, fp32 accumulate and arithmetic, fp32 ODE state, residual stream stored as fp16 (production) */
#define F5_PREC_FP32 1 /* fp32-input MFMA everywhere (debug / parity mode, ~1/16 of the bf16 rate) */
/* fp16 weights, activations and MFMA inputs (v_mfma_f32_*_f16: the bf16 rate and fragment layouts), fp32 accumulate and arithmetic, fp32 ODE
 * state, and the fp16 residual stream with its range guard exactly as in the bf16 mode: the dtype the reference casts its model to on a GPU
 * (infer/utils_infer.py:184-193).  Weights are rounded to nearest even on the host; a tensor that holds a non-finite value after the rounding
 * fails f5_model_finalize with F5_EINVAL and its name.  Every fp32 -> fp16 ACTIVATION store saturates at +-65504: an out-of-range activation
 * clips silently (the residual stream is the one buffer whose clipping is guarded).  The attention kernels keep their un-normalised softmax
 * numerators inside fp16: the exponent reference is always a score of the row (q is never pre-scaled: "attn_prescale_active" reads 0 and the
 * LayerNorm-fold tables carry plain q rows), and a tile whose row sums reach 2^15 against a stale reference is redone against the row maxima.
 * f5_plan_set_attn_dropout(prob > 0) answers F5_ENOTSUP on an fp16 plan; the vocoders, the front-end and the duration predictor keep their own
 * precisions. */
#define F5_PREC_FP16 2

/* ODE solvers of torchdiffeq's fixed-grid family used by cfm.py:197 (odeint_kwargs["method"]): euler, midpoint, and the explicit
 * Runge-Kutta methods rk4 (rk4_alt_step_func, the 3/8 rule), heun2 and heun3.  Network evaluations per step: 1 / 2 / 4 / 2 / 3
 * (f5_ode_evals_per_step).  Adaptive solvers and the Adams family are not provided. */
#define F5_ODE_EULER 0
#define F5_ODE_MIDPOINT 1
#define F5_ODE_RK4 2
#define F5_ODE_HEUN2 3
#define F5_ODE_HEUN3 4

typedef void* f5_stream_t; /* hipStream_t */
typedef struct f5_model_s* f5_model_t;
typedef struct f5_plan_s* f5_plan_t;
typedef struct f5_vocoder_s* f5_vocoder_t;

/* mirrors the kwargs of DiT.__init__ (f5_tts/model/backbones/dit.py:104-122) */
typedef struct f5_dit_config {
    int32_t dim;               /* model width (1024) */
    int32_t depth;             /* number of DiT blocks (22) */
    int32_t heads;             /* attention heads (16) */
    int32_t dim_head;          /* 64 (only 64 is implemented) */
    int32_t ff_inner;          /* int(dim * ff_mult) (2048) */
    int32_t mel_dim;           /* 100 */
    int32_t text_num_embeds;   /* vocab size V (embedding table has V+1 rows) */
    int32_t text_dim;          /* 512 */
    int32_t conv_layers;       /* ConvNeXtV2 blocks in the text embedder (4) */
    int32_t text_mask_padding; /* 0 (F5TTS_Base) / 1 (F5TTS_v1_Base) */
    int32_t pe_attn_head;      /* heads that receive RoPE; <= 0 means all heads (None) */
    int32_t qk_norm;           /* must be 0 (null in every shipped config) */
    int32_t long_skip;         /* must be 0 */
    int32_t precision;         /* F5_PREC_* */
    int32_t rope_layout;       /* F5_ROPE_* : which feature pairs of a head one rotary frequency turns (x_transformers is not vendored
                                * in the reference tree; the adjacent-pair form is the one the pinned >=1.31 releases publish) */
    int32_t backbone;          /* F5_BACKBONE_*: which class of plug point A (0 = DiT, the default of a zero-initialised struct) */
    int32_t skip_connect;      /* UNetT only: F5_SKIP_* (reference unett.py:118 skip_connect_type) */
} f5_dit_config;

/* backbones behind plug point A (reference infer/f5tts_wrapper.py:134: model_cls = f5_tts.model.<cfg.model.backbone>) */
#define F5_BACKBONE_DIT 0   /* model/backbones/dit.py:103   (F5-TTS) */
#define F5_BACKBONE_UNETT 1 /* model/backbones/unett.py:103 (E2-TTS: flat U-Net transformer; tensor names = UNetT.state_dict(): layers.<i>.{0.weight,
                             * 1.g, 2.to_q|to_k|to_v|to_out.0.{weight,bias}, 3.g, 4.ff.0.0.*, 4.ff.2.*}, norm_out.g; depth must be even) */
#define F5_BACKBONE_MMDIT 2 /* model/backbones/mmdit.py:85  (SD3-style joint text / audio blocks; tensor names = MMDiT.state_dict(): audio_embed.*,
                             * transformer_blocks.<i>.{attn_norm_x, attn_norm_c}.linear.*, .attn.{to_q,to_k,to_v}[_c].*, .attn.to_out.0.*, .attn.to_out_c.*,
                             * .ff_x.ff.*, .ff_c.ff.* (no to_out_c / ff_c in the last, context_pre_only block); text_dim must equal dim, conv_layers 0) */
#define F5_SKIP_CONCAT 0 /* x = Linear(2 dim -> dim, no bias)(cat(x, skip)) in the second half of the layers (default) */
#define F5_SKIP_ADD 1
#define F5_SKIP_NONE 2

/* rotary layouts of the q/k head features (dim_head = 64, 32 frequencies), reference model/modules.py:452-461 via x_transformers */
#define F5_ROPE_ADJACENT 0  /* frequency j turns features (2j, 2j+1): rotate_half on '... (d r) -> ... d r', r = 2 (default) */
#define F5_ROPE_HALF_SPLIT 1 /* frequency j turns features (j, j+32): rotate_half on the two halves of the head (GPT-NeoX form) */

F5_API const char* f5_last_error(void);
F5_API int f5_version(void);
/* number of usable gfx950 devices; name_out (>= 64 bytes, may be NULL) receives the arch string of device 0 */
F5_API int f5_device_count(char* name_out);

/* ------------------------------------------------------------------ model (weights resident in HBM) */
F5_API int f5_model_create(const f5_dit_config* cfg, f5_model_t* out);
/* name = DiT.state_dict() key, data = contiguous host fp32, shape as in the checkpoint.
 * Unknown names return F5_EINVAL (callers pass strict=False semantics by skipping names themselves). */
F5_API int f5_model_set_tensor(f5_model_t m, const char* name, const float* host_data, const int64_t* shape, int ndim);
/* returns 1/0 whether `name` is a tensor the model expects (and its element count in *numel if non-NULL) */
F5_API int f5_model_has_tensor(f5_model_t m, const char* name, int64_t* numel);
/* builds the fused device layouts (QKV concat, split input projection, rearranged grouped-conv taps, bf16 copies) */
F5_API int f5_model_finalize(f5_model_t m);
/* Destroy every plan of a model BEFORE the model: a plan may hold one of the model's LayerNorm-fold tables (round 4: per-time-grid weights
 * W' = fp16(W (1 + scale)), up to two grids per model, 231 MB per evaluation time at F5TTS_Base; built by the first f5_sample on a grid). */
F5_API int f5_model_destroy(f5_model_t m);

/* ------------------------------------------------------------------ plan (workspace for one (batch, seq) bucket) */
/* max_batch = utterances per call (CFG doubling is internal), max_seq = frames N, max_evals = network
 * evaluations times held at once (steps * f5_ode_evals_per_step(method): steps for euler, 2*steps for midpoint and heun2, 3*steps for
 * heun3, 4*steps for rk4).  A sample() with more evaluations than this returns F5_EINVAL before any work. */
F5_API int f5_plan_create(f5_model_t m, int max_batch, int max_seq, int max_evals, f5_plan_t* out);
/* network evaluations per step of an F5_ODE_* method (1 / 2 / 4 / 2 / 3), or F5_EINVAL for an unknown one */
F5_API int f5_ode_evals_per_step(int ode_method);
F5_API int f5_plan_destroy(f5_plan_t p);
F5_API int64_t f5_plan_workspace_bytes(f5_plan_t p);

/* CFM.sample (cfm.py:82-208) after text->ids and duration resolution:
 *   cond      dev f32 [B, N, mel]  prompt mel zero-padded to N (NOT yet masked by lens: the kernel applies cfm.py:148-150)
 *   text      dev i32 [B, nt]      token ids, -1 padded (utils.py:88-95)
 *   lens      dev i32 [B]          prompt lengths in frames (cond_mask = frame < lens)
 *   durations dev i32 [B] or NULL  total lengths; NULL = no key-padding mask (the batch==1 path, cfm.py:152-155)
 *   y0        dev f32 [B, N, mel]  initial noise, rows >= duration zero (cfm.py:178-183)
 *   tgrid     host f32 [steps+1]   time grid after sway sampling (cfm.py:193-195)
 *   out       dev f32 [B, N, mel]  where(cond_mask, cond, y(1)) (cfm.py:200-202)
 *   trajectory dev f32 [steps+1, B, N, mel] or NULL
 * use_graph != 0 replays a hipGraph captured for this exact (B, N, nt, steps, method, cfg on/off, mask on/off). */
F5_API int f5_sample(f5_plan_t p, int B, int N, const float* cond, const int32_t* text, int nt, const int32_t* lens,
              const int32_t* durations, const float* y0, const float* tgrid_host, int steps, float cfg_strength,
              int ode_method, float* out, float* trajectory, int use_graph, f5_stream_t stream);

/* Speech editing (reference infer/speech_edit.py -> CFM.sample(edit_mask=...), cfm.py:123-127): f5_sample with a per-frame condition mask in
 * place of the lens prefix.  Same arguments as f5_sample, plus
 *   cond_mask dev u8 [B, N]      1 = keep the prompt frame (lens_to_mask(lens) & edit_mask, False-padded to N); it replaces `frame < lens`
 *                                both in step_cond = where(cond_mask, cond, 0) (cfm.py:148-150) and in the final where(cond_mask, cond, y(1))
 *                                (cfm.py:200-202); `lens` is still read and must be valid.  The CFG null branch zeroes every frame as before.
 * The mask is staged into the plan, so a replayed hipGraph reads this call's mask; masked and unmasked calls keep separate captures.  The
 * deferred range guard (f5_sample_finish) and the fp32 fallback rerun reuse the staged mask.  f5_sample(...) computes exactly what
 * f5_sample_masked(..., cond_mask = (frame < lens), ...) computes. */
F5_API int f5_sample_masked(f5_plan_t p, int B, int N, const float* cond, const int32_t* text, int nt, const int32_t* lens,
                     const int32_t* durations, const float* y0, const float* tgrid_host, int steps, float cfg_strength,
                     int ode_method, const uint8_t* cond_mask, float* out, float* trajectory, int use_graph, f5_stream_t stream);

/* Deferred range-guard check (plan option "residual_guard" = 2): f5_sample then enqueues everything and returns without synchronising, so one
 * host thread can feed several plans on several streams (F5TTSWrapper.generate runs the text chunks of a call concurrently that way: they
 * are independent, reference infer/f5tts_wrapper.py:476-533).  f5_sample_finish(plan, stream) synchronises the stream, reads the flag and, if
 * it was raised, repeats the loop with fp32 residual storage and rewrites the outputs; it is a no-op when nothing is pending. */
F5_API int f5_sample_finish(f5_plan_t p, f5_stream_t stream);

/* The same ODE loop over B utterances of DIFFERENT frame counts in one set of launches -- no padding to a common length, no key mask:
 * what F5TTSWrapper.generate needs for the text chunks of one call (the reference samples them one after the other at batch 1,
 * infer/f5tts_wrapper.py:476-533; a batch-1 sample() has mask = None, model/cfm.py:152-155).  Each utterance gets the arithmetic of its own
 * batch-1 f5_sample call: bit-identical output whenever both calls take the tuned kernels (every frames_host[i] >= 256, bf16 mode) or both the
 * fp32 mode's.  frames_host: host int32 [B]; cond, y0, out: dev f32 [sum(frames), mel], the utterances one after the other; text dev int32
 * [B, nt] (-1 padded); lens dev int32 [B] (prompt frames); no trajectory, no hipGraph (shapes rarely recur); DiT backbone only.
 * Plan capacity: sum(frames_i + 16, each rounded up to 16) <= max_batch * max_seq, every frames_i and nt <= max_seq, B <= max_batch.  * Plan option "ragged_graph" = 1 (round 4): the call replays a hipGraph captured for this exact list of frame counts (+ nt, steps, method, CFG)
 * -- batch inference over fixed length buckets (eval/prompts.py) meets the same bucket shapes again; 0 (default): eager launches. */
F5_API int f5_sample_ragged(f5_plan_t p, int B, const int32_t* frames_host, const float* cond, const int32_t* text, int nt, const int32_t* lens,
                     const float* y0, const float* tgrid_host, int steps, float cfg_strength, int ode_method, float* out, f5_stream_t stream);

/* f5_sample_ragged for INDEPENDENT requests (F5TTSWrapper.generate_batch): a guidance strength and a per-frame condition mask of its own
 * for every utterance.  Detected by symbol, like the round-5 entries.  f5_sample_ragged(...) is this call with both pointers NULL.
 *   cfg_host   host f32 [B] or NULL (= cfg_strength for every utterance).  Utterance u is combined as pred + (pred - null_pred) * cfg_host[u]
 *              (cfm.py:173) with the operations of the scalar form, so its rows are bit-identical to its own batch-1 f5_sample call with
 *              cfg_strength = cfg_host[u].  The reference takes its single-pass branch below 1e-5 (cfm.py:167) and one doubled batch cannot
 *              hold both branches: a vector with values on both sides of 1e-5 (or a NaN) is refused with F5_EINVAL before anything is
 *              staged or launched -- keep such requests in different calls.  A vector below 1e-5 throughout runs the single pass.
 *              The values are staged as device data per call, outside the captured region: with plan option "ragged_graph" = 1 a replayed
 *              capture combines with the CURRENT call's vector (the capture key holds only whether a vector was given).  The fp16 range
 *              guard's fp32 rerun reads the same staged values.
 *   cond_mask  dev u8 [sum(frames)] or NULL (= frame < lens[u]): the condition mask of f5_sample_masked, utterance after utterance; rows
 *              bit-identical to the batch-1 f5_sample_masked call of each utterance. */
F5_API int f5_sample_ragged_ex(f5_plan_t p, int B, const int32_t* frames_host, const float* cond, const int32_t* text, int nt,
                        const int32_t* lens, const uint8_t* cond_mask, const float* y0, const float* tgrid_host, int steps,
                        float cfg_strength, const float* cfg_host, int ode_method, float* out, f5_stream_t stream);

/* TextEmbedding.forward (dit.py:49-79): text ids [B, nt] (-1 padded) -> dev f32 [B, N, text_dim].  An id outside [-1, text_num_embeds) is
 * clamped to the nearer end of that range (-1 is the filler) instead of being read outside the embedding table. */
F5_API int f5_text_embed(f5_plan_t p, int B, int N, const int32_t* text, int nt, int drop_text, float* out, f5_stream_t stream);

/* DiT.forward (dit.py:185-233) for one branch:
 *   x, cond dev f32 [B, N, mel]; text_embed dev f32 [B, N, text_dim] (from f5_text_embed; the Python module owns the
 *   cond/uncond cache of dit.py:202-210); time dev f32 [B]; mask dev u8 [B, N] or NULL; out dev f32 [B, N, mel]. */
F5_API int f5_dit_forward(f5_plan_t p, int B, int N, const float* x, const float* cond, const float* text_embed,
                   const float* time, int drop_audio_cond, const uint8_t* mask, float* out, f5_stream_t stream);

/* MMDiT.forward (mmdit.py:146-190) for one branch: as f5_dit_forward, with the text stream at its own length --
 *   text_embed dev f32 [B, nt, dim] (f5_text_embed on an F5_BACKBONE_MMDIT plan writes [B, nt, dim] and ignores N), nt <= the plan's max_seq. */
F5_API int f5_mmdit_forward(f5_plan_t p, int B, int N, int nt, const float* x, const float* cond, const float* text_embed,
                     const float* time, int drop_audio_cond, const uint8_t* mask, float* out, f5_stream_t stream);

/* ------------------------------------------------------------------ flow-matching loss (CFM.forward, cfm.py:210-283; forward only)
 * The flow-matching layer around ONE backbone evaluation (f5_dit_forward / f5_mmdit_forward with a time per sample), for validation runs: no
 * gradient of anything here exists.  Detected by symbol, like the round-5 entries.  All tensors dev f32 [B, N, mel] unless said otherwise;
 * span dev u8 [B, N] (1 = the frame lies in the random span: rand_span_mask & mask, cfm.py:241-245); time dev f32 [B].
 * Noising (cfm.py:257-263) in one pass over x1 (the mel) and x0 (the noise):
 *   phi  = (1 - t_b) * x0 + t_b * x1   the four fp32 operations rounded one by one, no FMA: torch's bits for cfm.py:259
 *   cond = span ? 0 : x1               cfm.py:263 */
F5_API int f5_cfm_noise(int B, int N, int mel, const float* x1, const float* x0, const float* time, const uint8_t* span, float* phi,
                        float* cond, f5_stream_t stream);
/* The loss (cfm.py:260, 280-283): per element (pred - (x1 - x0))^2 with every step rounded in fp32 as F.mse_loss(pred, x1 - x0, reduction =
 * "none") rounds it, summed in fp64 over the rows where span is set.  sums dev f64 [B]; counts dev i64 [B] = selected rows x mel; loss dev f32 [1]
 * = float(sum of sums / sum of counts): NaN when nothing is selected, as mean() of an empty tensor; an utterance without a selected row gets
 * sums = 0 and counts = 0.  The flow and the elementwise loss never reach memory, and rows outside the span are not read.  The sum has a fixed
 * order (per-workgroup partials in `workspace`, added by index; the partition depends on N and mel alone; no atomics): the same input gives the
 * same bits on every run.  workspace: dev, 8-byte aligned, at least the bytes the _workspace entry answers (a negative F5_* code for a shape it
 * refuses).  F5_EINVAL with a message for a null pointer or B, N or mel below 1.  16-byte loads when mel % 4 == 0 and the tensors are 16-byte
 * aligned, element loads otherwise.  Nothing synchronises. */
F5_API int64_t f5_cfm_loss_workspace(int B, int N, int mel);
F5_API int f5_cfm_loss(int B, int N, int mel, const float* pred, const float* x1, const float* x0, const uint8_t* span, double* sums,
                       int64_t* counts, float* loss, void* workspace, f5_stream_t stream);

/* ------------------------------------------------------------------ distillation losses (train/distil_reload.py:1070-1097; forward only)
 * The losses the reference's teacher-to-student distillation script logs per update, for judging a pruned model against the model it was cut
 * from: no gradient of anything here exists.  Detected by symbol.  student, teacher (the two backbones' predictions on the same phi and cond),
 * x1, x0 dev f32 [B, N, mel]; span dev u8 [B, N].  One pass forms, per element of a row where span is set, with every fp32 step rounded on its own,
 *   flow = x1 - x0;   term 0 = (student - flow)^2;   term 1 = (teacher - flow)^2;   term 2 = (student - teacher)^2;   term 3 = |student - teacher|
 * -- the values F.mse_loss / F.l1_loss(reduction = "none") form -- and sums each in fp64 in the fixed order of the flow-matching loss above (per-workgroup
 * partials in `workspace`, added by index, no atomics: the same input gives the same bits).  Rows outside the span are not read.
 *   sums   dev f64 [B, 4]   per utterance and term
 *   frames dev i64 [B]      selected FRAMES, not frames x mel: the script divides by rand_span_mask.sum() (:1072, :1093), so its losses are mel
 *                           times a mean.  The quirk is kept.
 *   batch  dev f32 [4]      each term summed over the utterances in order and divided by max(total frames, 1): the script's clamp(min = 1)
 *                           makes an empty span give 0, not NaN (unlike the flow-matching loss above)
 * workspace: dev, 8-byte aligned, at least the bytes the _workspace entry answers (a negative F5_* code for a shape it refuses).  Shape limits
 * and refusals as for the flow-matching loss: F5_EINVAL with a message for a null pointer or B, N or mel below 1.  16-byte loads when mel % 4 == 0
 * and the four tensors are 16-byte aligned, element loads otherwise.  Nothing synchronises. */
F5_API int64_t f5_distill_loss_workspace(int B, int N, int mel);
F5_API int f5_distill_loss(int B, int N, int mel, const float* student, const float* teacher, const float* x1, const float* x0,
                           const uint8_t* span, double* sums, int64_t* frames, float* batch, void* workspace, f5_stream_t stream);

/* ------------------------------------------------------------------ duration validation (Trainer.calculate_duration_loss, trainer.py:829-1068)
 * The training target of the duration predictor and its loss, forward only, for judging a duration_predictor_*.pt checkpoint: the phoneme x
 * mel similarity, the monotonic alignment search (alignment_utils.py:337-355: "viterbi" and "window"; "progressive" is not built: the trainer's
 * AlignmentMethodManager never selects it), the durations of the alignment and the masked loss.  Detected by symbol.  All tensors dev f32 in
 * PyTorch layouts unless said otherwise; nothing synchronises; the same input gives the same bits on every run (no atomics).
 * Shapes: 1 <= nt <= 1024 (one lane per phoneme row), 1 <= T <= 65536, 1 <= B <= 65535; anything else is F5_EINVAL with a message.  nt and T
 * are those of the PADDED batch, exactly as in the reference, with a consequence that is kept, not repaired: an utterance with fewer
 * phonemes than nt has all -inf in its last rows, the viterbi backtrack finds no positive gradient there, and the last padded row takes the
 * utterance's whole length (durations [0, ..., 0, T]).
 *
 * Similarity (trainer.py:925-970): embed [rows, K]; ids dev i32 [B, nt], used raw (no +1; an id outside [0, rows) reads nothing and stands for
 * a zero row); phoneme_lens, mel_lens dev i32 [B]; melspec [B, T, mel]; proj [mel, K]; sim [B, nt, T].  K <= 768.
 *   e = embed[id] / (|embed[id]| + 1e-8);  m = (melspec @ proj) / (|melspec @ proj| + 1e-8);  sim = e . m  (fp32 FMA dot products)
 *   + 3.0 on columns [max(0, c - w), min(m_len, c + w)) of row p < p_len, c = (p * m_len) / p_len in integers (the reference's int(p * m_len /
 *     p_len) in float64 is the same integer for operands below 2^26), w = max(3, m_len / 10), where p_len > 0 and m_len > 0  (:949-962)
 *   -inf on rows >= p_len and columns >= m_len  (:965-970) */
F5_API int f5_align_similarity(int B, int nt, int T, int mel, int K, int rows, const float* embed, const int32_t* ids,
                               const int32_t* phoneme_lens, const float* melspec, const int32_t* mel_lens, const float* proj, float* sim,
                               f5_stream_t stream);
/* bytes of workspace the two searches take for a [B, nt, T] problem (one i32 per cell), or the negative F5_* code of a refused shape */
F5_API int64_t f5_align_workspace(int B, int nt, int T);
/* "viterbi" (alignment_utils.py:154-212).  sim [B, nt, T] -> durations [B, nt] = frames per row; alignment [B, nt, T] of 0 / 1, or NULL for
 * durations alone.  Forward, every add ONE fp32 add in this association, so P has the reference's bits (row 0 is a serial running sum):
 *   P[0,0] = s[0,0];  P[n,0] = P[n-1,0] + s[n,0];  P[0,t] = P[0,t-1] + s[0,t];  P[n,t] = s[n,t] + max(P[n-1,t], P[n,t-1])
 * as an anti-diagonal wavefront, one workgroup per utterance, nt + T - 1 dependent steps.  Backtrack (:184-210): curr = T - 1; for n = nt-1 .. 0:
 * boundary = the last t in [0, curr-1] with P[n,t+1] - P[n,t] > 0 in fp32 (NaN from -inf - -inf compares false), 0 if there is none or n = 0;
 * row n takes columns boundary..curr; curr = boundary - 1; stop when curr < 0 (rows above keep duration 0).  Every column belongs to one row.
 * workspace: dev, 4-byte aligned, f5_align_workspace bytes: per cell the index of the last positive gradient at or before it, which is all
 * the backtrack asks of P. */
F5_API int f5_align_viterbi(int B, int nt, int T, const float* sim, float* durations, float* alignment, void* workspace, f5_stream_t stream);
/* "window" (alignment_utils.py:214-258), same arguments (workspace is not used and may be NULL).  frames_per_phone = T / nt in double; row n <
 * nt - 1 ends at the first maximum of sim[n] (torch.argmax) over [max(start, e - w), min(T - 1, e + w)], e = (int)((n + 1) * frames_per_phone),
 * w = max(2, (int)(T * 0.2)); the next row starts behind it; stop when start >= T; the last row takes the rest.  Where that window is empty
 * (start > e + w: possible only when nt > T; the reference raises there) the row takes the single frame `start`. */
F5_API int f5_align_window(int B, int nt, int T, const float* sim, float* durations, float* alignment, void* workspace, f5_stream_t stream);
/* The loss (trainer.py:984-1025) over the elements n < phoneme_lens[b] (clamped to [0, nt]).  logw, durations [B, nt]; per element, in fp64 from
 * the fp32 inputs:  d = max(dur, 0.1);  sq = (logw - log(d + 1e-6))^2;  ab = |exp(clamp(logw, -10, 10)) - d|.  sq_sums, abs_sums dev f64 [B],
 * counts dev i64 [B] (8-byte aligned), added in a fixed order; loss_mae dev f32 [2] = (sum sq, sum ab) / (sum counts + 1e-8) over the batch, as
 * the trainer logs them.  An utterance of length 0 gives 0, 0, 0. */
F5_API int f5_duration_loss(int B, int nt, const float* logw, const float* durations, const int32_t* phoneme_lens, double* sq_sums,
                            double* abs_sums, int64_t* counts, float* loss_mae, f5_stream_t stream);

/* debug/parity taps: after the next f5_dit_forward / f5_sample evaluation, copy the named internal stage
 * (converted to f32, row-major [rows, cols]) into `dst` (dev f32).  Names: "t_sin" (the 256 sinusoid features of every time), "t_emb",
 * "adaln" (the AdaLN modulation rows of every block and the final norm, [times, the model's modulation width]; DiT and MMDiT),
 * "input_embed", "blk<i>.n1", "blk<i>.attn", "blk<i>.out", "final_norm".  Pass dst = NULL to clear all taps. */
F5_API int f5_plan_set_tap(f5_plan_t p, const char* stage, float* dst);
/* Stage probes of the DiT backbone: as a tap, copy a named internal stage (f32, row-major) into `dst` (dev f32) -- but of the evaluation as it
 * runs WITHOUT them.  A tap switches the fp16 residual stream, the in-place residual epilogues, the LayerNorm fold and pre-scaled q off; a probe
 * enters no mode decision: it is a copy of a buffer the evaluation holds anyway, of its token rows only (never the padding rows of the block
 * GEMMs).  One evaluation writes them: f5_dit_forward's, or evaluation number "probe_eval" (f5_plan_set_option; default 0) of a sample loop.
 * While probes are set f5_sample* runs the loop eagerly and neither launches nor captures a graph; f5_sample_ragged* accepts probes.  Names
 * (J = position of the block in the walk, D = dim):
 *   "adaln"            this evaluation's AdaLN row                                                        [modulation width]
 *   "base"             the hoisted half of the input embedding (fp32; the x-projection adds its fp16 copy)   [rows, D]
 *   "input_embed"      the stream before block 0's first LayerNorm pass                                   [rows, D]
 *   "blk0.x_in"        the stream after that pass has added the position-conv branch (in-place stream)    [rows, D]
 *   "blkJ.n1"          the first LayerNorm pass's output (J = 0; every J of an unfolded evaluation)       [rows, D]
 *   "blkJ.stats1" J>0, "blkJ.stats2"   (mean, rstd) as the folded QKV / FF1 launch of block J consumed them    [rows, 2]
 *   "blkJ.qkv"         q|k|v after RoPE, q as the attention kernel reads it                               [rows, 3 inner]
 *   "blkJ.ctx"         attention output                                                                   [rows, inner]
 *   "blkJ.x_attn", "blkJ.x_ff"   the in-place stream after the out-projection / after FF2                 [rows, D]
 *   "blkJ.ff1"         FF1 output                                                                         [rows, ff]
 *   "final_norm", "vout"                                                                                  [rows, D], [rows, mel]
 * An unknown name is F5_EINVAL here (another backbone: F5_ENOTSUP).  A name whose buffer the running mode does not hold ("blk1.n1" under the
 * fold, "blk0.x_attn" on an fp32 stream) is F5_ESTATE from the call that would write it, before it stages an input or launches an evaluation.
 * stage = NULL or dst = NULL clears all probes.  Captured graphs are left alone. */
F5_API int f5_plan_set_probe(f5_plan_t p, const char* stage, float* dst);
/* in-situ timing of the dominant kernel: between begin and end, every fused-QKV GEMM launch of (eager) f5_sample /
 * f5_dit_forward calls on this plan is bracketed by a HIP event pair on the caller's stream; end synchronises the stream and
 * returns the mean device time per launch.  Used by bench.py for roofline.achieved. */
F5_API int f5_plan_timing_begin(f5_plan_t p, int max_launches);
F5_API int f5_plan_timing_end(f5_plan_t p, float* avg_ms, int* launches, f5_stream_t stream);
/* the same measurement for every kernel of a DiT evaluation: after f5_plan_timing_end, mean device time per launch of call site
 * `site`.  The event pairs live in a bounded ring of 512 pairs created once per plan (round 4; `max_launches` is accepted and ignored): when
 * the ring is full its older half is folded into the per-site sums, so any number of launches is covered with 1 024 live events. */
#define F5_SITE_QKV 0   /* fused QKV projection + RoPE            modules.py:452-461 */
#define F5_SITE_ATTN 1  /* scaled-dot-product attention           modules.py:483-497 */
#define F5_SITE_OUT 2   /* attention out-projection x gate_msa    modules.py:499-501,635 */
#define F5_SITE_FF1 3   /* FeedForward first linear + GELU(tanh)  modules.py:258-264 */
#define F5_SITE_FF2 4   /* FeedForward second linear x gate_mlp   modules.py:639 */
#define F5_SITE_LN1 5   /* residual add + AdaLN before attention  modules.py:301-317,632 */
#define F5_SITE_LN2 6   /* residual add + AdaLN before the FF     modules.py:637-638 */
#define F5_SITE_CONV 7  /* grouped Conv1d(k=31) + Mish (x2)       modules.py:167-190 */
#define F5_SITE_INPUT 8 /* input projection of the noisy mel      dit.py:88-96 */
#define F5_SITE_COUNT 9
F5_API int f5_plan_timing_site(f5_plan_t p, int site, float* avg_ms, int* launches);
/* kernel selection for A/B runs: key "gemm_kernel" / "attn_kernel"; value 0 = reference tile kernels, 1 or -1 = tuned
 * kernels wherever they support the problem (default).  Drops any captured graphs.
 * Residual-stream storage of the bf16 mode: key "residual_f16": 1 = fp16 (saturating), 0 = fp32, -1 = the process-wide
 * knob (default: fp16); key "residual_guard" (default 1): f5_sample reads, after the ODE loop, the flag word the LayerNorm passes raise when
 * an element of the fp16 stream reaches +-65504 or is NaN, repeats the loop with fp32 storage and keeps fp32 storage for this plan
 * (f5_sample then synchronises the stream once per call; 0 = no read, fully asynchronous, clipping goes unnoticed; 2 = the read is
 * deferred to f5_sample_finish).
 * Key "attn_prescale" (default -1 = the process-wide knob, which is on): 1 = the softmax scale times log2(e) is folded into the weights that
 * project q and the attention kernels apply none (bf16 DiT on the tuned attention kernels, no qk_norm, no stage taps, LayerNorm-fold
 * evaluations; everything else keeps q as projected), 0 = q as projected everywhere.  An F5_PREC_FP16 plan never pre-scales q, whatever the key says:
 * the reference-free attention build needs bf16's exponent range.
 * Key "probe_eval" (default 0, >= 0): the evaluation of a sample loop that writes the stage probes (f5_plan_set_probe); host-side only. */
F5_API int f5_plan_set_option(f5_plan_t p, const char* key, int value);
/* reads an option back; besides the keys above: "residual_fallbacks" = f5_sample calls of this plan that were repeated with fp32 residual
 * storage because the range guard fired ("residual_f16" then reads 0); "attn_prescale_active" = 1 when this plan wants pre-scaled q and may run it (0 e.g.
 * while a stage tap is set).  That is the plan's part only: an evaluation uses pre-scaled q where it also runs the LayerNorm fold, which
 * under automatic kernel choice needs at least 512 token rows and a time grid of at most 64 evaluation times -- a smaller call on a plan
 * that reports 1 still runs q as projected.
 * "graph_captures" / "graph_replays" (read-only; f5_plan_set_option refuses them as unknown keys): counters over the plan's life of the sample
 * loops of f5_sample* (use_graph != 0) and f5_sample_ragged* ("ragged_graph" = 1).  A loop that found no hipGraph of its key captured one and
 * launched it: graph_captures + 1, graph_replays unchanged (a capture's own launch is no replay).  A loop that launched a graph captured by
 * an earlier call: graph_replays + 1.  An eager loop raises neither; the fp32 rerun of the range guard is a loop of its own.  Dropping the
 * plan's graphs (a changed kernel option, tuning knob, block subset, dropout setting) does not reset them. */
F5_API int f5_plan_get_option(f5_plan_t p, const char* key, int* value);
/* Attention dropout, opt-in: the reference's F.scaled_dot_product_attention(dropout_p = 0.1) stays live under
 * model.eval() (modules.py:490, :582).  prob in [0, 1), 0 = off (the default: every output bit and launch as without this call).  With it on,
 * every attention call of the plan drops probabilities with the mask
 *   (o0..o3) = Philox4x32-10(counter = (k >> 2, q, bw * H + head, stream), key = (seed & 0xffffffff, seed >> 32)),
 *   keep(q, k) = o[k & 3] >= T,   out[q] = sum_k keep(q, k) P[q, k] v[k] / (1 - p),   P = softmax over all valid keys;
 *   T = round(p * 2^32), p = the shortest decimal that rounds to the float `prob` (0.1f -> 0.1, T = 429496730; the same p divides);
 * q / k: positions in the sequence the softmax runs over (UNetT: the time token is 0; MMDiT: [frames | text]); stream = base + e * depth + l
 * for block l of evaluation e of the call (solver order); bw = row of the CFG-doubled batch in f5_sample* (branch * B + b, the null half
 * second; f5_sample_ragged: branch * B + u), b in the forwards.  base is a device word of the plan: a sample advances it by evals * depth, a
 * forward by depth, a replayed graph too.  The call resets base to 0 and drops captured graphs.  The mask stream is this library's own,
 * not torch's: a run matches the reference in distribution, never bit for bit.  While it is on, q is never pre-scaled
 * ("attn_prescale_active" reads 0) and a ragged sample() is not bit-equal to its batch-1 calls.  f5_plan_get_option keys:
 * "attn_dropout_on", "attn_dropout_base" (host mirror of base).  prob > 0 on an F5_PREC_FP16 plan: F5_ENOTSUP (the dropout kernel is bf16 / fp32). */
F5_API int f5_plan_set_attn_dropout(f5_plan_t p, float prob, uint64_t seed);
/* Block subset (layer pruning, reference src/model_pruning): the plan runs only the listed blocks of its DiT, on the weights
 * already in HBM.  blocks_host: host i32 [count], strictly increasing, each in [0, depth), count >= 1; NULL with count 0 restores all blocks
 * (every launch and bit as before the first call).  Detected by symbol.  A plan with subset S behaves as a plan of the model whose blocks are S
 * renumbered 0 .. |S| - 1: position j of the walk takes the weights, AdaLN rows and prefetch sets of block S[j], and whatever speaks of the
 * first, previous or last block (the position-conv branch, the long-skip copy, the tap names "blk<j>.*", the range-guard tags, the dropout
 * call word base + e * |S| + j) speaks of positions.  f5_dit_forward and every f5_sample* entry honour it.  The LayerNorm fold and pre-scaled q
 * are off under a subset -- a list of ALL blocks included -- since the fold table and block 0's second weight copy are laid out for the full
 * depth; no table is built or held for such a call.  Refused before anything changes: F5_ENOTSUP for UNetT (skip connections pair its layers)
 * and MMDiT, F5_EINVAL for an empty, out-of-range or non-increasing list.  Completes a deferred sample() first and drops captured graphs. */
F5_API int f5_plan_set_blocks(f5_plan_t p, const int32_t* blocks_host, int count);
/* reads the subset back: returns its size (0 = none set) and writes the first min(size, cap) entries to blocks_host (may be NULL when cap = 0) */
F5_API int f5_plan_get_blocks(f5_plan_t p, int32_t* blocks_host, int cap);

/* ------------------------------------------------------------------ duration predictor
 * Replaces DurationPredictor.forward / .phoneme_forward (reference model/duration_predictor.py:28-46 / :48-68) as called from
 * F5TTSWrapper.calculate_duration_with_predictor (infer/f5tts_wrapper.py:381-406).  All tensors f32 on the device, PyTorch layouts:
 *   text_embed [vocab_rows, in_channels]; conv1_w [filter, in_channels, k]; conv2_w [filter, filter, k]; norm*_w/b [filter];
 *   proj_w [filter] (the [1, filter, 1] Conv1d weight); proj_b [1]; cond_w / cond_b of the optional speaker conditioning (f5_duration_predict_g). */
typedef struct f5_duration_weights {
    const float *text_embed, *conv1_w, *conv1_b, *norm1_w, *norm1_b, *conv2_w, *conv2_b, *norm2_w, *norm2_b, *proj_w, *proj_b;
    int32_t vocab_rows, in_channels, filter_channels, kernel_size;
    const float *cond_w, *cond_b; /* speaker conditioning Conv1d(gin -> in_channels, 1): [in_channels, gin] and [in_channels]; NULL when gin_channels = 0 */
    int32_t gin_channels;
} f5_duration_weights;
/* tokens i32 [batch, nt] (pad -1), add_one = 1 for forward() (ids shifted so that 0 is the filler), 0 for phoneme_forward();
 * mask i32 [batch, nt] (1 = real token); scratch f32 [2 * batch * filter_channels * nt]; out f32 [batch, nt] = log-durations * mask. */
F5_API int f5_duration_predict(const f5_duration_weights* w, int batch, int nt, const int32_t* tokens, int add_one, const int32_t* mask,
                        float* scratch, float* out, f5_stream_t stream);
/* the same with the speaker conditioning of duration_predictor.py:33-35: x = embedding + cond(g), g dev f32 [batch, gin_channels, g_nt] with
 * g_nt = 1 (one vector per utterance, broadcast over the tokens) or nt; scratch f32 [2 * batch * filter_channels * nt + batch * in_channels * g_nt];
 * g = NULL is f5_duration_predict. */
F5_API int f5_duration_predict_g(const f5_duration_weights* w, int batch, int nt, const int32_t* tokens, int add_one, const int32_t* mask,
                          const float* g, int g_nt, float* scratch, float* out, f5_stream_t stream);

/* ------------------------------------------------------------------ per-op entry points (parity tests, micro-benchmarks) */
/* out[M,N] = A[M,K] @ W[N,K]^T + bias ; A/W/out f32 dev; computed through the precision's GEMM kernel
 * (bf16 / fp16: inputs rounded to the 16-bit type on device, MFMA, f32 accumulate).  act: 0 none, 1 gelu-tanh, 2 gelu-erf, 3 mish.
 * kernel: 0 = reference tile kernel, 1 = tuned 256x256 LDS-DMA kernel (bf16 / fp16; shapes must be tile multiples). */
F5_API int f5_op_linear(int precision, int kernel, int M, int N, int K, const float* A, const float* W, const float* bias, int act,
                 float* out, f5_stream_t stream);
/* One DiT block linear with the fused store epilogue the sampler uses for it (bf16 path; output converted back to f32):
 *   epi 0: out = act(A W^T + b)                                      FeedForward first linear, reference model/modules.py:258-264
 *   epi 5: out = gate[n] * act(A W^T + b), rows with rowmask[m]==0 -> 0  attention to_out / FF second linear times the AdaLN gate,
 *                                                                    modules.py:499-501,635,639 (gate f32 [N] or NULL, rowmask u8 [M] or NULL)
 *   epi 2: out = out + gate[n] * (A W^T + b) IN PLACE on the fp16 residual stream (`out` is read, rounded to fp16, updated, returned as f32;
 *          rows with rowmask[m]==0 keep their value; M * N % 4 == 0): how the attention to_out and the FF second linear update the stream
 *          in the bf16 production mode, modules.py:635,639
 *   epi 4: out = rope(A W^T + b): fused QKV projection (N = 3*inner), x_transformers rotary on adjacent pairs of the q and k columns
 *          of the first rope_heads heads, modules.py:452-461; rope f32 [seq][32][2] (cos, sin), token position = m % seq
 * kernel: 0 = reference tile kernel, 1 = tuned kernels.  All pointers are device pointers. */
F5_API int f5_op_linear_fused(int kernel, int epi, int M, int N, int K, const float* A, const float* W, const float* bias, int act,
                       const float* gate, const uint8_t* rowmask, const float* rope, int rope_heads, int seq, float* out,
                       f5_stream_t stream);
/* f5_op_linear_fused in the 16-bit mode `precision` (F5_PREC_BF16 = f5_op_linear_fused itself, F5_PREC_FP16) */
F5_API int f5_op_linear_fused_p(int precision, int kernel, int epi, int M, int N, int K, const float* A, const float* W, const float* bias, int act,
                         const float* gate, const uint8_t* rowmask, const float* rope, int rope_heads, int seq, float* out,
                         f5_stream_t stream);
/* The LayerNorm fold of one call site end to end (round 4; parity tests).  x [M, D]: the fp16 residual stream, handed over and returned as f32.
 * (1) x += gate * (A . Wo^T + bo) in place by the tuned GEMM's EPI_RESID epilogue, which also writes partial row sums of the values it stores
 * (pivot = column 0 of `pivot` [M][2], or NULL); (2) stats [M][2] = (mean, rstd) of every row, eps 1e-6 (modules.py:308,624); (3) W' = fp16(W (1 +
 * scale)), c1 = rowsum W', c2 = bias + W . shift; (4) out [M, N] = epilogue(rstd (x . W'^T - mean c1) + c2) on v_mfma_f32_16x16x32_f16 --
 * epi 0: store with `act` (FF1 + GELU: modules.py:258-264, 637-638), epi 4: RoPE on the q | k columns (fused QKV: modules.py:301-317, 452-480). */
F5_API int f5_op_ln_fold(int epi, int M, int D, int N, int Kb, float* x, const float* A, const float* Wo, const float* bo, const float* gate,
                         const float* pivot, const float* W, const float* bias, const float* scale, const float* shift, int act, const float* rope,
                         int rope_heads, int seq, float* stats, float* out, f5_stream_t stream);
/* f5_op_ln_fold in the 16-bit mode `precision`: the stream, the statistics and W' are fp16 in both; A, Wo and the output take the mode's type */
F5_API int f5_op_ln_fold_p(int precision, int epi, int M, int D, int N, int Kb, float* x, const float* A, const float* Wo, const float* bo,
                           const float* gate, const float* pivot, const float* W, const float* bias, const float* scale, const float* shift, int act,
                           const float* rope, int rope_heads, int seq, float* stats, float* out, f5_stream_t stream);
/* The producer half of a LayerNorm-fold site on its own (parity tests of the in-place epilogue): x [M, N] (the fp16 residual stream as f32) +=
 * gate * (A . W^T + bias) on the rows where rowmask[m] != 0 (NULL: all), by the tuned GEMM's EPI_RESID epilogue in the 16-bit mode `precision`;
 * planes [N / 64][M][2] = its partial row sums per 64-feature plane (pivot = column 0 of `pivot` [M][2], or NULL), stats [M][2] = the (mean, rstd)
 * stats_finalize makes of them, guard = the six words of the fp16 range guard after the finalize (NULL: not returned).  N % 128 == 0, K % 32 == 0. */
F5_API int f5_op_resid_stats_p(int precision, int M, int N, int K, float* x, const float* A, const float* W, const float* bias, const float* gate,
                               const uint8_t* rowmask, const float* pivot, float* planes, float* stats, unsigned* guard, f5_stream_t stream);
/* LayerNorm(eps 1e-6, no affine) * (1 + scale) + shift ; x f32 [rows, dim]; scale/shift f32 [dim] */
F5_API int f5_op_layernorm_modulate(int rows, int dim, const float* x, const float* scale, const float* shift, float* out,
                             f5_stream_t stream);
/* multi-head attention on packed projections: qkv f32 [B, N, 3, H, 64] (already RoPE'd), mask u8 [B,N] or NULL
 * -> out f32 [B, N, H*64].  kernel: 0 = reference kernel, 1 = tuned flash kernel (bf16). */
F5_API int f5_op_attention(int precision, int kernel, int B, int N, int H, const float* qkv, const uint8_t* mask, float* out,
                    f5_stream_t stream);
/* f5_op_attention with the dropout mask of f5_plan_set_attn_dropout: call word `stream_word`, batch item b drawn with batch word batch0 + b.
 * kernel 0 = the reference kernel's dropout build, 1 = the MFMA flash kernel with dropout (bf16).  prob == 0 gives f5_op_attention's bits. */
F5_API int f5_op_attention_dropout(int precision, int kernel, int B, int N, int H, const float* qkv, const uint8_t* mask, float prob,
                                   uint64_t seed, uint32_t stream_word, uint32_t batch0, float* out, f5_stream_t stream);
/* The same on PRE-SCALED q (bf16 only): the q part of `qkv` already holds softmax_scale * log2(e) = 0.125 * 1.4426950408889634 times the
 * projected q, the form the production path's q projection stores when the plan option "attn_prescale" is active.  The
 * kernels apply no scale; the 64-queries-per-wave kernel runs its reference-free build with its two range guards. */
F5_API int f5_op_attention_prescaled(int kernel, int B, int N, int H, const float* qkv, const uint8_t* mask, float* out, f5_stream_t stream);
/* The LayerNorm fold's table builder on one block and one evaluation time (parity tests): W f32 [R, D], bias [R], (scale, shift) [D] of the
 * attention norm (rows < qkv_rows) and of the FF norm (the other rows) -> Wt f32 [R, D] = the fp16 values of W (1 + scale), c1 [R] = their row
 * sums, c2 [R] = bias + W . shift.  qscaled != 0: the first q_rows rows (the q projection) carry softmax_scale * log2(e), applied in fp32
 * ahead of the rounding. */
F5_API int f5_op_fold_weights(int R, int qkv_rows, int q_rows, int D, int qscaled, const float* W, const float* bias, const float* scale_msa,
                              const float* shift_msa, const float* scale_mlp, const float* shift_mlp, float* Wt, float* c1, float* c2,
                              f5_stream_t stream);
/* The attention call of the ragged sampler (f5_sample_ragged) on its own: `cnt` utterances of lengths n[u] at row offsets off[u] (host int
 * arrays) inside each of `nbr` branches that lie `rows` rows apart (the batch stride of every launch).  qkv f32 [nbr * rows, 3*H*64 +
 * ldq_extra], out f32 [nbr * rows, H*64 + ldo_extra] (the extras widen the leading dimensions, normally 0).  attn_kernel 0 = reference
 * kernels only, non-zero = the sampler's own selection (shared pipelined launches, or a launch of its own, per utterance).  `out` is staged
 * into the precision's dtype before the launches, so every element no launch writes comes back as the caller left it.  Refused before any
 * launch: n[u] < 1, off[u] < 0, off[u] + n[u] > rows. */
F5_API int f5_op_attention_ragged(int precision, int attn_kernel, int nbr, int cnt, const int* off, const int* n, int H, int rows,
                                  int ldq_extra, int ldo_extra, const float* qkv, float* out, f5_stream_t stream);
/* ConvPositionEmbedding (modules.py:167-190): x f32 [B, N, dim] -> mish(conv(mish(conv(x)))) ; weights f32
 * [dim, dim/16, 31] + bias [dim] (two layers) */
F5_API int f5_op_conv_pos_embed(int precision, int B, int N, int dim, const float* x, const float* w0, const float* b0,
                         const float* w1, const float* b1, float* out, f5_stream_t stream);
/* One of its convolutions alone (test hook): out f32 [B, N, dim] = act(conv(x) + b), grouped Conv1d(k = 31, groups = 16, padding 15) with exactly
 * the launch parameters of the first convolution above, the precision's dtype in and out.  act: 0 = none, 3 = mish.  kernel 0 = the reference
 * tile kernel, 1 = the tuned route as the model takes it (knobs "conv31", "conv31_tok"; the 16-bit modes). */
F5_API int f5_op_conv31(int precision, int kernel, int B, int N, int dim, const float* x, const float* w, const float* b, int act, float* out,
                        f5_stream_t stream);
/* The reference 64 x 64 tile kernel -- the only GEMM of the fp32 mode, of Vocos, BigVGAN and the mel front-end -- with every parameter its
 * epilogues branch on in the caller's hands (test hook; detect it by symbol).  All tensors f32 on the device, converted there.
 *   mode 0 (dense):   A [a_row_mod > 0 ? a_row_mod : M, K] (row m reads A[m % a_row_mod]), W [N, K], K % 32 == 0
 *   mode 1 (conv31):  A = x [M, N] with M = batches * rows_per_batch token rows and N = dim (dim % 128 == 0), W [dim, dim / 16, 31]; K unused
 *   epi  0  out_t = act(acc + bias)                          1  out_f = act(acc + bias)                     (dense only)
 *        2  out_f += gate * act(acc + bias) in place, rows with rowmask[m] == 0 untouched
 *        3  v = acc + bias + addend [M, ldadd];  out_t = v, out_f = v                                      (dense only)
 *        4  out_t = rope(acc + bias): N = 3 * inner, rope [rows_per_batch][32][2] (cos, sin), first rope_heads heads   (dense only)
 *        5  out_t = gate * act(acc + bias), rows with rowmask[m] == 0 zeros
 *   gate [N] (gate_bstride 0) or [batches][gate_bstride], batch = m / rows_per_batch (0: one batch of M rows); rowmask u8 [M]; both or NULL
 *   add2_f16 (epi 2 / 3): out_f and the addend hold fp16 elements, as in the bf16 mode's residual stream
 *   out_t [out_rows, ldo] is staged whole into the precision's type (a plain cast: NaN stays NaN), handed to the kernel and staged back whole;
 *   out_f [out_rows, ldof] is the kernel's own buffer (fp32), or staged the same way through fp16 (add2_f16).  out_rows >= M, ldo / ldof >= N,
 *   any alignment: what the kernel does not write -- padding columns, guard rows -- comes back as the caller left it. */
typedef struct f5_tile_gemm {
    const float *A, *W, *bias, *gate, *rope, *addend;
    const uint8_t* rowmask;
    float *out_t, *out_f;
    int32_t precision, mode, epi, M, N, K, a_row_mod, act, gate_bstride, rows_per_batch, rope_heads, ldadd, add2_f16, ldo, ldof, out_rows;
} f5_tile_gemm;
F5_API int f5_op_tile_gemm(const f5_tile_gemm* g, f5_stream_t stream);

/* Test and diagnostic entry points of the row-wise kernels: each stages its f32 device inputs into the dtypes the model path uses and calls
 * the production launcher, so the launcher's own dispatch (and its tuning knobs) decides which kernel runs.  All pointers are device pointers.
 *
 * The LayerNorm pass of the residual stream (launch_layernorm_res): x [rows, ldx] is the stream, staged as fp16 (xin_f16; an exact cast, so
 * the caller pre-rounds it) or fp32; y, y2 [rows, ldy] the residual branches (bf16 in the bf16 mode); ymode 0 = x, 1 = x + y written back,
 * 2 = x + y not written back, 3 = (x + y) + y2 written back; mul / add f32 [nb][mod_bstride] (or [dim] when mod_bstride = 0), batch =
 * row / rows_per_batch; out [rows, ldo] = LN(v) * (add_one + mul) + add in the precision's dtype, returned as f32 (columns past dim stay 0).
 * inplace = 1 writes the stream back into its own buffer (the only form that takes the multi-row kernel), 0 into a zeroed one of the same
 * leading dimension and storage type xout_f16; xback [rows, ldx] receives that buffer as f32.  guard (u32 [6] or NULL): the range guard's
 * words (flag, largest finite |element| as float bits, NaN seen, pass bits, block bits, 0x7fffffff - smallest offending row), zeroed
 * before the launch; sat_tag as the model passes it (pass | block << 4). */
F5_API int f5_op_layernorm_res(int precision, int xin_f16, int xout_f16, int rows, int dim, int ldx, int ldy, int ldo, const float* x,
                               const float* y, const float* y2, int ymode, const float* mul, const float* add, int mod_bstride,
                               int rows_per_batch, int add_one, int inplace, int sat_tag, float* out, float* xback, uint32_t* guard,
                               f5_stream_t stream);
/* The saturating fp32 -> fp16 copy of the hoisted input embedding (launch_f32_to_f16): dst f32 [n] = the fp16 values, widened; guard as above */
F5_API int f5_op_f32_to_f16(int64_t n, const float* src, float* dst, uint32_t* guard, f5_stream_t stream);
/* qk_norm = "rms_norm" (launch_qknorm_rope): qkv f32 [rows, 3 * heads * 64] -> out, q and k of every head RMS-normalised over 64 features
 * (eps 1e-6; weights wq, wk f32 [64]), then rotated on the first rope_heads heads by rope f32 [rows_per_batch][32][2] (cos, sin) at position
 * row % rows_per_batch; the v third is copied through.  The precision's dtype in between. */
F5_API int f5_op_qknorm_rope(int precision, int rows, int heads, int rope_heads, int rows_per_batch, const float* qkv, const float* wq,
                             const float* wk, const float* rope, float* out, f5_stream_t stream);
/* ConvNeXtV2 depthwise conv (k = 7, zero padding 3 inside each utterance) + LayerNorm(affine, eps 1e-6) (launch_dwconv7_ln): x f32 [B, N, C],
 * wt f32 [7][C], cbias / ln_w / ln_b f32 [C] -> out f32 [B, N, C] (the precision's dtype in between) */
F5_API int f5_op_dwconv7_ln(int precision, int B, int N, int C, const float* x, const float* wt, const float* cbias, const float* ln_w,
                            const float* ln_b, float* out, f5_stream_t stream);
/* ConvNeXtV2 GRN (launch_grn): h f32 [B, N, C] staged in the precision's dtype; out = gamma (h Nx) + beta + h with Nx = G / (mean_c G + 1e-6),
 * G[b][c] = ||h[b, :, c]||_2 over the utterance's N tokens */
F5_API int f5_op_grn(int precision, int B, int N, int C, const float* h, const float* gamma, const float* beta, float* out, f5_stream_t stream);
/* RMSNorm of UNetT (launch_rmsnorm): out = x / max(||x||_2, 1e-12) * sqrt(dim) * g ; x f32 [rows, dim], g f32 [dim] */
F5_API int f5_op_rmsnorm(int precision, int rows, int dim, const float* x, const float* g, float* out, f5_stream_t stream);

/* in-process kernel timing for the roofline leg of bench.py: `iters` back-to-back launches of ONE kernel bracketed by HIP
 * events on `stream`, random bf16 operands; *ms_avg = mean device time per launch.
 * site: 0 fused QKV projection + RoPE, 1 FF1 + GELU-tanh, 2 FF2 + gated residual, 3 attention out-projection + gated residual. */
F5_API int f5_bench_gemm_site(int kernel, int site, int rows, int seq, int dim, int heads, int ff_inner, int iters, float* ms_avg,
                       f5_stream_t stream);
F5_API int f5_bench_attention(int kernel, int B, int N, int H, int iters, float* ms_avg, f5_stream_t stream);
/* Sustained rate of a register-resident v_mfma_f32_16x16x32_bf16 stream on every CU (no memory traffic): random_operands = 0 zeros
 * (clock-limited), 1 pseudo-random bf16 values (power-limited: what a dense bf16 GEMM can approach on this device). */
F5_API int f5_bench_mfma_rate(int random_operands, float* tflops, f5_stream_t stream);
/* the clock the chip holds under the tuned GEMM: while dev_buf (dev u64 [workgroups * 4]) is non-NULL every workgroup writes (s_memtime,
 * s_memrealtime) at its start and end; clock = d(s_memtime) / d(s_memrealtime) x 100 MHz */
F5_API int f5_debug_gemm_clock(void* dev_buf);
/* What the last GEMM / conv31 launcher of this process launched (a host-side record; tests that force a tile prove with it that the tile ran):
 * family 0 = reference tile kernel, 1 = tuned 8-wave kernel, 2 = one-wave-per-SIMD kernel, 3 = conv31 (-1: nothing launched yet); bm x bn = token x
 * feature tile (conv31: tokens per workgroup x 64); schedule 0 = plain ring, 1 = staggered wave groups, 2 = persistent grid; flags: 1 = fp16
 * elements, 4 = fp32 elements (neither: bf16), 2 = LayerNorm-fold build, 8 = grouped conv as an implicit GEMM. */
F5_API int f5_debug_last_gemm(int* family, int* bm, int* bn, int* schedule, int* flags);
/* the same record for the last launch of one of the DiT block's four call sites -- site 1 the QKV projection, 2 the out-projection, 3 FF1, 4 FF2 --
 * and the number of launches that site has made in this process so far (a QKV projection that launches v apart makes two per block). */
F5_API int f5_debug_site_gemm(int site, int* family, int* bm, int* bn, int* schedule, int* flags, int* launches);
/* Which launch forms one DiT evaluation of nb x N token rows takes in the plan's present state (its options, stage taps, block subset, the fold
 * table and evaluation index its last call left, the tuning knobs in force); per_batch_rows != 0: per-sample times, as f5_dit_forward evaluates.
 * The function the evaluation itself decides with, called alone: no launch, no side effect.  out[F5_EVAL_MODES_N] = rows, rows_g (rows the block
 * GEMMs run over), defer, r16 (fp16 stream), rmw (in-place residual epilogues), lnf (LayerNorm fold), qs (pre-scaled q), wpf (weight prefetch),
 * ink_qkv, ink_ff1 (the folded projection finishes its row statistics in its own kernel), split_v (the tile arithmetic projects v apart from
 * q|k; the launch further needs a 16-bit mode, the tuned kernel and a fused projection the one-wave-per-SIMD kernel does not take), frow0 (first
 * fold-table row of the evaluation time).  F5_ENOTSUP on the other backbones; F5_ESTATE as the evaluation itself would refuse. */
#define F5_EVAL_MODES_N 12
F5_API int f5_debug_eval_modes(f5_plan_t plan, int nb, int N, int per_batch_rows, int32_t* out);
/* process-wide kernel tuning knobs for A/B measurements ("gemm_variant": main-loop schedule of the tuned GEMM) */
F5_API int f5_tuning_set(const char* key, int value);
/* The value a knob holds now (no side effect; F5_EINVAL for a null argument or an unknown key), and the key of knob `index` in the library's
 * table, NULL past the end: together they enumerate every knob with its value. */
F5_API int f5_tuning_get(const char* key, int* value);
F5_API const char* f5_tuning_key(int index);

/* ------------------------------------------------------------------ Vocos vocoder (plug point B) */
typedef struct f5_vocos_config {
    int32_t n_mels;    /* 100 */
    int32_t dim;       /* 512 */
    int32_t inter_dim; /* 1536 */
    int32_t layers;    /* 8 */
    int32_t n_fft;     /* 1024 */
    int32_t hop;       /* 256 */
} f5_vocos_config;
F5_API int f5_vocoder_create(const f5_vocos_config* cfg, f5_vocoder_t* out);
F5_API int f5_vocoder_set_tensor(f5_vocoder_t v, const char* name, const float* host_data, const int64_t* shape, int ndim);
F5_API int f5_vocoder_has_tensor(f5_vocoder_t v, const char* name, int64_t* numel);
/* Uploads the tensors.  F5_EINVAL when the final ISTFT window (periodic Hann, or the caller's "head.istft.window") violates the NOLA condition
 * at (n_fft, hop): min over j < hop of sum_m w^2[j + m * hop] below 1e-11, torch.istft's own threshold -- the overlap-add would divide by
 * zero and write NaN (e.g. Hann at hop == n_fft).  Only this steady-state envelope is judged: zeros that a custom window produces under
 * fewer frames than one full overlap are not detected. */
F5_API int f5_vocoder_finalize(f5_vocoder_t v);
F5_API int f5_vocoder_destroy(f5_vocoder_t v);
/* Vocos.decode: mel dev f32 [B, n_mels, T] -> wave dev f32 [B, (T-1)*hop] */
F5_API int f5_vocoder_decode(f5_vocoder_t v, int B, int T, const float* mel, float* wave, f5_stream_t stream);
/* Vocos.decode for B utterances of DIFFERENT frame counts in one set of launches (round 5): what f5_sample_ragged produced, decoded together.
 * mel is dev f32, FRAME-major [rows, ld] (ld >= n_mels: the sampler's own layout, no permute / contiguous copy); utterance i reads the
 * frames_host[i] >= 2 rows from row row_start_host[i] on (so a prompt prefix is skipped by the offset) and writes its (T_i - 1) * hop samples
 * behind those of utterance i - 1 into wave, dev f32 [sum (T_i - 1) * hop]; *total_samples (host, may be NULL) receives that sum.  Both arrays
 * are host memory, read before the call returns.  Utterance i is bit-identical to f5_vocoder_decode(v, 1, T_i, its own [n_mels, T_i] mel): the
 * convolutions pad with zeros at each utterance's own ends and never read a neighbour's rows, whatever those hold.  Nothing synchronises
 * (workspace growth aside, as for f5_vocoder_decode). */
F5_API int f5_vocoder_decode_ragged(f5_vocoder_t v, int B, const int32_t* row_start_host, const int32_t* frames_host, const float* mel, int ld,
                                    float* wave, int64_t* total_samples, f5_stream_t stream);
/* The tail behind the vocoder in ONE kernel (round 5): rms gain, linear cross-fade of consecutive utterances, int16 PCM -- byte for byte what
 * the host path gives (torch's `wave * rms / target_rms` where rms < target_rms, utils_infer.cross_fade_concat, streaming.wire.pcm16_bytes).
 *   wave            dev f32, the B utterances back to back, samples_host[i] > 0 samples each (host array)
 *   gain            either gain_host[B] + apply_host[B] (host: utterance i is multiplied by gain_host[i] and divided by target_rms where
 *                   apply_host[i] != 0 -- the caller has taken the decision `rms_i < target_rms` on the host values it already holds), or
 *                   rms_dev, a dev f32 scalar: the gain applies to every utterance when *rms_dev < target_rms, decided in the kernel, so the host
 *                   never waits for it; neither: no gain.  Always one fp32 multiply, then the division: gain_div = 1 an IEEE fp32 divide (torch
 *                   on CPU tensors), 0 a multiply by the fp32 reciprocal 1.0f / target_rms (torch's device kernel for a host-scalar divisor)
 *   cross-fade      n = xfade_samples (0: none; B = 1: none) samples of consecutive utterances overlap: out = double(a) * w_down[j] +
 *                   double(b) * w_up[j] as two fp64 products and one fp64 sum, w_down / w_up dev f64 [n] = numpy's linspace(1, 0, n) / (0, 1, n).
 *                   The first and the last utterance must hold n samples and every other 2 n; otherwise the reference's sequential joints mix an
 *                   already mixed region, which this kernel does not do: F5_ENOTSUP, take the host functions for that call
 *   outputs         each may be NULL: out_f32 (only when no joint mixed), out_f64 (only when one did: numpy promotes the whole signal to
 *                   float64 then), out_pcm16 = trunc(x * 32767) with the product in the float output's precision; products at or beyond
 *                   +-32768, which numpy's cast leaves undefined, saturate.  *total_samples_out (host) = sum samples - (B - 1) n
 * out_f32 may be `wave` itself when n = 0.  Nothing synchronises. */
F5_API int f5_wave_finish(int B, const float* wave, const int32_t* samples_host, const float* gain_host, const uint8_t* apply_host,
                          const float* rms_dev, float target_rms, int gain_div, int xfade_samples, const double* w_down, const double* w_up,
                          float* out_f32, double* out_f64, int16_t* out_pcm16, int64_t* total_samples_out, f5_stream_t stream);
/* f5_wave_finish in consecutive pushes: a caller that decodes its utterances group by group gets every output sample as soon as it is final.
 * For EVERY way of cutting an utterance list into consecutive pushes, the emitted pieces, concatenated, are byte-identical to one f5_wave_finish
 * over the whole list (float and PCM): it is the same kernel and the same host path (csrc/wave_tail.hip), the one-shot call being the push that
 * holds the whole list, reads no carry and writes none.
 *   create   total_utterances = length of the whole list, known up front; xfade_samples, w_down / w_up, rms_dev, target_rms, gain_div as for
 *            f5_wave_finish.  The device arrays (w_down, w_up, rms_dev) are read by every push and stay the caller's: keep them alive until destroy.
 *            n = xfade_samples when total_utterances >= 2, else 0.  float64 or float32 is a property of the WHOLE STREAM, not of a push: with
 *            n > 0 every push emits float64 and forms its PCM from the fp64 product -- also a first push of one utterance that mixes nothing
 *            itself (in the one-shot result that utterance is float64 too) -- and with n = 0 everything is float32 and nothing is carried.
 *   push     the next B utterances of the list, back to back in wave (dev f32), samples_host[B]; gain_host / apply_host as for f5_wave_finish
 *            (per utterance of this push; not together with a rms_dev given at create).  Emits the joint with the carried tail of the previous
 *            push, then everything of these B utterances except the last n samples of the last one, which are carried (with their gain applied)
 *            for the next push; the push that completes total_utterances emits its own tail too.  *emitted (host) = sum samples - (B - 1) n,
 *            minus n unless this push is the last: computed from the extents alone.  out_f32 / out_f64 / out_pcm16 [*emitted]: which float output
 *            must be NULL follows f5_wave_finish (out_f32 when n > 0, out_f64 when n = 0).  With ALL THREE outputs NULL a push only answers
 *            *emitted (and judges the extents): nothing is enqueued and the session does not advance, so a caller can size its buffers and push
 *            the same utterances again.  A push of one utterance of exactly n samples emits 0 samples and still carries: give it a non-NULL
 *            output pointer.
 *            The carry belongs to the session: once a push is enqueued the caller may overwrite or free its wave buffer, in stream order; the
 *            next push does not read it.  All pushes of a session go to one stream (or are ordered by the caller).
 *   extents  the chaining rule of f5_wave_finish over the WHOLE list: the first and the last utterance hold at least n samples, every other 2 n;
 *            a push that breaks it answers F5_ENOTSUP.  F5_EINVAL: more utterances than the stream has left, samples <= 0, a total (over all
 *            pushes) reaching 2^31 samples.  A refused push leaves the session unchanged.
 * More utterances than one kernel table holds are split into tables that overlap by one utterance, as in f5_wave_finish.  Nothing synchronises;
 * destroy frees the carry (and thereby waits for the device). */
typedef struct f5_wave_stream_s* f5_wave_stream_t;
F5_API int f5_wave_stream_create(int total_utterances, int xfade_samples, const double* w_down, const double* w_up, const float* rms_dev,
                                 float target_rms, int gain_div, f5_wave_stream_t* out);
F5_API int f5_wave_stream_push(f5_wave_stream_t s, int B, const float* wave, const int32_t* samples_host, const float* gain_host,
                               const uint8_t* apply_host, float* out_f32, double* out_f64, int16_t* out_pcm16, int64_t* emitted,
                               f5_stream_t stream);
F5_API int f5_wave_stream_destroy(f5_wave_stream_t s);
/* The same tail over SEGMENTS, for a script spoken in several voices (the reference's infer_cli.py:290-354 runs each tagged piece on its own and
 * joins the pieces with np.concatenate): cross-fades inside a segment, plain concatenation between segments, and the rms rule per voice.  Detected
 * by symbol like the entries above.  f5_wave_finish / f5_wave_stream_create ARE these calls with one segment and rms index 0: one kernel, the same
 * arithmetic (wave_gain, two fp64 products and one fp64 sum without contraction, saturating PCM), the same bytes.
 *   segments    seg_start_host[B] (host; NULL: one segment): a non-zero entry means utterance k begins a new segment; entry 0 always begins one.
 *               The joint before utterance k has n_k = xfade_samples when k continues a segment and n_k = 0 when it begins one: no table read, no
 *               left operand, no carry
 *   chaining    per segment: in a segment of two or more utterances the first and the last hold at least n samples and every inner one 2 n; a
 *               one-utterance segment has no constraint.  A violation answers F5_ENOTSUP naming the utterance
 *   dtype       the result is float64 exactly when xfade_samples > 0 and at least one utterance continues a segment (np.concatenate then promotes
 *               everything, segments that mixed nothing included, and the PCM product is taken in fp64 for every sample); otherwise fp32.  For a
 *               stream this is a property of the whole list.  *total_samples_out = sum samples - n * (number of in-segment joints)
 *   rms         rms_dev is an array of n_rms >= 1 dev f32 values, one per voice, and rms_index_host[B] (host; NULL: all 0; each in [0, n_rms)) names
 *               each utterance's entry: utterance k takes g = rms_dev[rms_index[k]] and the gain applies when g < target_rms, decided in the kernel;
 *               at a joint the left operand uses utterance k - 1's own entry.  gain_host / apply_host stay available, exclusive with rms_dev
 *   stream      seg_start_host and rms_index_host cover the WHOLE list (total_utterances entries, copied at create); the session is pushed with
 *               f5_wave_stream_push and freed with f5_wave_stream_destroy.  A push whose last utterance ends a segment emits all of it and carries
 *               nothing, and the next push's first utterance reads no carry; so does a push that ends the list.  For every way of cutting the list
 *               into consecutive pushes the pieces, concatenated, are byte-identical to the one-shot call.  The query form of a push (all outputs
 *               NULL) answers the emitted count and does not advance the session
 *   pcm_f32     pcm_f32_host[B] (host; NULL: none): a non-zero entry keeps utterance k's PCM product in fp32 inside a float64 result -- the int16
 *               that a call over this utterance alone gives (trunc(fp32(x * 32767)) can differ from trunc(double(x) * 32767) by one).  Only for an
 *               utterance that is a segment of its own (F5_EINVAL otherwise); without it the PCM follows the dtype rule above for every sample
 * Lists longer than one kernel table are split into tables that overlap by one utterance; a segment boundary may fall on the overlap. */
F5_API int f5_wave_finish_segments(int B, const float* wave, const int32_t* samples_host, const uint8_t* seg_start_host, const float* gain_host,
                                   const uint8_t* apply_host, const float* rms_dev, int n_rms, const int32_t* rms_index_host, float target_rms,
                                   int gain_div, int xfade_samples, const double* w_down, const double* w_up, const uint8_t* pcm_f32_host,
                                   float* out_f32, double* out_f64, int16_t* out_pcm16, int64_t* total_samples_out, f5_stream_t stream);
F5_API int f5_wave_stream_create_segments(int total_utterances, const uint8_t* seg_start_host, int xfade_samples, const double* w_down,
                                          const double* w_up, const float* rms_dev, int n_rms, const int32_t* rms_index_host, float target_rms,
                                          int gain_div, const uint8_t* pcm_f32_host, f5_wave_stream_t* out);
/* "Remove silence" on the finished wave, on the device: the reference's remove_silence_for_generated_wav (infer/utils_infer.py:569-578: pydub's
 * split_on_silence on the exported 16-bit file, the kept parts written back), detected by symbol like the round-5 entries.
 *   rule       this package's stand-in for pydub, infer/audio.py split_on_silence / detect_nonsilent / detect_silence / Segment.slice_ms /
 *              Segment.__len__, bit for bit: n_ms = round(1000 n_samples / sample_rate) half to even (the caller passes it; it is checked);
 *              millisecond m is sample F(m) = min(int(m * (sample_rate / 1000.0)), n_samples), a double product, truncated; window starts 0,
 *              seek_step, .. <= last = n_ms - min_silence_len, and last itself once more when last % seek_step != 0; a window covers
 *              [i, i + min_silence_len); a silent start i opens a new silent range only when i != prev + seek_step and i > prev + min_silence_len;
 *              the silent ranges are inverted (a leading [0, 0] dropped; all silent: no part; no silent window, or n_ms < min_silence_len: the one
 *              part [0, n_ms]), each part is padded by keep_silence, overlapping neighbours meet at (a_end + b_start) / 2, all is clamped to
 *              [0, n_ms]; samples behind F(n_ms) belong to no part
 *   PCM judged clip(rint(double(x) * 32767.0), -32768, 32767): the product in fp64, rint half to even -- what audio.write_wav puts into the file.
 *              It is formed in registers; it is never the truncating PCM of f5_wave_finish.  NaN counts as 0 (numpy leaves that cast undefined)
 *   decision   a window of n samples with the sum of squares S is silent when S < (R + 1)^2 n, R = threshold_floor = floor(10^(dB / 20) * 32768),
 *              taken by the caller: equal to the host's int(sqrt(S / n)) <= threshold while n < 2^22; 64-bit integers throughout, no
 *              sqrt, pow or division on the device
 *   wave       dev f32 (is_f64 = 0) or f64 (1), n_samples mono samples, aligned to its element
 *   workspace  dev, 16-byte aligned, at least the bytes the _workspace entry answers for the same n_samples, sample_rate, min_silence_len and
 *              seek_step (a negative F5_* code for arguments it refuses).  Nothing is allocated here
 *   outputs    each may be NULL, each with room for n_samples elements: out_wave (the kept samples, in the input's dtype), out_pcm16 (their
 *              rounded PCM, as above), out_pcm_in (the kept samples of pcm_in, dev int16 [n_samples]: the caller's truncating PCM; both or
 *              neither).  counts_dev: dev int64 [2] = (kept samples, parts); copy it before, or together with, the data
 *   refusals   F5_EINVAL with the argument's name, before any launch, the outputs untouched: a window of 2^22 samples or more
 *              (min_silence_len * sample_rate / 1000 + 1), n_samples < 0 or >= 2^31, min_silence_len < 1, seek_step < 1, keep_silence < 0,
 *              sample_rate < 1000, threshold_floor < 0, an n_ms other than the rule's, a short or misaligned workspace
 * Nothing synchronises.
 * The op-level entry stops behind the decision (for tests): flags_out dev u8 [W], W = the number of window starts above (0 when
 * n_ms < min_silence_len; give one byte at least), 1 = silent; table_out dev i32 [3 (n_ms / min_silence_len + 2)]: per part (first sample, end
 * sample, position of its first sample in the output); counts_dev as above. */
F5_API int64_t f5_wave_remove_silence_workspace(int64_t n_samples, int sample_rate, int min_silence_len, int seek_step);
F5_API int f5_wave_remove_silence(const void* wave, int is_f64, int64_t n_samples, int sample_rate, int64_t n_ms, int min_silence_len,
                                  int threshold_floor, int keep_silence, int seek_step, const int16_t* pcm_in, void* workspace,
                                  int64_t workspace_bytes, void* out_wave, int16_t* out_pcm16, int16_t* out_pcm_in, int64_t* counts_dev,
                                  f5_stream_t stream);
F5_API int f5_op_silence_ranges(const void* wave, int is_f64, int64_t n_samples, int sample_rate, int64_t n_ms, int min_silence_len,
                                int threshold_floor, int keep_silence, int seek_step, void* workspace, int64_t workspace_bytes,
                                uint8_t* flags_out, int32_t* table_out, int64_t* counts_dev, f5_stream_t stream);
/* The delivery stage behind the wave tail, on the device: the finished signal at another sample rate, as float32, as the truncating int16 PCM of
 * f5_wave_finish and as G.711, detected by symbol like the entries above.
 *   resample   torchaudio's sinc_interp_hann at its defaults (lowpass_filter_width 6, rolloff 0.99), the definition of f5_frontend_resample:
 *              g = gcd(in_rate, out_rate), orig = in_rate / g, nw = out_rate / g, base = min(orig, nw) * 0.99, width = ceil(6 orig / base),
 *              kw = 2 width + orig, target = ceil(nw n / orig); output j = blk * nw + ph is sum_k taps[ph][k] * x[blk * orig - width + k] over
 *              k = 0 .. kw - 1
 *   taps       dev f64 [nw][kw], the CALLER's table (as w_down / w_up are for the cross-fade): the formula in float64, cast to fp32 and back, as
 *              torchaudio casts its kernel to the waveform's dtype.  It must outlive a stream session
 *   arithmetic x widened to fp64; fp64 products; ONE fp64 accumulator from 0.0 over ascending k; multiply and add never contracted; a tap whose
 *              sample lies outside [0, n) is skipped, not added as zero.  So the result does not depend on how the work is cut
 *   wave       dev f32 (is_f64 = 0) or f64 (1), n > 0 mono samples, aligned to its element
 *   outputs    each may be NULL, each with room for target elements: out_f32 = (float)acc; out_pcm16 = trunc(out_f32 * 32767.0f), the product in
 *              fp32, saturating at or beyond +-32768, NaN -> 0 (the wave tail's rule); out_g711 = the G.711 code of that int16 under law.
 *              *out_samples (host) = target; with all three outputs NULL that is all the call does
 *   G.711      law 0 = mu-law, 1 = A-law, as CPython's audioop.lin2ulaw / lin2alaw give them for 16-bit input, with integer arithmetic only:
 *              mu-law  v = s >> 2, m = min(|v|, 8158) + 33, seg = floor(log2 m) - 5, code = seg << 4 | ((m >> (seg + 1)) & 15),
 *                      code ^ 0x7F for v < 0, code ^ 0xFF otherwise
 *              A-law   v = s >> 3, m = v for v >= 0 and -v - 1 for v < 0, seg = 0 for m < 32 and floor(log2 m) - 4 otherwise,
 *                      code = seg << 4 | ((seg < 2 ? m >> 1 : m >> seg) & 15), code ^ 0x55 for v < 0, code ^ 0xD5 otherwise
 *              The op-level entry encodes dev int16 [n] -> dev uint8 [n] on its own (the native rate: the wave tail's PCM16 is encoded as it is)
 *   refusals   F5_EINVAL before any launch: n <= 0 or >= 2^31, a rate that is not positive, in_rate == out_rate (nothing to resample: the caller
 *              keeps its signal), nw * kw above 2^20 table entries, a law other than 0 / 1, a null or misaligned wave or table
 * In pushes: a session is created with the rates, the table, is_f64 and law -- properties of the whole stream -- and a push hands over the next
 * n_k > 0 input samples and whether it is the last.  After a non-final push that brings the input to N samples, nw * max(0, (N - width) / orig)
 * samples (integer division) are out in all: the blocks whose whole support has arrived, so a push may emit none; the last push emits up to target
 * of the whole input.  The session keeps the input later blocks still need (fewer than kw samples) in a buffer of its own: the caller may free
 * its buffer in stream order.  For EVERY way of cutting a signal into pushes the pieces, concatenated, are byte for byte the one-shot result --
 * float, int16 and G.711.  With all three outputs NULL a push answers *emitted and leaves the session as it was.  F5_EINVAL, the session unchanged:
 * a push after the last one, n_k <= 0, 2^31 samples or more in all.  Nothing synchronises. */
typedef struct f5_convert_stream_s* f5_convert_stream_t;
F5_API int f5_op_g711_encode(int64_t n, const int16_t* pcm16, int law, uint8_t* out, f5_stream_t stream);
F5_API int f5_wave_convert(const void* wave, int is_f64, int64_t n, int in_rate, int out_rate, const double* taps, int law, float* out_f32,
                           int16_t* out_pcm16, uint8_t* out_g711, int64_t* out_samples, f5_stream_t stream);
F5_API int f5_wave_convert_stream_create(int in_rate, int out_rate, const double* taps, int is_f64, int law, f5_convert_stream_t* out);
F5_API int f5_wave_convert_stream_push(f5_convert_stream_t s, const void* wave, int64_t n_k, int last, float* out_f32, int16_t* out_pcm16,
                                       uint8_t* out_g711, int64_t* emitted, f5_stream_t stream);
F5_API int f5_wave_convert_stream_destroy(f5_convert_stream_t s);
/* The reference-voice front-end on the device: the host steps of F5TTSWrapper._preprocess_voice (the reference's f5tts_wrapper.py:256-379) by the
 * rule of this package's stand-in for pydub, infer/audio.py clip_reference / remove_silence_edges / Segment.silent_like / segment_to_float, bit
 * for bit up to the rms (below), detected by symbol.
 *   pcm        dev int16 [n_frames, channels] interleaved, channels 1 or 2, n_frames * channels < 2^31, sample_rate >= 1000
 *   lengths    len(x) = rint(1000 frames / sample_rate), half to even; millisecond m is frame F(m) = min(int(m * (sample_rate / 1000.0)), frames),
 *              a double product, truncated; an rms is over the interleaved samples of all channels
 *   clip       (clip_short != 0; otherwise the one part [0, n_frames)) pass 1 = the split_on_silence of f5_wave_remove_silence above with
 *              (min_silence_len_1, threshold_floor_1, keep_silence, seek_step) over the clip; its parts are appended while not
 *              (len(out) > soft_limit_ms and len(out + part) > hard_limit_ms), which sets clip bit 0 ("(1)").  If len(out) > hard_limit_ms, pass 2
 *              does the same over the ORIGINAL clip with (min_silence_len_2, threshold_floor_2) and replaces out (bit 1, "(2)").  If still
 *              len(out) > hard_limit_ms, out = its first int(hard_limit_ms * (sample_rate / 1000.0)) frames (bit 2, "(3)")
 *   edges      over the gathered frames out (their own millisecond grid, K frames, n_ms = len(out)): trim = 0; while trim < n_ms and the chunk
 *              [trim, min(trim + lead_chunk_ms, n_ms)) is empty or has S < r_lead^2 n: trim += lead_chunk_ms; lead = min(trim, n_ms).  The segment
 *              is re-sliced to frames [F(lead), F(n_ms)) -- K2 frames, n2 = len of them, its millisecond grid restarting there -- and milliseconds
 *              n2 - 1, n2 - 2, .. count as silent until one has n > 0 and S >= r_trail^2 n.  S = the int64 sum of squares of a slice's n
 *              interleaved samples; r_lead / r_trail are the caller's integers (audio.edge_threshold_integers: the smallest rms whose dBFS is not
 *              below / is above the threshold); equal to the host's float comparison while n < 2^22.  No pow, log or sqrt in a decision
 *   cut        the host's part: end = K2 / sample_rate; `end -= 0.001` once per silent millisecond; cut_ms = int(end * 1000).  The result keeps
 *              slice_ms(0, cut_ms) of the re-sliced segment (Python's rule: a negative cut_ms counts from n2; clamped to [0, n2]), then
 *              int(pad_ms * (sample_rate / 1000.0)) zero frames
 *   wave       out_wave[i] = fp32(sum of frame i's channels) / (32768 channels): exactly the mean over channels of int / 32768 in fp32.
 *              S = the int64 sum of the squared channel sums, pad included; rms32 = fp32(sqrt(fp64(S) / (channels^2 32768^2 out frames))), the
 *              division and the root in fp64, rounded once more to fp32.  When rms32 < target_rms every sample becomes
 *              (x * target_rms) / rms32: two fp32 operations, each correctly rounded.  (The host route's rms is torch's fp32 reduction, whose
 *              summation order is its own: the contract here is rms32.)
 *   counts_dev dev int64 [F5_REF_WORDS], indexed by F5_REF_*.  The decision stores PARTS, CLIP, GATHERED (K), GATHERED_MS, PASS2 (1: pass 2 ran),
 *              LEAD_MS, TRAIL_MS (silent milliseconds at the end), LEAD_FRAME (F(lead)), EDGE_FRAMES (K2), EDGE_MS (n2); the rest is stored by
 *              f5_reference_prepare: KEPT (frames before the pad), OUT_FRAMES, SUMSQ (S), BOOST (1: applied), RMS_BITS (rms32's bits)
 *   table_out  dev int32 [3 rows], rows = what the _table_rows entry answers: per part (first frame, end frame, position among the gathered
 *              frames) of the original clip; the PARTS rows concatenated are the K gathered frames (before the edges)
 *   workspace  dev, 16-byte aligned, at least the bytes the _workspace entry answers for the same arguments.  Nothing is allocated here
 *   prepare    planned = 0: the decision, then the wave.  planned != 0: workspace, table_out and counts_dev are as f5_op_reference_plan left them
 *              for the same arguments on the same stream (the caller read TRAIL_MS and EDGE_FRAMES in between to form cut_ms) and only the wave is
 *              made.  out_frames = the frames the caller expects (KEPT + the pad; at most n_frames + the pad): nothing is stored behind it;
 *              out_wave dev f32 [out_frames]; out_pcm (may be NULL) dev int16 [out_frames, channels]: the integers out_wave was made from
 *   refusals   F5_EINVAL with the argument's name, before any launch: channels other than 1 / 2, 2^31 samples or more, sample_rate < 1000, a
 *              window (either min_silence_len or lead_chunk_ms) of 2^22 samples or more, a length below 1, a negative keep_silence, floor, limit
 *              or pad, soft_limit_ms > hard_limit_ms, r_lead / r_trail outside 0 .. 32768, a short or misaligned workspace, a null pointer
 * Nothing synchronises.  f5_op_reference_plan stops behind the decision (tables and counts only). */
typedef struct f5_reference_rule {
    int32_t clip_short;
    int32_t min_silence_len_1, threshold_floor_1; /* 1000, floor(10^(-50 / 20) * 32768) = 103 */
    int32_t min_silence_len_2, threshold_floor_2; /* 100, 327 (-40 dB) */
    int32_t keep_silence, seek_step;              /* 1000, 10 */
    int32_t soft_limit_ms, hard_limit_ms;         /* 6000, 12000 */
    int32_t r_lead, r_trail;                      /* 261, 261 (-42 dB) */
    int32_t lead_chunk_ms, pad_ms;                /* 10, 50 */
    float target_rms;                             /* 0.1 */
} f5_reference_rule;
enum {
    F5_REF_KEPT = 0, F5_REF_PARTS, F5_REF_CLIP, F5_REF_LEAD_MS, F5_REF_TRAIL_MS, F5_REF_SUMSQ, F5_REF_BOOST, F5_REF_GATHERED, F5_REF_GATHERED_MS,
    F5_REF_LEAD_FRAME, F5_REF_EDGE_FRAMES, F5_REF_EDGE_MS, F5_REF_OUT_FRAMES, F5_REF_RMS_BITS, F5_REF_PASS2, F5_REF_WORDS = 16
};
F5_API int64_t f5_reference_prepare_workspace(int64_t n_frames, int channels, int sample_rate, const f5_reference_rule* rule);
F5_API int64_t f5_reference_table_rows(int64_t n_frames, int channels, int sample_rate, const f5_reference_rule* rule);
F5_API int f5_reference_prepare(const int16_t* pcm, int64_t n_frames, int channels, int sample_rate, const f5_reference_rule* rule, int planned,
                                int64_t cut_ms, void* workspace, int64_t workspace_bytes, int32_t* table_out, int64_t* counts_dev,
                                int64_t out_frames, float* out_wave, int16_t* out_pcm, f5_stream_t stream);
F5_API int f5_op_reference_plan(const int16_t* pcm, int64_t n_frames, int channels, int sample_rate, const f5_reference_rule* rule, void* workspace,
                                int64_t workspace_bytes, int32_t* table_out, int64_t* counts_dev, f5_stream_t stream);
/* ISTFT head alone (for the roofline measurement): spec dev f32 [B, T, n_fft+2] (head.out activations:
 * log-magnitude | phase) -> wave dev f32 [B, (T-1)*hop] */
F5_API int f5_vocoder_istft_head(f5_vocoder_t v, int B, int T, const float* head_out, float* wave, f5_stream_t stream);

/* ------------------------------------------------------------------ BigVGAN-v2 generator (round 4; plug point B, PARITY UNPINNED)
 * Replaces `third_party.BigVGAN.bigvgan.BigVGAN` as the reference uses it: infer/utils_infer.py:125-138 (from_pretrained + remove_weight_norm) and the
 * call `vocoder(mel)` of infer/f5tts_wrapper.py:526 / eval/eval_infer_batch.py:189.  That checkout is absent from the reference tree: the generator is
 * restated from the published BigVGAN-v2 source (conv_pre, per stage ConvTranspose1d + the mean of three AMPBlock1 with anti-aliased SnakeBeta
 * activations, conv_post, clamp / tanh); tensor names are the checkpoint's with weight norm REMOVED (`<module>.weight`, `.bias`, `....act.alpha`,
 * `....act.beta`), plus the optional 12-tap buffers `aa_up_filter` / `aa_down_filter` (default: the Kaiser-windowed sinc of the published filter). */
typedef struct f5_bigvgan_s* f5_bigvgan_t;
typedef struct f5_bigvgan_config {
    int32_t num_mels;                 /* 100 */
    int32_t upsample_initial_channel; /* 1536 */
    int32_t num_upsamples;            /* 6 (<= 8) */
    int32_t upsample_rates[8];        /* 4 4 2 2 2 2 */
    int32_t upsample_kernel_sizes[8]; /* 8 8 4 4 4 4 (a multiple of the rate, k - u even, k <= 3u: else F5_ENOTSUP) */
    int32_t num_kernels;              /* 3 (<= 4) AMP blocks per stage */
    int32_t resblock_kernel_sizes[4]; /* 3 7 11 */
    int32_t resblock_dilations[4][3]; /* 1 3 5 each */
    int32_t snake_logscale;           /* 1: alpha / beta are stored as logarithms */
    int32_t use_tanh_at_final;        /* 0: clamp(-1, 1) */
    int32_t use_bias_at_final;        /* 0: conv_post has no bias */
} f5_bigvgan_config;
F5_API int f5_bigvgan_create(const f5_bigvgan_config* cfg, f5_bigvgan_t* out);
F5_API int f5_bigvgan_set_tensor(f5_bigvgan_t v, const char* name, const float* host_data, const int64_t* shape, int ndim);
F5_API int f5_bigvgan_has_tensor(f5_bigvgan_t v, const char* name, int64_t* numel);
F5_API int f5_bigvgan_finalize(f5_bigvgan_t v);
F5_API int f5_bigvgan_destroy(f5_bigvgan_t v);
/* mel dev f32 [B][num_mels][T] -> wave dev f32 [B][T * prod(upsample_rates)]  (BigVGAN.forward, the [B, 1, samples] result without its unit axis) */
F5_API int f5_bigvgan_forward(f5_bigvgan_t v, int B, int T, const float* mel, float* wave, f5_stream_t stream);
/* Utterances of DIFFERENT frame counts through one set of launches (round 5; the shape of f5_vocoder_decode_ragged).  mel: dev f32, FRAME-major
 * [rows, ld] with ld >= num_mels (the sampler's own buffer: no permute / contiguous copy; columns past num_mels are never read).  Utterance i
 * reads frames_host[i] >= 1 rows from row row_start_host[i] on and writes its T_i * prod(upsample_rates) samples directly behind those of
 * utterance i - 1 in `wave`; *total_samples (may be NULL) receives the sum.  Both arrays are host memory, read before the call returns.
 * Utterance i is bit-identical to f5_bigvgan_forward(v, 1, T_i, its own [num_mels, T_i] mel): the convolutions pad with zeros and the
 * anti-aliased activations replicate at each utterance's own ends and never read a neighbour's rows, whatever those hold.  The list is cut, in
 * order, into launch sets of at most "bigvgan_group_frames" frames (tuning key, default 2048; a longer utterance is a set of its own), which
 * bounds the workspace and changes no bit.  F5_EINVAL, before any launch: B <= 0, ld < num_mels, a negative row start, a frame count below 1,
 * rows or samples beyond 32-bit indexing.  Nothing synchronises (workspace growth aside, as for f5_bigvgan_forward). */
F5_API int f5_bigvgan_decode_ragged(f5_bigvgan_t v, int B, const int32_t* row_start_host, const int32_t* frames_host, const float* mel, int ld,
                                    float* wave, int64_t* total_samples, f5_stream_t stream);
/* Test-only: the anti-aliased SnakeBeta kernel alone, launched exactly as the generator launches it for one utterance (the 64-channel tile when
 * C % 64 == 0, else the 32-channel one).  x, out: dev f32 [T, C] (time-major); a, invb: dev f32 [C], the kernel's own parameters exp(alpha) and
 * 1 / (beta + 1e-9f); up_f, dn_f: 12 HOST floats each, NULL = the library's Kaiser-windowed sinc.  out[t][c] = sum_j dn_f[j] z[clamp(2t + j - 5)],
 * z[n] = w + invb sin^2(a w), w = 2 sum_m xpad[m] up_f[n + 15 - 2m], xpad = x replicate-padded by 5, both clamps at the utterance's own ends. */
F5_API int f5_op_bigvgan_snake(int T, int C, const float* x, const float* a, const float* invb, const float* up_f, const float* dn_f, float* out,
                               f5_stream_t stream);
/* The same through the generator's ragged path: cnt utterances back to back, frames_host[u] * up rows each (host array; more than 64
 * utterances take several launches).  Every utterance gets the bits of the one-utterance op on its own rows. */
F5_API int f5_op_bigvgan_snake_ragged(int cnt, const int32_t* frames_host, int up, int C, const float* x, const float* a, const float* invb,
                                      const float* up_f, const float* dn_f, float* out, f5_stream_t stream);

/* ------------------------------------------------------------------ reference-audio front-end on the device
 * Replaces the two torchaudio transforms of the path:
 *   f5_frontend_mel       MelSpec / get_vocos_mel_spectrogram, reference model/modules.py:75-143 (as called from cfm.py:103-105):
 *                         wave dev f32 [B, nw] -> log-mel dev f32 [B, n_mels, nw / hop + 1]
 *   f5_frontend_resample  torchaudio.transforms.Resample(sr, target) of F5TTSWrapper.preprocess_reference (infer/f5tts_wrapper.py:338-341) and
 *                         infer_batch_process (infer/utils_infer.py:443-445): wave dev f32 [B, n] -> dev f32 [B, ceil(new * n / orig)] */
typedef struct f5_frontend_s* f5_frontend_t;
typedef struct f5_mel_config {
    int32_t n_fft;       /* 1024 */
    int32_t hop;         /* 256 */
    int32_t win;         /* 1024 (<= n_fft; centred) */
    int32_t n_mels;      /* 100 */
    int32_t sample_rate; /* 24000: the filterbank spans 0 .. sample_rate / 2 */
    int32_t mel_type;    /* F5_MEL_VOCOS (0): torchaudio MelSpectrogram, HTK scale, center = True -> nw / hop + 1 frames (modules.py:75-101);
                            F5_MEL_BIGVGAN (1, round 4): get_bigvgan_mel_spectrogram (modules.py:29-72): reflect padding of (n_fft - hop) / 2,
                            center = False -> (nw + 2 pad - n_fft) / hop + 1 frames, sqrt(re^2 + im^2 + 1e-9), librosa's Slaney-scale
                            area-normalised filterbank */
} f5_mel_config;
#define F5_MEL_VOCOS 0
#define F5_MEL_BIGVGAN 1
F5_API int f5_frontend_create(const f5_mel_config* cfg, f5_frontend_t* out);
F5_API int f5_frontend_destroy(f5_frontend_t h);
F5_API int f5_frontend_mel(f5_frontend_t h, int B, int nw, const float* wave, float* mel, f5_stream_t stream);
F5_API int f5_frontend_resample(f5_frontend_t h, int B, int n, int orig_freq, int new_freq, const float* wave, float* out, f5_stream_t stream);

/* ------------------------------------------------------------------ speaker-similarity head (ECAPA-TDNN, the "SIM" figure)
 * Everything of the reference's eval/ecapa_tdnn.py behind `self.feature_extract(...)` (ECAPA_TDNN.get_feat / forward, :283-309) with
 * global_context_att = False, as ECAPA_TDNN_SMALL and utils_eval.run_sim use it: forward only, eval mode, fp32 storage.  The feature extractor
 * (WavLM-large from s3prl in the reference) is a handle of its own (f5_wavlm_*, below): this one takes the hidden states.
 *   x = sum_l softmax(feature_weight)[l] hs[l] + 1e-6 -> InstanceNorm1d per utterance (biased variance, eps 1e-5) -> layer1 Conv1dReluBn(k 5)
 *   -> three SE_Res2Blocks (dilation 2, 3, 4; Res2 scale `scale`) -> cat -> Conv1d(3C -> cat_channels) + ReLU -> AttentiveStatsPool
 *   -> BatchNorm1d(2 cat_channels) -> Linear(-> emb_dim)
 * Tensor names are the reference state_dict()'s: feature_weight, layer1.conv.*, layer1.bn.*, layer{2,3,4}.Conv1dReluBn{1,2}.{conv,bn}.*,
 * layer{2,3,4}.Res2Conv1dReluBn.{convs,bns}.{0..scale-2}.*, layer{2,3,4}.SE_Connect.linear{1,2}.*, conv.*, pooling.linear{1,2}.*, bn.*, linear.*
 * (bn: weight, bias, running_mean, running_var).  has_tensor answers 0 for feature_extract.* and num_batches_tracked; finalize names the first
 * missing tensor.  A pooling.linear1.weight with 3 * cat_channels input channels (global_context_att = True) is refused by set_tensor with
 * F5_ENOTSUP: that model is another function, not an approximation of this one.
 * Per-channel statistics over time (instance norm, the SE mean, the pool's softmax denominator, its two weighted sums and the subtraction
 * E[x^2] - mean^2) are accumulated in fp64 in a fixed order; no sum uses atomics. */
typedef struct f5_speaker_s* f5_speaker_t;
typedef struct f5_speaker_config {
    int32_t feat_dim;           /* 1024 (WavLM-large); a multiple of 32 */
    int32_t channels;           /* 512; a multiple of 8 * scale */
    int32_t emb_dim;            /* 256 */
    int32_t layers;             /* 25 hidden-state layers */
    int32_t cat_channels;       /* 1536; a multiple of 32 */
    int32_t se_bottleneck;      /* 128 */
    int32_t attention_channels; /* 128; a multiple of 32 */
    int32_t scale;              /* 8 */
} f5_speaker_config;
F5_API int f5_speaker_create(const f5_speaker_config* cfg, f5_speaker_t* out);
F5_API int f5_speaker_set_tensor(f5_speaker_t h, const char* name, const float* host_data, const int64_t* shape, int ndim);
F5_API int f5_speaker_has_tensor(f5_speaker_t h, const char* name, int64_t* numel);
F5_API int f5_speaker_finalize(f5_speaker_t h);
F5_API int f5_speaker_destroy(f5_speaker_t h);
/* B utterances of DIFFERENT frame counts through one set of launches.  hs: dev f32 [layers, sum(frames), feat_dim], the utterances back to back
 * along the row axis; frames_host: host int32 [B], read before the call returns; emb: dev f32 [B, emb_dim].  Every kernel that looks across rows
 * stops at the utterance's own first and last frame (a Conv1d tap outside reads zero), so an utterance's embedding has the same bits whatever
 * shares the call with it and in every call.  Lists of more than 64 utterances (or 32768 frames: 64 utterances of 10 s) are cut, in order, into several launch sets,
 * which changes no bit.  F5_EINVAL before any launch: B <= 0, a frame count below 2 (InstanceNorm1d has no variance there; the reference
 * raises too), rows beyond 32-bit indexing.  Nothing synchronises (workspace growth aside). */
F5_API int f5_speaker_embed_ragged(f5_speaker_t h, int B, const int32_t* frames_host, const float* hs, float* emb, f5_stream_t stream);
/* Test hook: the next embed calls also copy an intermediate tensor, time-major [sum(frames), width] (pooling: [B, 2 cat_channels]), into `dev`
 * (NULL: stop).  Names: instance_norm (feat_dim), layer1 .. layer4 (channels), conv (cat_channels), pooling. */
F5_API int f5_speaker_set_tap(f5_speaker_t h, const char* name, float* dev);
/* Test-only: the pieces of the head one by one, launched as the head launches them, over cnt utterances back to back (frames_host as above).
 * Activations x / out: dev f32, time-major [sum(frames), channels].  Parameters are HOST arrays in PyTorch's layouts; every op stages them on the
 * device itself and synchronises the stream before it returns.  bn_host: [4][channels] = weight, bias, running_mean, running_var.
 *   featnorm       hs dev [L, rows, F], feature_weight_host [L] (before the softmax) -> out [rows, F]
 *   conv_relu_bn   bn(relu(Conv1d(cin -> cout, k odd, dilation dil, padding dil (k - 1) / 2)(x))); w_host [cout][cin][k]
 *   res2           Res2Conv1dReluBn(C, k 3, dilation dil, scale): w_host [scale - 1][C / scale][C / scale][3], b_host [scale - 1][C / scale],
 *                  bn_host [scale - 1][4][C / scale]
 *   se             x * sigmoid(linear2(relu(linear1(mean_t x)))) + resid (resid NULL: no add); w1_host [bott][C], w2_host [C][bott]
 *   pool           AttentiveStatsPool(C, att) -> out [cnt, 2 C] (mean | std); w1_host [att][C], w2_host [C][att] */
F5_API int f5_op_speaker_featnorm(int cnt, const int32_t* frames_host, int L, int F, const float* hs, const float* feature_weight_host, float* out,
                                  f5_stream_t stream);
F5_API int f5_op_speaker_conv_relu_bn(int cnt, const int32_t* frames_host, int cin, int cout, int k, int dil, const float* x, const float* w_host,
                                      const float* b_host, const float* bn_host, float eps, float* out, f5_stream_t stream);
F5_API int f5_op_speaker_res2(int cnt, const int32_t* frames_host, int C, int scale, int dil, const float* x, const float* w_host,
                              const float* b_host, const float* bn_host, float eps, float* out, f5_stream_t stream);
F5_API int f5_op_speaker_se(int cnt, const int32_t* frames_host, int C, int bott, const float* x, const float* resid, const float* w1_host,
                            const float* b1_host, const float* w2_host, const float* b2_host, float* out, f5_stream_t stream);
F5_API int f5_op_speaker_pool(int cnt, const int32_t* frames_host, int C, int att, const float* x, const float* w1_host, const float* b1_host,
                              const float* w2_host, const float* b2_host, float* out, f5_stream_t stream);

/* ------------------------------------------------------------------ WavLM feature extractor (in front of the speaker head: the "SIM" figure)
 * The network run_sim takes from s3prl as "wavlm_large", with the arithmetic of transformers' WavLMModel at feat_extract_norm = "layer",
 * do_stable_layer_norm = True (microsoft/wavlm-large): forward only, fp32 storage and accumulation, batch-1 semantics per utterance (no padding,
 * no mask).  Per utterance: optional F.layer_norm over the wave -> conv layers (Conv1d, LayerNorm over channels, GELU) -> LayerNorm + Linear ->
 * x + GELU(grouped positional Conv1d) -> N pre-LayerNorm encoder layers whose attention adds WavLM's gated relative position bias.
 * Tensor names are WavLMModel.state_dict()'s, with ONE exception: the positional convolution's weight-norm is folded by the caller and set as
 * encoder.pos_conv_embed.conv.weight [hidden, hidden / groups, k] (W = g * v / ||v||, the norm over dims (0, 1) per tap).  masked_spec_embed is
 * not a tensor of this handle.  create refuses, with F5_EINVAL and the field's name: feat_extract_norm other than "layer",
 * do_stable_layer_norm = 0, add_adapter, a hidden size the heads do not divide, a head dimension other than 16 or 64, widths that are not multiples
 * of 32, hidden / groups not a multiple of 16.
 * The relative position bucket of a distance uses a float log; it is evaluated by the caller exactly as the model does and handed over with
 * set_buckets (below) -- the device never computes a bucket. */
typedef struct f5_wavlm_s* f5_wavlm_t;
typedef struct f5_wavlm_config {
    int32_t num_conv_layers;      /* 7; at most 8 */
    int32_t conv_dim[8];          /* 512 x 7; multiples of 32 */
    int32_t conv_kernel[8];       /* 10, 3, 3, 3, 3, 2, 2 */
    int32_t conv_stride[8];       /* 5, 2, 2, 2, 2, 2, 2 */
    int32_t conv_bias;            /* 0 / 1 */
    int32_t hidden_size;          /* 1024 */
    int32_t num_hidden_layers;    /* 24 */
    int32_t num_attention_heads;  /* 16 */
    int32_t intermediate_size;    /* 4096 */
    int32_t num_conv_pos_embeddings;       /* 128 */
    int32_t num_conv_pos_embedding_groups; /* 16 */
    int32_t num_buckets;          /* 320 */
    int32_t max_bucket_distance;  /* 800 */
    int32_t feat_extract_norm;    /* 0 = "layer" (the only one implemented), 1 = "group" */
    int32_t do_stable_layer_norm; /* 1 (the only one implemented) */
    int32_t add_adapter;          /* 0 (the only one implemented) */
    int32_t normalize_input;      /* 1: F.layer_norm(wave, wave.shape), eps 1e-5, fp64 sums in a fixed order (s3prl's expert for the large model) */
    float layer_norm_eps;         /* 1e-5 */
} f5_wavlm_config;
F5_API int f5_wavlm_create(const f5_wavlm_config* cfg, f5_wavlm_t* out);
F5_API int f5_wavlm_set_tensor(f5_wavlm_t h, const char* name, const float* host_data, const int64_t* shape, int ndim);
F5_API int f5_wavlm_has_tensor(f5_wavlm_t h, const char* name, int64_t* numel);
F5_API int f5_wavlm_finalize(f5_wavlm_t h);
F5_API int f5_wavlm_destroy(f5_wavlm_t h);
/* frames an utterance of n_samples gives (per conv layer (T - k) / stride + 1, rounded down), or a negative number when it is too short for one */
F5_API int f5_wavlm_frames(f5_wavlm_t h, int64_t n_samples);
/* buckets_host: host int32 [2 n - 1], the model's relative position bucket of the distances d = key - query = -(n - 1) .. n - 1.  Builds the
 * device table R[h][d] = rel_attn_embed[bucket(d)][h] (layer 0's embedding, shared by all layers) that every later extract call reads; an
 * utterance of more than n frames is refused by extract until a larger table is set.  After finalize; waits for the device. */
F5_API int f5_wavlm_set_buckets(f5_wavlm_t h, int n, const int32_t* buckets_host);
/* B utterances of DIFFERENT lengths through one set of launches.  samples_host: host int32 [B], read before the call returns; wave_cat: dev f32,
 * the 16 kHz waves back to back; hs_out: dev f32 [L, sum(frames), hidden], L = num_hidden_layers + 1, the utterances back to back along the row
 * axis -- exactly what f5_speaker_embed_ragged takes.  Entry 0 is the encoder's input behind the positional convolution, entry i the output of
 * layer i; final_norm = 1 applies the encoder's LayerNorm to the last entry (WavLMModel(output_hidden_states=True)), 0 leaves it as the layer
 * left it.  Row-wise kernels run once over all rows; convolutions and attention work on one utterance's own extent, so an utterance's hidden
 * states have the same bits alone or in any ragged call, at any position.  Lists of more than 64 utterances or 2048 frames are cut, in order,
 * into several launch sets, which changes no bit.  F5_EINVAL before any launch: B <= 0, an utterance too short for one frame, a call beyond
 * 32-bit indexing; F5_ESTATE: not finalized, or no bucket table covers the longest utterance (f5_wavlm_set_buckets comes first, also for a caller
 * in C).  Nothing synchronises (workspace growth aside).  The workspace grows to the largest launch set seen and stays: about 0.6 GiB for a full
 * set at wavlm-large sizes, most of it the rows behind conv layer 0. */
F5_API int f5_wavlm_extract_ragged(f5_wavlm_t h, int B, const int32_t* samples_host, const float* wave_cat, int final_norm, float* hs_out,
                                   f5_stream_t stream);
/* Test hook: the next extract calls also copy an intermediate tensor, time-major and packed as the output is, into `dev` (NULL: stop).  Names:
 * conv{i} (behind LayerNorm and GELU, [sum frames_i, conv_dim[i]]), proj, posconv (= entry 0), layer{i}.attn (the stream behind the attention
 * residual), layer{i}.out (behind the layer, before any final norm): [sum frames, hidden]. */
F5_API int f5_wavlm_set_tap(f5_wavlm_t h, const char* name, float* dev);
/* The new kernels one by one (device tensors x, qkv, gate, rel, out; parameters marked host are HOST arrays in PyTorch's layouts, staged by the
 * op, which then waits for the stream):
 *   attention     qkv [T, 3 H dh] (q | k | v), gate [T, H] (the gate g itself), rel [H, 2 T - 1] (R[h][d] at column d + T - 1) -> out [T, H dh];
 *                 softmax((q . k) dh^-0.5 + g R) v, online softmax in fp32, dh 16 or 64
 *   pos_conv      x [T, C] -> out = x + gelu(Conv1d(C, C, k, padding k / 2, groups)(x)) without the last frame when k is even; w host
 *                 [C][C / groups][k] (weight-norm folded), b host [C]; out must not be x
 *   conv_ln_gelu  x [T_in, cin] -> gelu(LayerNorm(Conv1d(cin, cout, k, stride)(x))) [(T_in - k) / stride + 1, cout], eps 1e-5; w host
 *                 [cout][cin][k], b host [cout] or NULL; cin 1 (the direct kernel of conv layer 0) or a multiple of 32 */
F5_API int f5_op_wavlm_attention(int T, int H, int dh, const float* qkv, const float* gate, const float* rel, float* out, f5_stream_t stream);
F5_API int f5_op_wavlm_pos_conv(int T, int C, int k, int groups, const float* x, const float* w_host, const float* b_host, float* out,
                                f5_stream_t stream);
F5_API int f5_op_wavlm_conv_ln_gelu(int T_in, int cin, int cout, int k, int stride, const float* x, const float* w_host, const float* b_host_or_null,
                                    const float* ln_w_host, const float* ln_b_host, float* out, f5_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* F5HIP_H */
