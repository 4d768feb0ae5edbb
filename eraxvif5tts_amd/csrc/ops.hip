// ops.hip -- per-op C entry points used by the parity tests and micro-benchmarks (f32 device tensors in and out;
// conversion to the precision's activation dtype happens on the device, exactly as inside the model path).
#include <cstring>

#include "gemm.h"
#include "kernels.h"
#include "model_internal.h"
#include "runtime.h"
#include "tuning.h"

static int sync_and_release(DevArena& a, hipStream_t st, int rc) {
    hipError_t e = hipStreamSynchronize(st);
    a.release();
    if (rc != 0) return rc;
    if (e != hipSuccess) return f5_fail(F5_EHIP, "stream synchronize failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int f5_op_linear(int precision, int kernel, int M, int N, int K, const float* A, const float* W, const float* bias, int act,
                            float* out, f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (M <= 0 || N <= 0 || K <= 0 || !A || !W || !out) return f5_fail(F5_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int Kp = (int)round_up(K, 64), Mp = (int)round_up(M, 256), Np = (int)round_up(N, 256);
    const size_t es = f5_elem_size(precision);
    DevArena a;
    void *At = nullptr, *Wt = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&At, (size_t)Mp * Kp * es))) break;
        if ((rc = a.alloc(&Wt, (size_t)Np * Kp * es))) break;
        if ((rc = launch_convert_pad(precision, A, K, M, K, Kp, At, Kp, st))) break;
        if ((rc = launch_convert_pad(precision, W, K, N, K, Kp, Wt, Kp, st))) break;
        GemmParams g;
        memset(&g, 0, sizeof(g));
        g.A = At; g.lda = Kp; g.W = Wt; g.ldw = Kp; g.M = M; g.N = N; g.K = Kp;
        g.bias = bias; g.act = act; g.out_f = out; g.ldof = N;
        rc = launch_gemm(g, precision, GEMM_DENSE, EPI_STORE_F32, kernel, st);
    } while (0);
    return sync_and_release(a, st, rc);
}

// One DiT block linear with its fused store epilogue, as the sampler launches it (test hook; bf16 output converted back to fp32):
//   epi 0 (EPI_STORE_T): out = act(A W^T + b)                         FF1 (modules.py:258-264)
//   epi 5 (EPI_GATE_T):  out = gate[n] * act(A W^T + b), 0 where rowmask[m] == 0   attention out / FF2 with the AdaLN gate (modules.py:499-501,635,639)
//   epi 4 (EPI_ROPE_T):  out = rope(A W^T + b) on the q/k columns of the first rope_heads heads (N = 3 * inner, modules.py:452-461)
extern "C" int f5_op_linear_fused_p(int precision, int kernel, int epi, int M, int N, int K, const float* A, const float* W, const float* bias, int act,
                                  const float* gate, const uint8_t* rowmask, const float* rope, int rope_heads, int seq, float* out,
                                  f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (precision != F5_PREC_BF16 && precision != F5_PREC_FP16) return f5_fail(F5_EINVAL, "f5_op_linear_fused_p: a 16-bit precision mode (bf16 0, fp16 2), got %d", precision);
    if (M <= 0 || N <= 0 || K <= 0 || !A || !W || !out) return f5_fail(F5_EINVAL, "bad argument");
    if (!(epi == EPI_STORE_T || epi == EPI_GATE_T || epi == EPI_ROPE_T || epi == EPI_RESID)) return f5_fail(F5_EINVAL, "f5_op_linear_fused: epilogue %d", epi);
    if (epi == EPI_RESID && ((size_t)M * N) % 4 != 0) return f5_fail(F5_EINVAL, "f5_op_linear_fused: M * N must be a multiple of 4 for the in-place form");
    if (epi == EPI_ROPE_T && (!rope || seq <= 0 || M % seq != 0 || N % 3 != 0 || (N / 3) % 64 != 0)) return f5_fail(F5_EINVAL, "bad RoPE arguments");
    hipStream_t st = (hipStream_t)stream;
    const int Kp = (int)round_up(K, 64), Mp = (int)round_up(M, 256), Np = (int)round_up(N, 256);
    DevArena a;
    void *At = nullptr, *Wt = nullptr, *Ot = nullptr;
    uint8_t* bits = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&At, (size_t)Mp * Kp * 2))) break;
        if ((rc = a.alloc(&Wt, (size_t)Np * Kp * 2))) break;
        if ((rc = a.alloc(&Ot, (size_t)Mp * N * 2))) break;  // 16-bit output, or the fp16 stream of the in-place form
        if ((rc = a.alloc_t(&bits, (size_t)(Mp / 128 + 1) * 16))) break;
        if ((rc = launch_convert_pad(precision, A, K, M, K, Kp, At, Kp, st))) break;
        if ((rc = launch_convert_pad(precision, W, K, N, K, Kp, Wt, Kp, st))) break;
        GemmParams g;
        memset(&g, 0, sizeof(g));
        g.A = At; g.lda = Kp; g.W = Wt; g.ldw = Kp; g.M = M; g.N = N; g.K = Kp;
        g.bias = bias; g.act = act; g.out_t = Ot; g.ldo = N; g.rows_per_batch = seq > 0 ? seq : M;
        if (epi == EPI_RESID) {  // in-place update of the fp16 residual stream: `out` is read (rounded to fp16), updated and written back
            if ((rc = launch_f32_to_f16(out, Ot, (size_t)M * N, st))) break;
            g = gp_resid_stream(g, Ot, true);
        }
        if (epi == EPI_GATE_T || epi == EPI_RESID) {
            g.gate = gate;
            g.rowmask = rowmask;
            if (rowmask) {
                if ((rc = launch_rowbits(rowmask, M, bits, st))) break;
                g.rowbits = bits;
            }
        }
        if (epi == EPI_ROPE_T) { g.rope = rope; g.rope_inner = N / 3; g.rope_heads = rope_heads; }
        if ((rc = launch_gemm(g, precision, GEMM_DENSE, epi, kernel, st))) break;
        rc = epi == EPI_RESID ? launch_f16_to_f32(Ot, out, (size_t)M * N, st) : launch_convert_back(precision, Ot, N, M, N, out, N, st);
    } while (0);
    return sync_and_release(a, st, rc);
}

extern "C" int f5_op_linear_fused(int kernel, int epi, int M, int N, int K, const float* A, const float* W, const float* bias, int act,
                                  const float* gate, const uint8_t* rowmask, const float* rope, int rope_heads, int seq, float* out,
                                  f5_stream_t stream) {
    return f5_op_linear_fused_p(F5_PREC_BF16, kernel, epi, M, N, K, A, W, bias, act, gate, rowmask, rope, rope_heads, seq, out, stream);
}

// The LayerNorm fold of one call site end to end (parity tests; gemm.h, lnfold.hip).  `x` [M, D] is the fp16 residual stream, handed over and
// returned as f32: (1) x += gate * (A . Wo^T + bo) in place with partial row statistics (EPI_RESID + stats_out; pivots = column 0 of `pivot`
// [M][2] or none), (2) stats_finalize -> `stats` [M][2] = (mean, rstd), (3) W' / c1 / c2 from W [N, D], bias, scale, shift (fold_weights_kernel),
// (4) out [M, N] = epilogue(rstd (x . W'^T - mean c1) + c2): epi 0 = store with `act` (FF1: GELU tanh), epi 4 = RoPE (fused QKV, N = 3 * inner).
extern "C" int f5_op_ln_fold_p(int precision, int epi, int M, int D, int N, int Kb, float* x, const float* A, const float* Wo, const float* bo, const float* gate,
                             const float* pivot, const float* W, const float* bias, const float* scale, const float* shift, int act,
                             const float* rope, int rope_heads, int seq, float* stats, float* out, f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (precision != F5_PREC_BF16 && precision != F5_PREC_FP16) return f5_fail(F5_EINVAL, "f5_op_ln_fold_p: a 16-bit precision mode (bf16 0, fp16 2), got %d", precision);
    if (M <= 0 || D <= 0 || N <= 0 || Kb <= 0 || !x || !A || !Wo || !bo || !W || !bias || !scale || !shift || !stats || !out) return f5_fail(F5_EINVAL, "bad argument");
    if (D % 128 != 0 || Kb % 32 != 0 || N % 64 != 0 || (epi != EPI_STORE_T && epi != EPI_ROPE_T)) return f5_fail(F5_EINVAL, "f5_op_ln_fold: D % 128, Kb % 32, N % 64, epi 0 | 4");
    if (epi == EPI_ROPE_T && (!rope || seq <= 0 || M % seq != 0 || N % 3 != 0 || (N / 3) % 64 != 0)) return f5_fail(F5_EINVAL, "bad RoPE arguments");
    hipStream_t st = (hipStream_t)stream;
    const size_t Mp = round_up(M, 256) + 256;
    DevArena a;
    void *At = nullptr, *Wot = nullptr, *xs = nullptr, *Wt = nullptr, *Ot = nullptr;
    float *partial = nullptr, *st2 = nullptr, *mod = nullptr, *c1 = nullptr, *c2 = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&At, Mp * Kb * 2))) break;
        if ((rc = a.alloc(&Wot, (size_t)round_up(D, 256) * Kb * 2))) break;
        if ((rc = a.alloc(&xs, Mp * D * 2))) break;
        if ((rc = a.alloc(&Wt, (size_t)round_up(N, 256) * D * 2))) break;
        if ((rc = a.alloc(&Ot, Mp * N * 2))) break;
        if ((rc = a.alloc_t(&partial, (size_t)(D / 64) * Mp * 2))) break;
        if ((rc = a.alloc_t(&st2, Mp * 2))) break;
        if ((rc = a.alloc_t(&mod, (size_t)6 * D))) break;
        if ((rc = a.alloc_t(&c1, (size_t)N))) break;
        if ((rc = a.alloc_t(&c2, (size_t)N))) break;
        if ((rc = launch_convert_pad(precision, A, Kb, M, Kb, Kb, At, Kb, st))) break;
        if ((rc = launch_convert_pad(precision, Wo, Kb, D, Kb, Kb, Wot, Kb, st))) break;
        if ((rc = launch_f32_to_f16(x, xs, (size_t)M * D, st))) break;
        if (pivot) F5_HIP(hipMemcpyAsync(st2, pivot, (size_t)M * 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
        F5_HIP(hipMemcpyAsync(mod, shift, (size_t)D * sizeof(float), hipMemcpyDeviceToDevice, st));      // (shift_msa, scale_msa) slots of one block
        F5_HIP(hipMemcpyAsync(mod + D, scale, (size_t)D * sizeof(float), hipMemcpyDeviceToDevice, st));
        GemmParams g;
        memset(&g, 0, sizeof(g));
        g.A = At; g.lda = Kb; g.W = Wot; g.ldw = Kb; g.M = M; g.N = D; g.K = Kb; g.bias = bo; g.rows_per_batch = seq > 0 ? seq : M;
        g.out_f = reinterpret_cast<float*>(xs); g.ldof = D; g.add2_f16 = 1; g.gate = gate;
        g.stats_out = partial; g.stats_ld = (int)Mp; g.stats_pivot = pivot ? st2 : nullptr;
        if ((rc = launch_gemm(g, precision, GEMM_DENSE, EPI_RESID, 1, st))) break;
        if ((rc = launch_stats_finalize(partial, (int)Mp, D / 64, M, D, pivot ? st2 : nullptr, st2, nullptr, 0, st))) break;
        if ((rc = launch_fold_weights(W, bias, mod, 6 * D, 1, 1, N, N, D, Wt, c1, c2, st))) break;
        memset(&g, 0, sizeof(g));
        g.A = xs; g.lda = D; g.W = Wt; g.ldw = D; g.M = M; g.N = N; g.K = D; g.act = act; g.out_t = Ot; g.ldo = N; g.rows_per_batch = seq > 0 ? seq : M;
        g.lnf_stats = st2; g.lnf_c1 = c1; g.lnf_c2 = c2;
        if (epi == EPI_ROPE_T) { g.rope = rope; g.rope_inner = N / 3; g.rope_heads = rope_heads; }
        if ((rc = launch_gemm(g, precision, GEMM_DENSE, epi, 1, st))) break;
        if ((rc = launch_f16_to_f32(xs, x, (size_t)M * D, st))) break;
        F5_HIP(hipMemcpyAsync(stats, st2, (size_t)M * 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
        rc = launch_convert_back(precision, Ot, N, M, N, out, N, st);
    } while (0);
    return sync_and_release(a, st, rc);
}

extern "C" int f5_op_ln_fold(int epi, int M, int D, int N, int Kb, float* x, const float* A, const float* Wo, const float* bo, const float* gate,
                             const float* pivot, const float* W, const float* bias, const float* scale, const float* shift, int act,
                             const float* rope, int rope_heads, int seq, float* stats, float* out, f5_stream_t stream) {
    return f5_op_ln_fold_p(F5_PREC_BF16, epi, M, D, N, Kb, x, A, Wo, bo, gate, pivot, W, bias, scale, shift, act, rope, rope_heads, seq, stats, out, stream);
}

// The producer half of a LayerNorm-fold site on its own, with everything it writes handed back (parity tests of the in-place epilogue's lane maps):
// x [M, N] (the fp16 residual stream as f32) += gate * (A . W^T + bias) where rowmask[m] != 0, `planes` [N / 64][M][2] = the partial row sums
// (sum (h - pivot), sum (h - pivot)^2 per 64-feature plane, pivot = column 0 of `pivot` [M][2] or 0) as the GEMM stored them, `stats` [M][2] =
// stats_finalize's (mean, rstd), `guard` = the six words of the fp16 range guard (zeroed here, raised by the finalize) or NULL.
extern "C" int f5_op_resid_stats_p(int precision, int M, int N, int K, float* x, const float* A, const float* W, const float* bias, const float* gate,
                                   const uint8_t* rowmask, const float* pivot, float* planes, float* stats, unsigned* guard, f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (precision != F5_PREC_BF16 && precision != F5_PREC_FP16) return f5_fail(F5_EINVAL, "f5_op_resid_stats_p: a 16-bit precision mode (bf16 0, fp16 2), got %d", precision);
    if (M <= 0 || N <= 0 || K <= 0 || !x || !A || !W || !bias || !planes || !stats) return f5_fail(F5_EINVAL, "bad argument");
    if (N % 128 != 0 || K % 32 != 0) return f5_fail(F5_EINVAL, "f5_op_resid_stats_p: N % 128, K % 32");
    hipStream_t st = (hipStream_t)stream;
    const size_t Mp = round_up(M, 256) + 256;
    DevArena a;
    void *At = nullptr, *Wt = nullptr, *xs = nullptr;
    float *partial = nullptr, *st2 = nullptr;
    unsigned* sat = nullptr;
    uint8_t* bits = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&At, Mp * K * 2))) break;
        if ((rc = a.alloc(&Wt, (size_t)round_up(N, 256) * K * 2))) break;
        if ((rc = a.alloc(&xs, Mp * N * 2))) break;
        if ((rc = a.alloc_t(&partial, (size_t)(N / 64) * Mp * 2))) break;
        if ((rc = a.alloc_t(&st2, Mp * 2))) break;
        if ((rc = a.alloc_t(&sat, (size_t)8))) break;
        if ((rc = a.alloc_t(&bits, (size_t)(Mp / 128 + 1) * 16))) break;
        if ((rc = launch_convert_pad(precision, A, K, M, K, K, At, K, st))) break;
        if ((rc = launch_convert_pad(precision, W, K, N, K, K, Wt, K, st))) break;
        if ((rc = launch_f32_to_f16(x, xs, (size_t)M * N, st))) break;
        F5_HIP(hipMemsetAsync(partial, 0, (size_t)(N / 64) * Mp * 2 * sizeof(float), st));
        F5_HIP(hipMemsetAsync(sat, 0, 8 * sizeof(unsigned), st));
        if (pivot) F5_HIP(hipMemcpyAsync(st2, pivot, (size_t)M * 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
        GemmParams g;
        memset(&g, 0, sizeof(g));
        g.A = At; g.lda = K; g.W = Wt; g.ldw = K; g.M = M; g.N = N; g.K = K; g.bias = bias; g.rows_per_batch = M;
        g.out_f = reinterpret_cast<float*>(xs); g.ldof = N; g.add2_f16 = 1; g.gate = gate;
        g.stats_out = partial; g.stats_ld = (int)Mp; g.stats_pivot = pivot ? st2 : nullptr;
        if (rowmask) {
            if ((rc = launch_rowbits(rowmask, M, bits, st))) break;
            g.rowmask = rowmask; g.rowbits = bits;
        }
        if ((rc = launch_gemm(g, precision, GEMM_DENSE, EPI_RESID, 1, st))) break;
        if ((rc = launch_stats_finalize(partial, (int)Mp, N / 64, M, N, pivot ? st2 : nullptr, st2, sat, 0, st))) break;
        if ((rc = launch_f16_to_f32(xs, x, (size_t)M * N, st))) break;
        F5_HIP(hipMemcpy2DAsync(planes, (size_t)M * 2 * sizeof(float), partial, Mp * 2 * sizeof(float), (size_t)M * 2 * sizeof(float), N / 64, hipMemcpyDeviceToDevice, st));
        F5_HIP(hipMemcpyAsync(stats, st2, (size_t)M * 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (guard) F5_HIP(hipMemcpyAsync(guard, sat, 6 * sizeof(unsigned), hipMemcpyDeviceToDevice, st));
    } while (0);
    return sync_and_release(a, st, rc);
}

extern "C" int f5_op_layernorm_modulate(int rows, int dim, const float* x, const float* scale, const float* shift, float* out,
                                        f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (!x || !scale || !shift || !out) return f5_fail(F5_EINVAL, "null argument");
    return launch_layernorm(F5_PREC_FP32, x, dim, rows, dim, scale, shift, 0, rows, 1, out, dim, (hipStream_t)stream);
}

extern "C" int f5_op_attention(int precision, int kernel, int B, int N, int H, const float* qkv, const uint8_t* mask, float* out,
                               f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (B <= 0 || N <= 0 || H <= 0 || !qkv || !out) return f5_fail(F5_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int inner = H * 64, rows = B * N;
    const size_t es = f5_elem_size(precision);
    DevArena a;
    void *q = nullptr, *o = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&q, (size_t)rows * 3 * inner * es))) break;
        if ((rc = a.alloc(&o, (size_t)rows * inner * es))) break;
        if ((rc = launch_convert_pad(precision, qkv, 3 * inner, rows, 3 * inner, 3 * inner, q, 3 * inner, st))) break;
        if ((rc = launch_attention(precision, kernel, B, N, H, q, 3 * inner, mask, o, inner, st))) break;
        rc = launch_convert_back(precision, o, inner, rows, inner, out, inner, st);
    } while (0);
    return sync_and_release(a, st, rc);
}

// Attention with dropout (philox.h) on its own: the mask of call word `stream_word`, batch item b drawn with batch word
// batch0 + b.  kernel 0 = the flagged reference kernel, 1 = attention_dropout.hip's MFMA kernel (bf16).  prob == 0 is f5_op_attention.
extern "C" int f5_op_attention_dropout(int precision, int kernel, int B, int N, int H, const float* qkv, const uint8_t* mask, float prob, uint64_t seed,
                                       uint32_t stream_word, uint32_t batch0, float* out, f5_stream_t stream) {
    if (!(prob >= 0.f && prob < 1.f)) return f5_fail(F5_EINVAL, "f5_op_attention_dropout: prob must lie in [0, 1)");
    if (prob == 0.f) return f5_op_attention(precision, kernel, B, N, H, qkv, mask, out, stream);
    F5_TRY(f5_check_device());
    if (B <= 0 || N <= 0 || H <= 0 || !qkv || !out) return f5_fail(F5_EINVAL, "bad argument");
    if (kernel != 0 && kernel != 1) return f5_fail(F5_EINVAL, "f5_op_attention_dropout: kernel is 0 (reference) or 1 (MFMA, bf16)");
    hipStream_t st = (hipStream_t)stream;
    const int inner = H * 64, rows = B * N;
    const size_t es = f5_elem_size(precision);
    AttnDropout d;
    d.prob = attn_dropout_prob_of(prob);
    d.seed = seed;
    d.offset = stream_word;
    d.bw0 = batch0;
    DevArena a;
    void *q = nullptr, *o = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&q, (size_t)rows * 3 * inner * es))) break;
        if ((rc = a.alloc(&o, (size_t)rows * inner * es))) break;
        if ((rc = launch_convert_pad(precision, qkv, 3 * inner, rows, 3 * inner, 3 * inner, q, 3 * inner, st))) break;
        if ((rc = launch_attention(precision, kernel, B, N, H, q, 3 * inner, mask, o, inner, st, 0, 0, &d))) break;
        rc = launch_convert_back(precision, o, inner, rows, inner, out, inner, st);
    } while (0);
    return sync_and_release(a, st, rc);
}

// Attention on PRE-SCALED q (bf16): the q part of `qkv` already holds softmax_scale * log2(e) times the projected q, as the production path's
// q projection stores it; the kernels apply no scale, the 64-queries-per-wave kernel runs its reference-free build.
extern "C" int f5_op_attention_prescaled(int kernel, int B, int N, int H, const float* qkv, const uint8_t* mask, float* out, f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (B <= 0 || N <= 0 || H <= 0 || !qkv || !out) return f5_fail(F5_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int inner = H * 64, rows = B * N;
    DevArena a;
    void *q = nullptr, *o = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&q, (size_t)rows * 3 * inner * 2))) break;
        if ((rc = a.alloc(&o, (size_t)rows * inner * 2))) break;
        if ((rc = launch_convert_pad(F5_PREC_BF16, qkv, 3 * inner, rows, 3 * inner, 3 * inner, q, 3 * inner, st))) break;
        if ((rc = launch_attention(F5_PREC_BF16, kernel, B, N, H, q, 3 * inner, mask, o, inner, st, 0, 1))) break;
        rc = launch_convert_back(F5_PREC_BF16, o, inner, rows, inner, out, inner, st);
    } while (0);
    return sync_and_release(a, st, rc);
}

// The fold-table builder (lnfold.hip: fold_weights_kernel) on one block and one evaluation time: W [R, D], bias [R], the two norms' (scale,
// shift) [D] each -> W' [R, D] (fp16, returned as f32), c1 [R], c2 [R].  Rows below qkv_rows take the attention norm's pair, the others the FF
// norm's; qscaled: the first q_rows rows carry softmax_scale * log2(e) (pre-scaled q).
extern "C" int f5_op_fold_weights(int R, int qkv_rows, int q_rows, int D, int qscaled, const float* W, const float* bias, const float* scale_msa,
                                  const float* shift_msa, const float* scale_mlp, const float* shift_mlp, float* Wt, float* c1, float* c2,
                                  f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (R <= 0 || D <= 0 || D % 4 != 0 || qkv_rows < 0 || q_rows < 0 || q_rows > R || !W || !bias || !scale_msa || !shift_msa || !scale_mlp || !shift_mlp ||
        !Wt || !c1 || !c2)
        return f5_fail(F5_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    DevArena a;
    void* Wh = nullptr;
    float* mod = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&Wh, (size_t)R * D * 2))) break;
        if ((rc = a.alloc_t(&mod, (size_t)6 * D))) break;
        F5_HIP(hipMemsetAsync(mod, 0, (size_t)6 * D * sizeof(float), st));
        F5_HIP(hipMemcpyAsync(mod, shift_msa, (size_t)D * sizeof(float), hipMemcpyDeviceToDevice, st));  // slot order of one block: modules.py:312
        F5_HIP(hipMemcpyAsync(mod + D, scale_msa, (size_t)D * sizeof(float), hipMemcpyDeviceToDevice, st));
        F5_HIP(hipMemcpyAsync(mod + 3 * D, shift_mlp, (size_t)D * sizeof(float), hipMemcpyDeviceToDevice, st));
        F5_HIP(hipMemcpyAsync(mod + 4 * D, scale_mlp, (size_t)D * sizeof(float), hipMemcpyDeviceToDevice, st));
        if ((rc = launch_fold_weights(W, bias, mod, 6 * D, 1, 1, R, qkv_rows, D, Wh, c1, c2, st, qscaled ? q_rows : 0, qscaled ? F5_ATTN_QSCALE : 1.0f))) break;
        rc = launch_f16_to_f32(Wh, Wt, (size_t)R * D, st);
    } while (0);
    return sync_and_release(a, st, rc);
}

// The ragged sampler's attention call (dit_eval.hip) on its own: `cnt` utterances at rows off[u] .. off[u] + n[u] of each of the `nbr` branches,
// the branches `rows` apart (the batch stride).  `out` is staged into the activation dtype first, so rows no launch writes come back as given.
extern "C" int f5_op_attention_ragged(int precision, int attn_kernel, int nbr, int cnt, const int* off, const int* n, int H, int rows, int ldq_extra,
                                      int ldo_extra, const float* qkv, float* out, f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (nbr <= 0 || cnt <= 0 || H <= 0 || rows <= 0 || ldq_extra < 0 || ldo_extra < 0 || !off || !n || !qkv || !out) return f5_fail(F5_EINVAL, "bad argument");
    if ((long)nbr * rows > 0x7fffffffL) return f5_fail(F5_EINVAL, "f5_op_attention_ragged: nbr * rows exceeds the row index range");
    for (int u = 0; u < cnt; ++u) {
        if (n[u] < 1) return f5_fail(F5_EINVAL, "f5_op_attention_ragged: utterance %d has no rows (n = %d)", u, n[u]);
        if (off[u] < 0 || (long)off[u] + n[u] > rows)
            return f5_fail(F5_EINVAL, "f5_op_attention_ragged: utterance %d (rows %d .. %ld) lies outside the %d rows of a branch", u, off[u], (long)off[u] + n[u], rows);
    }
    hipStream_t st = (hipStream_t)stream;
    const int inner = H * 64, ldq = 3 * inner + ldq_extra, ldo = inner + ldo_extra, all = nbr * rows;
    const size_t es = f5_elem_size(precision);
    DevArena a;
    void *q = nullptr, *o = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&q, (size_t)all * ldq * es))) break;
        if ((rc = a.alloc(&o, (size_t)all * ldo * es))) break;
        if ((rc = launch_convert_pad(precision, qkv, ldq, all, ldq, ldq, q, ldq, st))) break;
        if ((rc = launch_convert_pad(precision, out, ldo, all, ldo, ldo, o, ldo, st))) break;
        if ((rc = launch_attention_ragged_all(precision, attn_kernel, nbr, cnt, off, n, H, q, ldq, o, ldo, st, rows))) break;
        rc = launch_convert_back(precision, o, ldo, all, ldo, out, ldo, st);
    } while (0);
    return sync_and_release(a, st, rc);
}


// the padded input-channel window one 64-channel output tile of the grouped Conv1d(k = 31, groups = 16) reads (GemmParams::conv_win)
static int conv31_window(int dim) {
    const int cg = dim / 16;
    int win = 0;
    for (int n0 = 0; n0 < dim; n0 += 64) win = std::max(win, ((n0 + 63) / cg + 1) * cg - (n0 / cg) * cg);
    return (int)round_up(win, 64);
}

// rearranges one conv weight [dim, dim/16, 31] (f32, on the device: copied back first) on the host into the tap-major image [31][dim][win] of
// GEMM_CONV31 and uploads it in the precision's dtype
static int upload_conv31_weight(DevArena& a, int precision, int dim, int win, const float* w, void** wr) {
    const int cg = dim / 16;
    std::vector<float> hw((size_t)dim * cg * 31), r((size_t)31 * dim * win, 0.f);
    if (hipMemcpy(hw.data(), w, hw.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return f5_fail(F5_EHIP, "weight copy failed");
    for (int n = 0; n < dim; ++n) {
        const int w0c = ((n / 64 * 64) / cg) * cg, g0 = (n / cg) * cg;
        for (int ci = 0; ci < cg; ++ci)
            for (int tap = 0; tap < 31; ++tap) r[((size_t)tap * dim + n) * win + (g0 + ci - w0c)] = hw[((size_t)n * cg + ci) * 31 + tap];
    }
    return f5_upload_t(a, precision, r.data(), r.size(), wr);
}

// One grouped Conv1d(k = 31, groups = 16, padding 15) + bias (+ Mish) on its own, through exactly the GemmParams of the first launch of
// f5_op_conv_pos_embed (test hook).  kernel 0 = the reference tile kernel, 1 = the tuned route as the model takes it (conv31 / conv31_tok knobs).
extern "C" int f5_op_conv31(int precision, int kernel, int B, int N, int dim, const float* x, const float* w, const float* b, int act, float* out,
                            f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (B <= 0 || N <= 0 || dim <= 0 || dim % 128 != 0 || !x || !w || !b || !out) return f5_fail(F5_EINVAL, "bad argument");
    if (act != ACT_NONE && act != ACT_MISH) return f5_fail(F5_EINVAL, "f5_op_conv31: act is none (0) or mish (3)");
    if (kernel != 0 && kernel != 1) return f5_fail(F5_EINVAL, "f5_op_conv31: kernel is 0 (tile kernel) or 1 (tuned route)");
    if (kernel == 1 && precision != F5_PREC_BF16 && precision != F5_PREC_FP16) return f5_fail(F5_EINVAL, "f5_op_conv31: the tuned route runs the 16-bit modes");
    hipStream_t st = (hipStream_t)stream;
    const int rows = B * N, cg = dim / 16, win = conv31_window(dim);
    const size_t es = f5_elem_size(precision);
    DevArena a;
    int rc = 0;
    do {
        void *wr = nullptr, *xt = nullptr, *c1 = nullptr;
        if ((rc = upload_conv31_weight(a, precision, dim, win, w, &wr))) break;
        if ((rc = a.alloc(&xt, (size_t)rows * dim * es))) break;
        if ((rc = a.alloc(&c1, (size_t)rows * dim * es))) break;
        if ((rc = launch_convert_pad(precision, x, dim, rows, dim, dim, xt, dim, st))) break;
        GemmParams g;
        memset(&g, 0, sizeof(g));
        g.A = xt; g.lda = dim; g.W = wr; g.M = rows; g.N = dim; g.K = 31 * win; g.bias = b; g.act = act;
        g.rows_per_batch = N; g.conv_cg = cg; g.conv_win = win; g.out_t = c1; g.ldo = dim;
        if (kernel == 1 && !gemm_fast_supported(g, precision, GEMM_CONV31, EPI_STORE_T)) { rc = f5_fail(F5_ENOTSUP, "f5_op_conv31: the tuned kernels cannot run this shape"); break; }
        if ((rc = launch_gemm(g, precision, GEMM_CONV31, EPI_STORE_T, kernel, st))) break;
        rc = launch_convert_back(precision, c1, dim, rows, dim, out, dim, st);
    } while (0);
    return sync_and_release(a, st, rc);
}

// Test staging of a caller's output buffer into the element type a kernel stores and back: plain casts over the whole buffer, padding columns
// and guard rows included, so that NaN fill survives and a write outside [M, N] shows.
template <typename T> __global__ __launch_bounds__(256) void stage_cast_kernel(const float* __restrict__ src, T* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = (T)src[i];
}
template <typename T> __global__ __launch_bounds__(256) void unstage_cast_kernel(const T* __restrict__ src, float* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = (float)src[i];
}
template <typename T> static int stage_cast(const float* src, void* dst, size_t n, hipStream_t st) {
    if (n == 0) return 0;
    hipLaunchKernelGGL((stage_cast_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, (T*)dst, n);
    F5_LAUNCH_CHECK();
    return 0;
}
template <typename T> static int unstage_cast(const void* src, float* dst, size_t n, hipStream_t st) {
    if (n == 0) return 0;
    hipLaunchKernelGGL((unstage_cast_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const T*)src, dst, n);
    F5_LAUNCH_CHECK();
    return 0;
}
static int stage_cast_p(int precision, const float* src, void* dst, size_t n, hipStream_t st) {
    return precision == F5_PREC_BF16 ? stage_cast<bf16_t>(src, dst, n, st) : precision == F5_PREC_FP16 ? stage_cast<f16_t>(src, dst, n, st) : stage_cast<float>(src, dst, n, st);
}
static int unstage_cast_p(int precision, const void* src, float* dst, size_t n, hipStream_t st) {
    return precision == F5_PREC_BF16 ? unstage_cast<bf16_t>(src, dst, n, st) : precision == F5_PREC_FP16 ? unstage_cast<f16_t>(src, dst, n, st) : unstage_cast<float>(src, dst, n, st);
}

// The reference tile kernel (gemm.hip: gemm_tile_kernel, kernel_kind 0) with every parameter its epilogues branch on in the caller's hands
// (test hook; include/f5hip.h: f5_tile_gemm).  The outputs are the caller's buffers [out_rows, ldo / ldof]: staged into the stored type whole,
// handed to the kernel, and staged back whole.
extern "C" int f5_op_tile_gemm(const f5_tile_gemm* t, f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (!t) return f5_fail(F5_EINVAL, "bad argument");
    const int P = t->precision, mode = t->mode, epi = t->epi, M = t->M, N = t->N, K = t->K;
    if (P != F5_PREC_BF16 && P != F5_PREC_FP32 && P != F5_PREC_FP16) return f5_fail(F5_EINVAL, "f5_op_tile_gemm: bad precision %d", P);
    if (mode != GEMM_DENSE && mode != GEMM_CONV31) return f5_fail(F5_EINVAL, "f5_op_tile_gemm: mode is 0 (dense) or 1 (conv31)");
    if (epi < EPI_STORE_T || epi > EPI_GATE_T || (mode == GEMM_CONV31 && epi != EPI_STORE_T && epi != EPI_RESID && epi != EPI_GATE_T))
        return f5_fail(F5_EINVAL, "f5_op_tile_gemm: unsupported mode/epilogue %d/%d", mode, epi);
    if (M <= 0 || N <= 0 || !t->A || !t->W) return f5_fail(F5_EINVAL, "bad argument");
    const int rpb = t->rows_per_batch > 0 ? t->rows_per_batch : M;
    if (mode == GEMM_DENSE && (K <= 0 || K % 32 != 0 || t->a_row_mod < 0)) return f5_fail(F5_EINVAL, "f5_op_tile_gemm: K must be a positive multiple of 32");
    if (mode == GEMM_CONV31 && (N % 128 != 0 || M % rpb != 0 || t->a_row_mod != 0)) return f5_fail(F5_EINVAL, "f5_op_tile_gemm(conv31): dim % 128, whole sequences");
    const bool needs_t = epi == EPI_STORE_T || epi == EPI_ROPE_T || epi == EPI_GATE_T || epi == EPI_ADD2;
    const bool needs_f = epi == EPI_STORE_F32 || epi == EPI_RESID || epi == EPI_ADD2;
    if (t->out_rows < M || (needs_t && (!t->out_t || t->ldo < N)) || (needs_f && (!t->out_f || t->ldof < N)))
        return f5_fail(F5_EINVAL, "f5_op_tile_gemm: an output buffer is missing or smaller than [M, N]");
    if (epi == EPI_ADD2 && (!t->addend || t->ldadd < N)) return f5_fail(F5_EINVAL, "f5_op_tile_gemm: EPI_ADD2 needs an addend [M, ldadd >= N]");
    if (t->add2_f16 && epi != EPI_RESID && epi != EPI_ADD2) return f5_fail(F5_EINVAL, "f5_op_tile_gemm: add2_f16 belongs to EPI_RESID / EPI_ADD2");
    if (t->gate_bstride < 0 || ((t->gate || t->rowmask) && epi != EPI_RESID && epi != EPI_GATE_T))
        return f5_fail(F5_EINVAL, "f5_op_tile_gemm: gate / rowmask belong to EPI_RESID / EPI_GATE_T");
    if (epi == EPI_ROPE_T && (!t->rope || N % 3 != 0 || (N / 3) % 64 != 0 || t->rope_heads < 0 || t->rope_heads > N / 192))
        return f5_fail(F5_EINVAL, "bad RoPE arguments");
    hipStream_t st = (hipStream_t)stream;
    const size_t es = f5_elem_size(P);
    const size_t nt = (size_t)t->out_rows * t->ldo, nf = (size_t)t->out_rows * t->ldof;
    DevArena a;
    void *At = nullptr, *Wt = nullptr, *Ot = nullptr, *Of = nullptr, *Ad = nullptr;
    int rc = 0;
    do {
        GemmParams g;
        memset(&g, 0, sizeof(g));
        if (mode == GEMM_DENSE) {
            const int arows = t->a_row_mod > 0 ? t->a_row_mod : M;
            if ((rc = a.alloc(&At, (size_t)arows * K * es))) break;
            if ((rc = a.alloc(&Wt, (size_t)N * K * es))) break;
            if ((rc = launch_convert_pad(P, t->A, K, arows, K, K, At, K, st))) break;
            if ((rc = launch_convert_pad(P, t->W, K, N, K, K, Wt, K, st))) break;
            g.lda = K; g.ldw = K; g.K = K; g.a_row_mod = t->a_row_mod;
        } else {
            const int win = conv31_window(N);
            if ((rc = upload_conv31_weight(a, P, N, win, t->W, &Wt))) break;
            if ((rc = a.alloc(&At, (size_t)M * N * es))) break;
            if ((rc = launch_convert_pad(P, t->A, N, M, N, N, At, N, st))) break;
            g.lda = N; g.K = 31 * win; g.conv_cg = N / 16; g.conv_win = win;
        }
        g.A = At; g.W = Wt; g.M = M; g.N = N; g.bias = t->bias; g.act = t->act;
        g.gate = t->gate; g.gate_bstride = t->gate_bstride; g.rows_per_batch = rpb; g.rowmask = t->rowmask;
        if (epi == EPI_ROPE_T) { g.rope = t->rope; g.rope_inner = N / 3; g.rope_heads = t->rope_heads; }
        if (needs_t) {
            if ((rc = a.alloc(&Ot, nt * es))) break;
            if ((rc = stage_cast_p(P, t->out_t, Ot, nt, st))) break;
            g.out_t = Ot; g.ldo = t->ldo;
        }
        if (needs_f) {
            g.out_f = t->out_f; g.ldof = t->ldof; g.add2_f16 = t->add2_f16 ? 1 : 0;
            if (t->add2_f16) {  // the fp16 residual stream
                if ((rc = a.alloc(&Of, nf * 2))) break;
                if ((rc = stage_cast<f16_t>(t->out_f, Of, nf, st))) break;
                g.out_f = reinterpret_cast<float*>(Of);
            }
        }
        if (epi == EPI_ADD2) {
            g.addend = t->addend; g.ldadd = t->ldadd;
            if (t->add2_f16) {
                if ((rc = a.alloc(&Ad, (size_t)M * t->ldadd * 2))) break;
                if ((rc = stage_cast<f16_t>(t->addend, Ad, (size_t)M * t->ldadd, st))) break;
                g.addend = reinterpret_cast<const float*>(Ad);
            }
        }
        if ((rc = launch_gemm(g, P, mode, epi, 0, st))) break;
        if (needs_t && (rc = unstage_cast_p(P, Ot, t->out_t, nt, st))) break;
        if (needs_f && t->add2_f16) rc = unstage_cast<f16_t>(Of, t->out_f, nf, st);
    } while (0);
    return sync_and_release(a, st, rc);
}

extern "C" int f5_op_conv_pos_embed(int precision, int B, int N, int dim, const float* x, const float* w0, const float* b0, const float* w1,
                                    const float* b1, float* out, f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (B <= 0 || N <= 0 || dim <= 0 || dim % 128 != 0 || !x || !w0 || !b0 || !w1 || !b1 || !out) return f5_fail(F5_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int rows = B * N, cg = dim / 16, win = conv31_window(dim);
    const size_t es = f5_elem_size(precision);
    DevArena a;
    int rc = 0;
    do {
        void* wr[2] = {nullptr, nullptr};
        const float* ws[2] = {w0, w1};
        for (int li = 0; li < 2 && rc == 0; ++li) rc = upload_conv31_weight(a, precision, dim, win, ws[li], &wr[li]);
        if (rc) break;
        void *xt = nullptr, *c1 = nullptr;
        float* acc = nullptr;
        if ((rc = a.alloc(&xt, (size_t)rows * dim * es))) break;
        if ((rc = a.alloc(&c1, (size_t)rows * dim * es))) break;
        if ((rc = a.alloc_t(&acc, (size_t)rows * dim))) break;  // zero-initialised accumulator for the RESID epilogue
        if ((rc = launch_convert_pad(precision, x, dim, rows, dim, dim, xt, dim, st))) break;
        GemmParams g;
        memset(&g, 0, sizeof(g));
        g.A = xt; g.lda = dim; g.W = wr[0]; g.M = rows; g.N = dim; g.K = 31 * win; g.bias = b0; g.act = ACT_MISH;
        g.rows_per_batch = N; g.conv_cg = cg; g.conv_win = win; g.out_t = c1; g.ldo = dim;
        // tuning knob "op_conv_kernel" = 1: the tuned kernels exactly as dit_eval launches them (store-only second conv, the 16-bit modes)
        const int kind = (g_op_conv_kernel && precision != F5_PREC_FP32 && gemm_fast_supported(g, precision, GEMM_CONV31, EPI_STORE_T)) ? 1 : 0;
        if ((rc = launch_gemm(g, precision, GEMM_CONV31, EPI_STORE_T, kind, st))) break;
        if (kind) {
            void* c2 = nullptr;
            if ((rc = a.alloc(&c2, (size_t)rows * dim * es))) break;
            g.A = c1; g.W = wr[1]; g.bias = b1; g.out_t = c2;
            if ((rc = launch_gemm(g, precision, GEMM_CONV31, EPI_GATE_T, 1, st))) break;
            rc = launch_convert_back(precision, c2, dim, rows, dim, out, dim, st);
            break;
        }
        g.A = c1; g.W = wr[1]; g.bias = b1; g.out_t = nullptr; g.out_f = acc; g.ldof = dim;
        if ((rc = launch_gemm(g, precision, GEMM_CONV31, EPI_RESID, 0, st))) break;
        rc = launch_convert_back(F5_PREC_FP32, acc, dim, rows, dim, out, dim, st);
    } while (0);
    return sync_and_release(a, st, rc);
}

// ----------------------------------------------------------------------------- row-wise kernels (test and diagnostic entry points)
// Test staging of an fp16 stream: a plain cast (round to nearest, overflow to inf, NaN kept), so that a test can hand the kernels the values
// a saturating producer never writes.  The model's own conversion is launch_f32_to_f16.
__global__ __launch_bounds__(256) void stage_f16_kernel(const float* __restrict__ src, _Float16* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = (_Float16)src[i];
}
static int stage_f16(const float* src, void* dst, size_t n, hipStream_t st) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(stage_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, (_Float16*)dst, n);
    F5_LAUNCH_CHECK();
    return 0;
}

extern "C" int f5_op_layernorm_res(int precision, int xin_f16, int xout_f16, int rows, int dim, int ldx, int ldy, int ldo, const float* x,
                                   const float* y, const float* y2, int ymode, const float* mul, const float* add, int mod_bstride,
                                   int rows_per_batch, int add_one, int inplace, int sat_tag, float* out, float* xback, uint32_t* guard,
                                   f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (rows <= 0 || dim <= 0 || !x || !mul || !add || !out || !xback) return f5_fail(F5_EINVAL, "bad argument");
    if (precision != F5_PREC_BF16 && precision != F5_PREC_FP32 && precision != F5_PREC_FP16) return f5_fail(F5_EINVAL, "bad precision %d", precision);
    if (ldx < dim || ldo < dim || (ldx & 3) || (ldo & 3) || (y && (ldy < dim || (ldy & 3)))) return f5_fail(F5_EINVAL, "leading dimensions below dim");
    if ((ymode != 0 && !y) || (ymode == 3 && !y2)) return f5_fail(F5_EINVAL, "residual mode %d needs its branches", ymode);
    if (inplace && xin_f16 != xout_f16) return f5_fail(F5_EINVAL, "in place needs one storage type");
    hipStream_t st = (hipStream_t)stream;
    const size_t es = f5_elem_size(precision), xn = (size_t)rows * ldx;
    DevArena a;
    void *xs = nullptr, *xo = nullptr, *ys = nullptr, *y2s = nullptr, *os = nullptr;
    unsigned* sat = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&xs, xn * (xin_f16 ? 2 : 4)))) break;
        if ((rc = a.alloc(&os, (size_t)rows * ldo * es))) break;  // zeroed: the columns past dim must stay 0
        if ((rc = a.alloc_t(&sat, 8))) break;
        if (y && (rc = a.alloc(&ys, (size_t)rows * ldy * es))) break;
        if (y2 && (rc = a.alloc(&y2s, (size_t)rows * ldy * es))) break;
        if (inplace) xo = xs;
        else if ((rc = a.alloc(&xo, xn * (xout_f16 ? 2 : 4)))) break;
        if (xin_f16) {
            if ((rc = stage_f16(x, xs, xn, st))) break;
        } else {
            F5_HIP(hipMemcpyAsync(xs, x, xn * 4, hipMemcpyDeviceToDevice, st));
        }
        if (y && (rc = launch_convert_pad(precision, y, ldy, rows, ldy, ldy, ys, ldy, st))) break;
        if (y2 && (rc = launch_convert_pad(precision, y2, ldy, rows, ldy, ldy, y2s, ldy, st))) break;
        if ((rc = launch_layernorm_res(precision, xs, xin_f16, xo, xout_f16, ldx, rows, dim, ys, ldy, y2s, ymode, mul, add, mod_bstride, rows_per_batch,
                                       add_one, os, ldo, st, nullptr, guard ? sat : nullptr, sat_tag)))
            break;
        if ((rc = launch_convert_back(precision, os, ldo, rows, ldo, out, ldo, st))) break;
        if ((rc = xout_f16 ? launch_f16_to_f32(xo, xback, xn, st) : launch_convert_back(F5_PREC_FP32, xo, ldx, rows, ldx, xback, ldx, st))) break;
        if (guard) F5_HIP(hipMemcpyAsync(guard, sat, 6 * sizeof(unsigned), hipMemcpyDeviceToDevice, st));
    } while (0);
    return sync_and_release(a, st, rc);
}

extern "C" int f5_op_f32_to_f16(int64_t n, const float* src, float* dst, uint32_t* guard, f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (n <= 0 || !src || !dst) return f5_fail(F5_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    DevArena a;
    void* h = nullptr;
    unsigned* sat = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&h, (size_t)n * 2))) break;
        if ((rc = a.alloc_t(&sat, 8))) break;
        if ((rc = launch_f32_to_f16(src, h, (size_t)n, st, guard ? sat : nullptr))) break;
        if ((rc = launch_f16_to_f32(h, dst, (size_t)n, st))) break;
        if (guard) F5_HIP(hipMemcpyAsync(guard, sat, 6 * sizeof(unsigned), hipMemcpyDeviceToDevice, st));
    } while (0);
    return sync_and_release(a, st, rc);
}

extern "C" int f5_op_qknorm_rope(int precision, int rows, int heads, int rope_heads, int rows_per_batch, const float* qkv, const float* wq,
                                 const float* wk, const float* rope, float* out, f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (rows <= 0 || heads <= 0 || rope_heads < 0 || rope_heads > heads || rows_per_batch <= 0 || !qkv || !wq || !wk || !out || (rope_heads && !rope))
        return f5_fail(F5_EINVAL, "bad argument");
    if (precision != F5_PREC_BF16 && precision != F5_PREC_FP32 && precision != F5_PREC_FP16) return f5_fail(F5_EINVAL, "bad precision %d", precision);
    hipStream_t st = (hipStream_t)stream;
    const int inner = heads * 64, ld = 3 * inner;
    DevArena a;
    void* q = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&q, (size_t)rows * ld * f5_elem_size(precision)))) break;
        if ((rc = launch_convert_pad(precision, qkv, ld, rows, ld, ld, q, ld, st))) break;
        if ((rc = launch_qknorm_rope(precision, q, ld, rows, inner, heads, rope_heads, wq, wk, rope, rows_per_batch, st))) break;
        rc = launch_convert_back(precision, q, ld, rows, ld, out, ld, st);
    } while (0);
    return sync_and_release(a, st, rc);
}

extern "C" int f5_op_dwconv7_ln(int precision, int B, int N, int C, const float* x, const float* wt, const float* cbias, const float* ln_w,
                                const float* ln_b, float* out, f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (B <= 0 || N <= 0 || C <= 0 || !x || !wt || !cbias || !ln_w || !ln_b || !out) return f5_fail(F5_EINVAL, "bad argument");
    if (precision != F5_PREC_BF16 && precision != F5_PREC_FP32 && precision != F5_PREC_FP16) return f5_fail(F5_EINVAL, "bad precision %d", precision);
    hipStream_t st = (hipStream_t)stream;
    const int rows = B * N;
    DevArena a;
    void* o = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&o, (size_t)rows * C * f5_elem_size(precision)))) break;
        if ((rc = launch_dwconv7_ln(precision, x, B, N, C, wt, cbias, ln_w, ln_b, o, C, st))) break;
        rc = launch_convert_back(precision, o, C, rows, C, out, C, st);
    } while (0);
    return sync_and_release(a, st, rc);
}

extern "C" int f5_op_grn(int precision, int B, int N, int C, const float* h, const float* gamma, const float* beta, float* out, f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (B <= 0 || N <= 0 || C <= 0 || !h || !gamma || !beta || !out) return f5_fail(F5_EINVAL, "bad argument");
    if (precision != F5_PREC_BF16 && precision != F5_PREC_FP32 && precision != F5_PREC_FP16) return f5_fail(F5_EINVAL, "bad precision %d", precision);
    hipStream_t st = (hipStream_t)stream;
    const int rows = B * N;
    DevArena a;
    void* hs = nullptr;
    float* scratch = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&hs, (size_t)rows * C * f5_elem_size(precision)))) break;
        if ((rc = a.alloc_t(&scratch, (size_t)B * C + B))) break;
        if ((rc = launch_convert_pad(precision, h, C, rows, C, C, hs, C, st))) break;
        if ((rc = launch_grn(precision, hs, B, N, C, gamma, beta, scratch, st))) break;
        rc = launch_convert_back(precision, hs, C, rows, C, out, C, st);
    } while (0);
    return sync_and_release(a, st, rc);
}

extern "C" int f5_op_rmsnorm(int precision, int rows, int dim, const float* x, const float* g, float* out, f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (rows <= 0 || dim <= 0 || !x || !g || !out) return f5_fail(F5_EINVAL, "bad argument");
    if (precision != F5_PREC_BF16 && precision != F5_PREC_FP32 && precision != F5_PREC_FP16) return f5_fail(F5_EINVAL, "bad precision %d", precision);
    hipStream_t st = (hipStream_t)stream;
    DevArena a;
    void* o = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&o, (size_t)rows * dim * f5_elem_size(precision)))) break;
        if ((rc = launch_rmsnorm(precision, x, dim, rows, dim, g, o, dim, st))) break;
        rc = launch_convert_back(precision, o, dim, rows, dim, out, dim, st);
    } while (0);
    return sync_and_release(a, st, rc);
}

// ----------------------------------------------------------------------------- in-process kernel timing (bench.py roofline leg)
__global__ __launch_bounds__(256) void fill_random_kernel(uint16_t* dst, size_t n, uint32_t seed, float scale) {
    // counter-based hash -> uniform [-scale, scale) in bf16: random operands (zero-filled ones raise the clock and flatter MFMA rates)
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t x = (uint32_t)i * 2654435761u ^ seed;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    const float u = ((float)(x >> 8) * (1.0f / 8388608.0f) - 1.0f) * scale;
    dst[i] = (uint16_t)(__float_as_uint(u) >> 16);
}
__global__ __launch_bounds__(256) void fill_random_f32_kernel(float* dst, size_t n, uint32_t seed, float scale) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t x = (uint32_t)i * 2654435761u ^ seed;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    dst[i] = ((float)(x >> 8) * (1.0f / 8388608.0f) - 1.0f) * scale;
}


// Times `iters` back-to-back launches of ONE GEMM kernel (bf16, the epilogue/shape of the DiT call site `site`) with HIP
// events on `stream`; *ms_avg = average device time of one launch.  site: 0 = fused QKV projection + RoPE (N = 3*inner),
// 1 = FF1 + GELU-tanh, 2 = FF2 + gate, 3 = attention out-projection + gate (store-only residual branches).
extern "C" int f5_bench_gemm_site(int kernel, int site, int rows, int seq, int dim, int heads, int ff_inner, int iters, float* ms_avg,
                                  f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (!ms_avg || rows <= 0 || iters <= 0 || seq <= 0 || rows % seq != 0) return f5_fail(F5_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int inner = heads * 64;
    int N, K, epi;
    switch (site) {
        case 0: N = 3 * inner; K = dim; epi = EPI_ROPE_T; break;
        case 1: N = ff_inner; K = dim; epi = EPI_STORE_T; break;
        case 2: N = dim; K = ff_inner; epi = EPI_GATE_T; break;
        case 3: N = dim; K = inner; epi = EPI_GATE_T; break;
        default: return f5_fail(F5_EINVAL, "bad site");
    }
    const size_t Mp = (size_t)round_up(rows, 256);
    const int lda = K + g_bench_pad_a, ldw = K + g_bench_pad_w;  // leading-dimension padding experiments (tuning knobs)
    DevArena a;
    void *A = nullptr, *W = nullptr, *out = nullptr;
    float *bias = nullptr, *resid = nullptr, *gate = nullptr, *rope = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&A, Mp * lda * 2))) break;
        if ((rc = a.alloc(&W, (size_t)round_up(N, 256) * ldw * 2))) break;
        if ((rc = a.alloc(&out, Mp * N * 2))) break;
        if ((rc = a.alloc_t(&bias, (size_t)N))) break;
        if ((rc = a.alloc_t(&resid, Mp * (size_t)dim))) break;
        if ((rc = a.alloc_t(&gate, (size_t)dim))) break;
        if ((rc = a.alloc_t(&rope, (size_t)seq * 64))) break;
        hipLaunchKernelGGL(fill_random_kernel, dim3((unsigned)((Mp * lda + 255) / 256)), dim3(256), 0, st, (uint16_t*)A, Mp * lda, 1u, 1.0f);
        hipLaunchKernelGGL(fill_random_kernel, dim3((unsigned)(((size_t)N * ldw + 255) / 256)), dim3(256), 0, st, (uint16_t*)W, (size_t)N * ldw, 2u, 0.05f);
        hipLaunchKernelGGL(fill_random_f32_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, bias, (size_t)N, 3u, 0.1f);
        hipLaunchKernelGGL(fill_random_f32_kernel, dim3((unsigned)((dim + 255) / 256)), dim3(256), 0, st, gate, (size_t)dim, 4u, 0.01f);
        hipLaunchKernelGGL(fill_random_f32_kernel, dim3((unsigned)((seq * 64 + 255) / 256)), dim3(256), 0, st, rope, (size_t)seq * 64, 5u, 0.7f);
        GemmParams g;
        memset(&g, 0, sizeof(g));
        g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.M = rows; g.N = N; g.K = K; g.bias = bias; g.rows_per_batch = seq;
        g.site = N == 3 * K ? 1 : (N == K ? 2 : (N == 2 * K ? 3 : (K == 2 * N ? 4 : 0)));  // (this bench entry times the ff_mult = 2 DiT call sites)
        if (epi == EPI_ROPE_T) { g.out_t = out; g.ldo = N; g.rope = rope; g.rope_inner = inner; g.rope_heads = 1; }
        if (epi == EPI_STORE_T) { g.out_t = out; g.ldo = N; g.act = ACT_GELU_TANH; }
        if (epi == EPI_GATE_T) { g.out_t = out; g.ldo = N; g.gate = gate; g.gate_bstride = 0; }
        if (kernel == 1 && !gemm_fast_supported(g, F5_PREC_BF16, GEMM_DENSE, epi)) { rc = f5_fail(F5_ENOTSUP, "tuned kernel cannot run this site"); break; }
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { rc = f5_fail(F5_EHIP, "hipEventCreate failed"); break; }
        for (int i = 0; i < 2 && rc == 0; ++i) rc = launch_gemm(g, F5_PREC_BF16, GEMM_DENSE, epi, kernel, st);
        if (rc) break;
        (void)hipEventRecord(e0, st);
        for (int i = 0; i < iters && rc == 0; ++i) rc = launch_gemm(g, F5_PREC_BF16, GEMM_DENSE, epi, kernel, st);
        (void)hipEventRecord(e1, st);
        if (rc) break;
        if (hipEventSynchronize(e1) != hipSuccess) { rc = f5_fail(F5_EHIP, "event sync failed: %s", hipGetErrorString(hipGetLastError())); break; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *ms_avg = ms / (float)iters;
    } while (0);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return sync_and_release(a, st, rc);
}

// same for the attention kernel: B x H heads of N x 64, bf16
extern "C" int f5_bench_attention(int kernel, int B, int N, int H, int iters, float* ms_avg, f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (!ms_avg || B <= 0 || N <= 0 || H <= 0 || iters <= 0) return f5_fail(F5_EINVAL, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int inner = H * 64;
    const size_t rows = (size_t)B * N;
    DevArena a;
    void *q = nullptr, *o = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc(&q, rows * 3 * inner * 2))) break;
        if ((rc = a.alloc(&o, rows * inner * 2))) break;
        hipLaunchKernelGGL(fill_random_kernel, dim3((unsigned)((rows * 3 * inner + 255) / 256)), dim3(256), 0, st, (uint16_t*)q, rows * 3 * inner, 7u, 1.5f);
        if (kernel == 1 && !attention_fast_supported(F5_PREC_BF16, N, H)) { rc = f5_fail(F5_ENOTSUP, "tuned attention cannot run this shape"); break; }
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { rc = f5_fail(F5_EHIP, "hipEventCreate failed"); break; }
        for (int i = 0; i < 2 && rc == 0; ++i) rc = launch_attention(F5_PREC_BF16, kernel, B, N, H, q, 3 * inner, nullptr, o, inner, st);
        if (rc) break;
        (void)hipEventRecord(e0, st);
        for (int i = 0; i < iters && rc == 0; ++i) rc = launch_attention(F5_PREC_BF16, kernel, B, N, H, q, 3 * inner, nullptr, o, inner, st);
        (void)hipEventRecord(e1, st);
        if (rc) break;
        if (hipEventSynchronize(e1) != hipSuccess) { rc = f5_fail(F5_EHIP, "event sync failed"); break; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *ms_avg = ms / (float)iters;
    } while (0);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return sync_and_release(a, st, rc);
}

// ----------------------------------------------------------------------------- what the matrix pipe sustains on this device
// Register-resident v_mfma_f32_16x16x32_bf16 stream: 4 waves per workgroup (one per SIMD), 64 independent accumulator tiles per
// wave, no memory traffic.  With zero operands the part holds its clock; with realistic (pseudo-random) operands the MFMA rate is
// power-limited -- that second number, not the data-sheet peak, is what a dense bf16 GEMM can approach here.
__global__ __launch_bounds__(256, 1) void mfma_rate_kernel(int iters, int random_operands, float* sink) {
    f32x4 acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 w[8], a[8];
    unsigned h = (threadIdx.x * 2654435761u) ^ (blockIdx.x * 40503u);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            h = h * 1664525u + 1013904223u;
            w[i][e] = random_operands ? (bf16_t)(((int)(h >> 20) & 0xfff) * (1.0f / 1024.0f) - 2.0f) : (bf16_t)0.f;
            h = h * 1664525u + 1013904223u;
            a[i][e] = random_operands ? (bf16_t)(((int)(h >> 20) & 0xfff) * (1.0f / 32768.0f) - 0.0625f) : (bf16_t)0.f;
        }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[i][j]) : "v"(w[i]), "v"(a[j]));
    }
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) s += acc[i][j][0];
    if (s == 12345.678f) sink[0] = s;  // keeps the accumulators alive
}

extern "C" int f5_bench_mfma_rate(int random_operands, float* tflops, f5_stream_t stream) {
    F5_TRY(f5_check_device());
    if (!tflops) return f5_fail(F5_EINVAL, "null argument");
    hipStream_t st = (hipStream_t)stream;
    int dev = 0, cus = 0;
    F5_HIP(hipGetDevice(&dev));
    F5_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const int iters = 2000, blocks = cus * 4;  // 4 workgroups per CU back to back: ~1.5 ms per launch
    DevArena a;
    float* sink = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = 0;
    do {
        if ((rc = a.alloc_t(&sink, 16))) break;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { rc = f5_fail(F5_EHIP, "hipEventCreate failed"); break; }
        for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(mfma_rate_kernel, dim3(blocks), dim3(256), 0, st, iters, random_operands, sink);  // clocks settle
        (void)hipEventRecord(e0, st);
        const int reps = 10;
        for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(mfma_rate_kernel, dim3(blocks), dim3(256), 0, st, iters, random_operands, sink);
        (void)hipEventRecord(e1, st);
        if (hipEventSynchronize(e1) != hipSuccess) { rc = f5_fail(F5_EHIP, "event sync failed"); break; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        const double flops = (double)reps * blocks * 4.0 * iters * 64.0 * (2.0 * 16 * 16 * 32);
        *tflops = (float)(flops / (ms * 1e-3) / 1e12);
    } while (0);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return sync_and_release(a, st, rc);
}

// diagnostic: while dev_buf (u64 [workgroups * 4]) is non-null the tuned GEMM writes (s_memtime, s_memrealtime) at workgroup start and end
extern "C" int f5_debug_gemm_clock(void* dev_buf) {
    g_gemm_clk_buf = reinterpret_cast<unsigned long long*>(dev_buf);
    return 0;
}

// diagnostic: what the last GEMM / conv31 launcher of this process launched (gemm.h: GemmLaunchRecord; family -1 = nothing yet)
extern "C" int f5_debug_last_gemm(int* family, int* bm, int* bn, int* schedule, int* flags) {
    if (!family || !bm || !bn || !schedule || !flags) return f5_fail(F5_EINVAL, "null argument");
    *family = g_last_gemm.family;
    *bm = g_last_gemm.bm;
    *bn = g_last_gemm.bn;
    *schedule = g_last_gemm.schedule;
    *flags = g_last_gemm.flags;
    return 0;
}
