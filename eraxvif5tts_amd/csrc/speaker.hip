// speaker.hip -- the ECAPA-TDNN speaker-verification head behind the reference's "SIM" figure: eval/ecapa_tdnn.py (ECAPA_TDNN.get_feat / forward,
// :283-309, global_context_att = False as ECAPA_TDNN_SMALL builds it) as utils_eval.run_sim calls it.  Forward only, eval mode, fp32 storage.  The
// feature extractor in front of it (WavLM-large from s3prl) is wavlm.hip: this head takes its hidden states, packed as f5_wavlm_extract_ragged writes them.
//   x[t][f] = sum_l softmax(feature_weight)[l] hs[l][t][f] + 1e-6;  InstanceNorm1d(F) per utterance over time (biased variance, eps 1e-5, no affine)
//   layer1  Conv1dReluBn(F -> C, k 5, pad 2)                        (conv -> ReLU -> BatchNorm: the BN cannot be folded into its own conv)
//   layer2..4  SE_Res2Block(C, k 3, dilation = padding = 2, 3, 4, scale 8):  Conv1dReluBn(1 x 1) -> Res2Conv1dReluBn -> Conv1dReluBn(1 x 1) -> SE_Connect, + x
//   cat(out2 | out3 | out4) -> Conv1d(3C -> 1536, 1 x 1) -> ReLU -> AttentiveStatsPool -> BatchNorm1d(3072) -> Linear(3072 -> emb)
//
// MI355X form: activations are TIME-major [rows, channels] fp32.  Every convolution is a GEMM on the fp32-input MFMA tile kernel (exact fp32
// products, one k order per output element): the 1 x 1 ones directly on the activations, layer1 and the seven dependent dilated convolutions of a
// Res2 chain through an im2col that reads the taps (and adds the chain's next split on the way).  ReLU + BatchNorm is one in-place pass behind the
// GEMM (scale / shift per channel, precomputed in fp64 at finalize).  A contraction longer than 512 goes in chunks of 512 that are added to the
// output (sp_gemm: blocked summation, so layer1's K = 5 x 1024 keeps the error of the other layers).  The head is launch- and bandwidth-bound, not
// MFMA-bound (about 8 GFLOP per 10 s utterance): what counts is that ALL utterances of a call share one set of launches.
//
// RAGGED: the utterances of a launch set sit back to back, no gap rows.  GEMMs and element-wise passes are row-local and run once over all rows
// with the K of a batch-1 call, so a row's arithmetic does not depend on what shares the launch.  The kernels that look across rows (im2col, the
// per-channel statistics, the SE scale, the pool) take the extents table BY VALUE (UttExtents, kernels.h: at most 64 utterances), blockIdx.y is the
// utterance, and they stop at its own first and last row: a convolution tap outside reads zero, never the neighbour.
//
// STATISTICS: per-channel sums over time (instance norm, SE mean, the pool's softmax denominator, its two weighted sums and E[x^2] - mean^2) are
// fp64, taken in a fixed order: four time-interleaved partial sums per channel, added 0 + 1 + 2 + 3.  No atomics anywhere.
#include <climits>
#include <cmath>
#include <cstring>

#include "gemm.h"
#include "kernels.h"
#include "runtime.h"

static constexpr int SP_GROUP_FRAMES = 32768;  // frames per launch set (bounds the workspace; an utterance longer than that is a set of its own)

struct SpConv {
    float *w = nullptr, *b = nullptr;          // [cout][kp] (column = tap * cin + c), [cout]
    float *scale = nullptr, *shift = nullptr;  // BatchNorm behind the ReLU: y = relu(v) * scale + shift
    int cin = 0, cout = 0, k = 1, dil = 1, kp = 0;
};
struct SpLinear {
    float *w = nullptr, *b = nullptr;  // [n][k], [n]
    int n = 0, k = 0;
};
struct SpBlock {
    SpConv c1, c2;
    std::vector<SpConv> res;  // scale - 1 dependent convolutions
    SpLinear se1, se2;
};
enum SpPost { SP_NONE = 0, SP_RELU_BN = 1, SP_RELU = 2, SP_TANH = 3 };

struct f5_speaker_s {
    f5_speaker_config cfg;
    SlotMap slots;
    bool finalized = false;
    DevArena arena, work;
    size_t work_rows = 0;
    float* mixw = nullptr;  // softmax(feature_weight) [layers]
    SpConv layer1, wide, att1, att2;
    SpBlock blocks[3];
    float *bn_scale = nullptr, *bn_shift = nullptr;  // the final BatchNorm1d(2 cat_channels)
    SpLinear linear;
    // workspace of one launch set
    float *x0 = nullptr, *col = nullptr, *out1 = nullptr, *t1 = nullptr, *t2 = nullptr, *t3 = nullptr, *cat = nullptr, *widebuf = nullptr, *attbuf = nullptr,
          *logits = nullptr, *stats = nullptr, *seh = nullptr, *ses = nullptr, *pooled = nullptr;
    std::map<std::string, float*> taps;
};

// ----------------------------------------------------------------------------- kernels
// x[r][f] = sum_l w[l] hs[l][r][f] + 1e-6 (products, then the sum over l in order: row-local)
__global__ __launch_bounds__(256) void sp_mix_kernel(const float* __restrict__ hs, size_t layer_stride, int L, const float* __restrict__ w,
                                                     float* __restrict__ x, size_t n4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const f32x4* src = reinterpret_cast<const f32x4*>(hs) + i;
    const size_t ls4 = layer_stride / 4;
    f32x4 acc = src[0] * w[0];
    for (int l = 1; l < L; ++l) acc = acc + src[(size_t)l * ls4] * w[l];
    reinterpret_cast<f32x4*>(x)[i] = acc + 1e-6f;
}
// per (utterance, channel) over the utterance's own rows, fp64 sums in a fixed order: stat[u][c] = (mean, 1 / sqrt(biased variance + eps)), or, mean_only,
// stat[u][c] = mean
__global__ __launch_bounds__(256) void sp_colstats_kernel(const float* __restrict__ x, int ldx, int C, double eps, int mean_only, float* __restrict__ stat,
                                                          const UttExtents ext) {
    __shared__ double sh[2][4][64];
    const int u = blockIdx.y, T = ext.frames[u];
    const int cl = threadIdx.x & 63, tg = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    const float* xp = x + (size_t)ext.row0[u] * ldx + c;
    double s = 0.0, q = 0.0;
    if (c < C)
        for (int t = tg; t < T; t += 4) {
            const double v = (double)xp[(size_t)t * ldx];
            s += v;
            q += v * v;
        }
    sh[0][tg][cl] = s;
    sh[1][tg][cl] = q;
    __syncthreads();
    if (tg == 0 && c < C) {
        const double st = ((sh[0][0][cl] + sh[0][1][cl]) + sh[0][2][cl]) + sh[0][3][cl];
        const double qt = ((sh[1][0][cl] + sh[1][1][cl]) + sh[1][2][cl]) + sh[1][3][cl];
        const double mean = st / (double)T;
        double var = qt / (double)T - mean * mean;
        if (var < 0.0) var = 0.0;
        if (mean_only) {
            stat[(size_t)u * C + c] = (float)mean;
        } else {
            stat[((size_t)u * C + c) * 2] = (float)mean;
            stat[((size_t)u * C + c) * 2 + 1] = (float)(1.0 / sqrt(var + eps));
        }
    }
}
// x = (x - mean) * rstd in place, per utterance
__global__ __launch_bounds__(256) void sp_normalize_kernel(float* __restrict__ x, int C, const float* __restrict__ stat, const UttExtents ext) {
    const int u = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)ext.frames[u] * C) return;
    const int c = (int)(i % C);
    float* p = x + (size_t)ext.row0[u] * C + i;
    *p = (*p - stat[((size_t)u * C + c) * 2]) * stat[((size_t)u * C + c) * 2 + 1];
}
// col[t][tap * C + c] = x[s][c] (+ add[s][c]) with s = t + (tap - (k - 1) / 2) * dil inside the utterance's own rows, else 0; columns k * C .. Kp - 1 zero
__global__ __launch_bounds__(256) void sp_im2col_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ add, int ldadd, int C, int k, int dil,
                                                        int Kp, float* __restrict__ col, const UttExtents ext) {
    const int u = blockIdx.y, T = ext.frames[u];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)T * Kp) return;
    const size_t r0 = (size_t)ext.row0[u];
    const int q = (int)(i % Kp), t = (int)(i / Kp);
    float v = 0.f;
    if (q < k * C) {
        const int tap = q / C, c = q - tap * C;
        const int s = t + (tap - (k - 1) / 2) * dil;
        if (s >= 0 && s < T) {
            v = x[(r0 + s) * ldx + c];
            if (add) v = v + add[(r0 + s) * ldadd + c];
        }
    }
    col[r0 * Kp + i] = v;
}
// in place behind a GEMM: y[r][n] = relu(y) * scale[n] + shift[n] (SP_RELU_BN), relu(y) (SP_RELU), tanh(y) (SP_TANH); row-local
__global__ __launch_bounds__(256) void sp_post_kernel(float* __restrict__ y, int ld, int N, size_t total, int post, const float* __restrict__ scale,
                                                      const float* __restrict__ shift) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int n = (int)(i % N);
    float* p = y + (i / N) * ld + n;
    const float v = *p;
    if (post == SP_TANH)
        *p = tanhf(v);
    else if (post == SP_RELU)
        *p = fmaxf(v, 0.f);
    else
        *p = __builtin_fmaf(fmaxf(v, 0.f), scale[n], shift[n]);
}
__global__ __launch_bounds__(256) void sp_copy_cols_kernel(const float* __restrict__ src, int lds, float* __restrict__ dst, int ldd, int N, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int n = (int)(i % N);
    dst[(i / N) * ldd + n] = src[(i / N) * lds + n];
}
// one wave per output: out[u][n] = act(b[n] + sum_k (in[u][k] * isc[k] + ish[k]) W[n][k]); lane partial sums over k = lane, lane + 64, ..., then a
// fixed butterfly.  act 0 none, 1 relu, 2 sigmoid.  grid (N, utterances)
__global__ __launch_bounds__(64) void sp_linear_kernel(const float* __restrict__ in, int ldi, const float* __restrict__ isc, const float* __restrict__ ish,
                                                       const float* __restrict__ W, const float* __restrict__ b, int K, int act, float* __restrict__ out, int ldo) {
    const int n = blockIdx.x, u = blockIdx.y, lane = threadIdx.x;
    const float* ip = in + (size_t)u * ldi;
    const float* wp = W + (size_t)n * K;
    float acc = 0.f;
    for (int k = lane; k < K; k += 64) {
        float v = ip[k];
        if (isc) v = __builtin_fmaf(v, isc[k], ish[k]);
        acc = __builtin_fmaf(v, wp[k], acc);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) {
        float v = acc + b[n];
        if (act == 1) v = fmaxf(v, 0.f);
        if (act == 2) v = 1.0f / (1.0f + expf(-v));
        out[(size_t)u * ldo + n] = v;
    }
}
// SE_Connect's scale and the block's residual: out[r][c] = x[r][c] * s[u][c] (+ resid[r][c])
__global__ __launch_bounds__(256) void sp_se_apply_kernel(const float* __restrict__ x, int C, const float* __restrict__ s, const float* __restrict__ resid, int ldr,
                                                          float* __restrict__ out, int ldo, const UttExtents ext) {
    const int u = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)ext.frames[u] * C) return;
    const int c = (int)(i % C);
    const size_t r = (size_t)ext.row0[u] + i / C;
    float v = x[r * C + c] * s[(size_t)u * C + c];
    if (resid) v = v + resid[r * ldr + c];
    out[r * ldo + c] = v;
}
// AttentiveStatsPool behind its two 1 x 1 convolutions: per (utterance, channel) the softmax of the logits over the utterance's own time axis, the
// weighted mean and sqrt(clamp(sum alpha x^2 - mean^2, 1e-9)).  The denominator, both weighted sums and the subtraction are fp64 (E[x^2] - mean^2
// cancels badly in fp32 for a channel that barely moves); out[u] = (mean[C] | std[C])
__global__ __launch_bounds__(256) void sp_pool_kernel(const float* __restrict__ logit, const float* __restrict__ x, int C, float* __restrict__ out, int out0,
                                                      const UttExtents ext) {
    __shared__ double sh[3][4][64];
    __shared__ float shm[4][64];
    const int u = blockIdx.y, T = ext.frames[u];
    const int cl = threadIdx.x & 63, tg = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    const bool ok = c < C;
    const size_t base = (size_t)ext.row0[u] * C + (ok ? c : 0);
    float mx = -INFINITY;
    if (ok)
        for (int t = tg; t < T; t += 4) mx = fmaxf(mx, logit[base + (size_t)t * C]);
    shm[tg][cl] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(shm[0][cl], shm[1][cl]), fmaxf(shm[2][cl], shm[3][cl]));
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (ok)
        for (int t = tg; t < T; t += 4) {
            const double e = exp((double)logit[base + (size_t)t * C] - (double)mx);
            const double v = (double)x[base + (size_t)t * C];
            s0 += e;
            s1 += e * v;
            s2 += e * (v * v);
        }
    sh[0][tg][cl] = s0;
    sh[1][tg][cl] = s1;
    sh[2][tg][cl] = s2;
    __syncthreads();
    if (tg == 0 && ok) {
        const double d = ((sh[0][0][cl] + sh[0][1][cl]) + sh[0][2][cl]) + sh[0][3][cl];
        const double a = ((sh[1][0][cl] + sh[1][1][cl]) + sh[1][2][cl]) + sh[1][3][cl];
        const double b = ((sh[2][0][cl] + sh[2][1][cl]) + sh[2][2][cl]) + sh[2][3][cl];
        const double mean = a / d;
        double res = b / d - mean * mean;
        const double lo = (double)1e-9f;  // torch clamps the fp32 tensor at float(1e-9)
        if (res < lo) res = lo;  // (a NaN stays a NaN, as under torch.clamp)
        float* o = out + (size_t)(out0 + u) * 2 * C;
        o[c] = (float)mean;
        o[C + c] = (float)sqrt(res);
    }
}

// ----------------------------------------------------------------------------- launch helpers
static unsigned sp_blocks(size_t n) { return (unsigned)((n + 255) / 256); }

// out = A . W^T + b.  The tile kernel adds an output's K products in one fp32 chain, whose rounding error grows with sqrt(K): at K = 5 x 1024
// (layer1 at the production width) that is five times the error of a blocked fp32 sum.  So a long K goes in chunks of SP_KCHUNK, each chunk's
// chain started from zero and added to the running output (EPI_RESID: out += acc) -- blocked summation, the same order for every row.
static constexpr int SP_KCHUNK = 512;
static int sp_gemm(const float* A, int lda, const SpConv& cv, int M, float* out, int ldo, hipStream_t st) {
    for (int k0 = 0; k0 < cv.kp; k0 += SP_KCHUNK) {
        GemmParams g;
        memset(&g, 0, sizeof(g));
        g.A = A + k0; g.lda = lda; g.W = cv.w + k0; g.ldw = cv.kp; g.M = M; g.N = cv.cout; g.K = std::min(SP_KCHUNK, cv.kp - k0); g.out_f = out; g.ldof = ldo;
        g.bias = k0 == 0 ? cv.b : nullptr;
        g.rows_per_batch = M;
        F5_TRY(launch_gemm(g, F5_PREC_FP32, GEMM_DENSE, k0 == 0 ? EPI_STORE_F32 : EPI_RESID, 0, st));
    }
    return 0;
}
static int sp_post(float* y, int ld, int N, int R, int post, const float* scale, const float* shift, hipStream_t st) {
    if (post == SP_NONE) return 0;
    const size_t total = (size_t)R * N;
    hipLaunchKernelGGL(sp_post_kernel, dim3(sp_blocks(total)), dim3(256), 0, st, y, ld, N, total, post, scale, shift);
    F5_LAUNCH_CHECK();
    return 0;
}
// post(Conv1d(x (+ add))) over the R rows of the table's utterances: x [R, ldx], out [R, ldo]; col: [R, kp] scratch (unused by a 1 x 1 convolution)
static int sp_conv(const SpConv& cv, const float* x, int ldx, const float* add, int ldadd, float* col, float* out, int ldo, int R, const UttExtents& e, int post,
                   hipStream_t st) {
    if (cv.k == 1 && !add && cv.kp == cv.cin && (ldx & 7) == 0) {
        F5_TRY(sp_gemm(x, ldx, cv, R, out, ldo, st));
    } else {
        hipLaunchKernelGGL(sp_im2col_kernel, dim3(sp_blocks((size_t)e.max_frames * cv.kp), (unsigned)e.cnt), dim3(256), 0, st, x, ldx, add, ldadd, cv.cin, cv.k,
                           cv.dil, cv.kp, col, e);
        F5_LAUNCH_CHECK();
        F5_TRY(sp_gemm(col, cv.kp, cv, R, out, ldo, st));
    }
    return sp_post(out, ldo, cv.cout, R, post, cv.scale, cv.shift, st);
}
static int sp_colstats(const float* x, int ldx, int C, double eps, int mean_only, float* stat, const UttExtents& e, hipStream_t st) {
    hipLaunchKernelGGL(sp_colstats_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)e.cnt), dim3(256), 0, st, x, ldx, C, eps, mean_only, stat, e);
    F5_LAUNCH_CHECK();
    return 0;
}
static int sp_linear(const SpLinear& l, const float* in, int ldi, const float* isc, const float* ish, int act, float* out, int ldo, int cnt, hipStream_t st) {
    hipLaunchKernelGGL(sp_linear_kernel, dim3((unsigned)l.n, (unsigned)cnt), dim3(64), 0, st, in, ldi, isc, ish, l.w, l.b, l.k, act, out, ldo);
    F5_LAUNCH_CHECK();
    return 0;
}
static int sp_featnorm(const float* hs, size_t layer_stride, int L, int F, const float* mixw, float* x, float* stat, int R, const UttExtents& e, hipStream_t st) {
    const size_t n4 = (size_t)R * F / 4;
    hipLaunchKernelGGL(sp_mix_kernel, dim3(sp_blocks(n4)), dim3(256), 0, st, hs, layer_stride, L, mixw, x, n4);
    F5_LAUNCH_CHECK();
    F5_TRY(sp_colstats(x, F, F, 1e-5, 0, stat, e, st));
    hipLaunchKernelGGL(sp_normalize_kernel, dim3(sp_blocks((size_t)e.max_frames * F), (unsigned)e.cnt), dim3(256), 0, st, x, F, stat, e);
    F5_LAUNCH_CHECK();
    return 0;
}
// Res2Conv1dReluBn: x [R, ldx] -> out [R, ldo]; conv i reads split i (+ the BN output of conv i - 1), the last split passes through
static int sp_res2(const std::vector<SpConv>& convs, const float* x, int ldx, float* col, float* out, int ldo, int R, const UttExtents& e, hipStream_t st) {
    const int w = convs[0].cin, nums = (int)convs.size();
    for (int i = 0; i < nums; ++i) {
        const float* in = i == 0 ? x : out + (size_t)(i - 1) * w;
        F5_TRY(sp_conv(convs[i], in, i == 0 ? ldx : ldo, i == 0 ? nullptr : x + (size_t)i * w, ldx, col, out + (size_t)i * w, ldo, R, e, SP_RELU_BN, st));
    }
    const size_t total = (size_t)R * w;
    hipLaunchKernelGGL(sp_copy_cols_kernel, dim3(sp_blocks(total)), dim3(256), 0, st, x + (size_t)nums * w, ldx, out + (size_t)nums * w, ldo, w, total);
    F5_LAUNCH_CHECK();
    return 0;
}
// SE_Connect (+ residual): x [R, C] -> out [R, ldo]; stat [cnt][C][2], hbuf [cnt][bott], sbuf [cnt][C] scratch
static int sp_se(const SpLinear& l1, const SpLinear& l2, const float* x, int C, const float* resid, int ldr, float* stat, float* hbuf, float* sbuf, float* out,
                 int ldo, const UttExtents& e, hipStream_t st) {
    F5_TRY(sp_colstats(x, C, C, 0.0, 1, stat, e, st));
    F5_TRY(sp_linear(l1, stat, C, nullptr, nullptr, 1, hbuf, l1.n, e.cnt, st));
    F5_TRY(sp_linear(l2, hbuf, l1.n, nullptr, nullptr, 2, sbuf, C, e.cnt, st));
    hipLaunchKernelGGL(sp_se_apply_kernel, dim3(sp_blocks((size_t)e.max_frames * C), (unsigned)e.cnt), dim3(256), 0, st, x, C, sbuf, resid, ldr, out, ldo, e);
    F5_LAUNCH_CHECK();
    return 0;
}
static int sp_pool(const SpConv& a1, const SpConv& a2, const float* x, int C, float* attbuf, float* logits, float* out, int out0, int R, const UttExtents& e,
                   hipStream_t st) {
    F5_TRY(sp_conv(a1, x, C, nullptr, 0, nullptr, attbuf, a1.cout, R, e, SP_TANH, st));
    F5_TRY(sp_conv(a2, attbuf, a1.cout, nullptr, 0, nullptr, logits, C, R, e, SP_NONE, st));
    hipLaunchKernelGGL(sp_pool_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)e.cnt), dim3(256), 0, st, logits, x, C, out, out0, e);
    F5_LAUNCH_CHECK();
    return 0;
}

// ----------------------------------------------------------------------------- parameter staging
static int sp_upload_conv(DevArena& a, const float* w /*[cout][cin][k]*/, const float* b, int cin, int cout, int k, int dil, SpConv* dst) {
    dst->cin = cin; dst->cout = cout; dst->k = k; dst->dil = dil; dst->kp = (int)round_up((int64_t)k * cin, 32);
    std::vector<float> r((size_t)cout * dst->kp, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int tap = 0; tap < k; ++tap) r[(size_t)co * dst->kp + (size_t)tap * cin + ci] = w[((size_t)co * cin + ci) * k + tap];
    F5_TRY(f5_upload_f32(a, r.data(), r.size(), &dst->w));
    return f5_upload_f32(a, b, cout, &dst->b);
}
// eval-mode BatchNorm as y = x * scale + shift: scale = weight / sqrt(var + eps), shift = bias - mean * scale (fp64, rounded once)
static int sp_upload_bn(DevArena& a, const float* wt, const float* bs, const float* mean, const float* var, float eps, int n, float** scale, float** shift) {
    std::vector<float> sc(n), sh(n);
    for (int i = 0; i < n; ++i) {
        const double s = (double)wt[i] / sqrt((double)var[i] + (double)eps);
        sc[i] = (float)s;
        sh[i] = (float)((double)bs[i] - (double)mean[i] * s);
    }
    F5_TRY(f5_upload_f32(a, sc.data(), n, scale));
    return f5_upload_f32(a, sh.data(), n, shift);
}
static int sp_upload_linear(DevArena& a, const float* w, const float* b, int n, int k, SpLinear* dst) {
    dst->n = n; dst->k = k;
    F5_TRY(f5_upload_f32(a, w, (size_t)n * k, &dst->w));
    return f5_upload_f32(a, b, n, &dst->b);
}
static int sp_upload_mix(DevArena& a, const float* fw, int L, float** dst) {  // softmax in fp32, as F.softmax(feature_weight) takes it
    std::vector<float> w(L);
    float mx = fw[0], sum = 0.f;
    for (int l = 1; l < L; ++l) mx = std::max(mx, fw[l]);
    for (int l = 0; l < L; ++l) sum += (w[l] = expf(fw[l] - mx));
    for (int l = 0; l < L; ++l) w[l] /= sum;
    return f5_upload_f32(a, w.data(), L, dst);
}
// frames_host -> extents tables of launch sets (<= MAXU utterances, <= SP_GROUP_FRAMES frames each); src0 = first row in the caller's buffer, out0 = utterance index
static int sp_tables(int cnt, const int32_t* frames_host, std::vector<UttExtents>* sets, int64_t* total_rows) {
    int64_t rows = 0;
    for (int u = 0; u < cnt; ++u) {
        const int t = frames_host[u];
        if (t < 2) return f5_fail(F5_EINVAL, "utterance %d has %d frame(s): the speaker head needs at least 2 (InstanceNorm1d has no variance over one frame)", u, t);
        if (rows + t > (int64_t)INT_MAX / 2) return f5_fail(F5_EINVAL, "utterance %d: the call's rows exceed 32-bit indexing", u);
        int set_rows = 0;
        if (!sets->empty()) {
            const UttExtents& b = sets->back();
            set_rows = b.row0[b.cnt - 1] + b.frames[b.cnt - 1];
        }
        if (sets->empty() || sets->back().cnt == UttExtents::MAXU || set_rows + (int64_t)t > (int64_t)SP_GROUP_FRAMES) {
            sets->emplace_back();
            set_rows = 0;
        }
        UttExtents& e = sets->back();
        e.row0[e.cnt] = set_rows;
        e.frames[e.cnt] = t;
        e.src0[e.cnt] = (int)rows;
        e.out0[e.cnt] = u;
        if (t > e.max_frames) e.max_frames = t;
        ++e.cnt;
        rows += t;
    }
    *total_rows = rows;
    return 0;
}
static int sp_set_rows(const UttExtents& e) { return e.row0[e.cnt - 1] + e.frames[e.cnt - 1]; }

// ----------------------------------------------------------------------------- handle
static void sslot(SlotMap& s, const std::string& n, std::vector<int64_t> shape) { s[n].shape = std::move(shape); }
static void sslot_bn(SlotMap& s, const std::string& p, int64_t n) {
    for (const char* f : {"weight", "bias", "running_mean", "running_var"}) sslot(s, p + f, {n});
}

extern "C" int f5_speaker_create(const f5_speaker_config* c, f5_speaker_t* out) {
    if (!c || !out) return f5_fail(F5_EINVAL, "null argument");
    *out = nullptr;
    F5_TRY(f5_check_device());
    if (c->feat_dim <= 0 || c->feat_dim % 32 != 0 || c->channels <= 0 || c->emb_dim <= 0 || c->layers <= 0 || c->cat_channels <= 0 || c->cat_channels % 32 != 0 ||
        c->se_bottleneck <= 0 || c->attention_channels <= 0 || c->attention_channels % 32 != 0 || c->scale < 2)
        return f5_fail(F5_EINVAL, "bad speaker config (feat_dim, cat_channels and attention_channels are multiples of 32, scale >= 2)");
    if (c->channels % (8 * c->scale) != 0 || c->channels % 32 != 0) return f5_fail(F5_EINVAL, "channels must be a multiple of 32 and of 8 x scale");
    f5_speaker_s* h = new f5_speaker_s();
    h->cfg = *c;
    SlotMap& s = h->slots;
    const int64_t F = c->feat_dim, C = c->channels, w = C / c->scale, W = c->cat_channels;
    sslot(s, "feature_weight", {c->layers});
    sslot(s, "layer1.conv.weight", {C, F, 5});
    sslot(s, "layer1.conv.bias", {C});
    sslot_bn(s, "layer1.bn.", C);
    for (int b = 2; b <= 4; ++b) {
        const std::string p = "layer" + std::to_string(b) + ".";
        for (const char* cb : {"Conv1dReluBn1.", "Conv1dReluBn2."}) {
            sslot(s, p + cb + "conv.weight", {C, C, 1});
            sslot(s, p + cb + "conv.bias", {C});
            sslot_bn(s, p + cb + "bn.", C);
        }
        for (int i = 0; i < c->scale - 1; ++i) {
            sslot(s, p + "Res2Conv1dReluBn.convs." + std::to_string(i) + ".weight", {w, w, 3});
            sslot(s, p + "Res2Conv1dReluBn.convs." + std::to_string(i) + ".bias", {w});
            sslot_bn(s, p + "Res2Conv1dReluBn.bns." + std::to_string(i) + ".", w);
        }
        sslot(s, p + "SE_Connect.linear1.weight", {c->se_bottleneck, C});
        sslot(s, p + "SE_Connect.linear1.bias", {c->se_bottleneck});
        sslot(s, p + "SE_Connect.linear2.weight", {C, c->se_bottleneck});
        sslot(s, p + "SE_Connect.linear2.bias", {C});
    }
    sslot(s, "conv.weight", {W, 3 * C, 1});
    sslot(s, "conv.bias", {W});
    sslot(s, "pooling.linear1.weight", {c->attention_channels, W, 1});
    sslot(s, "pooling.linear1.bias", {c->attention_channels});
    sslot(s, "pooling.linear2.weight", {W, c->attention_channels, 1});
    sslot(s, "pooling.linear2.bias", {W});
    sslot_bn(s, "bn.", 2 * W);
    sslot(s, "linear.weight", {c->emb_dim, 2 * W});
    sslot(s, "linear.bias", {c->emb_dim});
    *out = h;
    return 0;
}

extern "C" int f5_speaker_has_tensor(f5_speaker_t h, const char* name, int64_t* numel) {
    if (!h || !name) return 0;
    auto it = h->slots.find(name);
    if (it == h->slots.end()) return 0;
    if (numel) *numel = it->second.numel();
    return 1;
}

extern "C" int f5_speaker_set_tensor(f5_speaker_t h, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!h || !name || !host || !shape) return f5_fail(F5_EINVAL, "null argument");
    if (h->finalized) return f5_fail(F5_ESTATE, "speaker head already finalized");
    if (strcmp(name, "pooling.linear1.weight") == 0 && ndim >= 2 && shape[1] == 3 * (int64_t)h->cfg.cat_channels)
        return f5_fail(F5_ENOTSUP, "pooling.linear1.weight has %lld = 3 x %d input channels: a global_context_att=True checkpoint, which this head does not "
                                   "implement (ECAPA_TDNN_SMALL / run_sim use global_context_att=False)", (long long)shape[1], h->cfg.cat_channels);
    return f5_slot_set(h->slots, name, host, shape, ndim);
}

static int sp_slot_conv(f5_speaker_s* h, const std::string& conv, const std::string& bn, int cin, int cout, int k, int dil, SpConv* dst) {
    F5_TRY(sp_upload_conv(h->arena, h->slots[conv + ".weight"].host.data(), h->slots[conv + ".bias"].host.data(), cin, cout, k, dil, dst));
    if (bn.empty()) return 0;
    return sp_upload_bn(h->arena, h->slots[bn + ".weight"].host.data(), h->slots[bn + ".bias"].host.data(), h->slots[bn + ".running_mean"].host.data(),
                        h->slots[bn + ".running_var"].host.data(), 1e-5f, cout, &dst->scale, &dst->shift);
}

extern "C" int f5_speaker_finalize(f5_speaker_t h) {
    if (!h) return f5_fail(F5_EINVAL, "null speaker head");
    if (h->finalized) return 0;
    F5_TRY(f5_check_device());
    F5_TRY(f5_slots_all_set(h->slots));
    const f5_speaker_config& c = h->cfg;
    const int F = c.feat_dim, C = c.channels, w = C / c.scale, W = c.cat_channels;
    F5_TRY(sp_upload_mix(h->arena, h->slots["feature_weight"].host.data(), c.layers, &h->mixw));
    F5_TRY(sp_slot_conv(h, "layer1.conv", "layer1.bn", F, C, 5, 1, &h->layer1));
    for (int b = 0; b < 3; ++b) {
        const std::string p = "layer" + std::to_string(b + 2) + ".";
        SpBlock& blk = h->blocks[b];
        F5_TRY(sp_slot_conv(h, p + "Conv1dReluBn1.conv", p + "Conv1dReluBn1.bn", C, C, 1, 1, &blk.c1));
        F5_TRY(sp_slot_conv(h, p + "Conv1dReluBn2.conv", p + "Conv1dReluBn2.bn", C, C, 1, 1, &blk.c2));
        blk.res.resize(c.scale - 1);
        for (int i = 0; i < c.scale - 1; ++i)
            F5_TRY(sp_slot_conv(h, p + "Res2Conv1dReluBn.convs." + std::to_string(i), p + "Res2Conv1dReluBn.bns." + std::to_string(i), w, w, 3, b + 2, &blk.res[i]));
        F5_TRY(sp_upload_linear(h->arena, h->slots[p + "SE_Connect.linear1.weight"].host.data(), h->slots[p + "SE_Connect.linear1.bias"].host.data(),
                                c.se_bottleneck, C, &blk.se1));
        F5_TRY(sp_upload_linear(h->arena, h->slots[p + "SE_Connect.linear2.weight"].host.data(), h->slots[p + "SE_Connect.linear2.bias"].host.data(), C,
                                c.se_bottleneck, &blk.se2));
    }
    F5_TRY(sp_slot_conv(h, "conv", "", 3 * C, W, 1, 1, &h->wide));
    F5_TRY(sp_slot_conv(h, "pooling.linear1", "", W, c.attention_channels, 1, 1, &h->att1));
    F5_TRY(sp_slot_conv(h, "pooling.linear2", "", c.attention_channels, W, 1, 1, &h->att2));
    F5_TRY(sp_upload_bn(h->arena, h->slots["bn.weight"].host.data(), h->slots["bn.bias"].host.data(), h->slots["bn.running_mean"].host.data(),
                        h->slots["bn.running_var"].host.data(), 1e-5f, 2 * W, &h->bn_scale, &h->bn_shift));
    F5_TRY(sp_upload_linear(h->arena, h->slots["linear.weight"].host.data(), h->slots["linear.bias"].host.data(), c.emb_dim, 2 * W, &h->linear));
    for (auto& kv : h->slots) std::vector<float>().swap(kv.second.host);
    h->finalized = true;
    return 0;
}

extern "C" int f5_speaker_destroy(f5_speaker_t h) {
    delete h;
    return 0;
}

extern "C" int f5_speaker_set_tap(f5_speaker_t h, const char* name, float* dev) {
    if (!h || !name) return f5_fail(F5_EINVAL, "null argument");
    static const char* names[] = {"instance_norm", "layer1", "layer2", "layer3", "layer4", "conv", "pooling"};
    for (const char* n : names)
        if (strcmp(n, name) == 0) {
            if (dev) h->taps[name] = dev; else h->taps.erase(name);
            return 0;
        }
    return f5_fail(F5_EINVAL, "unknown speaker tap '%s'", name);
}

// the workspace for launch sets of up to `rows` rows (grown once per longest set; not a per-call allocation)
static int sp_ensure_work(f5_speaker_s* h, size_t rows, hipStream_t st) {
    if (rows <= h->work_rows) return 0;
    const f5_speaker_config& c = h->cfg;
    F5_HIP(hipStreamSynchronize(st));
    h->work.release();
    h->work_rows = 0;
    const size_t C = c.channels, F = c.feat_dim, W = c.cat_channels, U = UttExtents::MAXU;
    const size_t kp = std::max((size_t)h->layer1.kp, (size_t)h->blocks[0].res[0].kp);
    F5_TRY(h->work.alloc_t(&h->x0, rows * F, false));
    F5_TRY(h->work.alloc_t(&h->col, rows * kp, false));
    F5_TRY(h->work.alloc_t(&h->out1, rows * C, false));
    F5_TRY(h->work.alloc_t(&h->t1, rows * C, false));
    F5_TRY(h->work.alloc_t(&h->t2, rows * C, false));
    F5_TRY(h->work.alloc_t(&h->t3, rows * C, false));
    F5_TRY(h->work.alloc_t(&h->cat, rows * 3 * C, false));
    F5_TRY(h->work.alloc_t(&h->widebuf, rows * W, false));
    F5_TRY(h->work.alloc_t(&h->attbuf, rows * (size_t)c.attention_channels, false));
    F5_TRY(h->work.alloc_t(&h->logits, rows * W, false));
    F5_TRY(h->work.alloc_t(&h->stats, U * std::max(C, F) * 2, false));
    F5_TRY(h->work.alloc_t(&h->seh, U * (size_t)c.se_bottleneck, false));
    F5_TRY(h->work.alloc_t(&h->ses, U * C, false));
    F5_TRY(h->work.alloc_t(&h->pooled, U * 2 * W, false));
    h->work_rows = rows;
    return 0;
}
static int sp_tap(f5_speaker_s* h, const char* name, const float* src, int ld, int width, size_t row0, size_t rows, hipStream_t st) {
    auto it = h->taps.find(name);
    if (it == h->taps.end()) return 0;
    F5_HIP(hipMemcpy2DAsync(it->second + row0 * width, (size_t)width * 4, src, (size_t)ld * 4, (size_t)width * 4, rows, hipMemcpyDeviceToDevice, st));
    return 0;
}

// one launch set: hs points at layer 0 of the set's first row
static int sp_embed_set(f5_speaker_s* h, const UttExtents& e, const float* hs, size_t layer_stride, float* emb, hipStream_t st) {
    const f5_speaker_config& c = h->cfg;
    const int C = c.channels, F = c.feat_dim, W = c.cat_channels, R = sp_set_rows(e);
    const size_t r0 = (size_t)e.src0[0];
    F5_TRY(sp_featnorm(hs, layer_stride, c.layers, F, h->mixw, h->x0, h->stats, R, e, st));
    F5_TRY(sp_tap(h, "instance_norm", h->x0, F, F, r0, R, st));
    F5_TRY(sp_conv(h->layer1, h->x0, F, nullptr, 0, h->col, h->out1, C, R, e, SP_RELU_BN, st));
    F5_TRY(sp_tap(h, "layer1", h->out1, C, C, r0, R, st));
    for (int b = 0; b < 3; ++b) {
        const SpBlock& blk = h->blocks[b];
        const float* xin = b == 0 ? h->out1 : h->cat + (size_t)(b - 1) * C;
        const int ldin = b == 0 ? C : 3 * C;
        float* xout = h->cat + (size_t)b * C;
        F5_TRY(sp_conv(blk.c1, xin, ldin, nullptr, 0, h->col, h->t1, C, R, e, SP_RELU_BN, st));
        F5_TRY(sp_res2(blk.res, h->t1, C, h->col, h->t2, C, R, e, st));
        F5_TRY(sp_conv(blk.c2, h->t2, C, nullptr, 0, h->col, h->t3, C, R, e, SP_RELU_BN, st));
        F5_TRY(sp_se(blk.se1, blk.se2, h->t3, C, xin, ldin, h->stats, h->seh, h->ses, xout, 3 * C, e, st));
        const char* names[3] = {"layer2", "layer3", "layer4"};
        F5_TRY(sp_tap(h, names[b], xout, 3 * C, C, r0, R, st));
    }
    F5_TRY(sp_conv(h->wide, h->cat, 3 * C, nullptr, 0, h->col, h->widebuf, W, R, e, SP_RELU, st));
    F5_TRY(sp_tap(h, "conv", h->widebuf, W, W, r0, R, st));
    F5_TRY(sp_pool(h->att1, h->att2, h->widebuf, W, h->attbuf, h->logits, h->pooled, 0, R, e, st));
    F5_TRY(sp_tap(h, "pooling", h->pooled, 2 * W, 2 * W, (size_t)e.out0[0], (size_t)e.cnt, st));
    return sp_linear(h->linear, h->pooled, 2 * W, h->bn_scale, h->bn_shift, 0, emb + (size_t)e.out0[0] * c.emb_dim, c.emb_dim, e.cnt, st);
}

extern "C" int f5_speaker_embed_ragged(f5_speaker_t h, int B, const int32_t* frames_host, const float* hs, float* emb, f5_stream_t stream) {
    if (!h || !frames_host || !hs || !emb) return f5_fail(F5_EINVAL, "null argument");
    if (!h->finalized) return f5_fail(F5_ESTATE, "f5_speaker_finalize must be called first");
    if (B <= 0) return f5_fail(F5_EINVAL, "need B >= 1");
    F5_TRY(f5_check_device());
    hipStream_t st = (hipStream_t)stream;
    std::vector<UttExtents> sets;
    int64_t rows = 0;
    F5_TRY(sp_tables(B, frames_host, &sets, &rows));
    size_t max_rows = 0;
    for (const UttExtents& e : sets) max_rows = std::max(max_rows, (size_t)sp_set_rows(e));
    F5_TRY(sp_ensure_work(h, max_rows, st));
    const size_t F = h->cfg.feat_dim;
    for (const UttExtents& e : sets) F5_TRY(sp_embed_set(h, e, hs + (size_t)e.src0[0] * F, (size_t)rows * F, emb, st));
    return 0;
}

// ----------------------------------------------------------------------------- test-only ops (f5hip.h)
// Each stages its host parameters and scratch in an arena of its own, runs the head's own launch helpers set by set, and waits for the stream
// before the arena goes.
struct SpOp {
    DevArena arena;
    std::vector<UttExtents> sets;
    int64_t rows = 0;
    size_t max_rows = 0;
    hipStream_t st = nullptr;
    int begin(int cnt, const int32_t* frames_host, f5_stream_t stream) {
        if (cnt <= 0 || !frames_host) return f5_fail(F5_EINVAL, "bad argument");
        F5_TRY(f5_check_device());
        st = (hipStream_t)stream;
        F5_TRY(sp_tables(cnt, frames_host, &sets, &rows));
        for (const UttExtents& e : sets) max_rows = std::max(max_rows, (size_t)sp_set_rows(e));
        return 0;
    }
    int end() {
        F5_HIP(hipStreamSynchronize(st));
        return 0;
    }
};

extern "C" int f5_op_speaker_featnorm(int cnt, const int32_t* frames_host, int L, int F, const float* hs, const float* feature_weight_host, float* out,
                                      f5_stream_t stream) {
    if (L <= 0 || F <= 0 || F % 4 != 0 || !hs || !feature_weight_host || !out) return f5_fail(F5_EINVAL, "bad argument (F a multiple of 4)");
    SpOp op;
    F5_TRY(op.begin(cnt, frames_host, stream));
    float *mixw, *stat;
    F5_TRY(sp_upload_mix(op.arena, feature_weight_host, L, &mixw));
    F5_TRY(op.arena.alloc_t(&stat, (size_t)UttExtents::MAXU * F * 2, false));
    for (const UttExtents& e : op.sets)
        F5_TRY(sp_featnorm(hs + (size_t)e.src0[0] * F, (size_t)op.rows * F, L, F, mixw, out + (size_t)e.src0[0] * F, stat, sp_set_rows(e), e, op.st));
    return op.end();
}

extern "C" int f5_op_speaker_conv_relu_bn(int cnt, const int32_t* frames_host, int cin, int cout, int k, int dil, const float* x, const float* w_host,
                                          const float* b_host, const float* bn_host, float eps, float* out, f5_stream_t stream) {
    if (cin <= 0 || cout <= 0 || k <= 0 || k % 2 == 0 || dil <= 0 || !x || !w_host || !b_host || !bn_host || !out) return f5_fail(F5_EINVAL, "bad argument (k odd)");
    SpOp op;
    F5_TRY(op.begin(cnt, frames_host, stream));
    SpConv cv;
    F5_TRY(sp_upload_conv(op.arena, w_host, b_host, cin, cout, k, dil, &cv));
    F5_TRY(sp_upload_bn(op.arena, bn_host, bn_host + cout, bn_host + 2 * cout, bn_host + 3 * cout, eps, cout, &cv.scale, &cv.shift));
    float* col;
    F5_TRY(op.arena.alloc_t(&col, op.max_rows * cv.kp, false));
    for (const UttExtents& e : op.sets)
        F5_TRY(sp_conv(cv, x + (size_t)e.src0[0] * cin, cin, nullptr, 0, col, out + (size_t)e.src0[0] * cout, cout, sp_set_rows(e), e, SP_RELU_BN, op.st));
    return op.end();
}

extern "C" int f5_op_speaker_res2(int cnt, const int32_t* frames_host, int C, int scale, int dil, const float* x, const float* w_host, const float* b_host,
                                  const float* bn_host, float eps, float* out, f5_stream_t stream) {
    if (C <= 0 || scale < 2 || C % (4 * scale) != 0 || dil <= 0 || !x || !w_host || !b_host || !bn_host || !out)
        return f5_fail(F5_EINVAL, "bad argument (C a multiple of 4 x scale)");
    SpOp op;
    F5_TRY(op.begin(cnt, frames_host, stream));
    const int w = C / scale;
    std::vector<SpConv> convs(scale - 1);
    for (int i = 0; i < scale - 1; ++i) {
        F5_TRY(sp_upload_conv(op.arena, w_host + (size_t)i * w * w * 3, b_host + (size_t)i * w, w, w, 3, dil, &convs[i]));
        const float* bn = bn_host + (size_t)i * 4 * w;
        F5_TRY(sp_upload_bn(op.arena, bn, bn + w, bn + 2 * w, bn + 3 * w, eps, w, &convs[i].scale, &convs[i].shift));
    }
    float* col;
    F5_TRY(op.arena.alloc_t(&col, op.max_rows * convs[0].kp, false));
    for (const UttExtents& e : op.sets) F5_TRY(sp_res2(convs, x + (size_t)e.src0[0] * C, C, col, out + (size_t)e.src0[0] * C, C, sp_set_rows(e), e, op.st));
    return op.end();
}

extern "C" int f5_op_speaker_se(int cnt, const int32_t* frames_host, int C, int bott, const float* x, const float* resid, const float* w1_host,
                                const float* b1_host, const float* w2_host, const float* b2_host, float* out, f5_stream_t stream) {
    if (C <= 0 || bott <= 0 || !x || !w1_host || !b1_host || !w2_host || !b2_host || !out) return f5_fail(F5_EINVAL, "bad argument");
    SpOp op;
    F5_TRY(op.begin(cnt, frames_host, stream));
    SpLinear l1, l2;
    F5_TRY(sp_upload_linear(op.arena, w1_host, b1_host, bott, C, &l1));
    F5_TRY(sp_upload_linear(op.arena, w2_host, b2_host, C, bott, &l2));
    float *stat, *hbuf, *sbuf;
    F5_TRY(op.arena.alloc_t(&stat, (size_t)UttExtents::MAXU * C * 2, false));
    F5_TRY(op.arena.alloc_t(&hbuf, (size_t)UttExtents::MAXU * bott, false));
    F5_TRY(op.arena.alloc_t(&sbuf, (size_t)UttExtents::MAXU * C, false));
    for (const UttExtents& e : op.sets) {
        const size_t o = (size_t)e.src0[0] * C;
        F5_TRY(sp_se(l1, l2, x + o, C, resid ? resid + o : nullptr, C, stat, hbuf, sbuf, out + o, C, e, op.st));
    }
    return op.end();
}

extern "C" int f5_op_speaker_pool(int cnt, const int32_t* frames_host, int C, int att, const float* x, const float* w1_host, const float* b1_host,
                                  const float* w2_host, const float* b2_host, float* out, f5_stream_t stream) {
    if (C <= 0 || C % 32 != 0 || att <= 0 || att % 32 != 0 || !x || !w1_host || !b1_host || !w2_host || !b2_host || !out)
        return f5_fail(F5_EINVAL, "bad argument (C and att multiples of 32)");
    SpOp op;
    F5_TRY(op.begin(cnt, frames_host, stream));
    SpConv a1, a2;
    F5_TRY(sp_upload_conv(op.arena, w1_host, b1_host, C, att, 1, 1, &a1));
    F5_TRY(sp_upload_conv(op.arena, w2_host, b2_host, att, C, 1, 1, &a2));
    float *attbuf, *logits;
    F5_TRY(op.arena.alloc_t(&attbuf, op.max_rows * att, false));
    F5_TRY(op.arena.alloc_t(&logits, op.max_rows * C, false));
    for (const UttExtents& e : op.sets) F5_TRY(sp_pool(a1, a2, x + (size_t)e.src0[0] * C, C, attbuf, logits, out, e.out0[0], sp_set_rows(e), e, op.st));
    return op.end();
}
