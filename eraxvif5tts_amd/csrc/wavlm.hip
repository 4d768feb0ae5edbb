// wavlm.hip -- the WavLM feature extractor in front of the ECAPA-TDNN head (speaker.hip): what the reference's run_sim takes from s3prl as
// "wavlm_large".  Forward only, fp32 storage and accumulation, the arithmetic of transformers' WavLMModel at feat_extract_norm = "layer",
// do_stable_layer_norm = True (microsoft/wavlm-large).  Per utterance of n samples:
//   wave (optionally F.layer_norm(wave, wave.shape))
//   -> conv layers: Conv1d(no padding) -> LayerNorm(channels) -> GELU(erf)
//   -> LayerNorm -> Linear(-> hidden)                                                     "proj"
//   -> x + GELU(grouped Conv1d(k, padding k / 2, weight-norm folded by the caller))       "posconv" = hidden state 0
//   -> N x [ x += out_proj(attn(LN1 x));  x += W2 gelu(W1 LN2 x) ]                        hidden states 1 .. N
//   -> the encoder's LayerNorm on the last one (final_norm = 1, WavLMModel's form) or not (0).
// attn is multi-head attention with WavLM's gated relative position bias: S[h][i][j] = (q_i . k_j) dh^-0.5 + g[h][i] R[h][j - i], g from a
// Linear(dh -> 8) on the normalised input per head and row, R[h][d] = rel_attn_embed[bucket(d)][h] of layer 0 for every layer.  bucket(d) uses a
// float log: it is evaluated by the caller (f5_wavlm_set_buckets), never on the device.
//
// MI355X form: activations TIME-major [rows, channels] fp32, the utterances of a launch set back to back.
//   * Linear layers and conv layers 1.. are launch_gemm(F5_PREC_FP32) on v_mfma_f32_16x16x4_f32, K in chunks of 512 that are added to the output
//     (blocked summation, speaker.hip).  A conv layer needs no im2col: time-major rows make the k taps of output frame t the k * cin CONSECUTIVE
//     floats from input row t * stride, so the GEMM reads the activations themselves with lda = stride * cin.  That is one GEMM chain per utterance
//     and conv layer (a few hundred launches for 64 utterances): kept for the independence contract, its cost is not measured yet.
//   * wl_attn_kernel: one wave per (16 queries, head, utterance), flash style: S^T = K Q^T and O^T += V^T P^T on the fp32 MFMA, so the softmax
//     numerators leave the first MFMA in exactly the lane layout the second takes as its B operand (the key order inside a tile is permuted the
//     same way on both sides); online softmax in fp32, the [H, T, T] scores never exist.
//   * wl_posconv_kernel: the grouped convolution as an implicit GEMM on the same MFMA, one wave per (16 frames, 16 output channels, utterance),
//     partial sums folded every 64 terms.
//   * Row-wise kernels (LayerNorm with fp64 statistics, the gate) run once over all rows.
// Whatever looks across rows (wave normalisation, conv layer 0, the conv GEMMs, the positional conv, attention) works on one utterance's own
// extent, so an utterance's hidden states have the same bits alone or in any ragged call, at any position.
#include <climits>
#include <cmath>
#include <cstring>

#include "gemm.h"
#include "kernels.h"
#include "runtime.h"

static constexpr int WL_MAXU = 64;          // utterances per launch set (the extents travel by value)
// Output frames per launch set; a longer utterance is a set of its own.  It bounds the workspace, which grows to the largest set seen and is never
// shrunk: the two conv-stack buffers hold the rows behind conv layer 0 (64 per output frame at wavlm-large: 2 x 131072 x 512 floats = 512 MiB for a
// full set), the encoder buffers about 40 KiB per frame (80 MiB).  An utterance of T frames alone needs T / 2048 of that.
static constexpr int WL_SET_FRAMES = 2048;
static constexpr int WL_KCHUNK = 512;
static constexpr int WL_MAXCONV = 8;
static constexpr int WL_POSCONV_BLOCK = 64;  // terms per partial sum of the positional conv (one tap of a 64-channel group)

// extents of a launch set, by value: samples at wave + s0, conv layer 0's output rows c0row0 .. + c0frames, encoder rows row0 .. + frames
struct WlExt {
    int cnt = 0, max_frames = 0, max_c0frames = 0, max_samples = 0;
    int s0[WL_MAXU], samples[WL_MAXU], c0row0[WL_MAXU], c0frames[WL_MAXU], row0[WL_MAXU], frames[WL_MAXU];
};

struct WlLinear {
    float *w = nullptr, *b = nullptr;  // [n][k], [n] (b may stay null)
    int n = 0, k = 0;
};
struct WlNorm {
    float *w = nullptr, *b = nullptr;
};
struct WlLayer {
    WlNorm ln1, ln2;
    WlLinear qkv, out, ff1, ff2;
    float *gw = nullptr, *gb = nullptr, *gconst = nullptr;  // gru_rel_pos_linear [8][dh], [8]; gru_rel_pos_const [H]
};

struct f5_wavlm_s {
    f5_wavlm_config cfg;
    SlotMap slots;
    bool finalized = false;
    DevArena arena, work, relarena;
    int nconv = 0, dh = 0;
    float *c0w = nullptr, *c0b = nullptr;  // conv layer 0: [cout][k], [cout] or null
    WlLinear conv[WL_MAXCONV];             // conv layers 1..: [cout][k * cin] (column = tap * cin + c)
    WlNorm convln[WL_MAXCONV];
    WlNorm projln, encln;
    WlLinear proj;
    float *pcw = nullptr, *pcb = nullptr;  // positional conv: [C][k][C / groups], [C]
    std::vector<WlLayer> layers;
    std::vector<float> rel_embed;  // host copy of layer 0's rel_attn_embed [buckets][H]
    float* rel = nullptr;          // [H][2 rel_n - 1]
    int rel_n = 0;
    // workspace of one launch set
    size_t cap_rows = 0, cap_c0rows = 0, cap_samples = 0;
    float *wave_n = nullptr, *ca = nullptr, *cb = nullptr, *x0 = nullptr, *hbuf = nullptr, *qkv = nullptr, *attn = nullptr, *ff = nullptr, *gate = nullptr;
    std::map<std::string, float*> taps;
};

// ----------------------------------------------------------------------------- kernels
// F.layer_norm(wave, wave.shape) per utterance: fp64 sums in a fixed order (thread i takes samples i, i + 256, ...; the 256 partials are added
// 0 + 1 + ... by one thread), biased variance, eps 1e-5; then (x - mean) * rstd in fp32
__global__ __launch_bounds__(256) void wl_wave_norm_kernel(const float* __restrict__ wave, float* __restrict__ out, const WlExt ext) {
    __shared__ double sh[2][256];
    __shared__ float stat[2];
    const int u = blockIdx.x, n = ext.samples[u], tid = threadIdx.x;
    const float* x = wave + ext.s0[u];
    float* y = out + ext.s0[u];
    double s = 0.0, q = 0.0;
    for (int i = tid; i < n; i += 256) {
        const double v = (double)x[i];
        s += v;
        q += v * v;
    }
    sh[0][tid] = s;
    sh[1][tid] = q;
    __syncthreads();
    if (tid == 0) {
        double st = 0.0, qt = 0.0;
        for (int i = 0; i < 256; ++i) {
            st += sh[0][i];
            qt += sh[1][i];
        }
        const double mean = st / (double)n;
        double var = qt / (double)n - mean * mean;
        if (var < 0.0) var = 0.0;
        stat[0] = (float)mean;
        stat[1] = (float)(1.0 / sqrt(var + 1e-5));
    }
    __syncthreads();
    const float mean = stat[0], rstd = stat[1];
    for (int i = tid; i < n; i += 256) y[i] = (x[i] - mean) * rstd;
}
// conv layer 0 (one input channel): out[t][co] = b[co] + sum_tap w[co][tap] x[t * stride + tap], taps in order
__global__ __launch_bounds__(256) void wl_conv0_kernel(const float* __restrict__ wave, const float* __restrict__ w, const float* __restrict__ b, int cout, int k,
                                                       int stride, float* __restrict__ out, const WlExt ext) {
    const int u = blockIdx.y, T = ext.c0frames[u];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)T * cout) return;
    const int t = (int)(i / cout), co = (int)(i % cout);
    const float* x = wave + ext.s0[u] + (size_t)t * stride;
    const float* wp = w + (size_t)co * k;
    float acc = 0.f;
    for (int tap = 0; tap < k; ++tap) acc = __builtin_fmaf(wp[tap], x[tap], acc);
    if (b) acc += b[co];
    out[((size_t)ext.c0row0[u] + t) * cout + co] = acc;
}
// LayerNorm over the channels of a row, one wave per row: fp64 sums (lane i takes channels i, i + 64, ...; fixed butterfly), biased variance;
// out = ((x - mean) * rstd) * w + b, then GELU(erf) when gelu.  out may be x.
__global__ __launch_bounds__(256) void wl_ln_kernel(const float* x, int ldx, int rows, int dim, const float* __restrict__ w,
                                                    const float* __restrict__ b, float eps, int gelu, float* out, int ldo) {
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (size_t)rows) return;
    const float* xp = x + r * ldx;
    double s = 0.0, q = 0.0;
    for (int c = lane; c < dim; c += 64) {
        const double v = (double)xp[c];
        s += v;
        q += v * v;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        q += __shfl_xor(q, o, 64);
    }
    const double mean = s / (double)dim;
    double var = q / (double)dim - mean * mean;
    if (var < 0.0) var = 0.0;
    const float mf = (float)mean, rs = (float)(1.0 / sqrt(var + (double)eps));
    float* op = out + r * ldo;
    for (int c = lane; c < dim; c += 64) {
        float v = ((xp[c] - mf) * rs) * w[c] + b[c];
        if (gelu) v = act_gelu_erf(v);
        op[c] = v;
    }
}
__global__ __launch_bounds__(256) void wl_gelu_kernel(float* __restrict__ y, size_t n4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 v = reinterpret_cast<f32x4*>(y)[i];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = act_gelu_erf(v[r]);
    reinterpret_cast<f32x4*>(y)[i] = v;
}
// the gate of the relative position bias per (row, head): p = W hh + b (8 outputs, d in order), a = sigmoid(p0 + p1 + p2 + p3),
// b = sigmoid(p4 + .. + p7), g = a * (b * const[h] - 1) + 2
__global__ __launch_bounds__(256) void wl_gate_kernel(const float* __restrict__ h, int ldh, size_t rows, int H, int dh, const float* __restrict__ gw,
                                                      const float* __restrict__ gb, const float* __restrict__ gconst, float* __restrict__ gate) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * H) return;
    const size_t r = i / H;
    const int hd = (int)(i % H);
    const float* hp = h + r * ldh + (size_t)hd * dh;
    float p[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        float acc = 0.f;
        for (int d = 0; d < dh; ++d) acc = __builtin_fmaf(hp[d], gw[o * dh + d], acc);
        p[o] = acc + gb[o];
    }
    const float sa = ((p[0] + p[1]) + p[2]) + p[3], sb = ((p[4] + p[5]) + p[6]) + p[7];
    const float a = 1.0f / (1.0f + expf(-sa)), bb = 1.0f / (1.0f + expf(-sb));
    gate[i] = a * (bb * gconst[hd] - 1.0f) + 2.0f;
}

// Attention with the gated relative position bias.  qkv [rows, ldq] = (q | k | v) per row, each H * DH wide; gate [rows, H]; rel + h * rel_stride
// + rel_center + d = R[h][d]; out [rows, ldo].  grid (ceil(max T / 16), H, utterances), one wave each.
// MFMA 16x16x4 f32: lane l gives A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], and holds D[i = 4 (l >> 4) + r][j = l & 15], r < 4.
//   S^T = K Q^T:  i = key, j = query; the contraction index of step s is d = g * DH / 4 + s for lane group g = l >> 4 (both operands read
//                 DH / 4 consecutive floats of their row)
//   O^T += V^T P^T:  i = d, j = query; step r contracts the keys k0 + 4 g + r -- exactly the key whose numerator the lane holds in register r
template <int DH>
__global__ __launch_bounds__(64) void wl_attn_kernel(const float* __restrict__ qkv, int ldq, const float* __restrict__ gate, const float* __restrict__ rel,
                                                     int rel_stride, int rel_center, float* __restrict__ out, int ldo, int H, const WlExt ext) {
    constexpr int DQ = DH / 4, DT = DH / 16;
    const int u = blockIdx.z, T = ext.frames[u], q0 = blockIdx.x * 16;
    if (q0 >= T) return;
    const int h = blockIdx.y, lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const size_t r0 = (size_t)ext.row0[u];
    const int inner = H * DH;
    const float scale = DH == 64 ? 0.125f : 0.25f;  // dh^-0.5, exact for the head sizes built (16, 64)
    const int qi = min(q0 + c, T - 1);
    float qf[DQ];
    {
        const float* qp = qkv + (r0 + qi) * ldq + h * DH + g * DQ;
#pragma unroll
        for (int s = 0; s < DQ; s += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(qp + s);
#pragma unroll
            for (int e = 0; e < 4; ++e) qf[s + e] = v[e] * scale;
        }
    }
    const float gt = gate[(r0 + qi) * H + h];
    const float* relq = rel + (size_t)h * rel_stride + (rel_center - qi);  // relq[key] = R[h][key - qi]
    float m = -INFINITY, lsum = 0.f;
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* kbase = qkv + r0 * ldq + inner + h * DH + g * DQ;
    const float* vbase = qkv + r0 * ldq + 2 * inner + h * DH + c;
    for (int k0 = 0; k0 < T; k0 += 16) {
        const float* kp = kbase + (size_t)min(k0 + c, T - 1) * ldq;
        f32x4 s4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < DQ; s += 4) {
            const f32x4 kv = *reinterpret_cast<const f32x4*>(kp + s);
#pragma unroll
            for (int e = 0; e < 4; ++e) s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[e], qf[s + e], s4, 0, 0, 0);
        }
        float sv[4], tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = k0 + 4 * g + r;
            sv[r] = key < T ? s4[r] + gt * relq[key] : -INFINITY;
            tmax = fmaxf(tmax, sv[r]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m, tmax);  // finite: key k0 exists
        const float alpha = expf(m - mn);
        float p[4], ps = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[r] = expf(sv[r] - mn);  // exp(-inf) = 0 for a key beyond T
            ps += p[r];
        }
        lsum = lsum * alpha + ps;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = o[dt] * alpha;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* vp = vbase + (size_t)min(k0 + 4 * g + r, T - 1) * ldq;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[dt * 16], p[r], o[dt], 0, 0, 0);
        }
        m = mn;
    }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    if (q0 + c < T) {
        float* op = out + (r0 + q0 + c) * ldo + h * DH + 4 * g;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4*>(op + dt * 16) = o[dt] / lsum;
    }
}

// out[t][co] = x[t][co] + gelu(b[co] + sum_{tap, ci} w[co][tap][ci] x[t + tap - k / 2][group(co) * cg + ci]), zero outside the utterance's own
// frames (for an even k this is Conv1d(padding k / 2) with its last frame dropped).  w: [C][k][cg].  grid (ceil(max T / 16), C / 16, utterances),
// one wave each; cg a multiple of 16.  MFMA roles: i = output channel, j = frame, lane group g contracts the channels g * cg / 4 ..; the
// accumulator is folded into the total every `fold` taps (WL_POSCONV_BLOCK terms).  Short blocks are a heuristic, not an analysis: measured against fp64
// at C 1024, k 128, one block per tap roughly halved the error of blocks of 512 terms (profiles/wavlm_errors.txt holds the present figures).
__global__ __launch_bounds__(64) void wl_posconv_kernel(const float* __restrict__ x, int C, int k, int cg, int fold, const float* __restrict__ w,
                                                        const float* __restrict__ b, float* __restrict__ out, const WlExt ext) {
    const int u = blockIdx.z, T = ext.frames[u], t0 = blockIdx.x * 16;
    if (t0 >= T) return;
    const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
    const int co0 = blockIdx.y * 16, cbase = (co0 / cg) * cg, cq = cg / 4, pad = k / 2;
    const size_t r0 = (size_t)ext.row0[u];
    const float* wp = w + ((size_t)(co0 + c) * k) * cg + g * cq;
    const float* xp = x + r0 * C + cbase + g * cq;
    const int t = t0 + c;
    f32x4 tot = f32x4{0.f, 0.f, 0.f, 0.f}, acc = f32x4{0.f, 0.f, 0.f, 0.f};
    int infold = 0;
    for (int tap = 0; tap < k; ++tap) {
        const int src = t + tap - pad;
        const bool ok = t < T && src >= 0 && src < T;
        const float* xr = xp + (size_t)(ok ? src : 0) * C;
        const float* wr = wp + (size_t)tap * cg;
        for (int s = 0; s < cq; s += 4) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + s);
            f32x4 xv = *reinterpret_cast<const f32x4*>(xr + s);
            if (!ok) xv = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[e], xv[e], acc, 0, 0, 0);
        }
        if (++infold == fold) {
            tot = tot + acc;
            acc = f32x4{0.f, 0.f, 0.f, 0.f};
            infold = 0;
        }
    }
    if (infold) tot = tot + acc;
    if (t < T) {
        const int co = co0 + 4 * g;
        const f32x4 xin = *reinterpret_cast<const f32x4*>(x + (r0 + t) * C + co);
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = xin[r] + act_gelu_erf(tot[r] + b[co + r]);
        *reinterpret_cast<f32x4*>(out + (r0 + t) * C + co) = v;
    }
}

// ----------------------------------------------------------------------------- launch helpers
static unsigned wl_blocks(size_t n) { return (unsigned)((n + 255) / 256); }

// out (+)= act(A . W^T + b): K in chunks of WL_KCHUNK added to the output (blocked summation); resid: out += instead of out =.  The
// activation is fused when one chunk covers K, else it is a pass of its own behind the last chunk.
static int wl_gemm(const float* A, int lda, const WlLinear& l, int M, float* out, int ldo, bool resid, int act, hipStream_t st) {
    const bool one = l.k <= WL_KCHUNK;
    for (int k0 = 0; k0 < l.k; k0 += WL_KCHUNK) {
        GemmParams g;
        memset(&g, 0, sizeof(g));
        g.A = A + k0; g.lda = lda; g.W = l.w + k0; g.ldw = l.k; g.M = M; g.N = l.n; g.K = std::min(WL_KCHUNK, l.k - k0); g.out_f = out; g.ldof = ldo;
        g.bias = k0 == 0 ? l.b : nullptr;
        g.act = one ? act : ACT_NONE;
        g.rows_per_batch = M;
        F5_TRY(launch_gemm(g, F5_PREC_FP32, GEMM_DENSE, (k0 == 0 && !resid) ? EPI_STORE_F32 : EPI_RESID, 0, st));
    }
    if (!one && act == ACT_GELU_ERF) {
        if (resid || ldo != l.n || (l.n & 3)) return f5_fail(F5_ESTATE, "wavlm: activation pass needs a dense fresh output");
        const size_t n4 = (size_t)M * l.n / 4;
        hipLaunchKernelGGL(wl_gelu_kernel, dim3(wl_blocks(n4)), dim3(256), 0, st, out, n4);
        F5_LAUNCH_CHECK();
    }
    return 0;
}
static int wl_ln(const float* x, int ldx, size_t rows, int dim, const WlNorm& n, float eps, int gelu, float* out, int ldo, hipStream_t st) {
    if (rows == 0) return 0;
    hipLaunchKernelGGL(wl_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, ldx, (int)rows, dim, n.w, n.b, eps, gelu, out, ldo);
    F5_LAUNCH_CHECK();
    return 0;
}
// one conv layer >= 1 of one utterance: x [T_in, cin] -> LayerNorm + GELU(Conv1d) [T_out, cout]
static int wl_conv_layer(const WlLinear& cv, const WlNorm& ln, int cin, int stride, const float* x, int T_out, float eps, float* out, hipStream_t st) {
    F5_TRY(wl_gemm(x, stride * cin, cv, T_out, out, cv.n, false, ACT_NONE, st));
    return wl_ln(out, cv.n, (size_t)T_out, cv.n, ln, eps, 1, out, cv.n, st);
}
static int wl_conv0(const float* wave, const float* w, const float* b, int cout, int k, int stride, float* out, const WlExt& e, hipStream_t st) {
    hipLaunchKernelGGL(wl_conv0_kernel, dim3(wl_blocks((size_t)e.max_c0frames * cout), (unsigned)e.cnt), dim3(256), 0, st, wave, w, b, cout, k, stride, out, e);
    F5_LAUNCH_CHECK();
    return 0;
}
static bool wl_posconv_ok(int C, int k, int groups) { return C > 0 && k > 0 && groups > 0 && C % groups == 0 && (C / groups) % 16 == 0; }
static int wl_posconv(const float* x, int C, int k, int groups, const float* w, const float* b, float* out, const WlExt& e, hipStream_t st) {
    const int cg = C / groups;
    hipLaunchKernelGGL(wl_posconv_kernel, dim3((unsigned)cdiv(e.max_frames, 16), (unsigned)(C / 16), (unsigned)e.cnt), dim3(64), 0, st, x, C, k, cg,
                       std::max(1, WL_POSCONV_BLOCK / cg), w, b, out, e);
    F5_LAUNCH_CHECK();
    return 0;
}
static bool wl_attn_dh_ok(int dh) { return dh == 16 || dh == 64; }
static int wl_attention(const float* qkv, int ldq, const float* gate, const float* rel, int rel_stride, int rel_center, float* out, int ldo, int H, int dh,
                        const WlExt& e, hipStream_t st) {
    const dim3 grid((unsigned)cdiv(e.max_frames, 16), (unsigned)H, (unsigned)e.cnt);
    if (dh == 64)
        hipLaunchKernelGGL(wl_attn_kernel<64>, grid, dim3(64), 0, st, qkv, ldq, gate, rel, rel_stride, rel_center, out, ldo, H, e);
    else if (dh == 16)
        hipLaunchKernelGGL(wl_attn_kernel<16>, grid, dim3(64), 0, st, qkv, ldq, gate, rel, rel_stride, rel_center, out, ldo, H, e);
    else
        return f5_fail(F5_EINVAL, "wavlm attention: head dimension %d is not built (16, 64)", dh);
    F5_LAUNCH_CHECK();
    return 0;
}

// ----------------------------------------------------------------------------- parameter staging
// Conv1d weight [cout][cin][k] -> GEMM rows [cout][k * cin], column = tap * cin + c (the order of the time-major activations)
static int wl_upload_conv(DevArena& a, const float* w, const float* b, int cin, int cout, int k, WlLinear* dst) {
    dst->n = cout; dst->k = k * cin;
    std::vector<float> r((size_t)cout * dst->k);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int tap = 0; tap < k; ++tap) r[(size_t)co * dst->k + (size_t)tap * cin + ci] = w[((size_t)co * cin + ci) * k + tap];
    F5_TRY(f5_upload_f32(a, r.data(), r.size(), &dst->w));
    dst->b = nullptr;
    return b ? f5_upload_f32(a, b, cout, &dst->b) : 0;
}
// grouped Conv1d weight [C][cg][k] -> [C][k][cg]
static int wl_upload_posconv(DevArena& a, const float* w, int C, int cg, int k, float** dst) {
    std::vector<float> r((size_t)C * k * cg);
    for (int co = 0; co < C; ++co)
        for (int ci = 0; ci < cg; ++ci)
            for (int tap = 0; tap < k; ++tap) r[((size_t)co * k + tap) * cg + ci] = w[((size_t)co * cg + ci) * k + tap];
    return f5_upload_f32(a, r.data(), r.size(), dst);
}
static int wl_upload_linear(DevArena& a, const float* w, const float* b, int n, int k, WlLinear* dst) {
    dst->n = n; dst->k = k;
    F5_TRY(f5_upload_f32(a, w, (size_t)n * k, &dst->w));
    return f5_upload_f32(a, b, n, &dst->b);
}

static int wl_frames_of(const f5_wavlm_config& c, int64_t n) {
    for (int i = 0; i < c.num_conv_layers; ++i) {
        if (n < c.conv_kernel[i]) return -1;
        n = (n - c.conv_kernel[i]) / c.conv_stride[i] + 1;
    }
    return n > INT_MAX ? -1 : (int)n;
}

// ----------------------------------------------------------------------------- handle
static void wslot(SlotMap& s, const std::string& n, std::vector<int64_t> shape) { s[n].shape = std::move(shape); }
static void wslot_wb(SlotMap& s, const std::string& p, std::vector<int64_t> wshape, int64_t n) {
    wslot(s, p + ".weight", std::move(wshape));
    wslot(s, p + ".bias", {n});
}

static int wl_check_config(const f5_wavlm_config* c) {
    if (c->feat_extract_norm != 0) return f5_fail(F5_EINVAL, "feat_extract_norm: only \"layer\" is implemented (\"group\" is WavLM base, another network)");
    if (!c->do_stable_layer_norm) return f5_fail(F5_EINVAL, "do_stable_layer_norm: only True is implemented (the post-LayerNorm encoder is another network)");
    if (c->add_adapter) return f5_fail(F5_EINVAL, "add_adapter: adapters are not implemented");
    if (c->num_conv_layers < 1 || c->num_conv_layers > WL_MAXCONV) return f5_fail(F5_EINVAL, "num_conv_layers: 1 .. %d", WL_MAXCONV);
    for (int i = 0; i < c->num_conv_layers; ++i) {
        if (c->conv_dim[i] <= 0 || c->conv_dim[i] % 32 != 0) return f5_fail(F5_EINVAL, "conv_dim[%d] = %d: a positive multiple of 32", i, c->conv_dim[i]);
        if (c->conv_kernel[i] < 1 || c->conv_stride[i] < 1) return f5_fail(F5_EINVAL, "conv_kernel / conv_stride[%d]: at least 1", i);
    }
    if (c->hidden_size <= 0 || c->hidden_size % 32 != 0) return f5_fail(F5_EINVAL, "hidden_size = %d: a positive multiple of 32", c->hidden_size);
    if (c->num_attention_heads <= 0 || c->hidden_size % c->num_attention_heads != 0)
        return f5_fail(F5_EINVAL, "hidden_size = %d is not divisible by num_attention_heads = %d", c->hidden_size, c->num_attention_heads);
    if (!wl_attn_dh_ok(c->hidden_size / c->num_attention_heads))
        return f5_fail(F5_EINVAL, "num_attention_heads: head dimension %d is not built by the attention kernel (16, 64)", c->hidden_size / c->num_attention_heads);
    if (c->intermediate_size <= 0 || c->intermediate_size % 32 != 0) return f5_fail(F5_EINVAL, "intermediate_size = %d: a positive multiple of 32", c->intermediate_size);
    if (c->num_hidden_layers < 1) return f5_fail(F5_EINVAL, "num_hidden_layers: at least 1");
    if (!wl_posconv_ok(c->hidden_size, c->num_conv_pos_embeddings, c->num_conv_pos_embedding_groups))
        return f5_fail(F5_EINVAL, "num_conv_pos_embedding_groups = %d: hidden_size / groups must be a multiple of 16", c->num_conv_pos_embedding_groups);
    if (c->num_buckets < 4 || c->num_buckets % 2 != 0 || c->max_bucket_distance < 1) return f5_fail(F5_EINVAL, "num_buckets / max_bucket_distance out of range");
    if (!(c->layer_norm_eps > 0.f)) return f5_fail(F5_EINVAL, "layer_norm_eps must be positive");
    return 0;
}

extern "C" int f5_wavlm_create(const f5_wavlm_config* c, f5_wavlm_t* out) {
    if (!c || !out) return f5_fail(F5_EINVAL, "null argument");
    *out = nullptr;
    F5_TRY(wl_check_config(c));
    F5_TRY(f5_check_device());
    f5_wavlm_s* h = new f5_wavlm_s();
    h->cfg = *c;
    h->nconv = c->num_conv_layers;
    h->dh = c->hidden_size / c->num_attention_heads;
    SlotMap& s = h->slots;
    const int64_t F = c->hidden_size, H = c->num_attention_heads, I = c->intermediate_size;
    for (int i = 0; i < h->nconv; ++i) {
        const std::string p = "feature_extractor.conv_layers." + std::to_string(i);
        wslot(s, p + ".conv.weight", {c->conv_dim[i], i == 0 ? 1 : c->conv_dim[i - 1], c->conv_kernel[i]});
        if (c->conv_bias) wslot(s, p + ".conv.bias", {c->conv_dim[i]});
        wslot_wb(s, p + ".layer_norm", {c->conv_dim[i]}, c->conv_dim[i]);
    }
    const int64_t cl = c->conv_dim[h->nconv - 1];
    wslot_wb(s, "feature_projection.layer_norm", {cl}, cl);
    wslot_wb(s, "feature_projection.projection", {F, cl}, F);
    wslot_wb(s, "encoder.pos_conv_embed.conv", {F, F / c->num_conv_pos_embedding_groups, c->num_conv_pos_embeddings}, F);
    wslot_wb(s, "encoder.layer_norm", {F}, F);
    for (int i = 0; i < c->num_hidden_layers; ++i) {
        const std::string p = "encoder.layers." + std::to_string(i) + ".";
        for (const char* n : {"q_proj", "k_proj", "v_proj", "out_proj"}) wslot_wb(s, p + "attention." + n, {F, F}, F);
        wslot(s, p + "attention.gru_rel_pos_const", {1, H, 1, 1});
        wslot_wb(s, p + "attention.gru_rel_pos_linear", {8, h->dh}, 8);
        if (i == 0) wslot(s, p + "attention.rel_attn_embed.weight", {c->num_buckets, H});
        wslot_wb(s, p + "layer_norm", {F}, F);
        wslot_wb(s, p + "feed_forward.intermediate_dense", {I, F}, I);
        wslot_wb(s, p + "feed_forward.output_dense", {F, I}, F);
        wslot_wb(s, p + "final_layer_norm", {F}, F);
    }
    *out = h;
    return 0;
}

extern "C" int f5_wavlm_has_tensor(f5_wavlm_t h, const char* name, int64_t* numel) {
    if (!h || !name) return 0;
    auto it = h->slots.find(name);
    if (it == h->slots.end()) return 0;
    if (numel) *numel = it->second.numel();
    return 1;
}

extern "C" int f5_wavlm_set_tensor(f5_wavlm_t h, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!h || !name || !host || !shape) return f5_fail(F5_EINVAL, "null argument");
    if (h->finalized) return f5_fail(F5_ESTATE, "wavlm extractor already finalized");
    return f5_slot_set(h->slots, name, host, shape, ndim);
}

static const float* wl_host(f5_wavlm_s* h, const std::string& n) { return h->slots[n].host.data(); }
static int wl_slot_norm(f5_wavlm_s* h, const std::string& p, int n, WlNorm* dst) {
    F5_TRY(f5_upload_f32(h->arena, wl_host(h, p + ".weight"), n, &dst->w));
    return f5_upload_f32(h->arena, wl_host(h, p + ".bias"), n, &dst->b);
}

extern "C" int f5_wavlm_finalize(f5_wavlm_t h) {
    if (!h) return f5_fail(F5_EINVAL, "null wavlm extractor");
    if (h->finalized) return 0;
    F5_TRY(f5_check_device());
    F5_TRY(f5_slots_all_set(h->slots));
    const f5_wavlm_config& c = h->cfg;
    const int F = c.hidden_size, H = c.num_attention_heads, I = c.intermediate_size;
    for (int i = 0; i < h->nconv; ++i) {
        const std::string p = "feature_extractor.conv_layers." + std::to_string(i);
        const float* b = c.conv_bias ? wl_host(h, p + ".conv.bias") : nullptr;
        if (i == 0) {
            F5_TRY(f5_upload_f32(h->arena, wl_host(h, p + ".conv.weight"), (size_t)c.conv_dim[0] * c.conv_kernel[0], &h->c0w));
            if (b) F5_TRY(f5_upload_f32(h->arena, b, c.conv_dim[0], &h->c0b));
        } else {
            F5_TRY(wl_upload_conv(h->arena, wl_host(h, p + ".conv.weight"), b, c.conv_dim[i - 1], c.conv_dim[i], c.conv_kernel[i], &h->conv[i]));
        }
        F5_TRY(wl_slot_norm(h, p + ".layer_norm", c.conv_dim[i], &h->convln[i]));
    }
    const int cl = c.conv_dim[h->nconv - 1];
    F5_TRY(wl_slot_norm(h, "feature_projection.layer_norm", cl, &h->projln));
    F5_TRY(wl_upload_linear(h->arena, wl_host(h, "feature_projection.projection.weight"), wl_host(h, "feature_projection.projection.bias"), F, cl, &h->proj));
    F5_TRY(wl_upload_posconv(h->arena, wl_host(h, "encoder.pos_conv_embed.conv.weight"), F, F / c.num_conv_pos_embedding_groups, c.num_conv_pos_embeddings, &h->pcw));
    F5_TRY(f5_upload_f32(h->arena, wl_host(h, "encoder.pos_conv_embed.conv.bias"), F, &h->pcb));
    F5_TRY(wl_slot_norm(h, "encoder.layer_norm", F, &h->encln));
    h->layers.resize(c.num_hidden_layers);
    for (int i = 0; i < c.num_hidden_layers; ++i) {
        const std::string p = "encoder.layers." + std::to_string(i) + ".";
        WlLayer& L = h->layers[i];
        std::vector<float> w((size_t)3 * F * F), b((size_t)3 * F);
        const char* names[3] = {"q_proj", "k_proj", "v_proj"};
        for (int j = 0; j < 3; ++j) {
            memcpy(w.data() + (size_t)j * F * F, wl_host(h, p + "attention." + names[j] + ".weight"), (size_t)F * F * sizeof(float));
            memcpy(b.data() + (size_t)j * F, wl_host(h, p + "attention." + names[j] + ".bias"), (size_t)F * sizeof(float));
        }
        F5_TRY(wl_upload_linear(h->arena, w.data(), b.data(), 3 * F, F, &L.qkv));
        F5_TRY(wl_upload_linear(h->arena, wl_host(h, p + "attention.out_proj.weight"), wl_host(h, p + "attention.out_proj.bias"), F, F, &L.out));
        F5_TRY(f5_upload_f32(h->arena, wl_host(h, p + "attention.gru_rel_pos_linear.weight"), (size_t)8 * h->dh, &L.gw));
        F5_TRY(f5_upload_f32(h->arena, wl_host(h, p + "attention.gru_rel_pos_linear.bias"), 8, &L.gb));
        F5_TRY(f5_upload_f32(h->arena, wl_host(h, p + "attention.gru_rel_pos_const"), H, &L.gconst));
        F5_TRY(wl_slot_norm(h, p + "layer_norm", F, &L.ln1));
        F5_TRY(wl_slot_norm(h, p + "final_layer_norm", F, &L.ln2));
        F5_TRY(wl_upload_linear(h->arena, wl_host(h, p + "feed_forward.intermediate_dense.weight"), wl_host(h, p + "feed_forward.intermediate_dense.bias"), I, F, &L.ff1));
        F5_TRY(wl_upload_linear(h->arena, wl_host(h, p + "feed_forward.output_dense.weight"), wl_host(h, p + "feed_forward.output_dense.bias"), F, I, &L.ff2));
    }
    h->rel_embed = h->slots["encoder.layers.0.attention.rel_attn_embed.weight"].host;
    for (auto& kv : h->slots) std::vector<float>().swap(kv.second.host);
    h->finalized = true;
    return 0;
}

extern "C" int f5_wavlm_destroy(f5_wavlm_t h) {
    delete h;
    return 0;
}

extern "C" int f5_wavlm_frames(f5_wavlm_t h, int64_t n_samples) {
    if (!h) return f5_fail(F5_EINVAL, "null wavlm extractor");
    if (n_samples <= 0) return -1;
    return wl_frames_of(h->cfg, n_samples);
}

extern "C" int f5_wavlm_set_buckets(f5_wavlm_t h, int n, const int32_t* buckets_host) {
    if (!h || !buckets_host) return f5_fail(F5_EINVAL, "null argument");
    if (!h->finalized) return f5_fail(F5_ESTATE, "f5_wavlm_finalize must be called first");
    if (n < 1 || n > (1 << 24)) return f5_fail(F5_EINVAL, "set_buckets: n = %d out of range", n);
    const int H = h->cfg.num_attention_heads, W = 2 * n - 1;
    std::vector<float> r((size_t)H * W);
    for (int i = 0; i < W; ++i) {
        const int bk = buckets_host[i];
        if (bk < 0 || bk >= h->cfg.num_buckets) return f5_fail(F5_EINVAL, "set_buckets: bucket %d at distance %d is outside [0, num_buckets)", bk, i - (n - 1));
        for (int hd = 0; hd < H; ++hd) r[(size_t)hd * W + i] = h->rel_embed[(size_t)bk * H + hd];
    }
    F5_HIP(hipDeviceSynchronize());  // launches of an earlier call may still read the table this one replaces
    h->relarena.release();
    h->rel = nullptr;
    h->rel_n = 0;
    F5_TRY(f5_upload_f32(h->relarena, r.data(), r.size(), &h->rel));
    h->rel_n = n;
    return 0;
}

static bool wl_tap_name_ok(const f5_wavlm_s* h, const char* name) {
    if (strcmp(name, "proj") == 0 || strcmp(name, "posconv") == 0) return true;
    for (int i = 0; i < h->nconv; ++i)
        if (("conv" + std::to_string(i)) == name) return true;
    for (int i = 0; i < h->cfg.num_hidden_layers; ++i)
        if (("layer" + std::to_string(i) + ".attn") == name || ("layer" + std::to_string(i) + ".out") == name) return true;
    return false;
}
extern "C" int f5_wavlm_set_tap(f5_wavlm_t h, const char* name, float* dev) {
    if (!h || !name) return f5_fail(F5_EINVAL, "null argument");
    if (!wl_tap_name_ok(h, name)) return f5_fail(F5_EINVAL, "unknown wavlm tap '%s'", name);
    if (dev) h->taps[name] = dev; else h->taps.erase(name);
    return 0;
}
static int wl_tap(f5_wavlm_s* h, const std::string& name, const float* src, int width, size_t row0, size_t rows, hipStream_t st) {
    auto it = h->taps.find(name);
    if (it == h->taps.end() || rows == 0) return 0;
    F5_HIP(hipMemcpyAsync(it->second + row0 * width, src, rows * width * sizeof(float), hipMemcpyDeviceToDevice, st));
    return 0;
}

// the workspace of launch sets of up to (samples, rows behind conv layer 0, encoder rows); grown, never shrunk (not a per-call allocation)
static int wl_ensure_work(f5_wavlm_s* h, size_t samples, size_t c0rows, size_t rows, hipStream_t st) {
    if (samples <= h->cap_samples && c0rows <= h->cap_c0rows && rows <= h->cap_rows) return 0;
    samples = std::max(samples, h->cap_samples);
    c0rows = std::max(c0rows, h->cap_c0rows);
    rows = std::max(rows, h->cap_rows);
    const f5_wavlm_config& c = h->cfg;
    F5_HIP(hipStreamSynchronize(st));
    h->work.release();
    h->cap_samples = h->cap_c0rows = h->cap_rows = 0;
    size_t cd = 0;
    for (int i = 0; i < h->nconv; ++i) cd = std::max(cd, (size_t)c.conv_dim[i]);
    const size_t F = c.hidden_size;
    F5_TRY(h->work.alloc_t(&h->wave_n, samples, false));
    F5_TRY(h->work.alloc_t(&h->ca, c0rows * cd, false));
    F5_TRY(h->work.alloc_t(&h->cb, c0rows * cd, false));
    F5_TRY(h->work.alloc_t(&h->x0, rows * F, false));
    F5_TRY(h->work.alloc_t(&h->hbuf, rows * F, false));
    F5_TRY(h->work.alloc_t(&h->qkv, rows * 3 * F, false));
    F5_TRY(h->work.alloc_t(&h->attn, rows * F, false));
    F5_TRY(h->work.alloc_t(&h->ff, rows * (size_t)c.intermediate_size, false));
    F5_TRY(h->work.alloc_t(&h->gate, rows * (size_t)c.num_attention_heads, false));
    h->cap_samples = samples;
    h->cap_c0rows = c0rows;
    h->cap_rows = rows;
    return 0;
}

struct WlSet {
    WlExt e;
    int64_t wave0 = 0, out0 = 0;  // first sample / first output row of the set in the caller's buffers
    int64_t samples = 0, c0rows = 0, rows = 0;
    int64_t conv_out0[WL_MAXCONV];  // first row of the set in a tap of conv layer i
};

// one encoder layer over the R rows of a set, in place on x
static int wl_encoder_layer(f5_wavlm_s* h, const WlLayer& L, float* x, int R, const WlExt& e, const float* rel, int rel_stride, int rel_center, hipStream_t st,
                            const std::string* tap_attn, size_t tap_row0) {
    const f5_wavlm_config& c = h->cfg;
    const int F = c.hidden_size, H = c.num_attention_heads;
    F5_TRY(wl_ln(x, F, R, F, L.ln1, c.layer_norm_eps, 0, h->hbuf, F, st));
    F5_TRY(wl_gemm(h->hbuf, F, L.qkv, R, h->qkv, 3 * F, false, ACT_NONE, st));
    hipLaunchKernelGGL(wl_gate_kernel, dim3(wl_blocks((size_t)R * H)), dim3(256), 0, st, h->hbuf, F, (size_t)R, H, h->dh, L.gw, L.gb, L.gconst, h->gate);
    F5_LAUNCH_CHECK();
    F5_TRY(wl_attention(h->qkv, 3 * F, h->gate, rel, rel_stride, rel_center, h->attn, F, H, h->dh, e, st));
    F5_TRY(wl_gemm(h->attn, F, L.out, R, x, F, true, ACT_NONE, st));
    if (tap_attn) F5_TRY(wl_tap(h, *tap_attn, x, F, tap_row0, R, st));
    F5_TRY(wl_ln(x, F, R, F, L.ln2, c.layer_norm_eps, 0, h->hbuf, F, st));
    F5_TRY(wl_gemm(h->hbuf, F, L.ff1, R, h->ff, c.intermediate_size, false, ACT_GELU_ERF, st));
    return wl_gemm(h->ff, c.intermediate_size, L.ff2, R, x, F, true, ACT_NONE, st);
}

static int wl_run_set(f5_wavlm_s* h, const WlSet& s, const float* wave_cat, int normalize, int final_norm, float* hs_out, size_t layer_stride, hipStream_t st) {
    const f5_wavlm_config& c = h->cfg;
    const WlExt& e = s.e;
    const int F = c.hidden_size, R = (int)s.rows;
    const float eps = c.layer_norm_eps;
    const float* wave = wave_cat + s.wave0;
    if (normalize) {
        hipLaunchKernelGGL(wl_wave_norm_kernel, dim3((unsigned)e.cnt), dim3(256), 0, st, wave, h->wave_n, e);
        F5_LAUNCH_CHECK();
        wave = h->wave_n;
    }
    // conv stack: layer 0 over the set, layers 1.. one GEMM per utterance; per level the utterances sit back to back
    float *cur = h->ca, *nxt = h->cb;
    F5_TRY(wl_conv0(wave, h->c0w, h->c0b, c.conv_dim[0], c.conv_kernel[0], c.conv_stride[0], cur, e, st));
    F5_TRY(wl_ln(cur, c.conv_dim[0], (size_t)s.c0rows, c.conv_dim[0], h->convln[0], eps, 1, cur, c.conv_dim[0], st));
    F5_TRY(wl_tap(h, "conv0", cur, c.conv_dim[0], (size_t)s.conv_out0[0], (size_t)s.c0rows, st));
    std::vector<int> fr(e.c0frames, e.c0frames + e.cnt), nf(e.cnt);
    for (int i = 1; i < h->nconv; ++i) {
        size_t in0 = 0, o0 = 0;
        for (int u = 0; u < e.cnt; ++u) {
            nf[u] = (fr[u] - c.conv_kernel[i]) / c.conv_stride[i] + 1;
            F5_TRY(wl_conv_layer(h->conv[i], h->convln[i], c.conv_dim[i - 1], c.conv_stride[i], cur + in0 * c.conv_dim[i - 1], nf[u], eps, nxt + o0 * c.conv_dim[i], st));
            in0 += fr[u];
            o0 += nf[u];
        }
        F5_TRY(wl_tap(h, "conv" + std::to_string(i), nxt, c.conv_dim[i], (size_t)s.conv_out0[i], o0, st));
        fr = nf;
        std::swap(cur, nxt);
    }
    const int cl = c.conv_dim[h->nconv - 1];
    F5_TRY(wl_ln(cur, cl, R, cl, h->projln, eps, 0, nxt, cl, st));
    F5_TRY(wl_gemm(nxt, cl, h->proj, R, h->x0, F, false, ACT_NONE, st));
    F5_TRY(wl_tap(h, "proj", h->x0, F, (size_t)s.out0, R, st));
    float* x = hs_out + (size_t)s.out0 * F;
    F5_TRY(wl_posconv(h->x0, F, c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups, h->pcw, h->pcb, x, e, st));
    F5_TRY(wl_tap(h, "posconv", x, F, (size_t)s.out0, R, st));
    for (int i = 0; i < c.num_hidden_layers; ++i) {
        float* xn = x + layer_stride;
        F5_HIP(hipMemcpyAsync(xn, x, (size_t)R * F * sizeof(float), hipMemcpyDeviceToDevice, st));
        x = xn;
        const std::string ta = "layer" + std::to_string(i) + ".attn";
        F5_TRY(wl_encoder_layer(h, h->layers[i], x, R, e, h->rel, 2 * h->rel_n - 1, h->rel_n - 1, st, &ta, (size_t)s.out0));
        F5_TRY(wl_tap(h, "layer" + std::to_string(i) + ".out", x, F, (size_t)s.out0, R, st));
    }
    if (final_norm) F5_TRY(wl_ln(x, F, R, F, h->encln, eps, 0, x, F, st));
    return 0;
}

extern "C" int f5_wavlm_extract_ragged(f5_wavlm_t h, int B, const int32_t* samples_host, const float* wave_cat, int final_norm, float* hs_out,
                                       f5_stream_t stream) {
    if (!h || !samples_host || !wave_cat || !hs_out) return f5_fail(F5_EINVAL, "null argument");
    if (!h->finalized) return f5_fail(F5_ESTATE, "f5_wavlm_finalize must be called first");
    if (B <= 0) return f5_fail(F5_EINVAL, "need B >= 1");
    if (final_norm != 0 && final_norm != 1) return f5_fail(F5_EINVAL, "final_norm: 0 (last state as the layer left it) or 1 (the encoder's LayerNorm applied)");
    F5_TRY(f5_check_device());
    const f5_wavlm_config& c = h->cfg;
    hipStream_t st = (hipStream_t)stream;
    // every refusal comes before the first launch
    std::vector<WlSet> sets;
    int64_t wave0 = 0, out0 = 0, conv_out[WL_MAXCONV] = {0};
    int max_T = 0;
    for (int u = 0; u < B; ++u) {
        const int64_t n = samples_host[u];
        const int T = n > 0 ? wl_frames_of(c, n) : -1;
        if (T < 1) return f5_fail(F5_EINVAL, "utterance %d has %lld sample(s): too short for one frame", u, (long long)n);
        if (out0 + T > (int64_t)INT_MAX / 4 || wave0 + n > (int64_t)INT_MAX) return f5_fail(F5_EINVAL, "utterance %d: the call exceeds 32-bit indexing", u);
        max_T = std::max(max_T, T);
        if (sets.empty() || sets.back().e.cnt == WL_MAXU || sets.back().rows + T > WL_SET_FRAMES) {
            sets.emplace_back();
            WlSet& s = sets.back();
            s.wave0 = wave0;
            s.out0 = out0;
            for (int i = 0; i < h->nconv; ++i) s.conv_out0[i] = conv_out[i];
        }
        WlSet& s = sets.back();
        WlExt& e = s.e;
        const int j = e.cnt++;
        int64_t f = n;
        for (int i = 0; i < h->nconv; ++i) {
            f = (f - c.conv_kernel[i]) / c.conv_stride[i] + 1;
            conv_out[i] += f;
            if (i == 0) {
                e.c0row0[j] = (int)s.c0rows;
                e.c0frames[j] = (int)f;
                s.c0rows += f;
                e.max_c0frames = std::max(e.max_c0frames, (int)f);
            }
        }
        e.s0[j] = (int)s.samples;
        e.samples[j] = (int)n;
        e.row0[j] = (int)s.rows;
        e.frames[j] = T;
        e.max_frames = std::max(e.max_frames, T);
        e.max_samples = std::max(e.max_samples, (int)n);
        s.samples += n;
        s.rows += T;
        wave0 += n;
        out0 += T;
    }
    if (max_T > h->rel_n)
        return f5_fail(F5_ESTATE, "an utterance has %d frames but the relative position table covers %d: call f5_wavlm_set_buckets with n >= %d first", max_T,
                       h->rel_n, max_T);
    size_t ms = 0, mc = 0, mr = 0;
    for (const WlSet& s : sets) {
        ms = std::max(ms, (size_t)s.samples);
        mc = std::max(mc, (size_t)s.c0rows);
        mr = std::max(mr, (size_t)s.rows);
    }
    F5_TRY(wl_ensure_work(h, ms, mc, mr, st));
    for (const WlSet& s : sets) F5_TRY(wl_run_set(h, s, wave_cat, c.normalize_input, final_norm, hs_out, (size_t)out0 * c.hidden_size, st));
    return 0;
}

// ----------------------------------------------------------------------------- op-level entries (the new kernels one by one)
static WlExt wl_single(int T) {
    WlExt e;
    memset(&e, 0, sizeof(e));
    e.cnt = 1;
    e.max_frames = e.max_c0frames = T;
    e.frames[0] = e.c0frames[0] = T;
    return e;
}

extern "C" int f5_op_wavlm_attention(int T, int H, int dh, const float* qkv, const float* gate, const float* rel, float* out, f5_stream_t stream) {
    if (T < 1 || T > (1 << 20) || H < 1 || H > 65535 || !qkv || !gate || !rel || !out) return f5_fail(F5_EINVAL, "bad argument");
    if (!wl_attn_dh_ok(dh)) return f5_fail(F5_EINVAL, "wavlm attention: head dimension %d is not built (16, 64)", dh);
    F5_TRY(f5_check_device());
    return wl_attention(qkv, 3 * H * dh, gate, rel, 2 * T - 1, T - 1, out, H * dh, H, dh, wl_single(T), (hipStream_t)stream);
}

extern "C" int f5_op_wavlm_pos_conv(int T, int C, int k, int groups, const float* x, const float* w_host, const float* b_host, float* out, f5_stream_t stream) {
    if (T < 1 || T > (1 << 20) || !x || !w_host || !b_host || !out || x == out) return f5_fail(F5_EINVAL, "bad argument (out must not be x)");
    if (!wl_posconv_ok(C, k, groups)) return f5_fail(F5_EINVAL, "wavlm pos conv: C / groups must be a multiple of 16");
    F5_TRY(f5_check_device());
    hipStream_t st = (hipStream_t)stream;
    DevArena arena;
    float *w, *b;
    F5_TRY(wl_upload_posconv(arena, w_host, C, C / groups, k, &w));
    F5_TRY(f5_upload_f32(arena, b_host, C, &b));
    F5_TRY(wl_posconv(x, C, k, groups, w, b, out, wl_single(T), st));
    F5_HIP(hipStreamSynchronize(st));
    return 0;
}

extern "C" int f5_op_wavlm_conv_ln_gelu(int T_in, int cin, int cout, int k, int stride, const float* x, const float* w_host, const float* b_host_or_null,
                                        const float* ln_w_host, const float* ln_b_host, float* out, f5_stream_t stream) {
    if (T_in < 1 || cin < 1 || cout < 1 || k < 1 || stride < 1 || !x || !w_host || !ln_w_host || !ln_b_host || !out) return f5_fail(F5_EINVAL, "bad argument");
    if (T_in < k) return f5_fail(F5_EINVAL, "T_in = %d is shorter than the kernel (%d)", T_in, k);
    if (cin != 1 && (cin % 32 != 0)) return f5_fail(F5_EINVAL, "cin: 1 (the direct kernel) or a multiple of 32");
    F5_TRY(f5_check_device());
    hipStream_t st = (hipStream_t)stream;
    const int T_out = (T_in - k) / stride + 1;
    DevArena arena;
    WlNorm ln;
    F5_TRY(f5_upload_f32(arena, ln_w_host, cout, &ln.w));
    F5_TRY(f5_upload_f32(arena, ln_b_host, cout, &ln.b));
    if (cin == 1) {
        float *w, *b = nullptr;
        F5_TRY(f5_upload_f32(arena, w_host, (size_t)cout * k, &w));
        if (b_host_or_null) F5_TRY(f5_upload_f32(arena, b_host_or_null, cout, &b));
        WlExt e = wl_single(T_out);
        e.samples[0] = e.max_samples = T_in;
        F5_TRY(wl_conv0(x, w, b, cout, k, stride, out, e, st));
        F5_TRY(wl_ln(out, cout, (size_t)T_out, cout, ln, 1e-5f, 1, out, cout, st));
    } else {
        WlLinear cv;
        F5_TRY(wl_upload_conv(arena, w_host, b_host_or_null, cin, cout, k, &cv));
        F5_TRY(wl_conv_layer(cv, ln, cin, stride, x, T_out, 1e-5f, out, st));
    }
    F5_HIP(hipStreamSynchronize(st));
    return 0;
}
