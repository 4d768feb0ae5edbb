// bigvgan.hip -- the BigVGAN-v2 generator (mel -> waveform) behind plug point B of the reference: infer/utils_infer.py:125-138 loads it from a
// third-party checkout (`third_party.BigVGAN.bigvgan.BigVGAN.from_pretrained("nvidia/bigvgan_v2_24khz_100band_256x")`, remove_weight_norm()) and
// infer/f5tts_wrapper.py:526 / eval/eval_infer_batch.py:189 call `vocoder(mel)`.
//
// PARITY UNPINNED: that checkout is ABSENT from the reference tree, no checkpoint exists offline and no reference test covers it.  (Pinned instead:
// every kernel against the oracle's restatement at every width of the published model, tests/test_gpu_bigvgan_widths.py.)  The architecture
// is restated from the published BigVGAN-v2 source as recalled (oracle: oracle/cpu_ref.py bigvgan_forward, which the tests compare this file with):
//   conv_pre Conv1d(mels -> C0, k 7)
//   per stage i:  ConvTranspose1d(C -> C / 2, k_i, stride u_i, padding (k_i - u_i) / 2), then the MEAN of num_kernels AMPBlock1(C / 2, kernel, dilations):
//       for d in dilations:  xt = AA-snake(x); xt = Conv1d(k, dilation d)(xt); xt = AA-snake(xt); xt = Conv1d(k, dilation 1)(xt); x = xt + x
//   AA-snake (anti-aliased SnakeBeta: alias_free_activation Activation1d): 2x up-sampling by a 12-tap Kaiser-windowed sinc (replicate padding),
//       x + sin^2(alpha x) / (beta + 1e-9) per channel (alpha, beta stored as logarithms when snake_logscale), 2x low-pass down-sampling (12 taps)
//   AA-snake -> conv_post Conv1d(C -> 1, k 7, optional bias) -> clamp(-1, 1) or tanh.
//
// MI355X form: activations are TIME-major [T, C] fp32 (rows = time: every Conv1d is an im2col + GEMM on the fp32-input MFMA tile kernel, exact fp32
// products; the transposed convolution is a polyphase GEMM: k = R u, so every output sample takes R input frames, one GEMM of N = u x C_out;
// R <= 3 so that T + 1 gather rows suffice, f5_bigvgan_create refuses a longer kernel);
// the anti-aliased activation is ONE kernel (a 32-step x 32/64-channel tile staged in LDS: up-sampling, snake and down-sampling never touch HBM);
// the residual add of a block's second convolution rides in the GEMM epilogue (EPI_RESID).
//
// RAGGED (f5_bigvgan_decode_ragged): the utterances of a call sit back to back in the workspace and go through ONE set of launches.  At a stage
// with cumulative up-sampling factor U, utterance u owns rows U * off[u] .. U * (off[u] + T_u).  The GEMMs, the residual copies, the mean over the
// AMP blocks and the final clamp / tanh are row-local: they run once over all rows, with the K of a batch-1 call, so a row's arithmetic does not
// depend on how many rows share the launch.  The four kernel families that look across rows (im2col, the transposed convolution's gather and
// scatter, the anti-aliased snake) take the extents table BY VALUE (UttExtents, kernels.h: at most 64 utterances per launch) and stop at the
// utterance's own first and last row, so every utterance gets the bits of its own f5_bigvgan_forward(v, 1, T_u, ...) whatever its neighbours
// hold.  The polyphase GEMM of the transposed convolution needs T_u + 1 gather rows per utterance: there utterance u starts at row U * off[u] + u.
// f5_bigvgan_forward runs the same body without a table, one utterance at a time as before.
#include <climits>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "gemm.h"
#include "kernels.h"
#include "runtime.h"
#include "tuning.h"

struct BvConv {
    float *w = nullptr, *b = nullptr;  // [Cout][Kp] (column = tap * Cin + c), [Cout]
    int cin = 0, cout = 0, k = 0, kp = 0;
};
struct BvUp {
    float *w = nullptr, *b = nullptr;  // [(u * Cout)][Kp] (row = phase * Cout + co, column = m * Cin + ci for input frame t0 - m), [Cout]
    int cin = 0, cout = 0, k = 0, u = 0, R = 0, kp = 0, pad = 0;
};
struct BvSnake {
    float *a = nullptr, *invb = nullptr;  // alpha and 1 / (beta + 1e-9), both already exponentiated when snake_logscale
};
struct BvBlock {
    BvConv c1[3], c2[3];
    BvSnake act[6];
    int dil[3] = {1, 3, 5};
};

struct f5_bigvgan_s {
    f5_bigvgan_config cfg;
    SlotMap slots;
    bool finalized = false;
    DevArena arena, work;
    size_t work_T = 0, work_B = 0;  // the workspace holds work_T frames in work_B utterances (one more gather row per utterance)
    BvConv conv_pre, conv_post;
    std::vector<BvUp> ups;
    std::vector<BvBlock> blocks;
    BvSnake act_post;
    float up_f[12], dn_f[12];
    bool have_filters = false;
    float *x = nullptr, *y = nullptr, *xt = nullptr, *xt2 = nullptr, *xs = nullptr, *col = nullptr, *tmp = nullptr;
};

// ----------------------------------------------------------------------------- kernels
// The kernels that look across rows exist in two forms of one body.  EXT = BvNoExt: one utterance of T rows.  EXT = UttExtents (ragged): blockIdx.y
// is the utterance, which owns ext.frames[u] * up rows from row ext.row0[u] * up on (up = the stage's cumulative
// up-sampling factor, so one table serves every stage); blockIdx.x is clipped at its length.  The table is looked up with the block index only
// (uniform: scalar loads from the kernel arguments, no scratch).
struct BvNoExt {
    int unused;
};
template <typename EXT> constexpr bool bv_ragged = std::is_same<EXT, UttExtents>::value;

// col[t][tap * C + c] = x[t + (tap - (k - 1) / 2) * dil][c] (0 outside [0, T)); columns k * C .. Kp - 1 are zero.  chan_major: x is [C][T] (the mel input
// of f5_bigvgan_forward).  Ragged: T is the utterance's own row count, so a tap outside it contributes 0 and never reads a neighbour's row; with
// src_ld > 0 (conv_pre) x is the caller's frame-major mel [*, src_ld], read from row ext.src0[u].
template <typename EXT>
__global__ __launch_bounds__(256) void bv_im2col_kernel(const float* __restrict__ x, int T, int C, int k, int dil, int Kp, int chan_major,
                                                        float* __restrict__ col, size_t total, int up, int src_ld, const EXT ext) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int ldx = C;
    if constexpr (bv_ragged<EXT>) {
        const int u = blockIdx.y;
        T = ext.frames[u] * up;
        total = (size_t)T * Kp;
        const size_t r0 = (size_t)ext.row0[u] * up;
        col += r0 * Kp;
        if (src_ld > 0) {
            x += (size_t)ext.src0[u] * src_ld;
            ldx = src_ld;
        } else {
            x += r0 * C;
        }
    }
    if (i >= total) return;
    const int q = (int)(i % Kp);
    const int t = (int)(i / Kp);
    float v = 0.f;
    if (q < k * C) {
        const int tap = q / C, c = q - tap * C;
        const int s = t + (tap - (k - 1) / 2) * dil;
        if (s >= 0 && s < T) v = chan_major ? x[(size_t)c * T + s] : x[(size_t)s * ldx + c];
    }
    col[i] = v;
}
// transposed convolution, gather side: col[t0][m * C + c] = x[t0 - m][c] for t0 in [0, T], m in [0, R).  Ragged: utterance ubase + u of the launch
// set has its T + 1 gather rows from row ext.row0[u] * up + ubase + u on.
template <typename EXT>
__global__ __launch_bounds__(256) void bv_up_gather_kernel(const float* __restrict__ x, int T, int C, int R, int Kp, float* __restrict__ col, size_t total,
                                                           int up, int ubase, const EXT ext) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if constexpr (bv_ragged<EXT>) {
        const int u = blockIdx.y;
        T = ext.frames[u] * up;
        total = (size_t)(T + 1) * Kp;
        const size_t r0 = (size_t)ext.row0[u] * up;
        x += r0 * C;
        col += (r0 + ubase + u) * Kp;
    }
    if (i >= total) return;
    const int q = (int)(i % Kp);
    const int t0 = (int)(i / Kp);
    float v = 0.f;
    if (q < R * C) {
        const int m = q / C, c = q - m * C;
        const int s = t0 - m;
        if (s >= 0 && s < T) v = x[(size_t)s * C + c];
    }
    col[i] = v;
}
// transposed convolution, scatter side: y[p][co] = tmp[t0][r * Cout + co] + bias[co] with q = p + pad, t0 = q / u, r = q % u, p in [0, T u).  Ragged:
// the utterance's tmp rows start where its gather rows do, its y rows at ext.row0[u] * up * u.
template <typename EXT>
__global__ __launch_bounds__(256) void bv_up_scatter_kernel(const float* __restrict__ tmp, int T, int Cout, int u, int pad, const float* __restrict__ bias,
                                                            float* __restrict__ y, size_t total, int up, int ubase, const EXT ext) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if constexpr (bv_ragged<EXT>) {
        const int ut = blockIdx.y;
        T = ext.frames[ut] * up;
        total = (size_t)T * u * Cout;
        const size_t r0 = (size_t)ext.row0[ut] * up;
        tmp += (r0 + ubase + ut) * ((size_t)u * Cout);
        y += r0 * u * Cout;
    }
    if (i >= total) return;
    const int co = (int)(i % Cout);
    const int p = (int)(i / Cout);
    const int q = p + pad, t0 = q / u, r = q - t0 * u;
    y[i] = tmp[(size_t)t0 * (u * Cout) + r * Cout + co] + bias[co];
}
struct BvFilters {
    float up[12], dn[12];
};
// Anti-aliased SnakeBeta, one kernel.  Output step t needs the activated up-sampled signal z[n], n = 2t - 5 .. 2t + 6 (replicate-clamped to [0, 2T));
// z[n] = snake(up[n]), up[n] = 2 sum_m xpad[m] f_up[n + 15 - 2m] over the six m with 0 <= n + 15 - 2m <= 11, xpad[m] = x[clamp(m - 5, 0, T - 1)].
// Tile: TT = 32 output steps x CW channels; x rows t0 - 6 .. t0 + TT + 5 and z values 2 t0 - 5 .. 2 t0 + 2 TT + 4 live in LDS.
// Ragged: grid (time tiles of the longest utterance x channel blocks, utterances), channel blocks fastest as in the one-utterance form.  T is the
// utterance's own row count and x / out start at its first row, so both replicate paddings clamp to its own first and last row and a tile never
// straddles two utterances; a tile past its end returns before it touches LDS.
template <int CW, typename EXT>
__global__ __launch_bounds__(256) void bv_aa_snake_kernel(const float* __restrict__ x, int T, int C, const float* __restrict__ alpha, const float* __restrict__ invb,
                                                          BvFilters f, float* __restrict__ out, int up, const EXT ext) {
    constexpr int TT = 32, NX = TT + 12, NZ = 2 * TT + 10, TY = 256 / CW;
    __shared__ float xs[NX][CW], zs[NZ][CW];
    int cb = blockIdx.x, tb = blockIdx.y;
    if constexpr (bv_ragged<EXT>) {
        const int u = blockIdx.y, ncb = (C + CW - 1) / CW;
        T = ext.frames[u] * up;
        tb = blockIdx.x / ncb;
        cb = blockIdx.x - tb * ncb;
        if (tb * TT >= T) return;
        const size_t r0 = (size_t)ext.row0[u] * up;
        x += r0 * C;
        out += r0 * C;
    }
    const int cl = threadIdx.x % CW, ty = threadIdx.x / CW;
    const int c = cb * CW + cl;
    const int t0 = tb * TT;
    const bool okc = c < C;
    for (int r = ty; r < NX; r += TY) {
        int s = t0 - 6 + r;
        s = s < 0 ? 0 : (s > T - 1 ? T - 1 : s);
        xs[r][cl] = okc ? x[(size_t)s * C + c] : 0.f;
    }
    __syncthreads();
    const float a = okc ? alpha[c] : 1.f, ib = okc ? invb[c] : 0.f;
    for (int r = ty; r < NZ; r += TY) {
        int n = 2 * t0 - 5 + r;
        n = n < 0 ? 0 : (n > 2 * T - 1 ? 2 * T - 1 : n);
        // m from ceil((n + 4) / 2) to floor((n + 15) / 2); xpad[m] = x[clamp(m - 5)] = xs[clamp(m - 5) - (t0 - 6)]
        const int m_lo = (n + 5) >> 1;  // ceil((n + 4) / 2) for n >= 0
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const int m = m_lo + q;
            const int tap = n + 15 - 2 * m;
            int s = m - 5;
            s = s < 0 ? 0 : (s > T - 1 ? T - 1 : s);
            if (tap >= 0 && tap < 12) acc = __builtin_fmaf(xs[s - (t0 - 6)][cl], f.up[tap], acc);
        }
        const float u = 2.0f * acc;
        const float s1 = sinf(u * a);
        zs[r][cl] = u + ib * (s1 * s1);
    }
    __syncthreads();
    for (int r = ty; r < TT; r += TY) {
        const int t = t0 + r;
        if (t < T && okc) {
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                int n = 2 * t + j - 5;
                n = n < 0 ? 0 : (n > 2 * T - 1 ? 2 * T - 1 : n);
                acc = __builtin_fmaf(zs[n - (2 * t0 - 5)][cl], f.dn[j], acc);
            }
            out[(size_t)t * C + c] = acc;
        }
    }
}
// dst = dst * ds + src * ss
__global__ __launch_bounds__(256) void bv_axpby_kernel(float* __restrict__ dst, const float* __restrict__ src, float ds, float ss, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = dst[i] * ds + src[i] * ss;
}
__global__ __launch_bounds__(256) void bv_final_kernel(const float* __restrict__ src, int use_tanh, float* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = use_tanh ? tanhf(src[i]) : fminf(1.0f, fmaxf(-1.0f, src[i]));
}

// ----------------------------------------------------------------------------- handle
static void bslot(SlotMap& s, const std::string& n, std::vector<int64_t> shape) { s[n].shape = std::move(shape); }

// modified Bessel function I0 (torch.kaiser_window uses it): power series, converges fast for the beta of a 12-tap filter
static double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 64; ++k) {
        term *= q / ((double)k * k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}
// alias_free_activation/torch/filter.py: kaiser_sinc_filter1d(cutoff, half_width, kernel_size), even kernel sizes
static void kaiser_sinc_filter(double cutoff, double half_width, int ks, float* out) {
    const int half = ks / 2;
    const double delta_f = 4.0 * half_width, A = 2.285 * (half - 1) * M_PI * delta_f + 7.95;
    const double beta = A > 50.0 ? 0.1102 * (A - 8.7) : (A >= 21.0 ? 0.5842 * pow(A - 21.0, 0.4) + 0.07886 * (A - 21.0) : 0.0);
    std::vector<double> f(ks);
    double sum = 0.0;
    for (int i = 0; i < ks; ++i) {
        const double r = 2.0 * i / (ks - 1) - 1.0;  // torch.kaiser_window(periodic=False)
        const double win = bessel_i0(beta * sqrt(std::max(0.0, 1.0 - r * r))) / bessel_i0(beta);
        const double t = (i - half) + 0.5, a = 2.0 * cutoff * t;
        const double sinc = a == 0.0 ? 1.0 : sin(M_PI * a) / (M_PI * a);
        f[i] = 2.0 * cutoff * win * sinc;
        sum += f[i];
    }
    for (int i = 0; i < ks; ++i) out[i] = (float)(f[i] / sum);
}

extern "C" int f5_bigvgan_create(const f5_bigvgan_config* c, f5_bigvgan_t* out) {
    if (!c || !out) return f5_fail(F5_EINVAL, "null argument");
    *out = nullptr;
    F5_TRY(f5_check_device());
    if (c->num_mels <= 0 || c->upsample_initial_channel <= 0 || c->num_upsamples <= 0 || c->num_upsamples > 8 || c->num_kernels <= 0 || c->num_kernels > 4)
        return f5_fail(F5_EINVAL, "bad BigVGAN config");
    if (c->upsample_initial_channel % (1 << c->num_upsamples) != 0) return f5_fail(F5_EINVAL, "upsample_initial_channel must be divisible by 2^num_upsamples");
    for (int i = 0; i < c->num_upsamples; ++i) {
        const int u = c->upsample_rates[i], k = c->upsample_kernel_sizes[i];
        if (u <= 0 || k < u || k % u != 0 || ((k - u) & 1)) return f5_fail(F5_ENOTSUP, "upsample stage %d: kernel %d / rate %d (kernel must be a multiple of the rate, k - u even)", i, k, u);
        // the scatter reads tmp row (p + pad) / u <= T + (pad - 1) / u; the gather, the GEMM and the workspace provide rows 0 .. T only, which covers
        // pad = (k - u) / 2 <= u, that is k <= 3u (every published config has k = 2u)
        if (k > 3 * u) return f5_fail(F5_ENOTSUP, "upsample stage %d: kernel %d > 3 x rate %d (the transposed convolution keeps one gather row past the utterance's end)", i, k, u);
    }
    for (int j = 0; j < c->num_kernels; ++j)
        if (c->resblock_kernel_sizes[j] <= 0 || c->resblock_kernel_sizes[j] % 2 == 0) return f5_fail(F5_EINVAL, "resblock kernel sizes must be odd");
    f5_bigvgan_s* v = new f5_bigvgan_s();
    v->cfg = *c;
    SlotMap& s = v->slots;
    int64_t ch = c->upsample_initial_channel;
    bslot(s, "conv_pre.weight", {ch, c->num_mels, 7});
    bslot(s, "conv_pre.bias", {ch});
    for (int i = 0; i < c->num_upsamples; ++i) {
        const std::string p = "ups." + std::to_string(i) + ".0.";
        bslot(s, p + "weight", {ch, ch / 2, c->upsample_kernel_sizes[i]});
        bslot(s, p + "bias", {ch / 2});
        ch /= 2;
        for (int j = 0; j < c->num_kernels; ++j) {
            const std::string r = "resblocks." + std::to_string(i * c->num_kernels + j) + ".";
            for (int t = 0; t < 3; ++t)
                for (const char* cv : {"convs1.", "convs2."}) {
                    bslot(s, r + cv + std::to_string(t) + ".weight", {ch, ch, c->resblock_kernel_sizes[j]});
                    bslot(s, r + cv + std::to_string(t) + ".bias", {ch});
                }
            for (int a = 0; a < 6; ++a) {
                bslot(s, r + "activations." + std::to_string(a) + ".act.alpha", {ch});
                bslot(s, r + "activations." + std::to_string(a) + ".act.beta", {ch});
            }
        }
    }
    bslot(s, "activation_post.act.alpha", {ch});
    bslot(s, "activation_post.act.beta", {ch});
    bslot(s, "conv_post.weight", {1, ch, 7});
    if (c->use_bias_at_final) bslot(s, "conv_post.bias", {1});
    kaiser_sinc_filter(0.25, 0.3, 12, v->up_f);  // UpSample1d / DownSample1d(ratio 2): cutoff 0.5 / ratio, half_width 0.6 / ratio, 12 taps
    kaiser_sinc_filter(0.25, 0.3, 12, v->dn_f);
    *out = v;
    return 0;
}

extern "C" int f5_bigvgan_has_tensor(f5_bigvgan_t v, const char* name, int64_t* numel) {
    if (!v || !name) return 0;
    if (strcmp(name, "aa_up_filter") == 0 || strcmp(name, "aa_down_filter") == 0) {
        if (numel) *numel = 12;
        return 1;
    }
    auto it = v->slots.find(name);
    if (it == v->slots.end()) return 0;
    if (numel) *numel = it->second.numel();
    return 1;
}

extern "C" int f5_bigvgan_set_tensor(f5_bigvgan_t v, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!v || !name || !host || !shape) return f5_fail(F5_EINVAL, "null argument");
    if (v->finalized) return f5_fail(F5_ESTATE, "vocoder already finalized");
    if (strcmp(name, "aa_up_filter") == 0 || strcmp(name, "aa_down_filter") == 0) {  // the 12-tap filters a checkpoint carries as buffers (optional)
        int64_t n = 1;
        for (int i = 0; i < ndim; ++i) n *= shape[i];
        if (n != 12) return f5_fail(F5_EINVAL, "%s must have 12 taps", name);
        memcpy(name[3] == 'u' ? v->up_f : v->dn_f, host, 12 * sizeof(float));
        return 0;
    }
    return f5_slot_set(v->slots, name, host, shape, ndim);
}

static int bv_upload_conv(f5_bigvgan_s* v, const std::string& name, int cin, int cout, int k, bool bias, BvConv* dst) {
    const std::vector<float>& w = v->slots[name + ".weight"].host;  // [cout][cin][k]
    dst->cin = cin; dst->cout = cout; dst->k = k; dst->kp = (int)round_up((size_t)k * cin, 32);
    std::vector<float> r((size_t)cout * dst->kp, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int tap = 0; tap < k; ++tap) r[(size_t)co * dst->kp + (size_t)tap * cin + ci] = w[((size_t)co * cin + ci) * k + tap];
    F5_TRY(f5_upload_f32(v->arena, r.data(), r.size(), &dst->w));
    if (bias) return f5_upload_f32(v->arena, v->slots[name + ".bias"].host.data(), cout, &dst->b);
    std::vector<float> z(cout, 0.f);
    return f5_upload_f32(v->arena, z.data(), cout, &dst->b);
}
static int bv_upload_snake(f5_bigvgan_s* v, const std::string& name, int ch, BvSnake* dst) {
    const std::vector<float>&al = v->slots[name + ".alpha"].host, &be = v->slots[name + ".beta"].host;
    std::vector<float> a(ch), ib(ch);
    for (int c = 0; c < ch; ++c) {
        const float aa = v->cfg.snake_logscale ? expf(al[c]) : al[c], bb = v->cfg.snake_logscale ? expf(be[c]) : be[c];
        a[c] = aa;
        ib[c] = 1.0f / (bb + 1e-9f);
    }
    F5_TRY(f5_upload_f32(v->arena, a.data(), ch, &dst->a));
    return f5_upload_f32(v->arena, ib.data(), ch, &dst->invb);
}

extern "C" int f5_bigvgan_finalize(f5_bigvgan_t v) {
    if (!v) return f5_fail(F5_EINVAL, "null vocoder");
    if (v->finalized) return 0;
    F5_TRY(f5_check_device());
    F5_TRY(f5_slots_all_set(v->slots));
    const f5_bigvgan_config& c = v->cfg;
    int ch = c.upsample_initial_channel;
    F5_TRY(bv_upload_conv(v, "conv_pre", c.num_mels, ch, 7, true, &v->conv_pre));
    v->ups.resize(c.num_upsamples);
    v->blocks.resize((size_t)c.num_upsamples * c.num_kernels);
    for (int i = 0; i < c.num_upsamples; ++i) {
        BvUp& up = v->ups[i];
        const std::string p = "ups." + std::to_string(i) + ".0";
        up.cin = ch; up.cout = ch / 2; up.k = c.upsample_kernel_sizes[i]; up.u = c.upsample_rates[i]; up.R = up.k / up.u; up.pad = (up.k - up.u) / 2;
        up.kp = (int)round_up((size_t)up.R * up.cin, 32);
        const std::vector<float>& w = v->slots[p + ".weight"].host;  // [cin][cout][k]
        std::vector<float> r((size_t)up.u * up.cout * up.kp, 0.f);
        for (int ph = 0; ph < up.u; ++ph)
            for (int co = 0; co < up.cout; ++co)
                for (int m = 0; m < up.R; ++m)
                    for (int ci = 0; ci < up.cin; ++ci)
                        r[((size_t)ph * up.cout + co) * up.kp + (size_t)m * up.cin + ci] = w[((size_t)ci * up.cout + co) * up.k + ph + m * up.u];
        F5_TRY(f5_upload_f32(v->arena, r.data(), r.size(), &up.w));
        F5_TRY(f5_upload_f32(v->arena, v->slots[p + ".bias"].host.data(), up.cout, &up.b));
        ch /= 2;
        for (int j = 0; j < c.num_kernels; ++j) {
            BvBlock& b = v->blocks[(size_t)i * c.num_kernels + j];
            const std::string r2 = "resblocks." + std::to_string(i * c.num_kernels + j) + ".";
            for (int t = 0; t < 3; ++t) {
                b.dil[t] = c.resblock_dilations[j][t];
                F5_TRY(bv_upload_conv(v, r2 + "convs1." + std::to_string(t), ch, ch, c.resblock_kernel_sizes[j], true, &b.c1[t]));
                F5_TRY(bv_upload_conv(v, r2 + "convs2." + std::to_string(t), ch, ch, c.resblock_kernel_sizes[j], true, &b.c2[t]));
            }
            for (int a = 0; a < 6; ++a) F5_TRY(bv_upload_snake(v, r2 + "activations." + std::to_string(a) + ".act", ch, &b.act[a]));
        }
    }
    F5_TRY(bv_upload_snake(v, "activation_post.act", ch, &v->act_post));
    F5_TRY(bv_upload_conv(v, "conv_post", ch, 1, 7, c.use_bias_at_final != 0, &v->conv_post));
    for (auto& kv : v->slots) std::vector<float>().swap(kv.second.host);
    v->finalized = true;
    return 0;
}

extern "C" int f5_bigvgan_destroy(f5_bigvgan_t v) {
    delete v;
    return 0;
}

static unsigned bv_blocks(size_t n) { return (unsigned)((n + 255) / 256); }

// One launch set of a ragged call: the extents tables (at most UttExtents::MAXU utterances each: the row-crossing kernels launch once per table, the
// row-local ones once over all rows) of `cnt` utterances holding `frames` mel frames back to back.  row0 counts frames from the start of the set.
struct BvRagged {
    std::vector<UttExtents> tabs;
    int cnt = 0, frames = 0;
};

// x: T rows (ragged: of all utterances, `up` rows per mel frame; src_ld > 0: conv_pre from the caller's frame-major mel) -> out [T, cout]
static int bv_conv(f5_bigvgan_s* v, const BvConv& cv, const float* x, int T, int dil, int chan_major, float* out, bool residual, const BvRagged* rg, int up,
                   int src_ld, hipStream_t st) {
    const size_t total = (size_t)T * cv.kp;
    if (rg) {
        for (const UttExtents& e : rg->tabs) {
            hipLaunchKernelGGL(bv_im2col_kernel<UttExtents>, dim3(bv_blocks((size_t)e.max_frames * up * cv.kp), (unsigned)e.cnt), dim3(256), 0, st, x, 0, cv.cin,
                               cv.k, dil, cv.kp, 0, v->col, (size_t)0, up, src_ld, e);
            F5_LAUNCH_CHECK();
        }
    } else {
        hipLaunchKernelGGL(bv_im2col_kernel<BvNoExt>, dim3(bv_blocks(total)), dim3(256), 0, st, x, T, cv.cin, cv.k, dil, cv.kp, chan_major, v->col, total, 1, 0,
                           BvNoExt{});
        F5_LAUNCH_CHECK();
    }
    GemmParams g;
    memset(&g, 0, sizeof(g));
    g.A = v->col; g.lda = cv.kp; g.W = cv.w; g.ldw = cv.kp; g.M = T; g.N = cv.cout; g.K = cv.kp; g.bias = cv.b; g.out_f = out; g.ldof = cv.cout;
    g.rows_per_batch = T;
    return launch_gemm(g, F5_PREC_FP32, GEMM_DENSE, residual ? EPI_RESID : EPI_STORE_F32, 0, st);
}
// the one place that chooses the anti-aliased snake's instantiation (the generator and the f5_op_bigvgan_snake* entries)
static int bv_snake(const float* up_f, const float* dn_f, const BvSnake& s, const float* x, int T, int C, float* out, const BvRagged* rg, int up, hipStream_t st) {
    BvFilters f;
    memcpy(f.up, up_f, sizeof(f.up));
    memcpy(f.dn, dn_f, sizeof(f.dn));
    if (rg) {
        for (const UttExtents& e : rg->tabs) {
            const unsigned tiles = (unsigned)(((size_t)e.max_frames * up + 31) / 32);
            if (C % 64 == 0)
                hipLaunchKernelGGL((bv_aa_snake_kernel<64, UttExtents>), dim3(tiles * (unsigned)(C / 64), (unsigned)e.cnt), dim3(256), 0, st, x, 0, C, s.a, s.invb, f,
                                   out, up, e);
            else
                hipLaunchKernelGGL((bv_aa_snake_kernel<32, UttExtents>), dim3(tiles * (unsigned)((C + 31) / 32), (unsigned)e.cnt), dim3(256), 0, st, x, 0, C, s.a,
                                   s.invb, f, out, up, e);
            F5_LAUNCH_CHECK();
        }
        return 0;
    }
    if (C % 64 == 0)
        hipLaunchKernelGGL((bv_aa_snake_kernel<64, BvNoExt>), dim3((unsigned)(C / 64), (unsigned)((T + 31) / 32)), dim3(256), 0, st, x, T, C, s.a, s.invb, f, out, 1,
                           BvNoExt{});
    else
        hipLaunchKernelGGL((bv_aa_snake_kernel<32, BvNoExt>), dim3((unsigned)((C + 31) / 32), (unsigned)((T + 31) / 32)), dim3(256), 0, st, x, T, C, s.a, s.invb, f,
                           out, 1, BvNoExt{});
    F5_LAUNCH_CHECK();
    return 0;
}
// ConvTranspose1d in place on v->x: T rows (ragged: `up` rows per mel frame) -> T * u rows
static int bv_upsample(f5_bigvgan_s* v, const BvUp& up, int T, const BvRagged* rg, int upf, hipStream_t st) {
    const size_t rows = (size_t)T + (rg ? rg->cnt : 1);
    if (rg) {
        int ubase = 0;
        for (const UttExtents& e : rg->tabs) {
            hipLaunchKernelGGL(bv_up_gather_kernel<UttExtents>, dim3(bv_blocks(((size_t)e.max_frames * upf + 1) * up.kp), (unsigned)e.cnt), dim3(256), 0, st, v->x, 0,
                               up.cin, up.R, up.kp, v->col, (size_t)0, upf, ubase, e);
            F5_LAUNCH_CHECK();
            ubase += e.cnt;
        }
    } else {
        const size_t tg = rows * up.kp;
        hipLaunchKernelGGL(bv_up_gather_kernel<BvNoExt>, dim3(bv_blocks(tg)), dim3(256), 0, st, v->x, T, up.cin, up.R, up.kp, v->col, tg, 1, 0, BvNoExt{});
        F5_LAUNCH_CHECK();
    }
    GemmParams g;
    memset(&g, 0, sizeof(g));
    g.A = v->col; g.lda = up.kp; g.W = up.w; g.ldw = up.kp; g.M = (int)rows; g.N = up.u * up.cout; g.K = up.kp; g.out_f = v->tmp; g.ldof = up.u * up.cout;
    F5_TRY(launch_gemm(g, F5_PREC_FP32, GEMM_DENSE, EPI_STORE_F32, 0, st));
    if (rg) {
        int ubase = 0;
        for (const UttExtents& e : rg->tabs) {
            hipLaunchKernelGGL(bv_up_scatter_kernel<UttExtents>, dim3(bv_blocks((size_t)e.max_frames * upf * up.u * up.cout), (unsigned)e.cnt), dim3(256), 0, st,
                               v->tmp, 0, up.cout, up.u, up.pad, up.b, v->x, (size_t)0, upf, ubase, e);
            F5_LAUNCH_CHECK();
            ubase += e.cnt;
        }
    } else {
        const size_t ts = (size_t)T * up.u * up.cout;
        hipLaunchKernelGGL(bv_up_scatter_kernel<BvNoExt>, dim3(bv_blocks(ts)), dim3(256), 0, st, v->tmp, T, up.cout, up.u, up.pad, up.b, v->x, ts, 1, 0, BvNoExt{});
        F5_LAUNCH_CHECK();
    }
    return 0;
}

static size_t bv_total_up(const f5_bigvgan_config& c) {
    size_t total_up = 1;
    for (int i = 0; i < c.num_upsamples; ++i) total_up *= (size_t)c.upsample_rates[i];
    return total_up;
}

// the workspace for T frames in nb utterances (grown once per longest call; not a per-call allocation)
static int bv_ensure_work(f5_bigvgan_s* v, size_t T, size_t nb, hipStream_t st) {
    if (T <= v->work_T && nb <= v->work_B) return 0;
    const f5_bigvgan_config& c = v->cfg;
    T = std::max(T, v->work_T);
    nb = std::max(nb, v->work_B);
    F5_HIP(hipStreamSynchronize(st));
    v->work.release();
    v->work_T = v->work_B = 0;
    size_t act = T * c.upsample_initial_channel, col = T * v->conv_pre.kp, tmp = 0;
    size_t Ti = T;
    int ch = c.upsample_initial_channel;
    for (int i = 0; i < c.num_upsamples; ++i) {
        const BvUp& up = v->ups[i];
        col = std::max(col, (Ti + nb) * (size_t)up.kp);
        tmp = std::max(tmp, (Ti + nb) * (size_t)up.u * up.cout);
        Ti *= (size_t)up.u;
        ch /= 2;
        act = std::max(act, Ti * (size_t)ch);
        for (int j = 0; j < c.num_kernels; ++j) col = std::max(col, Ti * (size_t)v->blocks[(size_t)i * c.num_kernels + j].c1[0].kp);
    }
    col = std::max(col, Ti * (size_t)v->conv_post.kp);
    F5_TRY(v->work.alloc_t(&v->x, act, false));
    F5_TRY(v->work.alloc_t(&v->y, act, false));
    F5_TRY(v->work.alloc_t(&v->xt, act, false));
    F5_TRY(v->work.alloc_t(&v->xt2, act, false));
    F5_TRY(v->work.alloc_t(&v->xs, act, false));
    F5_TRY(v->work.alloc_t(&v->col, col, false));
    F5_TRY(v->work.alloc_t(&v->tmp, tmp, false));
    v->work_T = T;
    v->work_B = nb;
    return 0;
}

// mel -> wave over T mel frames: one utterance (mel channel-major [num_mels][T]), or, with rg, the utterances of one launch set back to back (mel
// frame-major [*, ld], read through the tables' src0).  wave receives T * prod(upsample_rates) samples.
static int bv_generate(f5_bigvgan_s* v, const BvRagged* rg, int T, const float* mel, int ld, float* wave, hipStream_t st) {
    const f5_bigvgan_config& c = v->cfg;
    int Ti = T, ch = c.upsample_initial_channel, U = 1;
    F5_TRY(bv_conv(v, v->conv_pre, mel, Ti, 1, rg ? 0 : 1, v->x, false, rg, U, rg ? ld : 0, st));
    for (int i = 0; i < c.num_upsamples; ++i) {
        const BvUp& up = v->ups[i];
        F5_TRY(bv_upsample(v, up, Ti, rg, U, st));
        Ti *= up.u;
        U *= up.u;
        ch /= 2;
        const size_t n = (size_t)Ti * ch;
        for (int j = 0; j < c.num_kernels; ++j) {
            const BvBlock& blk = v->blocks[(size_t)i * c.num_kernels + j];
            F5_HIP(hipMemcpyAsync(v->y, v->x, n * sizeof(float), hipMemcpyDeviceToDevice, st));
            for (int t = 0; t < 3; ++t) {
                F5_TRY(bv_snake(v->up_f, v->dn_f, blk.act[2 * t], v->y, Ti, ch, v->xt, rg, U, st));
                F5_TRY(bv_conv(v, blk.c1[t], v->xt, Ti, blk.dil[t], 0, v->xt2, false, rg, U, 0, st));
                F5_TRY(bv_snake(v->up_f, v->dn_f, blk.act[2 * t + 1], v->xt2, Ti, ch, v->xt, rg, U, st));
                F5_TRY(bv_conv(v, blk.c2[t], v->xt, Ti, 1, 0, v->y, true, rg, U, 0, st));  // y += conv2(...)
            }
            if (j == 0)
                F5_HIP(hipMemcpyAsync(v->xs, v->y, n * sizeof(float), hipMemcpyDeviceToDevice, st));
            else {
                hipLaunchKernelGGL(bv_axpby_kernel, dim3(bv_blocks(n)), dim3(256), 0, st, v->xs, v->y, 1.0f, 1.0f, n);
                F5_LAUNCH_CHECK();
            }
        }
        hipLaunchKernelGGL(bv_axpby_kernel, dim3(bv_blocks(n)), dim3(256), 0, st, v->x, v->xs, 0.0f, 1.0f / (float)c.num_kernels, n);
        F5_LAUNCH_CHECK();
    }
    F5_TRY(bv_snake(v->up_f, v->dn_f, v->act_post, v->x, Ti, ch, v->xt, rg, U, st));
    F5_TRY(bv_conv(v, v->conv_post, v->xt, Ti, 1, 0, v->y, false, rg, U, 0, st));
    hipLaunchKernelGGL(bv_final_kernel, dim3(bv_blocks((size_t)Ti)), dim3(256), 0, st, v->y, c.use_tanh_at_final, wave, (size_t)Ti);
    F5_LAUNCH_CHECK();
    return 0;
}

// mel [B][num_mels][T] f32 -> wave [B][T * prod(upsample_rates)] f32
extern "C" int f5_bigvgan_forward(f5_bigvgan_t v, int B, int T, const float* mel, float* wave, f5_stream_t stream) {
    if (!v || !mel || !wave || B <= 0 || T <= 0) return f5_fail(F5_EINVAL, "bad argument");
    if (!v->finalized) return f5_fail(F5_ESTATE, "f5_bigvgan_finalize must be called first");
    F5_TRY(f5_check_device());
    hipStream_t st = (hipStream_t)stream;
    const size_t total_up = bv_total_up(v->cfg);
    F5_TRY(bv_ensure_work(v, (size_t)T, 1, st));
    for (int b = 0; b < B; ++b) F5_TRY(bv_generate(v, nullptr, T, mel + (size_t)b * v->cfg.num_mels * T, 0, wave + (size_t)b * T * total_up, st));
    return 0;
}

// See f5hip.h.  The utterance list is cut, in order, into launch sets of at most g_bigvgan_group_frames frames (an utterance longer than that is a
// set of its own); every check is made, and the workspace grown to the largest set, before the first launch.
extern "C" int f5_bigvgan_decode_ragged(f5_bigvgan_t v, int B, const int32_t* row_start_host, const int32_t* frames_host, const float* mel, int ld,
                                        float* wave, int64_t* total_samples, f5_stream_t stream) {
    if (!v || !row_start_host || !frames_host || !mel || !wave) return f5_fail(F5_EINVAL, "null argument");
    if (!v->finalized) return f5_fail(F5_ESTATE, "f5_bigvgan_finalize must be called first");
    if (B <= 0 || ld < v->cfg.num_mels) return f5_fail(F5_EINVAL, "need B >= 1 and ld >= num_mels");
    F5_TRY(f5_check_device());
    hipStream_t st = (hipStream_t)stream;
    const int64_t total_up = (int64_t)bv_total_up(v->cfg);
    std::vector<BvRagged> sets;
    std::vector<int64_t> set_frame0;
    int64_t frames = 0;
    size_t max_frames = 0, max_cnt = 0;
    for (int u = 0; u < B; ++u) {
        const int t = frames_host[u];
        if (t < 1 || row_start_host[u] < 0) return f5_fail(F5_EINVAL, "utterance %d: need T >= 1 frames and a row start >= 0", u);
        // rows of the last stage (plus one gather row per utterance) and wave samples are 32-bit in the kernels; so are the mel row numbers
        if ((frames + t) * total_up + B > (int64_t)INT_MAX || (int64_t)row_start_host[u] + t > (int64_t)INT_MAX)
            return f5_fail(F5_EINVAL, "utterance %d: the call's rows or samples exceed 32-bit indexing", u);
        if (sets.empty() || sets.back().frames + (int64_t)t > (int64_t)g_bigvgan_group_frames) {
            sets.emplace_back();
            set_frame0.push_back(frames);
        }
        BvRagged& s = sets.back();
        if (s.tabs.empty() || s.tabs.back().cnt == UttExtents::MAXU) s.tabs.emplace_back();
        UttExtents& e = s.tabs.back();
        e.row0[e.cnt] = s.frames;
        e.frames[e.cnt] = t;
        e.src0[e.cnt] = row_start_host[u];
        e.out0[e.cnt] = (int)((int64_t)s.frames * total_up);
        if (t > e.max_frames) e.max_frames = t;
        ++e.cnt;
        ++s.cnt;
        s.frames += t;
        frames += t;
        max_frames = std::max(max_frames, (size_t)s.frames);
        max_cnt = std::max(max_cnt, (size_t)s.cnt);
    }
    if (total_samples) *total_samples = frames * total_up;
    F5_TRY(bv_ensure_work(v, max_frames, max_cnt, st));
    for (size_t k = 0; k < sets.size(); ++k) F5_TRY(bv_generate(v, &sets[k], sets[k].frames, mel, ld, wave + (size_t)(set_frame0[k] * total_up), st));
    return 0;
}

// ----------------------------------------------------------------------------- test-only ops (f5hip.h)
static void bv_op_filters(const float* up_f, const float* dn_f, float* up, float* dn) {
    if (up_f) memcpy(up, up_f, 12 * sizeof(float)); else kaiser_sinc_filter(0.25, 0.3, 12, up);
    if (dn_f) memcpy(dn, dn_f, 12 * sizeof(float)); else kaiser_sinc_filter(0.25, 0.3, 12, dn);
}
extern "C" int f5_op_bigvgan_snake(int T, int C, const float* x, const float* a, const float* invb, const float* up_f, const float* dn_f, float* out,
                                   f5_stream_t stream) {
    if (T <= 0 || C <= 0 || !x || !a || !invb || !out) return f5_fail(F5_EINVAL, "bad argument");
    F5_TRY(f5_check_device());
    float up[12], dn[12];
    bv_op_filters(up_f, dn_f, up, dn);
    BvSnake s;
    s.a = const_cast<float*>(a);
    s.invb = const_cast<float*>(invb);
    return bv_snake(up, dn, s, x, T, C, out, nullptr, 1, (hipStream_t)stream);
}
extern "C" int f5_op_bigvgan_snake_ragged(int cnt, const int32_t* frames_host, int up, int C, const float* x, const float* a, const float* invb,
                                          const float* up_f, const float* dn_f, float* out, f5_stream_t stream) {
    if (cnt <= 0 || up <= 0 || C <= 0 || !frames_host || !x || !a || !invb || !out) return f5_fail(F5_EINVAL, "bad argument");
    F5_TRY(f5_check_device());
    BvRagged rg;
    for (int u = 0; u < cnt; ++u) {
        const int t = frames_host[u];
        if (t < 1 || ((int64_t)rg.frames + t) * up > (int64_t)INT_MAX) return f5_fail(F5_EINVAL, "utterance %d: need 1 <= frames and 32-bit rows", u);
        if (rg.tabs.empty() || rg.tabs.back().cnt == UttExtents::MAXU) rg.tabs.emplace_back();
        UttExtents& e = rg.tabs.back();
        e.row0[e.cnt] = rg.frames;
        e.frames[e.cnt] = t;
        e.src0[e.cnt] = e.out0[e.cnt] = 0;  // (the snake reads neither)
        if (t > e.max_frames) e.max_frames = t;
        ++e.cnt;
        ++rg.cnt;
        rg.frames += t;
    }
    float fu[12], fd[12];
    bv_op_filters(up_f, dn_f, fu, fd);
    BvSnake s;
    s.a = const_cast<float*>(a);
    s.invb = const_cast<float*>(invb);
    return bv_snake(fu, fd, s, x, rg.frames * up, C, out, &rg, up, (hipStream_t)stream);
}
