// align.hip -- the training target of the duration predictor, for validating a duration_predictor_*.pt checkpoint (forward only):
//   similarity  phoneme x mel cosine similarity with the diagonal bias and the -inf padding     reference model/trainer.py:925-970
//   viterbi     monotonic alignment search, "viterbi"                                           reference model/alignment_utils.py:154-212
//   window      monotonic alignment search, "window"                                            reference model/alignment_utils.py:214-258
//   loss        masked squared log-duration error and duration MAE                              reference model/trainer.py:984-1025
// The viterbi recurrence P[n,t] = s[n,t] + max(P[n-1,t], P[n,t-1]) is one fp32 add per cell in the reference's association, so P has the
// reference's bits.  It runs as an anti-diagonal wavefront: one workgroup per utterance, lane n owns row n, and in step k lane n forms cell
// (n, k - n) from its own last value (the left neighbour) and lane n-1's last value (the upper neighbour): nt + T - 1 dependent steps.  Inside
// a wave the upper neighbour arrives by one DPP move (wave_shr:1); across waves lane 63 leaves its value in one of two LDS slots per wave, which
// the next wave's lane 0 picks up after the step's single barrier (two slots: a step writes the slot the previous step did not read).  A
// workgroup of one wave runs without barriers.  The similarity values are fetched eight steps ahead, so no step waits on memory.
// The backtrack asks one thing of row n of P: the last t <= curr - 1 with P[n,t+1] - P[n,t] > 0 (fp32; NaN from -inf - -inf compares false), or
// 0.  Each lane keeps that running index beside its P value and stores IT to the workspace, one i32 per cell, instead of P: the backtrack is then
// one lookup per row (thread 0, nt dependent loads) and P itself never reaches memory.
// The window search is serial in n by construction (a row's window starts where the previous row ended): one workgroup per utterance finds each
// row's first maximum with a fixed-order reduction.  Nothing here uses atomics; every sum has a fixed order.
#include <limits.h>

#include "common.h"
#include "runtime.h"

static constexpr int AL_MAX_NT = 1024;     // one lane per phoneme row: the largest workgroup
static constexpr int AL_MAX_T = 65536;     // (max_duration of the sampler is 4096)
static constexpr int AL_CHUNK = 8;         // similarity values fetched ahead per lane
static constexpr int AL_WIN_THREADS = 256;
static constexpr int SIM_THREADS = 256;
static constexpr int SIM_TT = 16;          // mel frames per workgroup of the similarity kernel
static constexpr int SIM_MAX_K = 768;      // LDS: (SIM_TT * (K + 1) + 4 * K) floats <= 64 KiB
static constexpr int DL_THREADS = 256;

// lane i receives lane i-1's value; lane 0 keeps its own (DPP wave_shr:1, control 0x138, all rows and banks enabled)
__device__ __forceinline__ float al_from_lane_below(float v) {
    const int x = __float_as_int(v);
    return __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x138, 0xf, 0xf, false));
}

// torch.maximum: a NaN on either side is the result
__device__ __forceinline__ float al_maximum(float a, float b) { return (a > b || a != a) ? a : b; }

// segments [seg_start[n], seg_end[n]] (empty when end < start) -> durations [nt] and, when asked for, the 0/1 matrix [nt, T]
__device__ __forceinline__ void al_write_outputs(int nt, int T, const int* seg_start, const int* seg_end, float* __restrict__ durations,
                                                 float* __restrict__ alignment) {
    for (int n = threadIdx.x; n < nt; n += blockDim.x) durations[n] = (float)(seg_end[n] - seg_start[n] + 1);
    if (!alignment) return;
    const int total = nt * T;  // <= 2^26
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int n = i / T, t = i - n * T;
        alignment[i] = (t >= seg_start[n] && t <= seg_end[n]) ? 1.0f : 0.0f;
    }
}

// workgroup b, blockDim = nt rounded up to whole waves; last: i32 [B, nt, T], cell (n, t) = the last u <= t with P[n,u+1] - P[n,u] > 0, else 0
// (cells t = T - 1 are never written or read)
__global__ __launch_bounds__(AL_MAX_NT) void align_viterbi_kernel(int nt, int T, const float* __restrict__ sim, int* __restrict__ last,
                                                                  float* __restrict__ durations, float* __restrict__ alignment) {
#pragma clang fp contract(off)
    __shared__ float xch[2][AL_MAX_NT / 64];
    __shared__ int seg_start[AL_MAX_NT], seg_end[AL_MAX_NT];
    const int b = blockIdx.x, n = threadIdx.x, lane = n & 63, wave = n >> 6;
    const bool multi = blockDim.x > 64, row = n < nt;
    const int64_t base = (int64_t)b * nt * T;
    const float* srow = sim + base + (int64_t)(row ? n : 0) * T;
    int* lrow = last + base + (int64_t)(row ? n : 0) * T;
    const int steps = nt + T - 1;
    float prev = 0.0f;  // this lane's last P value: P[n, t-1] when the step forms P[n, t]
    int lastpos = 0;
    float nxt[AL_CHUNK], cur[AL_CHUNK];
#pragma unroll
    for (int j = 0; j < AL_CHUNK; ++j) {
        const int t = j - n;
        nxt[j] = (row && t >= 0 && t < T) ? srow[t] : 0.0f;
    }
    for (int k0 = 0; k0 < steps; k0 += AL_CHUNK) {
#pragma unroll
        for (int j = 0; j < AL_CHUNK; ++j) {
            cur[j] = nxt[j];
            const int t = k0 + AL_CHUNK + j - n;
            nxt[j] = (row && t >= 0 && t < T) ? srow[t] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < AL_CHUNK; ++j) {
            const int k = k0 + j, t = k - n;
            float up = al_from_lane_below(prev);
            if (multi && lane == 0 && wave > 0) up = xch[(k + 1) & 1][wave - 1];  // written in step k - 1 (never used at k = 0: t < 0 there)
            if (row && t >= 0 && t < T) {
                const float s = cur[j];
                float v;
                if (n == 0)
                    v = t == 0 ? s : prev + s;  // row 0: the serial running sum
                else if (t == 0)
                    v = up + s;  // column 0
                else
                    v = s + al_maximum(up, prev);
                if (t > 0) {
                    const float g = v - prev;
                    if (g > 0.0f) lastpos = t - 1;
                    lrow[t - 1] = lastpos;
                }
                prev = v;
            }
            if (multi) {
                if (lane == 63) xch[k & 1][wave] = prev;
                __syncthreads();
            }
        }
    }
    if (row) {
        seg_start[n] = 0;
        seg_end[n] = -1;
    }
    __syncthreads();  // every row of `last` is visible to thread 0
    if (n == 0) {
        int curr = T - 1;
        for (int r = nt - 1; r >= 0; --r) {
            const int boundary = (r > 0 && curr >= 1) ? last[base + (int64_t)r * T + (curr - 1)] : 0;
            seg_start[r] = boundary;
            seg_end[r] = curr;
            curr = boundary - 1;
            if (curr < 0) break;
        }
    }
    __syncthreads();
    al_write_outputs(nt, T, seg_start, seg_end, durations + (int64_t)b * nt, alignment ? alignment + base : nullptr);
}

// (value, index) of the first maximum: the larger value wins, the smaller index among equals
__device__ __forceinline__ void al_argmax_merge(float& bv, int& bi, float v, int i) {
    if (v > bv || (v == bv && i < bi)) {
        bv = v;
        bi = i;
    }
}

__global__ __launch_bounds__(AL_WIN_THREADS) void align_window_kernel(int nt, int T, const float* __restrict__ sim, float* __restrict__ durations,
                                                                      float* __restrict__ alignment) {
    __shared__ int seg_start[AL_MAX_NT], seg_end[AL_MAX_NT];
    __shared__ float red_v[2][AL_WIN_THREADS / 64];
    __shared__ int red_i[2][AL_WIN_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = (int64_t)b * nt * T;
    for (int n = tid; n < nt; n += AL_WIN_THREADS) {
        seg_start[n] = 0;
        seg_end[n] = -1;
    }
    const double frames_per_phone = (double)T / (double)nt;
    const int tw = (int)((double)T * 0.2);
    const int window = tw > 2 ? tw : 2;
    int start = 0;  // the same in every thread
    for (int n = 0; n < nt - 1; ++n) {
        const int expected_end = (int)((double)(n + 1) * frames_per_phone);
        const int ws = start > expected_end - window ? start : expected_end - window;
        const int we = T - 1 < expected_end + window ? T - 1 : expected_end + window;
        const float* srow = sim + base + (int64_t)n * T;
        float bv = -INFINITY;
        int bi = INT_MAX;
        for (int i = ws + tid; i <= we; i += AL_WIN_THREADS) al_argmax_merge(bv, bi, srow[i], i);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            al_argmax_merge(bv, bi, ov, oi);
        }
        if (lane == 0) {
            red_v[n & 1][wave] = bv;
            red_i[n & 1][wave] = bi;
        }
        __syncthreads();  // (two slots: the next row's writes go to the other one)
        bv = red_v[n & 1][0];
        bi = red_i[n & 1][0];
#pragma unroll
        for (int w = 1; w < AL_WIN_THREADS / 64; ++w) al_argmax_merge(bv, bi, red_v[n & 1][w], red_i[n & 1][w]);
        const int best_end = bi == INT_MAX ? ws : bi;  // an empty window (possible only when nt > T; the reference raises): the row takes one frame
        if (tid == 0) {
            seg_start[n] = start;
            seg_end[n] = best_end;
        }
        start = best_end + 1;
        if (start >= T) break;
    }
    if (tid == 0 && start < T) {
        seg_start[nt - 1] = start;
        seg_end[nt - 1] = T - 1;
    }
    __syncthreads();
    al_write_outputs(nt, T, seg_start, seg_end, durations + (int64_t)b * nt, alignment ? alignment + base : nullptr);
}

// workgroup (tile, b): frames [tile * SIM_TT, +SIM_TT) of utterance b against every phoneme row.  LDS: the tile's normalised mel projections
// [SIM_TT][K + 1] and one normalised embedding row per wave [4][K].
__global__ __launch_bounds__(SIM_THREADS) void align_similarity_kernel(int nt, int T, int mel, int K, int rows, const float* __restrict__ embed,
                                                                       const int32_t* __restrict__ ids, const int32_t* __restrict__ p_lens,
                                                                       const float* __restrict__ melspec, const int32_t* __restrict__ m_lens,
                                                                       const float* __restrict__ proj, float* __restrict__ sim) {
    extern __shared__ float sim_lds[];
    const int ldm = K + 1;
    float* mp = sim_lds;
    float* en = sim_lds + SIM_TT * ldm;
    const int b = blockIdx.y, t0 = blockIdx.x * SIM_TT, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int item = tid; item < SIM_TT * K; item += SIM_THREADS) {
        const int tt = item / K, k = item - tt * K, t = t0 + tt;
        float acc = 0.0f;
        if (t < T) {
            const float* mrow = melspec + ((int64_t)b * T + t) * mel;
            for (int m = 0; m < mel; ++m) acc = fmaf(mrow[m], proj[(int64_t)m * K + k], acc);
        }
        mp[tt * ldm + k] = acc;
    }
    __syncthreads();
    for (int tt = wave; tt < SIM_TT; tt += SIM_THREADS / 64) {
        float ss = 0.0f;
        for (int k = lane; k < K; k += 64) ss = fmaf(mp[tt * ldm + k], mp[tt * ldm + k], ss);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
        const float d = sqrtf(ss) + 1e-8f;
        for (int k = lane; k < K; k += 64) mp[tt * ldm + k] = mp[tt * ldm + k] / d;
    }
    __syncthreads();
    const int p_raw = p_lens[b], m_len = m_lens[b];
    const int p_len = p_raw < 0 ? 0 : (p_raw > nt ? nt : p_raw);
    float* e = en + wave * K;
    for (int n0 = 0; n0 < nt; n0 += SIM_THREADS / 64) {
        const int n = n0 + wave;
        const bool active = n < nt;
        const int id = active ? ids[(int64_t)b * nt + n] : -1;
        const bool known = id >= 0 && id < rows;  // an id outside the table reads nothing and stands for a zero row
        float ss = 0.0f;
        for (int k = lane; k < K; k += 64) {
            const float v = known ? embed[(int64_t)id * K + k] : 0.0f;
            e[k] = v;
            ss = fmaf(v, v, ss);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
        const float d = sqrtf(ss) + 1e-8f;
        for (int k = lane; k < K; k += 64) e[k] = e[k] / d;
        __syncthreads();
        const int tt = lane & (SIM_TT - 1), part = lane / SIM_TT;
        float acc = 0.0f;
        for (int k = part; k < K; k += 64 / SIM_TT) acc = fmaf(e[k], mp[tt * ldm + k], acc);
        acc += __shfl_xor(acc, 16, 64);
        acc += __shfl_xor(acc, 32, 64);
        const int t = t0 + tt;
        if (active && lane < SIM_TT && t < T) {
            float v = acc;
            if (n < p_len && m_len > 0) {
                const int c = (int)(((int64_t)n * m_len) / p_len);
                const int w = m_len / 10 > 3 ? m_len / 10 : 3;
                const int lo = c - w > 0 ? c - w : 0, hi = c + w < m_len ? c + w : m_len;
                if (t >= lo && t < hi) v = v + 3.0f;
            }
            if (n >= p_len || t >= m_len) v = -INFINITY;
            sim[((int64_t)b * nt + n) * T + t] = v;
        }
        __syncthreads();  // the wave's embedding row is rewritten by the next round
    }
}

// fixed-order sum of one value per thread: the xor butterfly inside each wave, then the waves' totals in wave order
__device__ __forceinline__ double dl_block_sum(double v, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < DL_THREADS / 64; ++w) s += lds[w];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(DL_THREADS) void duration_loss_kernel(int nt, const float* __restrict__ logw, const float* __restrict__ durations,
                                                                   const int32_t* __restrict__ p_lens, double* __restrict__ sq_sums,
                                                                   double* __restrict__ abs_sums, int64_t* __restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ double lds[DL_THREADS / 64];
    const int b = blockIdx.x;
    const int p_raw = p_lens[b];
    const int len = p_raw < 0 ? 0 : (p_raw > nt ? nt : p_raw);
    double sq = 0.0, ab = 0.0;
    for (int n = threadIdx.x; n < len; n += DL_THREADS) {
        const double lw = (double)logw[(int64_t)b * nt + n];
        const double d = fmax((double)durations[(int64_t)b * nt + n], 0.1);
        const double target = log(d + 1e-6);
        const double diff = lw - target;
        const double sq1 = diff * diff;
        sq += sq1;
        const double clamped = fmin(fmax(lw, -10.0), 10.0);
        ab += fabs(exp(clamped) - d);
    }
    const double s = dl_block_sum(sq, lds);
    const double a = dl_block_sum(ab, lds);
    if (threadIdx.x == 0) {
        sq_sums[b] = s;
        abs_sums[b] = a;
        counts[b] = len;
    }
}

__global__ void duration_loss_final_kernel(int B, const double* __restrict__ sq_sums, const double* __restrict__ abs_sums,
                                           const int64_t* __restrict__ counts, float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0, a = 0.0;
    int64_t c = 0;
    for (int b = 0; b < B; ++b) {
        s += sq_sums[b];
        a += abs_sums[b];
        c += counts[b];
    }
    const double den = (double)c + 1e-8;
    out[0] = (float)(s / den);
    out[1] = (float)(a / den);
}

static int align_shape_check(int B, int nt, int T) {
    if (B < 1 || nt < 1 || T < 1) return f5_fail(F5_EINVAL, "align: B = %d, nt = %d, T = %d must all be at least 1", B, nt, T);
    if (nt > AL_MAX_NT) return f5_fail(F5_EINVAL, "align: nt = %d phoneme rows exceed the %d one workgroup holds (one lane per row)", nt, AL_MAX_NT);
    if (T > AL_MAX_T) return f5_fail(F5_EINVAL, "align: T = %d frames exceed the limit of %d", T, AL_MAX_T);
    if (B > 65535) return f5_fail(F5_EINVAL, "align: B = %d exceeds 65535 utterances per call", B);
    return 0;
}

extern "C" int64_t f5_align_workspace(int B, int nt, int T) {
    const int rc = align_shape_check(B, nt, T);
    if (rc != 0) return rc;
    return (int64_t)B * nt * T * (int64_t)sizeof(int32_t);
}

extern "C" int f5_align_viterbi(int B, int nt, int T, const float* sim, float* durations, float* alignment, void* workspace,
                                f5_stream_t stream) {
    F5_TRY(align_shape_check(B, nt, T));
    if (!sim || !durations || !workspace) return f5_fail(F5_EINVAL, "f5_align_viterbi: null argument");
    if (((uintptr_t)workspace & 3) != 0) return f5_fail(F5_EINVAL, "f5_align_viterbi: workspace must be 4-byte aligned");
    F5_TRY(f5_check_device());
    const int threads = (nt + 63) / 64 * 64;
    hipLaunchKernelGGL(align_viterbi_kernel, dim3(B), dim3(threads), 0, (hipStream_t)stream, nt, T, sim, (int*)workspace, durations, alignment);
    F5_LAUNCH_CHECK();
    return 0;
}

extern "C" int f5_align_window(int B, int nt, int T, const float* sim, float* durations, float* alignment, void* workspace,
                               f5_stream_t stream) {
    F5_TRY(align_shape_check(B, nt, T));
    if (!sim || !durations) return f5_fail(F5_EINVAL, "f5_align_window: null argument");
    (void)workspace;  // the window search keeps nothing between its passes
    F5_TRY(f5_check_device());
    hipLaunchKernelGGL(align_window_kernel, dim3(B), dim3(AL_WIN_THREADS), 0, (hipStream_t)stream, nt, T, sim, durations, alignment);
    F5_LAUNCH_CHECK();
    return 0;
}

extern "C" int f5_align_similarity(int B, int nt, int T, int mel, int K, int rows, const float* embed, const int32_t* ids,
                                   const int32_t* phoneme_lens, const float* melspec, const int32_t* mel_lens, const float* proj, float* sim,
                                   f5_stream_t stream) {
    F5_TRY(align_shape_check(B, nt, T));
    if (mel < 1 || K < 1 || rows < 1) return f5_fail(F5_EINVAL, "f5_align_similarity: mel = %d, K = %d, rows = %d must all be at least 1", mel, K, rows);
    if (K > SIM_MAX_K) return f5_fail(F5_EINVAL, "f5_align_similarity: K = %d exceeds the %d a workgroup's LDS tile holds", K, SIM_MAX_K);
    if (!embed || !ids || !phoneme_lens || !melspec || !mel_lens || !proj || !sim) return f5_fail(F5_EINVAL, "f5_align_similarity: null argument");
    F5_TRY(f5_check_device());
    const size_t lds = ((size_t)SIM_TT * (K + 1) + (size_t)(SIM_THREADS / 64) * K) * sizeof(float);
    hipLaunchKernelGGL(align_similarity_kernel, dim3((T + SIM_TT - 1) / SIM_TT, B), dim3(SIM_THREADS), lds, (hipStream_t)stream, nt, T, mel, K,
                       rows, embed, ids, phoneme_lens, melspec, mel_lens, proj, sim);
    F5_LAUNCH_CHECK();
    return 0;
}

extern "C" int f5_duration_loss(int B, int nt, const float* logw, const float* durations, const int32_t* phoneme_lens, double* sq_sums,
                                double* abs_sums, int64_t* counts, float* loss_mae, f5_stream_t stream) {
    if (B < 1 || nt < 1) return f5_fail(F5_EINVAL, "f5_duration_loss: B = %d, nt = %d must both be at least 1", B, nt);
    if (!logw || !durations || !phoneme_lens || !sq_sums || !abs_sums || !counts || !loss_mae)
        return f5_fail(F5_EINVAL, "f5_duration_loss: null argument");
    if ((((uintptr_t)sq_sums | (uintptr_t)abs_sums | (uintptr_t)counts) & 7) != 0)
        return f5_fail(F5_EINVAL, "f5_duration_loss: the sums and counts must be 8-byte aligned");
    F5_TRY(f5_check_device());
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(duration_loss_kernel, dim3(B), dim3(DL_THREADS), 0, st, nt, logw, durations, phoneme_lens, sq_sums, abs_sums, counts);
    F5_LAUNCH_CHECK();
    hipLaunchKernelGGL(duration_loss_final_kernel, dim3(1), dim3(64), 0, st, B, sq_sums, abs_sums, counts, loss_mae);
    F5_LAUNCH_CHECK();
    return 0;
}
