// distill_loss.hip -- the losses of the reference's teacher-to-student distillation step (train/distil_reload.py:1070-1097) for one batch,
// forward only, from ONE pass over the two predictions:
//   flow = x1 - x0;  (student - flow)^2;  (teacher - flow)^2;  (student - teacher)^2;  |student - teacher|
// -- the elementwise values F.mse_loss / F.l1_loss(reduction="none") form, every fp32 step rounded on its own (the library is built with
// -ffp-contract=off, and the kernel says so again) -- summed in fp64 over the rows of the random span.  The partition and the order of the sums
// are cfm_loss.hip's: a workgroup owns CHUNK consecutive elements of one utterance and writes four partials, a second kernel adds an
// utterance's partials by index and counts its selected rows, a third adds the utterances in order and divides.  No atomics: the same input
// gives the same bits.  The script divides by rand_span_mask.sum(), the number of selected FRAMES (not frames x mel), clamped to at least 1:
// its losses are mel times a mean, and an empty span gives 0, not NaN.  Both quirks are kept.
// Loads: flat 16-byte vectors when mel % 4 == 0 and the pointers are 16-byte aligned, elements otherwise; a row outside the span is not loaded.
#include "common.h"
#include "runtime.h"

static constexpr int DST_THREADS = 256;
static constexpr int DST_CHUNK = 2048;  // elements of one utterance per workgroup (cfm_loss.hip: CFM_CHUNK)
static constexpr int DST_TERMS = 4;     // student-flow MSE, teacher-flow MSE, student-teacher MSE, student-teacher L1

template <int W> struct DstVec;
template <> struct DstVec<4> {
    typedef f32x4 T;
    static __device__ __forceinline__ T load(const float* p) { return *(const f32x4*)p; }
    static __device__ __forceinline__ float get(const T& v, int j) { return v[j]; }
};
template <> struct DstVec<1> {
    typedef float T;
    static __device__ __forceinline__ T load(const float* p) { return *p; }
    static __device__ __forceinline__ float get(const T& v, int) { return v; }
};

// fixed-order sum of one value per thread: the xor butterfly inside each wave, then the waves' totals in wave order
__device__ __forceinline__ double dst_block_sum(double v, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[wave] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < DST_THREADS / 64; ++w) s += lds[w];
    __syncthreads();
    return s;
}

// workgroup (b, g): elements [g * CHUNK, (g + 1) * CHUNK) of utterance b -> partials[(b * G + g) * 4 + term]
template <int W>
__global__ __launch_bounds__(DST_THREADS) void distill_partial_kernel(int N, int mel, int G, const float* __restrict__ student,
                                                                      const float* __restrict__ teacher, const float* __restrict__ x1,
                                                                      const float* __restrict__ x0, const uint8_t* __restrict__ span,
                                                                      double* __restrict__ partials) {
#pragma clang fp contract(off)
    typedef DstVec<W> V;
    __shared__ double lds[DST_THREADS / 64];
    const int b = blockIdx.x / G, g = blockIdx.x - b * G;
    const int64_t per = (int64_t)N * mel;
    const int64_t start = (int64_t)g * DST_CHUNK;
    const int64_t end = start + DST_CHUNK < per ? start + DST_CHUNK : per;
    const int64_t base = (int64_t)b * per;
    const uint8_t* sp = span + (int64_t)b * N;
    double acc[DST_TERMS] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t e = start + (int64_t)threadIdx.x * W; e < end; e += (int64_t)DST_THREADS * W) {
        if (!sp[(uint32_t)e / (uint32_t)mel]) continue;  // e < N * mel < 2^31; W = 4: elements e .. e + 3 share the row (mel % 4 == 0)
        const typename V::T s4 = V::load(student + base + e), t4 = V::load(teacher + base + e), a1 = V::load(x1 + base + e),
                            a0 = V::load(x0 + base + e);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float s = V::get(s4, j), t = V::get(t4, j);
            const float flow = V::get(a1, j) - V::get(a0, j);
            const float ds = s - flow;
            const float dt = t - flow;
            const float dd = s - t;
            const float sq_s = ds * ds;
            const float sq_t = dt * dt;
            const float sq_d = dd * dd;
            acc[0] += (double)sq_s;
            acc[1] += (double)sq_t;
            acc[2] += (double)sq_d;
            acc[3] += (double)fabsf(dd);
        }
    }
#pragma unroll
    for (int k = 0; k < DST_TERMS; ++k) {
        const double s = dst_block_sum(acc[k], lds);
        if (threadIdx.x == 0) partials[((int64_t)b * G + g) * DST_TERMS + k] = s;
    }
}

// workgroup b: sums[b][term] = the utterance's partials added by index, frames[b] = its selected rows
__global__ __launch_bounds__(DST_THREADS) void distill_utterance_kernel(int N, int G, const double* __restrict__ partials,
                                                                        const uint8_t* __restrict__ span, double* __restrict__ sums,
                                                                        int64_t* __restrict__ frames) {
    __shared__ double lds[DST_THREADS / 64];
    __shared__ int rows_lds[DST_THREADS / 64];
    const int b = blockIdx.x;
#pragma unroll
    for (int k = 0; k < DST_TERMS; ++k) {
        double acc = 0.0;
        for (int g = threadIdx.x; g < G; g += DST_THREADS) acc += partials[((int64_t)b * G + g) * DST_TERMS + k];
        const double s = dst_block_sum(acc, lds);
        if (threadIdx.x == 0) sums[(int64_t)b * DST_TERMS + k] = s;
    }
    int rows = 0;
    for (int n = threadIdx.x; n < N; n += DST_THREADS) rows += span[(int64_t)b * N + n] != 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rows += __shfl_xor(rows, o, 64);
    if ((threadIdx.x & 63) == 0) rows_lds[threadIdx.x >> 6] = rows;
    __syncthreads();
    if (threadIdx.x == 0) {
        int r = 0;
        for (int w = 0; w < DST_THREADS / 64; ++w) r += rows_lds[w];
        frames[b] = (int64_t)r;
    }
}

// batch[term] = float(sum_b sums[b][term] / max(sum_b frames[b], 1)), the utterances in order (distil_reload.py:1072: .clamp(min=1))
__global__ void distill_final_kernel(int B, const double* __restrict__ sums, const int64_t* __restrict__ frames, float* __restrict__ batch) {
    if (blockIdx.x != 0 || threadIdx.x >= DST_TERMS) return;
    const int k = threadIdx.x;
    double s = 0.0;
    int64_t c = 0;
    for (int b = 0; b < B; ++b) {
        s += sums[(int64_t)b * DST_TERMS + k];
        c += frames[b];
    }
    batch[k] = (float)(s / (double)(c > 1 ? c : 1));
}

static int64_t dst_cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
static bool dst_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// (the limits of cfm_loss.hip: cfm_shape_check)
static int distill_shape_check(int B, int N, int mel) {
    if (B < 1 || N < 1 || mel < 1) return f5_fail(F5_EINVAL, "distill: B = %d, N = %d, mel = %d must all be at least 1", B, N, mel);
    const int64_t per = (int64_t)N * mel;
    if (per >= ((int64_t)1 << 31) || (int64_t)B * N >= ((int64_t)1 << 31) || (int64_t)B * dst_cdiv64(per, DST_CHUNK) >= ((int64_t)1 << 31))
        return f5_fail(F5_EINVAL, "distill: B = %d, N = %d, mel = %d is beyond the launch grid", B, N, mel);
    return 0;
}

extern "C" int64_t f5_distill_loss_workspace(int B, int N, int mel) {
    const int rc = distill_shape_check(B, N, mel);
    if (rc != 0) return rc;
    return (int64_t)B * dst_cdiv64((int64_t)N * mel, DST_CHUNK) * DST_TERMS * (int64_t)sizeof(double);
}

extern "C" int f5_distill_loss(int B, int N, int mel, const float* student, const float* teacher, const float* x1, const float* x0,
                               const uint8_t* span, double* sums, int64_t* frames, float* batch, void* workspace, f5_stream_t stream) {
    F5_TRY(distill_shape_check(B, N, mel));
    if (!student || !teacher || !x1 || !x0 || !span || !sums || !frames || !batch || !workspace)
        return f5_fail(F5_EINVAL, "f5_distill_loss: null argument");
    if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)sums & 7) != 0 || ((uintptr_t)frames & 7) != 0)
        return f5_fail(F5_EINVAL, "f5_distill_loss: workspace, sums and frames must be 8-byte aligned");
    F5_TRY(f5_check_device());
    hipStream_t st = (hipStream_t)stream;
    const int G = (int)dst_cdiv64((int64_t)N * mel, DST_CHUNK);
    double* partials = (double*)workspace;
    const bool vec = mel % 4 == 0 && dst_aligned16(student) && dst_aligned16(teacher) && dst_aligned16(x1) && dst_aligned16(x0);
    if (vec)
        hipLaunchKernelGGL(distill_partial_kernel<4>, dim3(B * G), dim3(DST_THREADS), 0, st, N, mel, G, student, teacher, x1, x0, span, partials);
    else
        hipLaunchKernelGGL(distill_partial_kernel<1>, dim3(B * G), dim3(DST_THREADS), 0, st, N, mel, G, student, teacher, x1, x0, span, partials);
    F5_LAUNCH_CHECK();
    hipLaunchKernelGGL(distill_utterance_kernel, dim3(B), dim3(DST_THREADS), 0, st, N, G, partials, span, sums, frames);
    F5_LAUNCH_CHECK();
    hipLaunchKernelGGL(distill_final_kernel, dim3(1), dim3(64), 0, st, B, sums, frames, batch);
    F5_LAUNCH_CHECK();
    return 0;
}
