// cfm_loss.hip -- the flow-matching layer of CFM.forward (reference model/cfm.py:257-283) around one backbone evaluation, forward only:
//   noise   phi = (1 - t_b) x0 + t_b x1 and cond = span ? 0 : x1 in one pass over x1 and x0 (cfm.py:258-263)
//   loss    F.mse_loss(pred, x1 - x0, reduction="none")[span].mean() (cfm.py:280-283): the flow and the elementwise loss live in registers only
// Every fp32 step is rounded on its own, as torch's separate elementwise kernels round it (the library is built with -ffp-contract=off, and the
// functions below say so again): phi and cond are torch's bits, and the squared differences are the fp32 values mse_loss forms.
// The selected squares are summed in fp64 in a FIXED order, so two runs give the same bits on any device: a workgroup owns CHUNK consecutive
// elements of one utterance (a partition that depends on N and mel only) and writes one partial to the workspace; a second kernel adds an
// utterance's partials by index and counts its selected rows; a third adds the utterances in order and divides.  No atomics anywhere.
// Loads: the [B * N * mel] arrays are read flat, 16 bytes per lane, whenever mel % 4 == 0 (a vector then lies inside one row; mel = 100 makes a row
// 400 bytes, so rows do not line up with a wave's 1 KiB footprint and are not the unit of work) and the pointers are 16-byte aligned; any other
// width or alignment takes the same kernels one element at a time.  The span flag is fetched per row; a row that is not selected is not loaded.
#include "common.h"
#include "runtime.h"

static constexpr int CFM_THREADS = 256;
static constexpr int CFM_CHUNK = 2048;  // elements of one utterance per workgroup of the loss pass: 2 vectors per lane; 8 utterances of
                                        // 1024 x 100 make 400 workgroups, more than the device has compute units

// one vector of W consecutive elements starting at element e of the flat array; W = 4: one 16-byte load
template <int W> struct CfmVec;
template <> struct CfmVec<4> {
    typedef f32x4 T;
    static __device__ __forceinline__ T load(const float* p) { return *(const f32x4*)p; }
    static __device__ __forceinline__ void store(float* p, T v) { *(f32x4*)p = v; }
    static __device__ __forceinline__ float get(const T& v, int j) { return v[j]; }
    static __device__ __forceinline__ void set(T& v, int j, float x) { v[j] = x; }
};
template <> struct CfmVec<1> {
    typedef float T;
    static __device__ __forceinline__ T load(const float* p) { return *p; }
    static __device__ __forceinline__ void store(float* p, T v) { *p = v; }
    static __device__ __forceinline__ float get(const T& v, int) { return v; }
    static __device__ __forceinline__ void set(T& v, int, float x) { v = x; }
};

// W = 4 needs mel % 4 == 0: elements e .. e + 3 then share the row e / mel
template <int W>
__global__ __launch_bounds__(CFM_THREADS) void cfm_noise_kernel(int64_t total, int N, int mel, const float* __restrict__ x1,
                                                                const float* __restrict__ x0, const float* __restrict__ time,
                                                                const uint8_t* __restrict__ span, float* __restrict__ phi, float* __restrict__ cond) {
#pragma clang fp contract(off)
    typedef CfmVec<W> V;
    const int64_t stride = (int64_t)gridDim.x * CFM_THREADS * W;
    for (int64_t e = ((int64_t)blockIdx.x * CFM_THREADS + threadIdx.x) * W; e < total; e += stride) {
        const int64_t row = total >> 32 ? e / mel : (int64_t)((uint32_t)e / (uint32_t)mel);  // (a 64-bit division costs several times a 32-bit one)
        const float t = time[(uint32_t)row / (uint32_t)N];  // B * N < 2^31 (cfm_shape_check)
        const float omt = 1.0f - t;
        const bool sp = span[row] != 0;
        const typename V::T a1 = V::load(x1 + e), a0 = V::load(x0 + e);
        typename V::T p, c;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float v1 = V::get(a1, j), v0 = V::get(a0, j);
            const float l = omt * v0;
            const float r = t * v1;
            V::set(p, j, l + r);
            V::set(c, j, sp ? 0.0f : v1);
        }
        V::store(phi + e, p);
        V::store(cond + e, c);
    }
}

// fixed-order sum of one value per thread: the xor butterfly inside each wave, then the waves' totals in wave order
__device__ __forceinline__ double cfm_block_sum(double v, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[wave] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < CFM_THREADS / 64; ++w) s += lds[w];
    __syncthreads();
    return s;
}

// workgroup (b, g): elements [g * CHUNK, (g + 1) * CHUNK) of utterance b -> partials[b * G + g]
template <int W>
__global__ __launch_bounds__(CFM_THREADS) void cfm_loss_partial_kernel(int N, int mel, int G, const float* __restrict__ pred,
                                                                       const float* __restrict__ x1, const float* __restrict__ x0,
                                                                       const uint8_t* __restrict__ span, double* __restrict__ partials) {
#pragma clang fp contract(off)
    typedef CfmVec<W> V;
    __shared__ double lds[CFM_THREADS / 64];
    const int b = blockIdx.x / G, g = blockIdx.x - b * G;
    const int64_t per = (int64_t)N * mel;
    const int64_t start = (int64_t)g * CFM_CHUNK;
    const int64_t end = start + CFM_CHUNK < per ? start + CFM_CHUNK : per;
    const int64_t base = (int64_t)b * per;
    const uint8_t* sp = span + (int64_t)b * N;
    double acc = 0.0;
    for (int64_t e = start + (int64_t)threadIdx.x * W; e < end; e += (int64_t)CFM_THREADS * W) {
        if (!sp[(uint32_t)e / (uint32_t)mel]) continue;  // e < N * mel < 2^31
        const typename V::T p = V::load(pred + base + e), a1 = V::load(x1 + base + e), a0 = V::load(x0 + base + e);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float flow = V::get(a1, j) - V::get(a0, j);
            const float d = V::get(p, j) - flow;
            const float sq = d * d;
            acc += (double)sq;
        }
    }
    const double s = cfm_block_sum(acc, lds);
    if (threadIdx.x == 0) partials[(int64_t)b * G + g] = s;
}

// workgroup b: sums[b] = the utterance's partials added by index, counts[b] = its selected rows x mel
__global__ __launch_bounds__(CFM_THREADS) void cfm_loss_utterance_kernel(int N, int mel, int G, const double* __restrict__ partials,
                                                                         const uint8_t* __restrict__ span, double* __restrict__ sums,
                                                                         int64_t* __restrict__ counts) {
    __shared__ double lds[CFM_THREADS / 64];
    __shared__ int rows_lds[CFM_THREADS / 64];
    const int b = blockIdx.x;
    double acc = 0.0;
    for (int g = threadIdx.x; g < G; g += CFM_THREADS) acc += partials[(int64_t)b * G + g];
    const double s = cfm_block_sum(acc, lds);
    int rows = 0;
    for (int n = threadIdx.x; n < N; n += CFM_THREADS) rows += span[(int64_t)b * N + n] != 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rows += __shfl_xor(rows, o, 64);
    if ((threadIdx.x & 63) == 0) rows_lds[threadIdx.x >> 6] = rows;
    __syncthreads();
    if (threadIdx.x == 0) {
        int r = 0;
        for (int w = 0; w < CFM_THREADS / 64; ++w) r += rows_lds[w];
        sums[b] = s;
        counts[b] = (int64_t)r * mel;
    }
}

// loss = float(sum_b sums / sum_b counts), the utterances in order; nothing selected: 0 / 0 = NaN, the mean of an empty tensor
__global__ void cfm_loss_final_kernel(int B, const double* __restrict__ sums, const int64_t* __restrict__ counts, float* __restrict__ loss) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    int64_t c = 0;
    for (int b = 0; b < B; ++b) {
        s += sums[b];
        c += counts[b];
    }
    *loss = (float)(s / (double)c);
}

static int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
static bool cfm_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int cfm_shape_check(int B, int N, int mel) {
    if (B < 1 || N < 1 || mel < 1) return f5_fail(F5_EINVAL, "cfm: B = %d, N = %d, mel = %d must all be at least 1", B, N, mel);
    const int64_t per = (int64_t)N * mel;
    if (per >= ((int64_t)1 << 31) || (int64_t)B * N >= ((int64_t)1 << 31) || (int64_t)B * cdiv64(per, CFM_CHUNK) >= ((int64_t)1 << 31))
        return f5_fail(F5_EINVAL, "cfm: B = %d, N = %d, mel = %d is beyond the launch grid", B, N, mel);
    return 0;
}

extern "C" int f5_cfm_noise(int B, int N, int mel, const float* x1, const float* x0, const float* time, const uint8_t* span, float* phi,
                            float* cond, f5_stream_t stream) {
    F5_TRY(cfm_shape_check(B, N, mel));
    if (!x1 || !x0 || !time || !span || !phi || !cond) return f5_fail(F5_EINVAL, "f5_cfm_noise: null argument");
    F5_TRY(f5_check_device());
    const int64_t total = (int64_t)B * N * mel;
    const bool vec = mel % 4 == 0 && cfm_aligned16(x1) && cfm_aligned16(x0) && cfm_aligned16(phi) && cfm_aligned16(cond);
    const int64_t items = vec ? total / 4 : total;
    const int64_t want = (items + CFM_THREADS - 1) / CFM_THREADS;
    const int grid = (int)(want < 8192 ? want : 8192);  // grid-stride beyond: 32 workgroups per compute unit keep every lane's loads in flight
    if (vec)
        hipLaunchKernelGGL(cfm_noise_kernel<4>, dim3(grid), dim3(CFM_THREADS), 0, (hipStream_t)stream, total, N, mel, x1, x0, time, span, phi, cond);
    else
        hipLaunchKernelGGL(cfm_noise_kernel<1>, dim3(grid), dim3(CFM_THREADS), 0, (hipStream_t)stream, total, N, mel, x1, x0, time, span, phi, cond);
    F5_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t f5_cfm_loss_workspace(int B, int N, int mel) {
    const int rc = cfm_shape_check(B, N, mel);
    if (rc != 0) return rc;
    return (int64_t)B * cdiv64((int64_t)N * mel, CFM_CHUNK) * (int64_t)sizeof(double);
}

extern "C" int f5_cfm_loss(int B, int N, int mel, const float* pred, const float* x1, const float* x0, const uint8_t* span, double* sums,
                           int64_t* counts, float* loss, void* workspace, f5_stream_t stream) {
    F5_TRY(cfm_shape_check(B, N, mel));
    if (!pred || !x1 || !x0 || !span || !sums || !counts || !loss || !workspace) return f5_fail(F5_EINVAL, "f5_cfm_loss: null argument");
    if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)sums & 7) != 0 || ((uintptr_t)counts & 7) != 0)
        return f5_fail(F5_EINVAL, "f5_cfm_loss: workspace, sums and counts must be 8-byte aligned");
    F5_TRY(f5_check_device());
    hipStream_t st = (hipStream_t)stream;
    const int G = (int)cdiv64((int64_t)N * mel, CFM_CHUNK);
    double* partials = (double*)workspace;
    const bool vec = mel % 4 == 0 && cfm_aligned16(pred) && cfm_aligned16(x1) && cfm_aligned16(x0);
    if (vec)
        hipLaunchKernelGGL(cfm_loss_partial_kernel<4>, dim3(B * G), dim3(CFM_THREADS), 0, st, N, mel, G, pred, x1, x0, span, partials);
    else
        hipLaunchKernelGGL(cfm_loss_partial_kernel<1>, dim3(B * G), dim3(CFM_THREADS), 0, st, N, mel, G, pred, x1, x0, span, partials);
    F5_LAUNCH_CHECK();
    hipLaunchKernelGGL(cfm_loss_utterance_kernel, dim3(B), dim3(CFM_THREADS), 0, st, N, mel, G, partials, span, sums, counts);
    F5_LAUNCH_CHECK();
    hipLaunchKernelGGL(cfm_loss_final_kernel, dim3(1), dim3(64), 0, st, B, sums, counts, loss);
    F5_LAUNCH_CHECK();
    return 0;
}
