// silence.hip -- "remove silence" on the finished wave, on the device: the reference's remove_silence_for_generated_wav (infer/utils_infer.py:569-578,
// pydub split_on_silence on the exported 16-bit file) by the rule of this project's stand-in, infer/audio.py split_on_silence / detect_nonsilent /
// detect_silence / Segment.slice_ms / Segment.__len__.  Everything is integer arithmetic on the PCM the file would hold, so the result is the host
// functions' bit for bit:
//   PCM     clip(rint(double(x) * 32767.0), -32768, 32767), the product in fp64, rint to even (np.round, libsndfile); NaN counts as 0.  Formed in
//           registers, never stored, and never the truncating streaming PCM
//   cells   millisecond m covers samples [F(m), F(m + 1)), F(m) = min(int(m * (rate / 1000.0)), n_samples): one int64 sum of squares each.  A window
//           [i, i + min_silence_len) is a difference of the cells' prefix sums, whatever its start and whether or not a millisecond is a whole
//           number of samples
//   silent  int(sqrt(S / n)) <= thresh  <=>  S < (R + 1)^2 n with R = floor(thresh): no sqrt, pow or division here (DESIGN.md gives the argument,
//           which needs n < 2^22)
//   ranges  one workgroup: prefix scan, window flags, then one wave walks the flags 64 at a time (a ballot; runs of consecutive silent starts merge
//           by the rule itself), inverts the silent ranges, pads by keep_silence with the midpoint rule and writes the segment table
//           (silence_rule.h, which reference.hip includes too)
//   gather  one thread per output sample and a binary search in the table, as wave_tail_kernel does
// Stores to device memory are plain C++; no atomics: one workgroup owns the table and the counts.
#include <cmath>

#include "kernels.h"
#include "runtime.h"
#include "silence_rule.h"

__device__ __forceinline__ int pcm_rint(double x) {  // what audio.write_wav stores for x
#pragma clang fp contract(off)
    const double r = __builtin_rint(x * 32767.0);
    if (r >= 32767.0) return 32767;
    if (r <= -32768.0) return -32768;
    return r == r ? (int)r : 0;
}

static constexpr int SIL_TILE = 8192;  // samples staged per pass (uint32 squares: 32 KiB of LDS)

// Cells c0 = blockIdx.x * cells_per_block ...: the block's samples come in with 16-byte loads (scalar ahead of the first aligned address and behind the
// last whole vector), their squares go to LDS, and thread t sums the squares of cell c0 + t.  sums[m + 1] = cell m (sums[0] is the scan's zero).
template <typename T>
__global__ __launch_bounds__(256) void silence_cells_kernel(const T* __restrict__ wave, int64_t n, int64_t n_ms, double spm, int cells_per_block,
                                                            int64_t* __restrict__ sums) {
    constexpr int V = 16 / sizeof(T);
    typedef __attribute__((ext_vector_type(V))) T vec_t;
    __shared__ uint32_t sq[SIL_TILE];
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * cells_per_block;
    const int64_t c1 = c0 + cells_per_block < n_ms ? c0 + cells_per_block : n_ms;
    const int64_t s0 = ms_frame(c0, spm, n), s1 = ms_frame(c1, spm, n);
    const int64_t c = c0 + tid;
    const bool mine = tid < cells_per_block && c < c1;
    const int64_t f0 = mine ? ms_frame(c, spm, n) : 0, f1 = mine ? ms_frame(c + 1, spm, n) : 0;
    int64_t acc = 0;
    for (int64_t ts = s0; ts < s1; ts += SIL_TILE) {
        const int len = (int)(s1 - ts < SIL_TILE ? s1 - ts : SIL_TILE);
        const T* p = wave + ts;
        const int mis = (int)(((uintptr_t)p & 15) / sizeof(T));
        int head = mis ? V - mis : 0;
        if (head > len) head = len;
        const int nvec = (len - head) / V;
        if (tid < head) {
            const int v = pcm_rint((double)p[tid]);
            sq[tid] = (uint32_t)(v * v);
        }
        const vec_t* pv = reinterpret_cast<const vec_t*>(p + head);
        for (int k = tid; k < nvec; k += 256) {
            const vec_t x = pv[k];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int v = pcm_rint((double)x[j]);
                sq[head + k * V + j] = (uint32_t)(v * v);
            }
        }
        const int done = head + nvec * V;
        if (done + tid < len) {  // fewer than V samples
            const int v = pcm_rint((double)p[done + tid]);
            sq[done + tid] = (uint32_t)(v * v);
        }
        __syncthreads();
        const int64_t lo = f0 > ts ? f0 : ts, hi = f1 < ts + len ? f1 : ts + len;
        for (int64_t j = lo; j < hi; ++j) acc += (int64_t)sq[(int)(j - ts)];
        __syncthreads();
    }
    if (mine) sums[c + 1] = acc;
}

// One workgroup: (1) sums[k] becomes the sum of the cells below k, (2) flags[w] = window w is silent, (3) wave 0 turns the flags into the table
// (in_start, in_end, out_start) of the parts split_on_silence returns, in samples, and counts = (kept samples, parts).  (silence_rule.h)
__global__ __launch_bounds__(1024) void silence_ranges_kernel(const SilenceParams q, int64_t* __restrict__ sums, uint8_t* __restrict__ flags,
                                                              int32_t* __restrict__ table, int64_t* __restrict__ counts) {
    __shared__ int64_t part[1024];
    silence_scan(q.n_ms, sums, part);
    silence_flags(q, sums, flags);
    if (threadIdx.x >= 64) return;
    int64_t kept;
    int parts;
    silence_table(q, flags, table, &kept, &parts);
    if (threadIdx.x == 0) {
        counts[0] = kept;
        counts[1] = parts;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void silence_gather_kernel(const T* __restrict__ wave, const int16_t* __restrict__ pcm_in,
                                                             const int32_t* __restrict__ table, const int64_t* __restrict__ counts, int cap,
                                                             T* __restrict__ out_wave, int16_t* __restrict__ out_pcm, int16_t* __restrict__ out_pcm_in) {
    const int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pos >= counts[0]) return;
    int lo = 0, hi = (int)(counts[1] < cap ? counts[1] : cap) - 1;
    while (lo < hi) {  // last part whose first output sample is at or before pos
        const int mid = (lo + hi + 1) >> 1;
        if (table[3 * mid + 2] <= pos) lo = mid; else hi = mid - 1;
    }
    const int64_t src = (int64_t)table[3 * lo] + (pos - table[3 * lo + 2]);
    const T x = wave[src];
    if (out_wave) out_wave[pos] = x;
    if (out_pcm) out_pcm[pos] = (int16_t)pcm_rint((double)x);
    if (out_pcm_in) out_pcm_in[pos] = pcm_in[src];
}

// ---- host side
struct SilencePlan {
    SilenceParams q;
    int cells_per_block;
    size_t off_table, off_flags, bytes;
};

static int silence_plan(const void* wave, int is_f64, int64_t n_samples, int sample_rate, int64_t n_ms, int min_silence_len, int threshold_floor,
                        int keep_silence, int seek_step, bool check_ms, SilencePlan* out) {
    if (n_samples < 0 || n_samples >= (int64_t)1 << 31) return f5_fail(F5_EINVAL, "n_samples = %lld: 0 .. 2^31 - 1", (long long)n_samples);
    if (sample_rate < 1000) return f5_fail(F5_EINVAL, "sample_rate = %d: at least 1000 (a millisecond holds a sample)", sample_rate);
    if (min_silence_len < 1) return f5_fail(F5_EINVAL, "min_silence_len = %d: at least 1", min_silence_len);
    if (seek_step < 1) return f5_fail(F5_EINVAL, "seek_step = %d: at least 1", seek_step);
    if (keep_silence < 0) return f5_fail(F5_EINVAL, "keep_silence = %d: not negative", keep_silence);
    if (threshold_floor < 0) return f5_fail(F5_EINVAL, "threshold_floor = %d: not negative", threshold_floor);
    const double spm = sample_rate / 1000.0;
    if ((double)min_silence_len * spm + 1.0 >= 4194304.0)
        return f5_fail(F5_EINVAL, "min_silence_len = %d at %d Hz: a window of 2^22 samples or more (the integer decision holds below that)",
                       min_silence_len, sample_rate);
    const int64_t want_ms = (int64_t)std::rint(1000.0 * (double)n_samples / (double)sample_rate);  // Python's round(): half to even
    if (check_ms && n_ms != want_ms)
        return f5_fail(F5_EINVAL, "n_ms = %lld: round(1000 * n_samples / sample_rate) is %lld", (long long)n_ms, (long long)want_ms);
    if (!check_ms) n_ms = want_ms;
    if (wave && ((uintptr_t)wave % (is_f64 ? 8 : 4)) != 0) return f5_fail(F5_EINVAL, "wave is not aligned to its element size");
    SilenceParams& q = out->q;
    q.n = n_samples;
    q.n_ms = n_ms;
    q.spm = spm;
    q.L = min_silence_len;
    q.step = seek_step;
    q.keep = keep_silence;
    const int64_t R = threshold_floor < 32768 ? threshold_floor : 32768;  // an rms never exceeds 32768
    q.lim = (R + 1) * (R + 1);
    q.cmul = 1;
    silence_set_windows(q);
    int cpb = (int)(SIL_TILE / (spm + 1.0));
    out->cells_per_block = cpb < 1 ? 1 : (cpb > 256 ? 256 : cpb);
    out->off_table = (size_t)round_up((n_ms + 1) * 8, 16);
    out->off_flags = out->off_table + (size_t)round_up((int64_t)q.cap * 12, 16);
    out->bytes = out->off_flags + (size_t)round_up(q.W > 0 ? q.W : 1, 16);
    return 0;
}

static int silence_decide(const SilencePlan& pl, const void* wave, int is_f64, int64_t* sums, uint8_t* flags, int32_t* table, int64_t* counts,
                          hipStream_t st) {
    const SilenceParams& q = pl.q;
    if (q.n_ms > 0) {
        const dim3 grid((unsigned)((q.n_ms + pl.cells_per_block - 1) / pl.cells_per_block));
        if (is_f64)
            hipLaunchKernelGGL(silence_cells_kernel<double>, grid, dim3(256), 0, st, (const double*)wave, q.n, q.n_ms, q.spm, pl.cells_per_block, sums);
        else
            hipLaunchKernelGGL(silence_cells_kernel<float>, grid, dim3(256), 0, st, (const float*)wave, q.n, q.n_ms, q.spm, pl.cells_per_block, sums);
        F5_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(silence_ranges_kernel, dim3(1), dim3(1024), 0, st, q, sums, flags, table, counts);
    F5_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t f5_wave_remove_silence_workspace(int64_t n_samples, int sample_rate, int min_silence_len, int seek_step) {
    SilencePlan pl;
    const int rc = silence_plan(nullptr, 0, n_samples, sample_rate, 0, min_silence_len, 0, 0, seek_step, false, &pl);
    return rc != 0 ? (int64_t)rc : (int64_t)pl.bytes;
}

extern "C" int f5_op_silence_ranges(const void* wave, int is_f64, int64_t n_samples, int sample_rate, int64_t n_ms, int min_silence_len,
                                    int threshold_floor, int keep_silence, int seek_step, void* workspace, int64_t workspace_bytes,
                                    uint8_t* flags_out, int32_t* table_out, int64_t* counts_dev, f5_stream_t stream) {
    SilencePlan pl;
    F5_TRY(silence_plan(wave, is_f64, n_samples, sample_rate, n_ms, min_silence_len, threshold_floor, keep_silence, seek_step, true, &pl));
    if ((!wave && n_samples > 0) || !workspace || !flags_out || !table_out || !counts_dev) return f5_fail(F5_EINVAL, "null argument");
    if (workspace_bytes < (int64_t)pl.bytes || ((uintptr_t)workspace & 15) != 0)
        return f5_fail(F5_EINVAL, "workspace: %lld bytes given, %lld needed, 16-byte aligned", (long long)workspace_bytes, (long long)pl.bytes);
    F5_TRY(f5_check_device());
    return silence_decide(pl, wave, is_f64, (int64_t*)workspace, flags_out, table_out, counts_dev, (hipStream_t)stream);
}

extern "C" int f5_wave_remove_silence(const void* wave, int is_f64, int64_t n_samples, int sample_rate, int64_t n_ms, int min_silence_len,
                                      int threshold_floor, int keep_silence, int seek_step, const int16_t* pcm_in, void* workspace,
                                      int64_t workspace_bytes, void* out_wave, int16_t* out_pcm16, int16_t* out_pcm_in, int64_t* counts_dev,
                                      f5_stream_t stream) {
    SilencePlan pl;
    F5_TRY(silence_plan(wave, is_f64, n_samples, sample_rate, n_ms, min_silence_len, threshold_floor, keep_silence, seek_step, true, &pl));
    if ((!wave && n_samples > 0) || !workspace || !counts_dev) return f5_fail(F5_EINVAL, "null argument");
    if ((out_pcm_in != nullptr) != (pcm_in != nullptr)) return f5_fail(F5_EINVAL, "pcm_in and out_pcm_in go together");
    if (!out_wave && !out_pcm16 && !out_pcm_in) return f5_fail(F5_EINVAL, "no output");
    if (workspace_bytes < (int64_t)pl.bytes || ((uintptr_t)workspace & 15) != 0)
        return f5_fail(F5_EINVAL, "workspace: %lld bytes given, %lld needed, 16-byte aligned", (long long)workspace_bytes, (long long)pl.bytes);
    F5_TRY(f5_check_device());
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int32_t* table = (int32_t*)(ws + pl.off_table);
    F5_TRY(silence_decide(pl, wave, is_f64, (int64_t*)ws, (uint8_t*)(ws + pl.off_flags), table, counts_dev, st));
    const int64_t end_ms = (int64_t)((double)pl.q.n_ms * pl.q.spm);
    const int64_t most = end_ms < n_samples ? end_ms : n_samples;  // samples behind int(n_ms * rate / 1000.0) belong to no part
    if (most <= 0) return 0;
    const dim3 grid((unsigned)((most + 255) / 256));
    if (is_f64)
        hipLaunchKernelGGL(silence_gather_kernel<double>, grid, dim3(256), 0, st, (const double*)wave, pcm_in, table, counts_dev, pl.q.cap,
                           (double*)out_wave, out_pcm16, out_pcm_in);
    else
        hipLaunchKernelGGL(silence_gather_kernel<float>, grid, dim3(256), 0, st, (const float*)wave, pcm_in, table, counts_dev, pl.q.cap,
                           (float*)out_wave, out_pcm16, out_pcm_in);
    F5_LAUNCH_CHECK();
    return 0;
}
