// deliver.hip -- the delivery stage behind the wave tail, on the device: the finished 24 kHz signal at another sample rate, as float32, as the
// truncating int16 PCM of the wave tail and as G.711 (mu-law / A-law), one shot (f5_wave_convert) or in pushes (f5_wave_convert_stream_*) whose
// pieces, concatenated, are the one-shot bytes.  The arithmetic is fixed so that this holds for every way of cutting the signal:
//   resample  torchaudio's sinc_interp_hann polyphase sum (lowpass_filter_width 6, rolloff 0.99; the definition of f5_frontend_resample and
//             oracle/cpu_ref.resample): g = gcd(in, out), orig = in / g, nw = out / g, width = ceil(6 orig / (0.99 min(orig, nw))),
//             kw = 2 width + orig; output j = blk * nw + ph is sum_k taps[ph][k] * x[blk * orig - width + k], k = 0 .. kw - 1.  The taps are the
//             CALLER's doubles [nw][kw]; x is widened to fp64, every product is fp64, ONE fp64 accumulator starts at 0.0 and takes the products in
//             ascending k, multiply and add are never contracted (the build has -ffp-contract=off, and the pragma below says so again), and a tap
//             whose sample lies outside the signal is skipped, never added as zero
//   float     (float)acc
//   PCM       trunc(float * 32767.0f), the product in fp32, saturating outside int16, NaN -> 0: the wave tail's rule
//   G.711     the ITU-T tables as CPython's audioop.lin2ulaw / lin2alaw give them for 16-bit input, in closed form with an integer count of
//             leading zeros (deliver_g711 below; include/f5hip.h states both forms)
// One workgroup of 256 threads computes 256 consecutive outputs.  The input span they read is staged once in LDS as fp64 where it fits
// (DLV_SPAN doubles: every ratio of the common audio rates does), and is read from memory otherwise: the same values in the same order either way.
// In a push the span may begin in the session's carry (the input samples later blocks still need: fewer than kw, held as fp64) and continue in the
// caller's buffer; absolute sample positions address both, so the kernel is the one-shot kernel.
#include <cmath>
#include <numeric>

#include "kernels.h"
#include "pcm_rule.h"
#include "runtime.h"

static constexpr int DLV_SPAN = 4096;                    // doubles of LDS per workgroup (32 KiB)
static constexpr int64_t DLV_MAX_TAPS = (int64_t)1 << 20;  // nw * kw: the table a caller may hand over

__device__ __forceinline__ uint8_t deliver_g711(int s, int law) {
    if (law == 0) {  // mu-law
        const int v = s >> 2;
        const int a = v < 0 ? -v : v;
        const int m = a < 8158 ? a + 33 : 8191;  // (audioop answers its top code for everything from 8158 up)
        const int seg = 26 - __clz(m);           // floor(log2 m) - 5, m in 33 .. 8191
        const int code = (seg << 4) | ((m >> (seg + 1)) & 15);
        return (uint8_t)(code ^ (v < 0 ? 0x7F : 0xFF));
    }
    const int v = s >> 3;
    const int m = v >= 0 ? v : -v - 1;
    const int seg = m < 32 ? 0 : 27 - __clz(m);  // floor(log2 m) - 4, m in 32 .. 4095
    const int code = (seg << 4) | ((seg < 2 ? m >> 1 : m >> seg) & 15);
    return (uint8_t)(code ^ (v < 0 ? 0x55 : 0xD5));
}

__global__ __launch_bounds__(256) void deliver_g711_kernel(const int16_t* __restrict__ pcm, int64_t n, int law, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = deliver_g711((int)pcm[i], law);
}

struct DeliverSource {  // the signal by absolute position: [c0, p) in the carry (fp64), [p, n_end) in the caller's buffer
    const void* wave;
    const double* carry;
    int64_t c0, p, n_end;
};

template <typename T>
__device__ __forceinline__ double deliver_sample(const DeliverSource& s, int64_t idx) {
    return idx >= s.p ? (double)((const T*)s.wave)[idx - s.p] : s.carry[idx - s.c0];
}

// outputs j0 .. j0 + count - 1 (absolute positions of the whole signal's result) -> out_*[j - j0]
template <typename T>
__global__ __launch_bounds__(256) void deliver_convert_kernel(const DeliverSource src, int orig, int nw, int width, int kw,
                                                              const double* __restrict__ taps, int64_t j0, int64_t count, int law,
                                                              float* __restrict__ out_f32, int16_t* __restrict__ out_pcm,
                                                              uint8_t* __restrict__ out_g711) {
#pragma clang fp contract(off)
    __shared__ double xs[DLV_SPAN];
    const int64_t rel0 = (int64_t)blockIdx.x * 256;
    const int64_t rel1 = rel0 + 255 < count - 1 ? rel0 + 255 : count - 1;  // this workgroup's last output
    int64_t lo = (j0 + rel0) / nw * orig - width, hi = (j0 + rel1) / nw * orig - width + kw;
    if (lo < src.c0) lo = src.c0;  // (positions before c0 are negative, or belong to blocks that are out already)
    if (hi > src.n_end) hi = src.n_end;
    const bool staged = hi - lo <= DLV_SPAN;  // uniform over the workgroup
    if (staged) {
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256) xs[i - lo] = deliver_sample<T>(src, i);
        __syncthreads();
    }
    const int64_t rel = rel0 + threadIdx.x;
    if (rel >= count) return;
    const int64_t j = j0 + rel, blk = j / nw;
    const int ph = (int)(j - blk * nw);
    const int64_t first = blk * orig - width;  // the sample tap 0 meets
    const int k_lo = first < 0 ? (int)-first : 0;
    const int k_hi = src.n_end - first < kw ? (int)(src.n_end - first) : kw;
    const double* h = taps + (size_t)ph * kw;
    double acc = 0.0;
    if (staged) {
        const double* x = xs + (first - lo);
        for (int k = k_lo; k < k_hi; ++k) {
            const double prod = x[k] * h[k];
            acc = acc + prod;
        }
    } else {
        for (int k = k_lo; k < k_hi; ++k) {
            const double prod = deliver_sample<T>(src, first + k) * h[k];
            acc = acc + prod;
        }
    }
    const float f = (float)acc;
    if (out_f32) out_f32[rel] = f;
    if (out_pcm || out_g711) {
        const int16_t s = pcm_sat((double)(f * 32767.0f));  // (the product in fp32)
        if (out_pcm) out_pcm[rel] = s;
        if (out_g711) out_g711[rel] = deliver_g711((int)s, law);
    }
}

// the session's next carry: samples [c0_new, n_end) of the signal, from the old carry and this push's buffer
template <typename T>
__global__ __launch_bounds__(256) void deliver_carry_kernel(const DeliverSource src, int64_t c0_new, int count, double* __restrict__ carry_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) carry_out[i] = deliver_sample<T>(src, c0_new + i);
}

// ---- host side
struct DeliverRates {
    int orig = 0, nw = 0, width = 0, kw = 0;
};

static int deliver_rates(int in_rate, int out_rate, DeliverRates* r) {
    if (in_rate <= 0 || out_rate <= 0) return f5_fail(F5_EINVAL, "in_rate = %d, out_rate = %d: both positive", in_rate, out_rate);
    if (in_rate == out_rate) return f5_fail(F5_EINVAL, "in_rate == out_rate = %d: nothing to resample (the caller keeps its signal)", in_rate);
    const int g = std::gcd(in_rate, out_rate);
    r->orig = in_rate / g;
    r->nw = out_rate / g;
    const double base = (double)(r->orig < r->nw ? r->orig : r->nw) * 0.99;
    const double w = std::ceil(6.0 * (double)r->orig / base);
    const double kw = 2.0 * w + (double)r->orig;
    if (kw * (double)r->nw > (double)DLV_MAX_TAPS)
        return f5_fail(F5_EINVAL, "%d -> %d Hz: a table of %d x %.0f taps is beyond 2^20 entries", in_rate, out_rate, r->nw, kw);
    r->width = (int)w;
    r->kw = (int)kw;
    return 0;
}

static int64_t deliver_target(const DeliverRates& r, int64_t n) { return ((int64_t)r.nw * n + r.orig - 1) / r.orig; }  // ceil(nw n / orig)

static int deliver_check_outputs(const void* taps, int law, const float* out_f32, const uint8_t* out_g711) {
    if (!taps || ((uintptr_t)taps & 7) != 0) return f5_fail(F5_EINVAL, "taps: a device table of doubles [out_rate / g][kw]");
    if (out_g711 && law != 0 && law != 1) return f5_fail(F5_EINVAL, "law = %d: 0 (mu-law) or 1 (A-law)", law);
    if (out_f32 && ((uintptr_t)out_f32 & 3) != 0) return f5_fail(F5_EINVAL, "out_f32 is not aligned");
    return 0;
}

static int deliver_launch(const DeliverSource& src, int is_f64, const DeliverRates& r, const double* taps, int64_t j0, int64_t count, int law,
                          float* out_f32, int16_t* out_pcm16, uint8_t* out_g711, hipStream_t st) {
    if (count <= 0) return 0;
    const dim3 grid((unsigned)((count + 255) / 256));
    if (is_f64)
        hipLaunchKernelGGL(deliver_convert_kernel<double>, grid, dim3(256), 0, st, src, r.orig, r.nw, r.width, r.kw, taps, j0, count, law, out_f32,
                           out_pcm16, out_g711);
    else
        hipLaunchKernelGGL(deliver_convert_kernel<float>, grid, dim3(256), 0, st, src, r.orig, r.nw, r.width, r.kw, taps, j0, count, law, out_f32,
                           out_pcm16, out_g711);
    F5_LAUNCH_CHECK();
    return 0;
}

extern "C" int f5_op_g711_encode(int64_t n, const int16_t* pcm, int law, uint8_t* out, f5_stream_t stream) {
    if (n < 0 || n >= (int64_t)1 << 31) return f5_fail(F5_EINVAL, "n = %lld: 0 .. 2^31 - 1", (long long)n);
    if (law != 0 && law != 1) return f5_fail(F5_EINVAL, "law = %d: 0 (mu-law) or 1 (A-law)", law);
    if (n == 0) return 0;
    if (!pcm || !out || ((uintptr_t)pcm & 1) != 0) return f5_fail(F5_EINVAL, "null or misaligned argument");
    F5_TRY(f5_check_device());
    hipLaunchKernelGGL(deliver_g711_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pcm, n, law, out);
    F5_LAUNCH_CHECK();
    return 0;
}

extern "C" int f5_wave_convert(const void* wave, int is_f64, int64_t n, int in_rate, int out_rate, const double* taps, int law, float* out_f32,
                               int16_t* out_pcm16, uint8_t* out_g711, int64_t* out_samples, f5_stream_t stream) {
    if (n <= 0 || n >= (int64_t)1 << 31) return f5_fail(F5_EINVAL, "n = %lld: 1 .. 2^31 - 1 samples", (long long)n);
    DeliverRates r;
    F5_TRY(deliver_rates(in_rate, out_rate, &r));
    const int64_t target = deliver_target(r, n);
    if (out_samples) *out_samples = target;
    if (!out_f32 && !out_pcm16 && !out_g711) return 0;  // "how many samples": nothing is enqueued
    if (!wave || ((uintptr_t)wave % (is_f64 ? 8 : 4)) != 0) return f5_fail(F5_EINVAL, "wave is null or not aligned to its element size");
    F5_TRY(deliver_check_outputs(taps, law, out_f32, out_g711));
    F5_TRY(f5_check_device());
    const DeliverSource src{wave, nullptr, 0, 0, n};
    return deliver_launch(src, is_f64, r, taps, 0, target, law, out_f32, out_pcm16, out_g711, (hipStream_t)stream);
}

// ---- the same conversion in pushes.  taken = input samples so far, blocks = whole output blocks (nw samples each) handed out so far; the carry
// holds the samples [c0, taken) -- c0 = max(0, blocks * orig - width), what block `blocks` reads first -- in carry[cur]; a push reads it and
// writes the next one into the other buffer.
struct f5_convert_stream_s {
    DeliverRates r;
    const double* taps = nullptr;
    int is_f64 = 0, law = 0, cur = 0;
    bool finished = false;
    int64_t taken = 0, emitted = 0, c0 = 0;
    double* carry[2] = {nullptr, nullptr};
    DevArena arena;
};

extern "C" int f5_wave_convert_stream_create(int in_rate, int out_rate, const double* taps, int is_f64, int law, f5_convert_stream_t* out) {
    if (!out) return f5_fail(F5_EINVAL, "null argument");
    *out = nullptr;
    DeliverRates r;
    F5_TRY(deliver_rates(in_rate, out_rate, &r));
    if (!taps || ((uintptr_t)taps & 7) != 0) return f5_fail(F5_EINVAL, "taps: a device table of doubles [out_rate / g][kw]");
    if (law != 0 && law != 1) return f5_fail(F5_EINVAL, "law = %d: 0 (mu-law) or 1 (A-law)", law);
    F5_TRY(f5_check_device());
    f5_convert_stream_s* s = new f5_convert_stream_s();
    s->r = r;
    s->taps = taps;
    s->is_f64 = is_f64 ? 1 : 0;
    s->law = law;
    double* both = nullptr;
    const int rc = s->arena.alloc_t(&both, (size_t)2 * r.kw);
    if (rc != 0) {
        delete s;
        return rc;
    }
    s->carry[0] = both;
    s->carry[1] = both + r.kw;
    *out = s;
    return 0;
}

extern "C" int f5_wave_convert_stream_destroy(f5_convert_stream_t s) {
    delete s;  // (the arena's hipFree waits for the pushes still in flight)
    return 0;
}

extern "C" int f5_wave_convert_stream_push(f5_convert_stream_t s, const void* wave, int64_t n_k, int last, float* out_f32, int16_t* out_pcm16,
                                           uint8_t* out_g711, int64_t* emitted, f5_stream_t stream) {
    if (!s) return f5_fail(F5_EINVAL, "null session");
    if (s->finished) return f5_fail(F5_EINVAL, "the stream has had its last push");
    if (n_k <= 0) return f5_fail(F5_EINVAL, "n_k = %lld: a push holds at least one sample", (long long)n_k);
    const DeliverRates& r = s->r;
    const int64_t total = s->taken + n_k;
    if (total >= (int64_t)1 << 31) return f5_fail(F5_EINVAL, "more than 2^31 samples");
    // non-final: the blocks whose whole support has arrived; final: everything up to ceil(nw * total / orig)
    const int64_t blocks = total > r.width ? (total - r.width) / r.orig : 0;
    const int64_t upto = last ? deliver_target(r, total) : blocks * r.nw;
    const int64_t count = upto - s->emitted;
    if (emitted) *emitted = count;
    if (!out_f32 && !out_pcm16 && !out_g711) return 0;  // "how many would this push emit": nothing is enqueued, the session stays as it is
    if (!wave || ((uintptr_t)wave % (s->is_f64 ? 8 : 4)) != 0) return f5_fail(F5_EINVAL, "wave is null or not aligned to its element size");
    F5_TRY(deliver_check_outputs(s->taps, s->law, out_f32, out_g711));
    F5_TRY(f5_check_device());
    hipStream_t st = (hipStream_t)stream;
    const DeliverSource src{wave, s->carry[s->cur], s->c0, s->taken, total};
    F5_TRY(deliver_launch(src, s->is_f64, r, s->taps, s->emitted, count, s->law, out_f32, out_pcm16, out_g711, st));
    if (!last) {
        const int64_t c0_new = blocks * r.orig > r.width ? blocks * r.orig - r.width : 0;
        const int keep = (int)(total - c0_new);  // below kw: total - width < (blocks + 1) * orig
        double* next = s->carry[s->cur ^ 1];
        if (s->is_f64)
            hipLaunchKernelGGL(deliver_carry_kernel<double>, dim3(cdiv(keep, 256)), dim3(256), 0, st, src, c0_new, keep, next);
        else
            hipLaunchKernelGGL(deliver_carry_kernel<float>, dim3(cdiv(keep, 256)), dim3(256), 0, st, src, c0_new, keep, next);
        F5_LAUNCH_CHECK();
        s->cur ^= 1;
        s->c0 = c0_new;
    }
    s->taken = total;
    s->emitted = upto;
    s->finished = last != 0;
    return 0;
}
