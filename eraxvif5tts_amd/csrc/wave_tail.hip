// wave_tail.hip -- the tail of generate() behind the vocoder, on the device: the rms rule (f5tts_wrapper.py:529-531, utils_infer.py:491-492,
// eval_infer_batch.py:190-191), the linear cross-fade of consecutive chunks (utils_infer.py:519-555) and the server's int16 PCM
// (f5tts-fastapi-server.py:246-250), one thread per OUTPUT sample.  Every operation is the one the host path performs, in its order and
// precision, so the result is byte-identical to torch's gain + numpy's cross_fade_concat + pcm16_bytes:
//   gain      (w * rms) in fp32, then / target: an IEEE fp32 divide (torch on CPU tensors), or a multiply by the fp32 reciprocal of target, which is
//             what torch's device kernel does for a host-scalar divisor (gain_div = 0); never fused, never reassociated
//   joint     double(a) * w_down[j] + double(b) * w_up[j]: two fp64 products and one fp64 sum, no FMA (contraction is off in this file's kernel);
//             w_down / w_up are numpy's own linspace values, uploaded by the caller
//   PCM       trunc(x * 32767): the product in fp64 when a joint mixed (np.concatenate promoted the whole array), else in fp32; products outside
//             int16 saturate (numpy leaves that cast undefined)
// Segments (f5_wave_finish_segments, a script in several voices): the joint before utterance k mixes nj[k] samples -- the cross-fade length where k
// continues a segment, 0 where it begins one (np.concatenate of the segments: no table read, no left operand) -- and with a device rms vector every
// utterance takes its own voice's entry, the joint's left operand that of utterance k - 1.  The entry points without segments fill the same table
// with one segment and entry 0, so there is one kernel for both.  pcm32[k] (a segment of one utterance only): that utterance's PCM product stays
// fp32 inside a float64 result -- the int16 a call over this utterance alone gives.
#include "kernels.h"

__device__ __forceinline__ float wave_gain(float w, float g, bool apply, float target, float inv_target, int gain_div) {
#pragma clang fp contract(off)
    if (!apply) return w;
    const float m = w * g;
    return gain_div ? m / target : m * inv_target;
}

__device__ __forceinline__ int16_t pcm_sat(double p) {  // truncation toward zero inside int16, saturation outside, NaN -> 0
    if (p >= 32767.0) return (int16_t)32767;
    if (p <= -32768.0) return (int16_t)-32768;
    return p == p ? (int16_t)(int)p : (int16_t)0;
}

template <bool F64>
__global__ __launch_bounds__(256) void wave_finish_kernel(const float* __restrict__ wave, const WaveTable tb, int first, int pos0, int pos_end,
                                                          const double* __restrict__ w_down, const double* __restrict__ w_up,
                                                          const float* __restrict__ rms_dev, float target, float inv_target, int gain_div,
                                                          float* __restrict__ out_f32, double* __restrict__ out_f64, int16_t* __restrict__ out_pcm) {
#pragma clang fp contract(off)
    const int pos = pos0 + blockIdx.x * 256 + threadIdx.x;
    if (pos >= pos_end) return;
    int lo = first, hi = tb.cnt - 1;
    while (lo < hi) {  // last utterance whose first output sample is at or before pos
        const int mid = (lo + hi + 1) >> 1;
        if (tb.out0[mid] <= pos) lo = mid; else hi = mid - 1;
    }
    const int k = lo, j = pos - tb.out0[k];
    float gk = tb.gain[k];
    bool ak = tb.apply[k] != 0;
    if (rms_dev) {  // the decision is taken here, so the host never waits for the prompts' rms
        gk = rms_dev[tb.ridx[k]];
        ak = gk < target;
    }
    const float b = wave_gain(wave[(size_t)tb.in0[k] + j], gk, ak, target, inv_target, gain_div);
    if constexpr (F64) {
        double v = (double)b;
        const int n = k > 0 ? tb.nj[k] : 0;
        if (j < n) {
            float gp = tb.gain[k - 1];
            bool ap = tb.apply[k - 1] != 0;
            if (rms_dev) {  // the left operand is utterance k-1's: its own voice's rms
                gp = rms_dev[tb.ridx[k - 1]];
                ap = gp < target;
            }
            const float a = wave_gain(wave[(size_t)tb.in0[k - 1] + tb.len[k - 1] - n + j], gp, ap, target, inv_target, gain_div);
            const double pa = (double)a * w_down[j], pb = (double)b * w_up[j];
            v = pa + pb;
        }
        if (out_f64) out_f64[pos] = v;
        if (out_pcm) out_pcm[pos] = tb.pcm32[k] ? pcm_sat((double)(b * 32767.0f)) : pcm_sat(v * 32767.0);  // (pcm32: never a mixed sample)
    } else {
        if (out_f32) out_f32[pos] = b;
        if (out_pcm) out_pcm[pos] = pcm_sat((double)(b * 32767.0f));
    }
}

int launch_wave_finish(const float* wave, const WaveTable& tb, int first, int pos0, int pos_end, const double* w_down, const double* w_up,
                       const float* rms_dev, float target, int gain_div, bool f64, float* out_f32, double* out_f64, int16_t* out_pcm, hipStream_t stream) {
    if (pos_end <= pos0 || tb.cnt <= 0) return 0;
    const dim3 grid(cdiv(pos_end - pos0, 256));
    const float inv_target = 1.0f / target;
    if (f64)
        hipLaunchKernelGGL(wave_finish_kernel<true>, grid, dim3(256), 0, stream, wave, tb, first, pos0, pos_end, w_down, w_up, rms_dev, target, inv_target,
                           gain_div, out_f32, out_f64, out_pcm);
    else
        hipLaunchKernelGGL(wave_finish_kernel<false>, grid, dim3(256), 0, stream, wave, tb, first, pos0, pos_end, w_down, w_up, rms_dev, target, inv_target,
                           gain_div, out_f32, out_f64, out_pcm);
    F5_LAUNCH_CHECK();
    return 0;
}

// The same tail, one push of a stream at a time (f5_wave_stream_push): positions are those of THIS push's output.  Utterance 0 of the push (table
// with first = 0) joins the session's carry -- the previous push's last n samples, stored with their gain applied, fp32 as wave_gain gives them,
// so the joint's left operand has the bits the one-shot kernel reads from its wave buffer -- where it continues a segment (nj[0] > 0: carry_in is
// given); the threads behind pos_end (carry_out given: the next push's first utterance continues this one's segment) store the last n_carry samples
// of the table's last utterance into the OTHER carry buffer for that push.
template <bool F64>
__global__ __launch_bounds__(256) void wave_stream_kernel(const float* __restrict__ wave, const WaveTable tb, int first, int pos0, int pos_end, int n_carry,
                                                          const double* __restrict__ w_down, const double* __restrict__ w_up,
                                                          const float* __restrict__ rms_dev, float target, float inv_target, int gain_div,
                                                          const float* __restrict__ carry_in, float* __restrict__ carry_out,
                                                          float* __restrict__ out_f32, double* __restrict__ out_f64, int16_t* __restrict__ out_pcm) {
#pragma clang fp contract(off)
    const int pos = pos0 + blockIdx.x * 256 + threadIdx.x;
    if (pos >= pos_end + (carry_out ? n_carry : 0)) return;
    const bool dev = rms_dev != nullptr;
    if (pos >= pos_end) {  // the carry of the next push
        const int kl = tb.cnt - 1, j = pos - pos_end;
        const float gl = dev ? rms_dev[tb.ridx[kl]] : tb.gain[kl];
        carry_out[j] = wave_gain(wave[(size_t)tb.in0[kl] + tb.len[kl] - n_carry + j], gl, dev ? gl < target : tb.apply[kl] != 0, target, inv_target,
                                 gain_div);
        return;
    }
    int lo = first, hi = tb.cnt - 1;
    while (lo < hi) {  // last utterance whose first output sample is at or before pos
        const int mid = (lo + hi + 1) >> 1;
        if (tb.out0[mid] <= pos) lo = mid; else hi = mid - 1;
    }
    const int k = lo, j = pos - tb.out0[k];
    const float gk = dev ? rms_dev[tb.ridx[k]] : tb.gain[k];
    const float b = wave_gain(wave[(size_t)tb.in0[k] + j], gk, dev ? gk < target : tb.apply[k] != 0, target, inv_target, gain_div);
    if constexpr (F64) {
        double v = (double)b;
        const int n = (k > 0 || carry_in) ? tb.nj[k] : 0;
        if (j < n) {
            float a;
            if (k > 0) {
                const float gp = dev ? rms_dev[tb.ridx[k - 1]] : tb.gain[k - 1];
                a = wave_gain(wave[(size_t)tb.in0[k - 1] + tb.len[k - 1] - n + j], gp, dev ? gp < target : tb.apply[k - 1] != 0, target, inv_target,
                              gain_div);
            } else {
                a = carry_in[j];
            }
            const double pa = (double)a * w_down[j], pb = (double)b * w_up[j];
            v = pa + pb;
        }
        if (out_f64) out_f64[pos] = v;
        if (out_pcm) out_pcm[pos] = tb.pcm32[k] ? pcm_sat((double)(b * 32767.0f)) : pcm_sat(v * 32767.0);  // (pcm32: never a mixed sample)
    } else {
        if (out_f32) out_f32[pos] = b;
        if (out_pcm) out_pcm[pos] = pcm_sat((double)(b * 32767.0f));
    }
}

int launch_wave_stream(const float* wave, const WaveTable& tb, int first, int pos0, int pos_end, int n_carry, const double* w_down, const double* w_up,
                       const float* rms_dev, float target, int gain_div, bool f64, const float* carry_in, float* carry_out, float* out_f32,
                       double* out_f64, int16_t* out_pcm, hipStream_t stream) {
    const int count = pos_end - pos0 + (carry_out ? n_carry : 0);
    if (count <= 0 || tb.cnt <= 0) return 0;
    const dim3 grid(cdiv(count, 256));
    const float inv_target = 1.0f / target;
    if (f64)
        hipLaunchKernelGGL(wave_stream_kernel<true>, grid, dim3(256), 0, stream, wave, tb, first, pos0, pos_end, n_carry, w_down, w_up, rms_dev, target,
                           inv_target, gain_div, carry_in, carry_out, out_f32, out_f64, out_pcm);
    else
        hipLaunchKernelGGL(wave_stream_kernel<false>, grid, dim3(256), 0, stream, wave, tb, first, pos0, pos_end, n_carry, w_down, w_up, rms_dev, target,
                           inv_target, gain_div, carry_in, carry_out, out_f32, out_f64, out_pcm);
    F5_LAUNCH_CHECK();
    return 0;
}
