// wave_tail.hip -- the tail of generate() behind the vocoder, on the device: the rms rule (f5tts_wrapper.py:529-531, utils_infer.py:491-492,
// eval_infer_batch.py:190-191), the linear cross-fade of consecutive chunks (utils_infer.py:519-555) and the server's int16 PCM
// (f5tts-fastapi-server.py:246-250), one thread per OUTPUT sample; the kernel, and behind it the f5_wave_finish* / f5_wave_stream_* entry points.  Every operation is the one the host path performs, in its order and
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
#include <vector>

#include "kernels.h"
#include "pcm_rule.h"
#include "runtime.h"

__device__ __forceinline__ float wave_gain(float w, float g, bool apply, float target, float inv_target, int gain_div) {
#pragma clang fp contract(off)
    if (!apply) return w;
    const float m = w * g;
    return gain_div ? m / target : m * inv_target;
}

// One kernel for a whole list (f5_wave_finish*) and for one push of a stream (f5_wave_stream_push); positions are those of THIS call's output.  In
// a push, utterance 0 (table with first = 0) joins the session's carry -- the previous push's last n samples, stored with their gain applied, fp32
// as wave_gain gives them, so the joint's left operand has the bits a one-shot call reads from its wave buffer -- where it continues a segment
// (nj[0] > 0: carry_in is given); the threads behind pos_end (carry_out given: the next push's first utterance continues this one's segment) store
// the last n_carry samples of the table's last utterance into the OTHER carry buffer for that push.  A one-shot call is the push that holds the
// whole list: no carry either way, n_carry = 0.
template <bool F64>
__global__ __launch_bounds__(256) void wave_tail_kernel(const float* __restrict__ wave, const WaveTable tb, int first, int pos0, int pos_end, int n_carry,
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

int launch_wave_tail(const float* wave, const WaveTable& tb, int first, int pos0, int pos_end, int n_carry, const double* w_down, const double* w_up,
                     const float* rms_dev, float target, int gain_div, bool f64, const float* carry_in, float* carry_out, float* out_f32,
                     double* out_f64, int16_t* out_pcm, hipStream_t stream) {
    const int count = pos_end - pos0 + (carry_out ? n_carry : 0);
    if (count <= 0 || tb.cnt <= 0) return 0;
    const dim3 grid(cdiv(count, 256));
    const float inv_target = 1.0f / target;
    if (f64)
        hipLaunchKernelGGL(wave_tail_kernel<true>, grid, dim3(256), 0, stream, wave, tb, first, pos0, pos_end, n_carry, w_down, w_up, rms_dev, target,
                           inv_target, gain_div, carry_in, carry_out, out_f32, out_f64, out_pcm);
    else
        hipLaunchKernelGGL(wave_tail_kernel<false>, grid, dim3(256), 0, stream, wave, tb, first, pos0, pos_end, n_carry, w_down, w_up, rms_dev, target,
                           inv_target, gain_div, carry_in, carry_out, out_f32, out_f64, out_pcm);
    F5_LAUNCH_CHECK();
    return 0;
}

// ---- host side (see f5hip.h).  Only lists whose joints do not chain are taken: inside a segment the first and the last utterance hold at least
// n = xfade_samples samples and every one between them 2 n, so that each joint mixes n untouched samples of either side (cross_fade_concat then takes
// n = xfade_samples at every joint of the segment).  Shorter utterances make the reference mix an already mixed region in sequence: F5_ENOTSUP, the
// caller takes the host functions.  Segments are joined without a fade (np.concatenate), so a one-utterance segment has no constraint.
// A one-shot call is a stream whose single push holds the whole list and carries nothing: both routes describe the list once (TailList), lay the
// utterances of a call out with tail_layout and enqueue them with tail_launch.
namespace {
struct TailList {  // the WHOLE utterance list; whether the signal is float64 is decided here, so every push of a stream answers in one dtype
    int total = 0, n = 0;
    bool f64 = false;  // a mixed joint is float64 and np.concatenate promotes the whole signal
    const double *w_down = nullptr, *w_up = nullptr;
    const float* rms_dev = nullptr;
    float target = 0.f;
    int gain_div = 0;
    const uint8_t* seg_start = nullptr;  // [total] host arrays, each may be null: one segment / rms entry 0 / no flag
    const int32_t* rms_index = nullptr;
    const uint8_t* pcm32 = nullptr;
};

struct TailLayout {  // utterances done .. done + B - 1 of a list: input offset, output position and joint length of each
    std::vector<int> vin, vout, vn;
    int64_t in0 = 0, emitted = 0;  // input samples of the call; output samples it makes final
    bool carries = false;          // the next utterance continues this call's last segment: its last n samples are held back
};

inline bool continues_segment(const uint8_t* seg_start, int g) { return g > 0 && !(seg_start && seg_start[g]); }

// samples utterance g of a list of `total` must hold: n per joint it takes part in
inline int chain_need(int total, const uint8_t* seg_start, int g, int n) {
    return n * ((continues_segment(seg_start, g) ? 1 : 0) + ((g + 1 < total && continues_segment(seg_start, g + 1)) ? 1 : 0));
}

// What create and the one-shot call judge alike, and the list they then work from.  pcm_f32[g] asks for the fp32 PCM product of a call over
// utterance g alone: only an utterance that is a segment of its own mixes nothing.  n is xfade_samples when some utterance continues a segment.
int tail_list(int total, const uint8_t* seg_start, int xfade_samples, const double* w_down, const double* w_up, const float* rms_dev, int n_rms,
              const int32_t* rms_index, float target_rms, int gain_div, const uint8_t* pcm_f32, TailList& L) {
    if (rms_dev && n_rms < 1) return f5_fail(F5_EINVAL, "rms_dev needs n_rms >= 1 values");
    for (int g = 0; rms_dev && rms_index && g < total; ++g)
        if (rms_index[g] < 0 || rms_index[g] >= n_rms)
            return f5_fail(F5_EINVAL, "utterance %d: rms_index %d outside the %d rms values", g, rms_index[g], n_rms);
    for (int g = 0; pcm_f32 && g < total; ++g)
        if (pcm_f32[g] && chain_need(total, seg_start, g, 1) > 0) return f5_fail(F5_EINVAL, "utterance %d: pcm_f32 is for a segment of one utterance", g);
    F5_TRY(f5_check_device());
    int n = 0;
    for (int g = 1; g < total && xfade_samples > 0 && n == 0; ++g)
        if (continues_segment(seg_start, g)) n = xfade_samples;
    if (n > 0 && (!w_down || !w_up)) return f5_fail(F5_EINVAL, "a cross-fade needs the w_down / w_up tables");
    L = TailList{total, n, n > 0, w_down, w_up, rms_dev, target_rms, gain_div, seg_start, rms_dev ? rms_index : nullptr, pcm_f32};
    return 0;
}

// The B utterances behind the `done` first ones of the list, `in_before` input samples taken by earlier calls.  The joint with what came before
// (a stream's carry) lands on the call's first samples and nothing is taken back for it; with done = 0 there is none (vn[0] = 0).
int tail_layout(const TailList& L, int done, int B, const int32_t* samples_host, int64_t in_before, TailLayout& o) {
    const int n = L.n;
    int64_t in0 = 0, out0 = 0;
    o.vin.resize(B);
    o.vout.resize(B);
    o.vn.resize(B);
    for (int u = 0; u < B; ++u) {
        const int len = samples_host[u], g = done + u;
        if (len <= 0) return f5_fail(F5_EINVAL, "utterance %d: no samples", g);
        if (len < chain_need(L.total, L.seg_start, g, n))
            return f5_fail(F5_ENOTSUP, "utterance %d (%d samples) is shorter than its cross-fades (%d samples each): the joints chain", g, len, n);
        o.vn[u] = continues_segment(L.seg_start, g) ? n : 0;
        if (u > 0) out0 -= o.vn[u];
        o.vin[u] = (int)in0;
        o.vout[u] = (int)out0;
        in0 += len;
        out0 += len;
        if (in_before + in0 >= (int64_t)1 << 31) return f5_fail(F5_EINVAL, "more than 2^31 samples");  // (input samples of the whole list)
    }
    o.carries = n > 0 && done + B < L.total && continues_segment(L.seg_start, done + B);
    if (o.carries) out0 -= n;
    o.in0 = in0;
    o.emitted = out0;
    return 0;
}

// Tables of MAXU utterances that overlap by one: a joint needs its left neighbour.  carry_in goes to the first table, carry_out to the last.
int tail_launch(const TailList& L, int done, int B, const TailLayout& o, const float* wave, const int32_t* samples_host, const float* gain_host,
                const uint8_t* apply_host, const float* carry_in, float* carry_out, float* out_f32, double* out_f64, int16_t* out_pcm16,
                hipStream_t st) {
    for (int a = 0; a < B; a += WaveTable::MAXU - 1) {
        WaveTable tb;
        const int b = a + WaveTable::MAXU < B ? a + WaveTable::MAXU : B;
        tb.cnt = b - a;
        for (int k = a; k < b; ++k) {
            tb.in0[k - a] = o.vin[k];
            tb.len[k - a] = samples_host[k];
            tb.out0[k - a] = o.vout[k];
            tb.nj[k - a] = o.vn[k];
            tb.ridx[k - a] = L.rms_index ? L.rms_index[done + k] : 0;
            tb.gain[k - a] = gain_host ? gain_host[k] : 0.f;
            tb.apply[k - a] = gain_host ? (apply_host[k] != 0) : 0;
            tb.pcm32[k - a] = (L.pcm32 && L.pcm32[done + k]) ? 1 : 0;
        }
        const int first = a == 0 ? 0 : 1;
        if (first >= tb.cnt) break;
        const int pos0 = o.vout[a + first], pos_end = b < B ? o.vout[b] : (int)o.emitted;
        F5_TRY(launch_wave_tail(wave, tb, first, pos0, pos_end, carry_out ? L.n : 0, L.w_down, L.w_up, L.rms_dev, L.target, L.gain_div, L.f64,
                                a == 0 ? carry_in : nullptr, b == B ? carry_out : nullptr, out_f32, out_f64, out_pcm16, st));
        if (b == B) break;
    }
    return 0;
}
}  // namespace

extern "C" int f5_wave_finish_segments(int B, const float* wave, const int32_t* samples_host, const uint8_t* seg_start_host, const float* gain_host,
                                       const uint8_t* apply_host, const float* rms_dev, int n_rms, const int32_t* rms_index_host, float target_rms,
                                       int gain_div, int xfade_samples, const double* w_down, const double* w_up, const uint8_t* pcm_f32_host,
                                       float* out_f32, double* out_f64, int16_t* out_pcm16, int64_t* total_samples_out, f5_stream_t stream) {
    if (!wave || !samples_host || B <= 0) return f5_fail(F5_EINVAL, "null argument or B <= 0");
    if (gain_host && !apply_host) return f5_fail(F5_EINVAL, "gain_host needs apply_host");
    if (gain_host && rms_dev) return f5_fail(F5_EINVAL, "give the rms either as host gains or as device values");
    if ((gain_host || rms_dev) && !(target_rms > 0.f)) return f5_fail(F5_EINVAL, "target_rms must be positive");
    TailList L;
    F5_TRY(tail_list(B, seg_start_host, xfade_samples, w_down, w_up, rms_dev, n_rms, rms_index_host, target_rms, gain_div, pcm_f32_host, L));
    TailLayout o;
    F5_TRY(tail_layout(L, 0, B, samples_host, 0, o));
    if (total_samples_out) *total_samples_out = o.emitted;
    // (the extents are judged first: a caller may ask "can you take this call" before it allocates the outputs)
    if (L.f64 ? out_f32 != nullptr : out_f64 != nullptr)
        return f5_fail(F5_EINVAL, "the float result is float64 exactly when a joint mixed (out_f32 / out_f64)");
    if (!out_f32 && !out_f64 && !out_pcm16) return f5_fail(F5_EINVAL, "no output");
    return tail_launch(L, 0, B, o, wave, samples_host, gain_host, apply_host, nullptr, nullptr, out_f32, out_f64, out_pcm16, (hipStream_t)stream);
}

extern "C" int f5_wave_finish(int B, const float* wave, const int32_t* samples_host, const float* gain_host, const uint8_t* apply_host,
                              const float* rms_dev, float target_rms, int gain_div, int xfade_samples, const double* w_down, const double* w_up,
                              float* out_f32, double* out_f64, int16_t* out_pcm16, int64_t* total_samples_out, f5_stream_t stream) {
    return f5_wave_finish_segments(B, wave, samples_host, nullptr, gain_host, apply_host, rms_dev, 1, nullptr, target_rms, gain_div, xfade_samples,
                                   w_down, w_up, nullptr, out_f32, out_f64, out_pcm16, total_samples_out, stream);
}

// ---- the same list in consecutive pushes.  The session owns the list's host arrays and what one call's wave buffer held for the next joint: the
// last n samples of the utterance to the left, with their gain applied, in one of two buffers used in alternation (a push reads one and writes the
// other in the same launch).  A push whose last utterance ends a segment carries nothing, and the next push's first utterance reads no carry.
struct f5_wave_stream_s {
    TailList list;  // (its three arrays point into the vectors below)
    std::vector<uint8_t> seg_start, pcm32;
    std::vector<int32_t> rms_index;
    int done = 0, cur = 0;  // utterances taken so far; carry[cur] holds the tail of utterance done - 1
    int64_t in_total = 0;   // input samples taken so far
    float* carry[2] = {nullptr, nullptr};
    DevArena arena;
};

extern "C" int f5_wave_stream_create_segments(int total_utterances, const uint8_t* seg_start_host, int xfade_samples, const double* w_down,
                                              const double* w_up, const float* rms_dev, int n_rms, const int32_t* rms_index_host, float target_rms,
                                              int gain_div, const uint8_t* pcm_f32_host, f5_wave_stream_t* out) {
    if (!out) return f5_fail(F5_EINVAL, "null argument");
    *out = nullptr;
    if (total_utterances <= 0 || xfade_samples < 0) return f5_fail(F5_EINVAL, "need total_utterances >= 1 and xfade_samples >= 0");
    if (rms_dev && !(target_rms > 0.f)) return f5_fail(F5_EINVAL, "target_rms must be positive");
    TailList L;
    F5_TRY(tail_list(total_utterances, seg_start_host, xfade_samples, w_down, w_up, rms_dev, n_rms, rms_index_host, target_rms, gain_div,
                     pcm_f32_host, L));
    f5_wave_stream_s* s = new f5_wave_stream_s();
    s->list = L;
    auto keep = [&](auto& vec, auto*& p) {  // the caller's array, copied: the pushes come later
        if (!p) return;
        vec.assign(p, p + L.total);
        p = vec.data();
    };
    keep(s->seg_start, s->list.seg_start);
    keep(s->rms_index, s->list.rms_index);
    keep(s->pcm32, s->list.pcm32);
    if (L.n > 0) {
        float* both = nullptr;
        const int rc = s->arena.alloc_t(&both, (size_t)2 * L.n);
        if (rc != 0) {
            delete s;
            return rc;
        }
        s->carry[0] = both;
        s->carry[1] = both + L.n;
    }
    *out = s;
    return 0;
}

extern "C" int f5_wave_stream_create(int total_utterances, int xfade_samples, const double* w_down, const double* w_up, const float* rms_dev,
                                     float target_rms, int gain_div, f5_wave_stream_t* out) {
    return f5_wave_stream_create_segments(total_utterances, nullptr, xfade_samples, w_down, w_up, rms_dev, 1, nullptr, target_rms, gain_div, nullptr, out);
}

extern "C" int f5_wave_stream_destroy(f5_wave_stream_t s) {
    delete s;  // (the arena's hipFree waits for the pushes still in flight)
    return 0;
}

extern "C" int f5_wave_stream_push(f5_wave_stream_t s, int B, const float* wave, const int32_t* samples_host, const float* gain_host,
                                   const uint8_t* apply_host, float* out_f32, double* out_f64, int16_t* out_pcm16, int64_t* emitted,
                                   f5_stream_t stream) {
    if (!s || !samples_host || B <= 0) return f5_fail(F5_EINVAL, "null argument or B <= 0");
    const TailList& L = s->list;
    if (B > L.total - s->done) return f5_fail(F5_EINVAL, "%d utterances pushed where %d of the stream's %d are left", B, L.total - s->done, L.total);
    if (gain_host && !apply_host) return f5_fail(F5_EINVAL, "gain_host needs apply_host");
    if (gain_host && L.rms_dev) return f5_fail(F5_EINVAL, "give the rms either as host gains or as device values");
    if (gain_host && !(L.target > 0.f)) return f5_fail(F5_EINVAL, "target_rms must be positive");
    TailLayout o;
    F5_TRY(tail_layout(L, s->done, B, samples_host, s->in_total, o));
    if (emitted) *emitted = o.emitted;
    if (!out_f32 && !out_f64 && !out_pcm16) return 0;  // "how many would this push emit": nothing is enqueued, the session stays as it is
    if (!wave) return f5_fail(F5_EINVAL, "null wave");
    if (L.f64 ? out_f32 != nullptr : out_f64 != nullptr)
        return f5_fail(F5_EINVAL, "the float result is float64 exactly when the stream cross-fades (out_f32 / out_f64)");
    F5_TRY(f5_check_device());
    // the joint with the previous push / with the next one: only inside a segment
    const float* carry_in = o.vn[0] > 0 ? s->carry[s->cur] : nullptr;
    float* carry_out = o.carries ? s->carry[s->cur ^ 1] : nullptr;
    F5_TRY(tail_launch(L, s->done, B, o, wave, samples_host, gain_host, apply_host, carry_in, carry_out, out_f32, out_f64, out_pcm16,
                       (hipStream_t)stream));
    s->done += B;
    s->in_total += o.in0;
    if (carry_out) s->cur ^= 1;
    return 0;
}
