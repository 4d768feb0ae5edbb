// reference.hip -- the reference-voice front-end on the device: the host steps of F5TTSWrapper._preprocess_voice (the reference's
// f5tts_wrapper.py:256-379 by the rule of this project's stand-in for pydub, infer/audio.py clip_reference / remove_silence_edges / silent_like /
// segment_to_float), on the interleaved 16-bit PCM of the file.  Integer arithmetic up to the float conversion, so every sample is the host's:
//   cells   millisecond m covers frames [F(m), F(m + 1)), F(m) = min(int(m * (rate / 1000.0)), n_frames): one int64 sum of squares over all
//           channels (Segment.rms is over the interleaved samples).  16-byte loads; the cells are scanned once and serve both passes
//   plan    one workgroup: scan, then per pass the window flags and the part table of split_on_silence (silence_rule.h, shared with silence.hip),
//           then thread 0 applies clip_reference's rule: parts are appended until len(out) > soft and len(out + part) > hard; pass 2 runs on the
//           ORIGINAL cells when pass 1 left more than `hard` ms; the final slice_ms(0, hard).  len() = rint(1000 frames / rate), half to even
//   gather  one thread per kept interleaved sample, a binary search in the table
//   edges   over the GATHERED samples (their millisecond grid is not the original's when 1 ms is no whole number of frames): cells again, then one
//           workgroup: leading chunks while S < r_lead^2 n (a min-index reduction), the segment re-sliced there, and 1 ms slices from the end
//           until S >= r_trail^2 n (a max-index reduction).  r_lead / r_trail come from the host: no pow, log or sqrt in a decision
//   finish  mono sum, the zero pad, float conversion and per-block int64 sums of squares; one block adds them (integers: the order cannot
//           matter), forms rms32 = fp32(sqrt(fp64(S) / (ch^2 32768^2 n))) and decides rms32 < target; the boost is (x * target) / rms32 in fp32
// The trailing cut is the host's (a float loop, `end -= 0.001`, kept there): the decision reports the silent milliseconds, the caller answers cut_ms.
// Stores to device memory are plain C++; no atomics: one workgroup owns the tables and the counts.
#include <algorithm>
#include <cmath>

#include "kernels.h"
#include "runtime.h"
#include "silence_rule.h"

static constexpr int REF_TILE = 8192;  // interleaved samples staged per pass (uint32 squares: 32 KiB of LDS)

__device__ __forceinline__ int64_t frames_ms(int64_t frames, int rate) {  // Segment.__len__: round(1000.0 * frames / rate), half to even
#pragma clang fp contract(off)
    return (int64_t)__builtin_rint(1000.0 * (double)frames / (double)rate);
}

// Cells c0 = blockIdx.x * cells_per_block ...: as silence_cells_kernel, from int16 and over `ch` interleaved channels.  sums[m + 1] = cell m.
// dims (device, may be null): (frames, milliseconds) when the host cannot know them (the gathered samples); both are clamped to the host's bounds.
__global__ __launch_bounds__(256) void ref_cells_kernel(const int16_t* __restrict__ pcm, int64_t n_host, int64_t n_ms_host,
                                                        const int64_t* __restrict__ dims, int ch, double spm, int cells_per_block,
                                                        int64_t* __restrict__ sums) {
    typedef __attribute__((ext_vector_type(8))) short vec_t;
    __shared__ uint32_t sq[REF_TILE];
    const int tid = threadIdx.x;
    int64_t n = n_host, n_ms = n_ms_host;
    if (dims) {
        n = dims[0] < n_host ? dims[0] : n_host;
        n_ms = dims[1] < n_ms_host ? dims[1] : n_ms_host;
    }
    const int64_t c0 = (int64_t)blockIdx.x * cells_per_block;
    if (c0 >= n_ms) return;  // (the whole block)
    const int64_t c1 = c0 + cells_per_block < n_ms ? c0 + cells_per_block : n_ms;
    const int64_t s0 = ms_frame(c0, spm, n) * ch, s1 = ms_frame(c1, spm, n) * ch;
    const int64_t c = c0 + tid;
    const bool mine = tid < cells_per_block && c < c1;
    const int64_t f0 = mine ? ms_frame(c, spm, n) * ch : 0, f1 = mine ? ms_frame(c + 1, spm, n) * ch : 0;
    int64_t acc = 0;
    for (int64_t ts = s0; ts < s1; ts += REF_TILE) {
        const int len = (int)(s1 - ts < REF_TILE ? s1 - ts : REF_TILE);
        const int16_t* p = pcm + ts;
        const int mis = (int)(((uintptr_t)p & 15) / sizeof(int16_t));
        int head = mis ? 8 - mis : 0;
        if (head > len) head = len;
        const int nvec = (len - head) / 8;
        if (tid < head) {
            const int v = p[tid];
            sq[tid] = (uint32_t)(v * v);
        }
        const vec_t* pv = reinterpret_cast<const vec_t*>(p + head);
        for (int k = tid; k < nvec; k += 256) {
            const vec_t x = pv[k];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int v = x[j];
                sq[head + k * 8 + j] = (uint32_t)(v * v);
            }
        }
        const int done = head + nvec * 8;
        if (done + tid < len) {  // fewer than 8 samples
            const int v = p[done + tid];
            sq[done + tid] = (uint32_t)(v * v);
        }
        __syncthreads();
        const int64_t lo = f0 > ts ? f0 : ts, hi = f1 < ts + len ? f1 : ts + len;
        for (int64_t j = lo; j < hi; ++j) acc += (int64_t)sq[(int)(j - ts)];
        __syncthreads();
    }
    if (mine) sums[c + 1] = acc;
}

struct RefParams {
    SilenceParams q[2];   // the two passes of clip_reference, both over the original clip
    int64_t soft, hard;   // ms
    int64_t hard_frames;  // int(hard * spm)
    int64_t lead2, trail2;  // r_lead^2, r_trail^2
    int64_t chunk;        // ms
    int rate, ch, clip_short, table_rows;
};

// One workgroup.  counts: F5_REF_PARTS, F5_REF_CLIP (bit 0 / 1 / 2: message (1) / (2) / (3)), F5_REF_GATHERED, F5_REF_GATHERED_MS, F5_REF_PASS2; dims = (gathered
// frames, their milliseconds) for the kernels behind; table_out rows (first frame, end frame, position in the gathered samples).
__global__ __launch_bounds__(1024) void ref_plan_kernel(const RefParams p, int64_t* __restrict__ sums, uint8_t* __restrict__ flags,
                                                        int32_t* __restrict__ tab0, int32_t* __restrict__ tab1, int32_t* __restrict__ table_out,
                                                        int64_t* __restrict__ counts, int64_t* __restrict__ dims) {
    __shared__ int64_t part[1024];
    __shared__ int need2;
    const int tid = threadIdx.x;
    // thread 0: clip_reference's gather() over one pass's table
    int64_t frames = 0;
    int used = 0, clip = 0, pass = 0;
    auto gather = [&](const int32_t* tab, int parts, int cap, int bit) {
        frames = 0;
        used = 0;
        if (parts > cap) parts = cap;
        for (int r = 0; r < parts; ++r) {
            const int64_t len = (int64_t)tab[3 * r + 1] - tab[3 * r];
            if (frames_ms(frames, p.rate) > p.soft && frames_ms(frames + len, p.rate) > p.hard) {
                clip |= bit;
                break;
            }
            frames += len;
            ++used;
        }
    };
    if (p.clip_short) {
        silence_scan(p.q[0].n_ms, sums, part);
        silence_flags(p.q[0], sums, flags);
        if (tid < 64) {
            int64_t kept;
            int parts;
            silence_table(p.q[0], flags, tab0, &kept, &parts);
            if (tid == 0) {
                gather(tab0, parts, p.q[0].cap, 1);
                need2 = frames_ms(frames, p.rate) > p.hard ? 1 : 0;
            }
        }
        __syncthreads();
        if (need2) {  // (the whole workgroup)
            silence_flags(p.q[1], sums, flags);
            if (tid < 64) {
                int64_t kept;
                int parts;
                silence_table(p.q[1], flags, tab1, &kept, &parts);
                if (tid == 0) {
                    gather(tab1, parts, p.q[1].cap, 2);
                    pass = 1;
                }
            }
        }
    }
    if (tid != 0) return;
    const int32_t* tab = pass ? tab1 : tab0;
    if (!p.clip_short) {  // the clip as it is, every frame of it
        frames = p.q[0].n;
        used = 1;
    }
    if (p.clip_short && frames_ms(frames, p.rate) > p.hard) {  // slice_ms(0, hard) of the gathered samples
        if (p.hard_frames < frames) frames = p.hard_frames;
        clip |= 4;
    }
    if (used > p.table_rows) used = p.table_rows;
    for (int r = 0; r < used; ++r) {
        int64_t first = 0, len = p.q[0].n, pos = 0;
        if (p.clip_short) {
            first = tab[3 * r];
            len = (int64_t)tab[3 * r + 1] - first;
            pos = tab[3 * r + 2];
        }
        const int64_t room = frames > pos ? frames - pos : 0;
        if (len > room) len = room;
        table_out[3 * r] = (int32_t)first;
        table_out[3 * r + 1] = (int32_t)(first + len);
        table_out[3 * r + 2] = (int32_t)(pos < frames ? pos : frames);
    }
    const int64_t g_ms = frames_ms(frames, p.rate);
    counts[F5_REF_PARTS] = used;
    counts[F5_REF_CLIP] = clip;
    counts[F5_REF_GATHERED] = frames;
    counts[F5_REF_GATHERED_MS] = g_ms;
    counts[F5_REF_PASS2] = pass;
    dims[0] = frames;
    dims[1] = g_ms;
}

// gathered[pos] for every interleaved sample of the kept frames (capacity: n_frames * ch)
__global__ __launch_bounds__(256) void ref_gather_kernel(const int16_t* __restrict__ pcm, int64_t n_frames, int ch, const int32_t* __restrict__ table,
                                                         const int64_t* __restrict__ counts, int table_rows, int16_t* __restrict__ gathered) {
    const int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t kept = counts[F5_REF_GATHERED] < n_frames ? counts[F5_REF_GATHERED] : n_frames;
    if (pos >= kept * ch) return;
    const int64_t frame = pos / ch;
    int lo = 0, hi = (int)(counts[F5_REF_PARTS] < table_rows ? counts[F5_REF_PARTS] : table_rows) - 1;
    while (lo < hi) {  // last part whose first gathered frame is at or before this one
        const int mid = (lo + hi + 1) >> 1;
        if (table[3 * mid + 2] <= frame) lo = mid; else hi = mid - 1;
    }
    const int64_t src = (int64_t)table[3 * lo] + (frame - table[3 * lo + 2]);
    if (src < 0 || src >= n_frames) return;  // (no table row leads here)
    gathered[pos] = pcm[src * ch + (pos - frame * ch)];
}

// One workgroup over the gathered samples g (dims = frames K, milliseconds n_ms; cells[m + 1] = cell m of THEIR grid, not scanned):
//   lead   chunks [j chunk, min((j + 1) chunk, n_ms)) while dBFS < T, i.e. S < lead2 * n or empty; trim = min(j chunk, n_ms)
//   slice  slice_ms(trim, None): frames [o, e) = [F(trim), F(n_ms)) clamped to K, whose own length in ms is n2
//   trail  1 ms slices of that segment (its grid restarts at o) from the end until dBFS > T, i.e. n > 0 and S >= trail2 * n
__global__ __launch_bounds__(1024) void ref_edges_kernel(const RefParams p, const int16_t* __restrict__ g, const int64_t* __restrict__ cells,
                                                         const int64_t* __restrict__ dims, int64_t* __restrict__ counts) {
    __shared__ int64_t red[1024];
    const int tid = threadIdx.x;
    const double spm = p.q[0].spm;
    const int64_t K = dims[0] < p.q[0].n ? dims[0] : p.q[0].n;
    const int64_t n_ms = dims[1] < p.q[0].n_ms ? dims[1] : p.q[0].n_ms;
    const int64_t chunks = (n_ms + p.chunk - 1) / p.chunk;
    int64_t best = chunks;
    for (int64_t j = tid; j < chunks; j += 1024) {
        const int64_t m0 = j * p.chunk, m1 = m0 + p.chunk < n_ms ? m0 + p.chunk : n_ms;
        int64_t S = 0;
        for (int64_t m = m0; m < m1; ++m) S += cells[m + 1];
        const int64_t cnt = (ms_frame(m1, spm, K) - ms_frame(m0, spm, K)) * p.ch;
        const bool silent = cnt <= 0 || S < p.lead2 * cnt;
        if (!silent && j < best) best = j;
    }
    red[tid] = best;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o && red[tid + o] < red[tid]) red[tid] = red[tid + o];
        __syncthreads();
    }
    int64_t trim = red[0] * p.chunk;
    if (trim > n_ms) trim = n_ms;
    __syncthreads();
    const int64_t o0 = ms_frame(trim, spm, K);
    int64_t e0 = ms_frame(n_ms, spm, K);
    if (e0 < o0) e0 = o0;
    const int64_t K2 = e0 - o0, n2 = frames_ms(K2, p.rate);
    int64_t loud = -1;
    for (int64_t m = tid; m < n2; m += 1024) {
        const int64_t f0 = ms_frame(m, spm, K2), f1 = ms_frame(m + 1, spm, K2);
        int64_t S = 0;
        for (int64_t j = (o0 + f0) * p.ch; j < (o0 + f1) * p.ch; ++j) {
            const int64_t v = g[j];
            S += v * v;
        }
        const int64_t cnt = (f1 - f0) * p.ch;
        if (cnt > 0 && S >= p.trail2 * cnt && m > loud) loud = m;
    }
    red[tid] = loud;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o && red[tid + o] > red[tid]) red[tid] = red[tid + o];
        __syncthreads();
    }
    if (tid != 0) return;
    counts[F5_REF_LEAD_MS] = trim;
    counts[F5_REF_TRAIL_MS] = n2 - 1 - red[0];
    counts[F5_REF_LEAD_FRAME] = o0;
    counts[F5_REF_EDGE_FRAMES] = K2;
    counts[F5_REF_EDGE_MS] = n2;
}

// The kept frames behind slice_ms(0, cut_ms) of the edge segment (Python's slice rule: a negative cut counts from the end), then the pad
__device__ __forceinline__ void ref_out_frames(const int64_t* counts, int64_t cut_ms, double spm, int64_t pad_frames, int64_t cap, int64_t* kept,
                                               int64_t* total) {
    const int64_t K2 = counts[F5_REF_EDGE_FRAMES], n2 = counts[F5_REF_EDGE_MS];
    int64_t e = cut_ms >= 0 ? cut_ms : n2 + cut_ms;
    e = e < 0 ? 0 : (e > n2 ? n2 : e);
    int64_t k = ms_frame(e, spm, K2);
    if (k > cap) k = cap;
    *kept = k;
    *total = k + pad_frames < cap ? k + pad_frames : cap;
}

// Frame pos of the result: the channels' sum v (0 in the pad), wave = fp32(v) / (32768 ch) -- exactly the mean of the host's int / 32768 --,
// the integers themselves when asked for, and partial[block] = the block's sum of v^2.
__global__ __launch_bounds__(256) void ref_finish_kernel(const int16_t* __restrict__ g, int64_t g_frames, int ch, double spm, int64_t cut_ms,
                                                         int64_t pad_frames, int64_t cap, int64_t* __restrict__ counts, float* __restrict__ wave,
                                                         int16_t* __restrict__ out_pcm, int64_t* __restrict__ partial) {
    __shared__ int64_t red[256];
    const int tid = threadIdx.x;
    int64_t kept, total;
    ref_out_frames(counts, cut_ms, spm, pad_frames, cap, &kept, &total);
    const int64_t o0 = counts[F5_REF_LEAD_FRAME];
    const int64_t pos = (int64_t)blockIdx.x * 256 + tid;
    int64_t v = 0;
    if (pos < total) {
        const bool live = pos < kept && o0 + pos < g_frames;
        for (int c = 0; c < ch; ++c) {
            const int s = live ? g[(o0 + pos) * ch + c] : 0;
            v += s;
            if (out_pcm) out_pcm[pos * ch + c] = (int16_t)s;
        }
        wave[pos] = (float)v / (32768.0f * (float)ch);
    }
    red[tid] = v * v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = red[0];
}

// One block: S, rms32 and the decision.  (The last kernel that reads F5_REF_EDGE_*: it stores F5_REF_KEPT and F5_REF_OUT_FRAMES.)
__global__ __launch_bounds__(256) void ref_rms_kernel(const int64_t* __restrict__ partial, int blocks, int ch, double spm, int64_t cut_ms,
                                                      int64_t pad_frames, int64_t cap, float target_rms, int64_t* __restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ int64_t red[256];
    const int tid = threadIdx.x;
    int64_t s = 0;
    for (int b = tid; b < blocks; b += 256) s += partial[b];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid != 0) return;
    int64_t kept, total;
    ref_out_frames(counts, cut_ms, spm, pad_frames, cap, &kept, &total);
    const double denom = (double)ch * (double)ch * 32768.0 * 32768.0 * (double)total;
    const float rms32 = total > 0 ? (float)__builtin_sqrt((double)red[0] / denom) : __builtin_nanf("");
    counts[F5_REF_KEPT] = kept;
    counts[F5_REF_OUT_FRAMES] = total;
    counts[F5_REF_SUMSQ] = red[0];
    counts[F5_REF_BOOST] = rms32 < target_rms ? 1 : 0;
    counts[F5_REF_RMS_BITS] = (int64_t)__float_as_uint(rms32);
}

// `audio * target_rms / rms`: two fp32 operations per sample, in this order
__global__ __launch_bounds__(256) void ref_boost_kernel(float* __restrict__ wave, const int64_t* __restrict__ counts, int64_t cap, float target_rms) {
#pragma clang fp contract(off)
    if (!counts[F5_REF_BOOST]) return;
    const int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = counts[F5_REF_OUT_FRAMES] < cap ? counts[F5_REF_OUT_FRAMES] : cap;
    if (pos >= total) return;
    const float rms32 = __uint_as_float((uint32_t)counts[F5_REF_RMS_BITS]);
    const float scaled = wave[pos] * target_rms;
    wave[pos] = scaled / rms32;
}

// ---- host side
struct RefPlan {
    RefParams p;
    int64_t n_ms, pad_frames;
    int cells_per_block;
    size_t off_flags, off_tab0, off_tab1, off_gathered, off_cells, off_dims, off_partial, bytes;
};

static int64_t ref_window_samples(int ms, double spm, int ch) { return (int64_t)(((double)ms * spm + 1.0) * ch); }

static int ref_plan(int64_t n_frames, int channels, int sample_rate, const f5_reference_rule* r, RefPlan* out) {
    if (!r) return f5_fail(F5_EINVAL, "rule is null");
    if (channels != 1 && channels != 2) return f5_fail(F5_EINVAL, "channels = %d: 1 or 2", channels);
    if (n_frames < 0 || n_frames * channels >= (int64_t)1 << 31)
        return f5_fail(F5_EINVAL, "n_frames = %lld with %d channels: 0 .. 2^31 - 1 samples", (long long)n_frames, channels);
    if (sample_rate < 1000) return f5_fail(F5_EINVAL, "sample_rate = %d: at least 1000 (a millisecond holds a frame)", sample_rate);
    if (r->min_silence_len_1 < 1 || r->min_silence_len_2 < 1) return f5_fail(F5_EINVAL, "min_silence_len: at least 1");
    if (r->seek_step < 1) return f5_fail(F5_EINVAL, "seek_step = %d: at least 1", r->seek_step);
    if (r->keep_silence < 0) return f5_fail(F5_EINVAL, "keep_silence = %d: not negative", r->keep_silence);
    if (r->threshold_floor_1 < 0 || r->threshold_floor_2 < 0) return f5_fail(F5_EINVAL, "threshold_floor: not negative");
    if (r->soft_limit_ms < 0 || r->hard_limit_ms < r->soft_limit_ms) return f5_fail(F5_EINVAL, "limits: 0 <= soft_limit_ms <= hard_limit_ms");
    if (r->r_lead < 0 || r->r_lead > 32768 || r->r_trail < 0 || r->r_trail > 32768) return f5_fail(F5_EINVAL, "r_lead, r_trail: 0 .. 32768");
    if (r->lead_chunk_ms < 1) return f5_fail(F5_EINVAL, "lead_chunk_ms = %d: at least 1", r->lead_chunk_ms);
    if (r->pad_ms < 0) return f5_fail(F5_EINVAL, "pad_ms = %d: not negative", r->pad_ms);
    const double spm = sample_rate / 1000.0;
    const int longest = std::max(std::max(r->min_silence_len_1, r->min_silence_len_2), r->lead_chunk_ms);
    if (ref_window_samples(longest, spm, channels) >= 4194304)
        return f5_fail(F5_EINVAL, "a window of %d ms at %d Hz, %d channels: 2^22 samples or more (the integer decision holds below that)", longest,
                       sample_rate, channels);
    if ((double)r->pad_ms * spm >= 2147483648.0) return f5_fail(F5_EINVAL, "pad_ms = %d: 2^31 frames or more", r->pad_ms);
    const int64_t n_ms = (int64_t)std::rint(1000.0 * (double)n_frames / (double)sample_rate);  // Python's round(): half to even
    RefParams& p = out->p;
    const int L[2] = {r->min_silence_len_1, r->min_silence_len_2}, R[2] = {r->threshold_floor_1, r->threshold_floor_2};
    for (int k = 0; k < 2; ++k) {
        SilenceParams& q = p.q[k];
        q.n = n_frames;
        q.n_ms = n_ms;
        q.spm = spm;
        q.L = L[k];
        q.step = r->seek_step;
        q.keep = r->keep_silence;
        const int64_t Rk = R[k] < 32768 ? R[k] : 32768;  // an rms never exceeds 32768
        q.lim = (Rk + 1) * (Rk + 1);
        q.cmul = channels;
        silence_set_windows(q);
    }
    p.soft = r->soft_limit_ms;
    p.hard = r->hard_limit_ms;
    p.hard_frames = (int64_t)((double)r->hard_limit_ms * spm);
    p.lead2 = (int64_t)r->r_lead * r->r_lead;
    p.trail2 = (int64_t)r->r_trail * r->r_trail;
    p.chunk = r->lead_chunk_ms;
    p.rate = sample_rate;
    p.ch = channels;
    p.clip_short = r->clip_short ? 1 : 0;
    p.table_rows = std::max(p.q[0].cap, p.q[1].cap);
    out->n_ms = n_ms;
    out->pad_frames = (int64_t)((double)r->pad_ms * spm);  // silent_like: _frame(pad_ms)
    int cpb = (int)(REF_TILE / ((spm + 1.0) * channels));
    out->cells_per_block = cpb < 1 ? 1 : (cpb > 256 ? 256 : cpb);
    const int64_t W = std::max<int64_t>(std::max(p.q[0].W, p.q[1].W), 1);
    const int64_t blocks = (n_frames + out->pad_frames + 255) / 256 + 1;
    size_t o = (size_t)round_up((n_ms + 2) * 8, 16);  // the original's cells / prefix sums first
    out->off_flags = o;
    o += (size_t)round_up(W, 16);
    out->off_tab0 = o;
    o += (size_t)round_up((int64_t)p.q[0].cap * 12, 16);
    out->off_tab1 = o;
    o += (size_t)round_up((int64_t)p.q[1].cap * 12, 16);
    out->off_gathered = o;
    o += (size_t)round_up(std::max<int64_t>(n_frames * channels, 1) * 2, 16);
    out->off_cells = o;
    o += (size_t)round_up((n_ms + 2) * 8, 16);
    out->off_dims = o;
    o += 32;
    out->off_partial = o;
    o += (size_t)round_up(blocks * 8, 16);
    out->bytes = o;
    return 0;
}

static int ref_check_buffers(const RefPlan& pl, const int16_t* pcm, int64_t n_frames, const void* workspace, int64_t workspace_bytes,
                             const int32_t* table_out, const int64_t* counts_dev) {
    if ((!pcm && n_frames > 0) || !workspace || !table_out || !counts_dev) return f5_fail(F5_EINVAL, "null argument");
    if (((uintptr_t)pcm & 1) != 0) return f5_fail(F5_EINVAL, "pcm is not aligned to its element size");
    if (workspace_bytes < (int64_t)pl.bytes || ((uintptr_t)workspace & 15) != 0)
        return f5_fail(F5_EINVAL, "workspace: %lld bytes given, %lld needed, 16-byte aligned", (long long)workspace_bytes, (long long)pl.bytes);
    return 0;
}

static int ref_decide(const RefPlan& pl, const int16_t* pcm, char* ws, int32_t* table_out, int64_t* counts, hipStream_t st) {
    const RefParams& p = pl.p;
    const int64_t n = p.q[0].n;
    int64_t* sums = (int64_t*)ws;
    int64_t* cells = (int64_t*)(ws + pl.off_cells);
    int64_t* dims = (int64_t*)(ws + pl.off_dims);
    int16_t* gathered = (int16_t*)(ws + pl.off_gathered);
    const dim3 cgrid((unsigned)((pl.n_ms + pl.cells_per_block - 1) / pl.cells_per_block));
    if (pl.n_ms > 0 && p.clip_short) {
        hipLaunchKernelGGL(ref_cells_kernel, cgrid, dim3(256), 0, st, pcm, n, pl.n_ms, (const int64_t*)nullptr, p.ch, p.q[0].spm, pl.cells_per_block,
                           sums);
        F5_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ref_plan_kernel, dim3(1), dim3(1024), 0, st, p, sums, (uint8_t*)(ws + pl.off_flags), (int32_t*)(ws + pl.off_tab0),
                       (int32_t*)(ws + pl.off_tab1), table_out, counts, dims);
    F5_LAUNCH_CHECK();
    if (n > 0) {
        hipLaunchKernelGGL(ref_gather_kernel, dim3((unsigned)((n * p.ch + 255) / 256)), dim3(256), 0, st, pcm, n, p.ch, (const int32_t*)table_out,
                           (const int64_t*)counts, p.table_rows, gathered);
        F5_LAUNCH_CHECK();
    }
    if (pl.n_ms > 0) {
        hipLaunchKernelGGL(ref_cells_kernel, cgrid, dim3(256), 0, st, (const int16_t*)gathered, n, pl.n_ms, (const int64_t*)dims, p.ch, p.q[0].spm,
                           pl.cells_per_block, cells);
        F5_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ref_edges_kernel, dim3(1), dim3(1024), 0, st, p, (const int16_t*)gathered, (const int64_t*)cells, (const int64_t*)dims, counts);
    F5_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t f5_reference_prepare_workspace(int64_t n_frames, int channels, int sample_rate, const f5_reference_rule* rule) {
    RefPlan pl;
    const int rc = ref_plan(n_frames, channels, sample_rate, rule, &pl);
    return rc != 0 ? (int64_t)rc : (int64_t)pl.bytes;
}

extern "C" int64_t f5_reference_table_rows(int64_t n_frames, int channels, int sample_rate, const f5_reference_rule* rule) {
    RefPlan pl;
    const int rc = ref_plan(n_frames, channels, sample_rate, rule, &pl);
    return rc != 0 ? (int64_t)rc : (int64_t)pl.p.table_rows;
}

extern "C" int f5_op_reference_plan(const int16_t* pcm, int64_t n_frames, int channels, int sample_rate, const f5_reference_rule* rule,
                                    void* workspace, int64_t workspace_bytes, int32_t* table_out, int64_t* counts_dev, f5_stream_t stream) {
    RefPlan pl;
    F5_TRY(ref_plan(n_frames, channels, sample_rate, rule, &pl));
    F5_TRY(ref_check_buffers(pl, pcm, n_frames, workspace, workspace_bytes, table_out, counts_dev));
    F5_TRY(f5_check_device());
    return ref_decide(pl, pcm, (char*)workspace, table_out, counts_dev, (hipStream_t)stream);
}

extern "C" int f5_reference_prepare(const int16_t* pcm, int64_t n_frames, int channels, int sample_rate, const f5_reference_rule* rule, int planned,
                                    int64_t cut_ms, void* workspace, int64_t workspace_bytes, int32_t* table_out, int64_t* counts_dev,
                                    int64_t out_frames, float* out_wave, int16_t* out_pcm, f5_stream_t stream) {
    RefPlan pl;
    F5_TRY(ref_plan(n_frames, channels, sample_rate, rule, &pl));
    F5_TRY(ref_check_buffers(pl, pcm, n_frames, workspace, workspace_bytes, table_out, counts_dev));
    if (out_frames < 0 || out_frames > n_frames + pl.pad_frames)
        return f5_fail(F5_EINVAL, "out_frames = %lld: 0 .. n_frames + the pad's %lld", (long long)out_frames, (long long)pl.pad_frames);
    if (!out_wave && out_frames > 0) return f5_fail(F5_EINVAL, "out_wave is null");
    F5_TRY(f5_check_device());
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    if (!planned) F5_TRY(ref_decide(pl, pcm, ws, table_out, counts_dev, st));
    const RefParams& p = pl.p;
    const int blocks = (int)((out_frames + 255) / 256) > 0 ? (int)((out_frames + 255) / 256) : 1;
    int64_t* partial = (int64_t*)(ws + pl.off_partial);
    hipLaunchKernelGGL(ref_finish_kernel, dim3(blocks), dim3(256), 0, st, (const int16_t*)(ws + pl.off_gathered), n_frames, p.ch, p.q[0].spm, cut_ms,
                       pl.pad_frames, out_frames, counts_dev, out_wave, out_pcm, partial);
    F5_LAUNCH_CHECK();
    hipLaunchKernelGGL(ref_rms_kernel, dim3(1), dim3(256), 0, st, (const int64_t*)partial, blocks, p.ch, p.q[0].spm, cut_ms, pl.pad_frames, out_frames,
                       rule->target_rms, counts_dev);
    F5_LAUNCH_CHECK();
    hipLaunchKernelGGL(ref_boost_kernel, dim3(blocks), dim3(256), 0, st, out_wave, (const int64_t*)counts_dev, out_frames, rule->target_rms);
    F5_LAUNCH_CHECK();
    return 0;
}
