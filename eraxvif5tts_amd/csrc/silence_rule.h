// silence_rule.h -- the split_on_silence decision of infer/audio.py as device code, shared by silence.hip (the finished wave) and reference.hip
// (the reference voice): prefix scan of the per-millisecond cells, window flags, and the walk that turns the flags into the part table.  One
// workgroup of 1024 threads owns the cells, the flags and the table; everything is 64-bit integer arithmetic (silence.hip states the rule).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

__device__ __forceinline__ int64_t ms_frame(int64_t ms, double spm, int64_t n) {  // Segment._frame, then numpy's slice clamp
    const int64_t f = (int64_t)((double)ms * spm);
    return f < n ? f : n;
}

struct SilenceParams {
    int64_t n, n_ms;  // frames, milliseconds (Segment.__len__)
    double spm;       // rate / 1000.0
    int64_t L, step, keep;
    int64_t lim;      // (R + 1)^2
    int64_t W_reg;    // window starts 0, step, .. <= last
    int64_t W;        // W_reg, + 1 when last % step != 0
    int cap;          // table entries
    int cmul;         // interleaved samples per frame: Segment.rms is over all of them (1 for a mono wave)
};

static inline void silence_set_windows(SilenceParams& q) {  // W_reg, W and cap from n_ms, L and step
    if (q.n_ms < q.L) {
        q.W_reg = q.W = 0;
    } else {
        const int64_t last = q.n_ms - q.L;
        q.W_reg = last / q.step + 1;
        q.W = q.W_reg + (last % q.step ? 1 : 0);
    }
    q.cap = (int)(q.n_ms / q.L + 2);
}

// All 1024 threads: sums[k] (k = 1 .. n_ms holding cell k - 1) becomes the sum of the cells below k, sums[0] = 0.  `part` is int64 [1024] of LDS.
// Each thread owns `chunk` consecutive cells; the threads' totals are scanned in LDS.  Ends with a barrier.
__device__ __forceinline__ void silence_scan(int64_t n_ms, int64_t* __restrict__ sums, int64_t* part) {
    const int tid = threadIdx.x;
    const int64_t chunk = (n_ms + 1023) / 1024;
    int64_t a = 1 + tid * chunk, b = a + chunk;
    if (a > n_ms + 1) a = n_ms + 1;
    if (b > n_ms + 1) b = n_ms + 1;
    int64_t tot = 0;
    for (int64_t k = a; k < b; ++k) tot += sums[k];
    part[tid] = tot;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t add = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    int64_t run = part[tid] - tot;  // the sum of everything before this thread's cells
    for (int64_t k = a; k < b; ++k) {
        run += sums[k];
        sums[k] = run;
    }
    if (tid == 0) sums[0] = 0;
    __syncthreads();
}

// All 1024 threads: flags[w] = window w is silent.  Ends with a barrier.
__device__ __forceinline__ void silence_flags(const SilenceParams& q, const int64_t* __restrict__ sums, uint8_t* __restrict__ flags) {
    const int64_t last = q.n_ms - q.L;
    for (int64_t w = threadIdx.x; w < q.W; w += 1024) {
        const int64_t i = w < q.W_reg ? w * q.step : last;
        const int64_t cnt = (ms_frame(i + q.L, q.spm, q.n) - ms_frame(i, q.spm, q.n)) * q.cmul;
        const int64_t S = sums[i + q.L] - sums[i];
        flags[w] = (cnt <= 0 || S < q.lim * cnt) ? 1 : 0;  // (an empty slice has rms 0)
    }
    __syncthreads();
}

// Wave 0 alone (threads 0 .. 63, all of them): the flags become the table (first frame, end frame, position in the output) of the parts
// split_on_silence returns; every lane carries the same state and lane 0 stores.  *kept = frames of all parts, *parts = their number (which
// may exceed q.cap: the rows behind the cap are not stored).
__device__ __forceinline__ void silence_table(const SilenceParams& q, const uint8_t* __restrict__ flags, int32_t* __restrict__ table, int64_t* kept,
                                              int* parts) {
    const int tid = threadIdx.x;
    const int64_t last = q.n_ms - q.L;
    bool have = false, pend = false;
    int64_t cur = 0, prev = 0, prev_end = 0, pend_s = 0, pend_e = 0, out_pos = 0;
    int nseg = 0;
    auto flush = [&](int64_t s, int64_t e) {  // one part: clamp, slice_ms, append
        const int64_t s_ms = s > 0 ? s : 0, e_ms = e < q.n_ms ? e : q.n_ms;
        const int64_t i0 = ms_frame(s_ms, q.spm, q.n);
        int64_t i1 = ms_frame(e_ms, q.spm, q.n);
        if (i1 < i0) i1 = i0;
        if (tid == 0 && nseg < q.cap) {
            table[3 * nseg] = (int32_t)i0;
            table[3 * nseg + 1] = (int32_t)i1;
            table[3 * nseg + 2] = (int32_t)out_pos;
        }
        out_pos += i1 - i0;
        ++nseg;
    };
    auto nonsilent = [&](int64_t s, int64_t e) {  // a range of detect_nonsilent: pad it, meet the one before at the midpoint
        int64_t ps = s - q.keep;
        const int64_t pe = e + q.keep;
        if (pend) {
            if (ps < pend_e) {
                pend_e = (pend_e + ps) / 2;  // (a non-negative sum: Python's // and this division agree)
                ps = pend_e;
            }
            flush(pend_s, pend_e);
        }
        pend = true;
        pend_s = ps;
        pend_e = pe;
    };
    auto silent_range = [&](int64_t s, int64_t e) {  // a range of detect_silence
        if (!(prev_end == 0 && s == 0 && !pend)) nonsilent(prev_end, s);  // (the leading [0, 0] is popped)
        prev_end = e;
    };
    auto silent_start = [&](int64_t i) {
        if (!have) {
            have = true;
            cur = i;
        } else if (i != prev + q.step && i > prev + q.L) {
            silent_range(cur, prev + q.L);
            cur = i;
        }
        prev = i;
    };
    for (int64_t base = 0; base < q.W_reg; base += 64) {
        const int64_t w = base + tid;
        unsigned long long mask = __ballot(w < q.W_reg && flags[w] != 0);
        while (mask) {  // a run of consecutive starts: its first start is judged by the rule, every other one is `prev + step` and merges
            const int lo = __builtin_ctzll(mask);
            const unsigned long long inv = ~(mask >> lo);
            const int len = inv ? __builtin_ctzll(inv) : 64;
            silent_start((base + lo) * q.step);
            prev = (base + lo + len - 1) * q.step;
            mask = lo + len >= 64 ? 0ull : mask & ~((1ull << (lo + len)) - 1ull);
        }
    }
    if (q.W > q.W_reg && flags[q.W - 1] != 0) silent_start(last);
    if (!have) {
        nonsilent(0, q.n_ms);  // no silence, or shorter than one window
    } else {
        silent_range(cur, prev + q.L);
        if (prev_end != q.n_ms) nonsilent(prev_end, q.n_ms);
    }
    if (pend) flush(pend_s, pend_e);
    *kept = out_pos;
    *parts = nseg;
}
