// philox.h -- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 generator) and the keep
// mask of the attention-dropout mode built on it.  Plain C++: compiles as host code without HIP, and as __host__ __device__ under hipcc, so
// the kernels (attention.hip, attention_dropout.hip) and a host check run the same text.
//
// The mask of one attention call:
//   (o0, o1, o2, o3) = Philox4x32-10(counter = (k >> 2, q, bw * H + head, stream), key = (seed & 0xffffffff, seed >> 32))
//   keep(q, k)       = o[k & 3] >= T,   T = round(p * 2^32)
// q / k: query / key index in the sequence the softmax runs over, bw: batch word, stream: call word.  One call covers 4 consecutive keys of
// one query.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define F5_PHILOX_FN __host__ __device__ __forceinline__
#else
#define F5_PHILOX_FN inline
#endif

struct Philox4 {
    uint32_t v[4];
};

F5_PHILOX_FN Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += W0;
        k1 += W1;
    }
    Philox4 o;
    o.v[0] = c0;
    o.v[1] = c1;
    o.v[2] = c2;
    o.v[3] = c3;
    return o;
}

// the four draws that decide keys 4 * kq .. 4 * kq + 3 of query q
F5_PHILOX_FN Philox4 attn_dropout_draws(uint32_t kq, uint32_t q, uint32_t bh, uint32_t stream, uint64_t seed) {
    return philox4x32_10(kq, q, bh, stream, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
}

// T = round(p * 2^32) for p in [0, 1) given as a double
static inline uint32_t attn_dropout_threshold(double p) {
    const double t = p * 4294967296.0 + 0.5;
    return t <= 0.0 ? 0u : (t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t);
}
