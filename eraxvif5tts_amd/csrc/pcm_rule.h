// pcm_rule.h -- the truncating int16 PCM (streaming.wire.pcm16_bytes: trunc(x * 32767)) of the wave tail and of the delivery stage: one rule.
#pragma once
#include <stdint.h>

// p = x * 32767, the product taken by the caller in ITS precision: truncation toward zero inside int16, saturation outside (numpy leaves that
// cast undefined), NaN -> 0.  An fp32 product comes in widened: float -> double is exact and keeps the order, so the compares and the truncation
// give what they give on the float itself.
__device__ __forceinline__ int16_t pcm_sat(double p) {
    if (p >= 32767.0) return (int16_t)32767;
    if (p <= -32768.0) return (int16_t)-32768;
    return p == p ? (int16_t)(int)p : (int16_t)0;
}
