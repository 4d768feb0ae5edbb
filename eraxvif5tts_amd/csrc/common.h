// common.h -- shared device/host helpers for libf5hip (gfx950 only: wave64, MFMA, LDS).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "../../include/f5hip.h"

// ----------------------------------------------------------------------------- error plumbing
void f5_set_error(const char* fmt, ...);
int f5_fail(int code, const char* fmt, ...);

#define F5_HIP(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess) return f5_fail(F5_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                             __FILE__, __LINE__);                                            \
    } while (0)

#define F5_TRY(expr)          \
    do {                      \
        int _rc = (expr);     \
        if (_rc != 0) return _rc; \
    } while (0)

#define F5_LAUNCH_CHECK()                                                                                     \
    do {                                                                                                      \
        hipError_t _e = hipGetLastError();                                                                    \
        if (_e != hipSuccess) return f5_fail(F5_EHIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), \
                                             __FILE__, __LINE__);                                             \
    } while (0)

// ----------------------------------------------------------------------------- device types
typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
// fp16 elements (F5_PREC_FP16): the same 16-bit containers and MFMA fragment layouts as bf16, three more mantissa bits, range +-65504
typedef _Float16 f16_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

#if defined(__HIPCC__)
__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(bf16_t v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float v) { return (bf16_t)v; }  // v_cvt_pk_bf16_f32 (RNE, NaN-safe)
// fp16 activation stores SATURATE: an out-of-range value clips to +-65504 instead of becoming inf (and NaN in the next softmax).  A NaN
// stays a NaN: v_med3_f32 alone answers a NaN operand with the minimum of the other two, which would turn it into a large finite number.
__device__ __forceinline__ float to_f32(f16_t v) { return (float)v; }
__device__ __forceinline__ float f16_sat(float v) { return v != v ? v : __builtin_amdgcn_fmed3f(v, -65504.0f, 65504.0f); }
template <> __device__ __forceinline__ f16_t from_f32<f16_t>(float v) { return (f16_t)f16_sat(v); }  // clamp, then v_cvt_pk_f16_f32 (RNE)

// The 16-bit element type of a production mode as a template parameter (Elem<bf16_t> is the default everywhere, Elem<f16_t> the fp16 mode):
// the element and its vectors, the two MFMA shapes, the RNE pack of a store, and the range the un-normalised softmax numerators may use.
template <typename E> struct Elem;
template <> struct Elem<bf16_t> {
    typedef bf16_t T;
    typedef bf16x4 x4;
    typedef bf16x8 x8;
    static constexpr bool F16 = false;
    static constexpr int ATTN_DEFER_LOG2 = 16;   // attention_pipe.hip: a row's reference moves when its maximum outgrows it by more than 2^16
    static constexpr int ATTN_SUM_LOG2 = 64;     // attention_fast.hip: a tile is redone the classic way when a row sum reaches 2^64
    static __device__ __forceinline__ x4 pack4(float a, float b, float c, float d) { return x4{(T)a, (T)b, (T)c, (T)d}; }
    static __device__ __forceinline__ f32x4 mfma16(x8 a, x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x16 mfma32(x8 a, x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Elem<f16_t> {
    typedef f16_t T;
    typedef f16x4 x4;
    typedef f16x8 x8;
    static constexpr bool F16 = true;
    static constexpr int ATTN_DEFER_LOG2 = 14;   // un-normalised numerators stay at or below 2^14, inside fp16 (largest finite value 65504 < 2^16)
    static constexpr int ATTN_SUM_LOG2 = 15;     // a row sum of at least 2^15 redoes the tile (a single numerator can then not pass 65504)
    static __device__ __forceinline__ x4 pack4(float a, float b, float c, float d) { return x4{(T)f16_sat(a), (T)f16_sat(b), (T)f16_sat(c), (T)f16_sat(d)}; }
    static __device__ __forceinline__ f32x4 mfma16(x8 a, x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x16 mfma32(x8 a, x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
// The kernels move both types in the bf16 vector types (16-bit containers, same fragment layouts); these take and return the containers.
template <typename EL> __device__ __forceinline__ f32x16 el_mfma32(const bf16x8& a, const bf16x8& b, const f32x16& c) {
    return Elem<EL>::mfma32(__builtin_bit_cast(typename Elem<EL>::x8, a), __builtin_bit_cast(typename Elem<EL>::x8, b), c);
}
template <typename EL> __device__ __forceinline__ bf16x4 el_pack4(float a, float b, float c, float d) { return __builtin_bit_cast(bf16x4, Elem<EL>::pack4(a, b, c, d)); }
// eight softmax numerators -> MFMA operand, RNE, NO clamp: the attention kernels keep them inside the type's range (ATTN_* above)
template <typename EL> __device__ __forceinline__ bf16x8 el_pack_p8(const float (&p)[8]) {
    typename Elem<EL>::x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (typename Elem<EL>::T)p[j];
    return __builtin_bit_cast(bf16x8, r);
}

// wave64 butterfly reductions (DPP/ds_swizzle chosen by the compiler from __shfl_xor)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// activations, written exactly as the reference's torch ops define them
__device__ __forceinline__ float act_gelu_tanh(float x) {  // nn.GELU(approximate="tanh"), modules.py:625
    const float k0 = 0.7978845608028654f, k1 = 0.044715f;
    return 0.5f * x * (1.0f + tanhf(k0 * (x + k1 * x * x * x)));
}
__device__ __forceinline__ float act_gelu_erf(float x) {  // nn.GELU(), modules.py:255
    return 0.5f * x * (1.0f + erff(x * 0.7071067811865476f));
}
__device__ __forceinline__ float act_mish(float x) {  // nn.Mish: x * tanh(softplus(x)), softplus threshold 20
    float sp = x > 20.0f ? x : log1pf(expf(x));
    return x * tanhf(sp);
}
__device__ __forceinline__ float act_silu(float x) { return x / (1.0f + expf(-x)); }
#endif

enum Act { ACT_NONE = 0, ACT_GELU_TANH = 1, ACT_GELU_ERF = 2, ACT_MISH = 3 };
