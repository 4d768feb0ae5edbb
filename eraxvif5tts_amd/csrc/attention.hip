// attention.hip -- non-causal multi-head attention with a key-padding mask over packed q|k|v projections.
//   * attn_ref_kernel : reference kernel, fp32 VALU math (exact softmax order-independent up to rounding),
//                       any sequence length, both activation dtypes.  Used by the fp32 parity mode and
//                       as the cross-check of the tuned kernel.
//                       DROP (attention dropout, philox.h): a thread owns keys 4 * tx + j of a query, i.e. exactly one Philox call; the row
//                       sum takes the undropped P, the PV product the dropped one, 1 / (1 - p) rides on the final normalisation.  The
//                       DROP = false instantiations carry an empty argument and no dropout code.
//   * tuned bf16 flash kernel: attention_fast.hip; bf16 flash kernel with dropout: attention_dropout.hip.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "kernels.h"
#include "philox.h"

struct AttnNoDrop {};

template <typename T, bool DROP = false>
__global__ __launch_bounds__(256) void attn_ref_kernel(const T* __restrict__ qkv, int ldq, int inner, const uint8_t* __restrict__ mask,
                                                       T* __restrict__ out, int ldo, int N, int bs /* rows between batch items (N, or more: ragged sampler) */, float scale,
                                                       std::conditional_t<DROP, AttnDropArgs, AttnNoDrop> da) {
    constexpr int D = 64, TQ = 64, TK = 64, LD = 65;
    __shared__ float Qs[TQ * LD], Ks[TK * LD], Vs[TK * LD], Ps[TQ * LD];
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * TQ;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const T* base = qkv + (size_t)b * bs * ldq + h * D;
    uint32_t dstream = 0u, dbh = 0u;  // DROP: call word, batch word * H + head
    if constexpr (DROP) {
        dstream = (da.base ? *da.base : 0u) + da.offset;
        dbh = (da.bw0 + (uint32_t)b * da.bw_step) * gridDim.y + (uint32_t)h;
    }

    for (int i = tid; i < TQ * D; i += 256) {
        const int r = i >> 6, d = i & 63;
        Qs[r * LD + d] = (q0 + r < N) ? to_f32(base[(size_t)(q0 + r) * ldq + d]) : 0.f;
    }
    float m_i[4], l_i[4], o[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m_i[i] = -INFINITY;
        l_i[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[i][j] = 0.f;
    }
    for (int k0 = 0; k0 < N; k0 += TK) {
        __syncthreads();  // previous tile's Ps/Vs reads are done (and Qs visible on the first pass)
        for (int i = tid; i < TK * D; i += 256) {
            const int r = i >> 6, d = i & 63;
            const bool ok = k0 + r < N;
            Ks[r * LD + d] = ok ? to_f32(base[(size_t)(k0 + r) * ldq + inner + d]) : 0.f;
            Vs[r * LD + d] = ok ? to_f32(base[(size_t)(k0 + r) * ldq + 2 * inner + d]) : 0.f;
        }
        __syncthreads();
        float s[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[i][j] = 0.f;
        for (int d = 0; d < D; ++d) {
            float qv[4], kv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) qv[i] = Qs[(4 * ty + i) * LD + d];
#pragma unroll
            for (int j = 0; j < 4; ++j) kv[j] = Ks[(4 * tx + j) * LD + d];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) s[i][j] += qv[i] * kv[j];
        }
        bool kvalid[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int key = k0 + 4 * tx + j;
            kvalid[j] = key < N && (mask == nullptr || mask[(size_t)b * N + key] != 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float mt = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s[i][j] = kvalid[j] ? s[i][j] * scale : -INFINITY;
                mt = fmaxf(mt, s[i][j]);
            }
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) mt = fmaxf(mt, __shfl_xor(mt, off, 64));  // the 16 tx lanes of a row are contiguous
            const float m_new = fmaxf(m_i[i], mt);
            const float alpha = (m_i[i] == -INFINITY) ? 0.f : expf(m_i[i] - m_new);
            float rs = 0.f;
            Philox4 dr;
            if constexpr (DROP) dr = attn_dropout_draws((uint32_t)(k0 >> 2) + tx, (uint32_t)(q0 + 4 * ty + i), dbh, dstream, da.seed);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float p = (s[i][j] == -INFINITY) ? 0.f : expf(s[i][j] - m_new);
                if constexpr (DROP)
                    Ps[(4 * ty + i) * LD + 4 * tx + j] = dr.v[j] >= da.thresh ? p : 0.f;
                else
                    Ps[(4 * ty + i) * LD + 4 * tx + j] = p;
                rs += p;
            }
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) rs += __shfl_xor(rs, off, 64);
            l_i[i] = l_i[i] * alpha + rs;
            m_i[i] = m_new;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[i][j] *= alpha;
        }
        __syncthreads();
        for (int key = 0; key < TK; ++key) {
            float pv[4], vv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) pv[i] = Ps[(4 * ty + i) * LD + key];
#pragma unroll
            for (int j = 0; j < 4; ++j) vv[j] = Vs[key * LD + 4 * tx + j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) o[i][j] += pv[i] * vv[j];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = q0 + 4 * ty + i;
        if (q < N) {
            float inv = l_i[i] > 0.f ? 1.0f / l_i[i] : 0.f;
            if constexpr (DROP) inv *= da.rscale;
#pragma unroll
            for (int j = 0; j < 4; ++j) out[((size_t)b * bs + q) * ldo + h * D + 4 * tx + j] = from_f32<T>(o[i][j] * inv);
        }
    }
}

int launch_attention_fast(int precision, int B, int N, int H, const void* qkv, int ldq, const uint8_t* mask, void* out, int ldo, hipStream_t stream,
                          int bstride, int qscaled);  // attention_fast.hip

double attn_dropout_prob_of(float prob) {
    char buf[32];
    for (int digits = 1; digits <= 9; ++digits) {
        snprintf(buf, sizeof(buf), "%.*g", digits, (double)prob);
        if (strtof(buf, nullptr) == prob) return strtod(buf, nullptr);
    }
    return (double)prob;
}

AttnDropArgs attn_drop_args(const AttnDropout& d) {
    return AttnDropArgs{d.base, d.seed, d.offset, d.bw0, d.bw_step, attn_dropout_threshold(d.prob), (float)(1.0 / (1.0 - d.prob))};
}

int launch_attention(int precision, int kernel_kind, int B, int N, int H, const void* qkv, int ldq, const uint8_t* mask, void* out, int ldo,
                     hipStream_t stream, int bstride, int qscaled, const AttnDropout* drop) {
    if (B <= 0 || N <= 0 || H <= 0) return 0;
    if (bstride <= 0) bstride = N;
    if (bstride < N || (bstride != N && mask)) return f5_fail(F5_EINVAL, "attention: batch stride below N, or a key mask with a batch stride");
    if (drop && drop->prob > 0.0) {
        if (!(drop->prob < 1.0) || qscaled) return f5_fail(F5_EINVAL, "attention: dropout needs a probability below 1 and q as projected");
        if (kernel_kind == 1) {
            if (precision != F5_PREC_BF16) return f5_fail(F5_EINVAL, "attention: the MFMA dropout kernel is bf16");
            return launch_attention_dropout(B, N, H, qkv, ldq, mask, out, ldo, stream, bstride, *drop);
        }
        const AttnDropArgs da = attn_drop_args(*drop);
        dim3 grid(cdiv(N, 64), H, B), block(256);
        if (precision == F5_PREC_FP16) return f5_fail(F5_ENOTSUP, "attention: dropout is not built for the fp16 mode");
        if (precision == F5_PREC_BF16)
            hipLaunchKernelGGL((attn_ref_kernel<bf16_t, true>), grid, block, 0, stream, (const bf16_t*)qkv, ldq, H * 64, mask, (bf16_t*)out, ldo, N, bstride, 0.125f, da);
        else
            hipLaunchKernelGGL((attn_ref_kernel<float, true>), grid, block, 0, stream, (const float*)qkv, ldq, H * 64, mask, (float*)out, ldo, N, bstride, 0.125f, da);
        F5_LAUNCH_CHECK();
        return 0;
    }
    if (kernel_kind == 1) {
        if (!attention_fast_supported(precision, N, H)) return f5_fail(F5_EINVAL, "attention: tuned kernel does not support this problem");
        if (qscaled && precision == F5_PREC_FP16) return f5_fail(F5_EINVAL, "attention: the fp16 mode takes q as projected");
        return launch_attention_fast(precision, B, N, H, qkv, ldq, mask, out, ldo, stream, bstride, qscaled);
    }
    // 1/sqrt(64) (SDPA default scale, modules.py:490); pre-scaled q carries 1/sqrt(64) * log2(e): exp(s ln 2) = exp2(s)
    const float scale = qscaled ? 0.6931471805599453f : 0.125f;
    dim3 grid(cdiv(N, 64), H, B), block(256);
    if (precision == F5_PREC_BF16)
        hipLaunchKernelGGL((attn_ref_kernel<bf16_t>), grid, block, 0, stream, (const bf16_t*)qkv, ldq, H * 64, mask, (bf16_t*)out, ldo, N, bstride, scale, AttnNoDrop{});
    else if (precision == F5_PREC_FP16)
        hipLaunchKernelGGL((attn_ref_kernel<f16_t>), grid, block, 0, stream, (const f16_t*)qkv, ldq, H * 64, mask, (f16_t*)out, ldo, N, bstride, scale, AttnNoDrop{});
    else
        hipLaunchKernelGGL((attn_ref_kernel<float>), grid, block, 0, stream, (const float*)qkv, ldq, H * 64, mask, (float*)out, ldo, N, bstride, scale, AttnNoDrop{});
    F5_LAUNCH_CHECK();
    return 0;
}
