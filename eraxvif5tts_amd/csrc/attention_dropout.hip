// attention_dropout.hip -- bf16 flash attention WITH attention dropout for gfx950 (head dim 64, non-causal, key-padding mask): the opt-in
// mode that reproduces the reference's live F.scaled_dot_product_attention(dropout_p = 0.1) (model/modules.py:490, :582).
// One kernel for every grid size, written plainly and scheduled by the compiler -- Philox costs 40 32-bit multiplies per 4 probabilities on a
// kernel family that is vector-ALU bound to begin with, so there is nothing for hand placement to win here.
//
//   * a workgroup is 4 wavefronts x 32 queries of one (batch, head); K/V tiles of 64 keys go through LDS (K row-major, V transposed by the
//     staging stores), one tile at a time between two barriers;
//   * swapped products as in attention_pipe.hip: S^T = K.Q^T and O^T = V^T.P^T with v_mfma_f32_32x32x16_bf16.  Accumulator register i of a
//     lane is key 32 * kb + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5) of query lane & 31: registers 4g .. 4g + 3 are 4 consecutive keys of one
//     query, which is what one Philox call decides (philox.h), and 8 registers in a row are the B operand of one PV step;
//   * classic online softmax (exact running maximum, exp2 with the scale folded into one fma).  The row sum is taken from the UNDROPPED P in
//     fp32, as SDPA's math path normalises before it drops; the PV product takes the dropped P rounded to bf16; 1 / (1 - p) rides on the
//     final normalisation.
#include "kernels.h"
#include "philox.h"

namespace {

constexpr int KT = 64;    // keys per tile
constexpr int LDT = 72;   // bf16 elements per LDS row: 64 + 8 (rows stay 16-byte aligned, consecutive rows land on different banks)

__global__ __launch_bounds__(256) void attn_dropout_kernel(const bf16_t* __restrict__ qkv, int ldq, int inner, const uint8_t* __restrict__ mask,
                                                           bf16_t* __restrict__ out, int ldo, int N, int bs /* rows between batch items */, float c /* scale * log2(e) */,
                                                           AttnDropArgs da) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[KT * LDT];  // [key][d]
    __shared__ __attribute__((aligned(16))) bf16_t Vt[64 * LDT];  // [d][key]
    __shared__ __attribute__((aligned(4))) uint8_t Ms[KT];                                    // key validity of the tile

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, head = blockIdx.y, q0 = blockIdx.x * 128 + wave * 32;
    const int r = lane & 31, h = lane >> 5;
    const size_t row0 = (size_t)b * bs;
    const bf16_t* base = qkv + row0 * ldq + head * 64;
    const bf16_t* kbase = base + inner;
    const bf16_t* vbase = base + 2 * inner;
    const uint32_t dstream = (da.base ? *da.base : 0u) + da.offset;
    const uint32_t dbh = (da.bw0 + (uint32_t)b * da.bw_step) * gridDim.y + (uint32_t)head;
    const uint32_t dq = (uint32_t)(q0 + r);

    // Q fragments (B operand: Q[query r][d = 16 * ds + 8 * h .. + 7]); rows past the sequence are computed on its last row and dropped
    bf16x8 qf[4];
    {
        const int qrow = q0 + r < N ? q0 + r : N - 1;
        const bf16_t* qp = base + (size_t)qrow * ldq + 8 * h;
#pragma unroll
        for (int ds = 0; ds < 4; ++ds) qf[ds] = *reinterpret_cast<const bf16x8*>(qp + 16 * ds);
    }

    f32x16 o_acc[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) o_acc[0][i] = o_acc[1][i] = 0.f;
    float m_run = -1e30f, l_run = 0.f;  // (finite start: a fully masked tile leaves both alone)

    for (int k0 = 0; k0 < N; k0 += KT) {
        __syncthreads();  // the previous tile's fragment reads are done
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) {  // 64 keys x 8 chunks of 8 dims: two chunks per thread
            const int idx = tid + 256 * pc, row = idx >> 3, chunk = idx & 7;
            const int key = k0 + row < N ? k0 + row : N - 1;  // rows past the sequence re-read its last key (masked out below)
            const bf16x8 kv = *reinterpret_cast<const bf16x8*>(kbase + (size_t)key * ldq + 8 * chunk);
            const bf16x8 vv = *reinterpret_cast<const bf16x8*>(vbase + (size_t)key * ldq + 8 * chunk);
            *reinterpret_cast<bf16x8*>(&Ks[row * LDT + 8 * chunk]) = kv;
#pragma unroll
            for (int e = 0; e < 8; ++e) Vt[(8 * chunk + e) * LDT + row] = vv[e];
        }
        if (tid < KT) {
            const int key = k0 + tid;
            Ms[tid] = key < N && (mask == nullptr || mask[(size_t)b * N + key] != 0) ? 1 : 0;
        }
        __syncthreads();

        // ---- S^T = K . Q^T
        f32x16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) s[kb][i] = 0.f;
#pragma unroll
            for (int ds = 0; ds < 4; ++ds) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&Ks[(32 * kb + r) * LDT + 16 * ds + 8 * h]);
                s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ds], s[kb], 0, 0, 0);
            }
        }
        // ---- key validity, row maximum (this lane: one query, 32 of the tile's keys; lane ^ 32 holds the other 32)
        float mt = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t v4 = *reinterpret_cast<const uint32_t*>(&Ms[32 * kb + 8 * g + 4 * h]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x = ((v4 >> (8 * e)) & 0xffu) ? s[kb][4 * g + e] : -INFINITY;
                    s[kb][4 * g + e] = x;
                    mt = fmaxf(mt, x);
                }
            }
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64)) * c;
        const float m_new = fmaxf(m_run, mt);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        // ---- P = exp2(s c - m): fp32 row sum of the undropped P; the dropped P, rounded to bf16, is the B operand of the PV steps
        float rs = 0.f;
        bf16x8 pf[4];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const Philox4 dr = attn_dropout_draws((uint32_t)(k0 >> 2) + 8 * kb + 2 * g + h, dq, dbh, dstream, da.seed);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][4 * g + e], c, -m_new));  // (-inf -> 0)
                    rs += p;
                    pf[2 * kb + (g >> 1)][4 * (g & 1) + e] = (bf16_t)(dr.v[e] >= da.thresh ? p : 0.f);
                }
            }
        l_run = l_run * alpha + rs;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            o_acc[0][i] *= alpha;
            o_acc[1][i] *= alpha;
        }
        // ---- O^T += V^T . P^T: step st covers keys 16 * st .. + 15; contraction slot (h, j) is key 16 * st + 4 * h + (j & 3) + 8 * (j >> 2),
        //      the order the P registers come in
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                const bf16_t* vp = &Vt[(32 * mb + r) * LDT + 16 * st + 4 * h];
                const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vp), hi = *reinterpret_cast<const bf16x4*>(vp + 8);
                const bf16x8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                o_acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[st], o_acc[mb], 0, 0, 0);
            }
    }

    // ---- normalise and store: this lane holds query q0 + r, dims 32 * mb + (i & 3) + 8 * (i >> 2) + 4 * h
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = l_tot > 0.f ? da.rscale / l_tot : 0.f;
    if (q0 + r < N) {
        bf16_t* op = out + (row0 + q0 + r) * ldo + head * 64 + 4 * h;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bf16x4 v4;
#pragma unroll
                for (int e = 0; e < 4; ++e) v4[e] = (bf16_t)(o_acc[mb][4 * g + e] * inv);
                *reinterpret_cast<bf16x4*>(op + 32 * mb + 8 * g) = v4;
            }
    }
}

__global__ void attn_dropout_advance_kernel(uint32_t* base, uint32_t by) { *base += by; }
__global__ void attn_dropout_set_kernel(uint32_t* base, uint32_t value) { *base = value; }

}  // namespace

int launch_attention_dropout(int B, int N, int H, const void* qkv, int ldq, const uint8_t* mask, void* out, int ldo, hipStream_t stream, int bstride,
                             const AttnDropout& drop) {
    if (B <= 0 || N <= 0 || H <= 0) return 0;
    if ((ldq & 7) || (ldo & 7)) return f5_fail(F5_EINVAL, "attention_dropout: ldq and ldo must be multiples of 8");
    if (bstride < N) return f5_fail(F5_EINVAL, "attention_dropout: batch stride below N");
    const dim3 grid(cdiv(N, 128), H, B);
    hipLaunchKernelGGL(attn_dropout_kernel, grid, dim3(256), 0, stream, (const bf16_t*)qkv, ldq, H * 64, mask, (bf16_t*)out, ldo, N, bstride, F5_ATTN_QSCALE,
                       attn_drop_args(drop));
    F5_LAUNCH_CHECK();
    return 0;
}

int launch_attn_dropout_advance(uint32_t* base, uint32_t by, hipStream_t stream) {
    hipLaunchKernelGGL(attn_dropout_advance_kernel, dim3(1), dim3(1), 0, stream, base, by);
    F5_LAUNCH_CHECK();
    return 0;
}

int launch_attn_dropout_set(uint32_t* base, uint32_t value, hipStream_t stream) {
    hipLaunchKernelGGL(attn_dropout_set_kernel, dim3(1), dim3(1), 0, stream, base, value);
    F5_LAUNCH_CHECK();
    return 0;
}
