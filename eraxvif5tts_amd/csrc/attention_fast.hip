// attention_fast.hip -- flash attention for the DiT blocks on gfx950 (bf16 in/out, or fp16 with EL = f16_t; head dim 64, non-causal, key-padding mask;
// reference model/modules.py:483-497): the 64-queries-per-wavefront kernel and the launcher that picks between it and the
// software-pipelined 32-queries-per-wavefront kernel of attention_pipe.hip.
//
// Structure (see /opt/skills/guides/cdna_hip_programming.md, Appendix B "Fused attention prefill"):
//   * one workgroup = 4 wavefronts = 256 queries of one (batch, head); each wave owns TWO 32-query blocks, so every K fragment,
//     V^T fragment, K/V tile refresh and barrier is amortised over 64 queries (profiles/r2_attention_*.txt: on one SIMD the matrix
//     pipe and the vector ALU mostly serialise and the LDS -> VGPR fragment traffic is hidden by neither, so halving the fragment
//     bytes per FLOP is worth more than instruction placement);
//   * swapped QK^T: S^T = K.Q^T with v_mfma_f32_32x32x16_bf16, so a lane holds 16 keys x ONE query per 32-key block: sums (and the
//     rare maximum) are in-register, and the un-normalised P converted to bf16 is directly the B operand of the PV product;
//   * O^T = V^T.P^T: the V^T fragments come from the row-major V tile through ds_read_b64_tr_b16 (hardware transpose);
//   * K tile XOR-swizzled for conflict-free ds_read_b128, V tile swizzled for the transposed reads;
//   * exp2 with the softmax scale folded into one fma, fp32 sums and output accumulators, plain (unpacked) fp32 vector code: the file
//     is built with -fno-slp-vectorize (packed fp32 VALU beside MFMAs is slower, MI355X_MICROARCH.md cycle constants).
// K/V staging, fragment reads and the maximum-free softmax are described at the kernel.
#include "kernels.h"
#include "tuning.h"
#include <type_traits>

typedef __attribute__((address_space(3))) bf16x4* lds_bf16x4_ptr;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

__device__ __forceinline__ float max3_asm(float a, float b, float c) {
    float d;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
template <typename EL> __device__ __forceinline__ bf16x8 pack8(const f32x16& s, int base) {
    float p[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = s[base + j];
    return el_pack_p8<EL>(p);
}

// attn_wide_kernel:
//   * K/V tiles by LDS-DMA (global_load_lds_dwordx4, swizzle on the SOURCE address) through a ring of three tile buffers: tile t+2 is
//     requested at the start of tile t, a counted s_waitcnt vmcnt + ONE raw s_barrier per tile publish tile t+1.  No staging registers,
//     no ds_write, no address arithmetic beyond one 64-bit add per piece (the register-staged refresh cost 19 % of the kernel);
//   * LDS fragment reads as inline asm with hand-counted s_waitcnt lgkmcnt (reads the compiler can see make it drain the LDS-DMA with
//     vmcnt(0) in front of each of them);
//   * NO row maximum on the common path: P = exp2(s*c - m_ref) is taken against the reference the query already has; softmax does not
//     depend on the reference, fp32 / bf16 keep their relative precision at any scale, so all that can go wrong is range.  The row sums
//     are checked against 2^64 once per tile (any P >= 2^64, inf or NaN trips it); only then the wave takes the classic step: scores
//     recomputed from the K tile still in LDS, exact running maximum, rescale of O and l.  The first tile of a block sets the reference
//     to its exact maximum (nothing to rescale yet).  With that the 22-deep max3 chain in front of the exponentials is gone from the
//     steady state (-8 % on its own).
//   * QS build (q arrives multiplied by softmax_scale * log2 e: the scale sits in the weights that project q): the
//     reference is ZERO.  P = exp2(s), no first-tile maximum, no fma in front of the exponential.  Two guards keep the range:
//       high side -- the same per-tile test !(rs < 2^64).  The wave takes the classic step in place (m_run starts at 0, so the new
//         reference is max(0, row maximum)) and from then on runs the subtracting build of the loop (wave-uniform: a branch, no select);
//       low side -- a row whose every score is far below zero underflows against reference 0.  Once per item, behind the last tile: any
//         query whose l is not >= 2^-64 (0 and NaN included) raises one LDS word, one barrier, and the WHOLE workgroup (the four waves
//         share the DMA ring and its barriers) runs the item again the way the other build does: exact first-tile maximum, subtracting
//         numerators.  A tile that underflows inside a row whose total is >= 2^-64 holds less than 2^-60 of the row (64 keys x 2^-126
//         against 2^-64): nothing to do.  A fully masked tile gives rs = 0 legitimately; only the end-of-item test decides.
//     Bounds (both builds): per-lane tile sums stay below 2^64 or the classic step runs, so l_run < nt * 2^64 (2^68 at N = 1024, 2^71 at
//     the 128 tiles of the masked build) and |O| < nt * 2^65 * max|v| per element (two half-waves of keys per tile): inside fp32.
#if defined(F5_ATTN_GUARD_COUNT) && !defined(F5_F16_TU)  // diagnostic build only (tools/attn_guard_count.py): how often the QS build's two guards fire
__device__ unsigned g_attn_guard_count[3];  // [0] items (workgroups) of the QS build, [1] high-side trips (waves), [2] low-side re-runs (workgroups)
extern "C" __attribute__((visibility("default"))) int f5_debug_attn_guard_counts(unsigned* out3, int reset) {
    if (out3 && hipMemcpyFromSymbol(out3, HIP_SYMBOL(g_attn_guard_count), sizeof(g_attn_guard_count)) != hipSuccess) return -1;
    const unsigned zero[3] = {0u, 0u, 0u};
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_attn_guard_count), zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
#define F5_GUARD_COUNT(i, who) \
    if (who) atomicAdd(&g_attn_guard_count[i], 1u)
#else
#define F5_GUARD_COUNT(i, who)
#endif
template <bool MASKED, bool QS, typename EL = bf16_t>
__global__ __launch_bounds__(256, 2) void attn_wide_kernel(const bf16_t* __restrict__ qkv, int ldq, int inner, const uint8_t* __restrict__ mask,
                                                           bf16_t* __restrict__ out, int ldo, int N, int bs /* rows between batch items */, float c) {
    constexpr int KT = 64, QB = 2, TB = KT * 128, NBUF = 3, BUF = 2 * TB, WAVES = 4;
    constexpr int PCS = 8 / WAVES;  // K (and V) pieces per wave per tile
    constexpr int MAXT = 128;  // tiles whose key validity bits fit the LDS table (launcher: N <= 64 * MAXT when masked)
    __shared__ __attribute__((aligned(1024))) char smem[NBUF * BUF + (MASKED ? MAXT * 8 : 0) + (QS ? 16 : 0)];
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NQ = gridDim.x, BH = gridDim.y * gridDim.z;
    int qblk = blockIdx.x, bh = blockIdx.y + blockIdx.z * gridDim.y;
    if ((BH & 7) == 0) {  // XCD-aware order: all query blocks of one (batch, head) share an XCD
        const int id = blockIdx.x + NQ * bh;
        const int xcd = id & 7, j = id >> 3;
        qblk = j % NQ;
        bh = (j / NQ) * 8 + xcd;
    }
    const int b = bh / gridDim.y, head = bh - b * gridDim.y, q0 = qblk * (32 * QB * WAVES) + wave * (32 * QB);
    const int r = lane & 31, h = lane >> 5;
    const bf16_t* base = qkv + (size_t)b * bs * ldq + head * 64;
    const bf16_t* kbase = base + inner;
    const bf16_t* vbase = base + 2 * inner;
    const int nt = (N + KT - 1) / KT;
    if constexpr (QS) c = 1.0f;  // the scale is in q
    unsigned* const vote = reinterpret_cast<unsigned*>(smem + NBUF * BUF + (MASKED ? MAXT * 8 : 0));  // QS: the low-side guard's word
    if constexpr (QS) {
        if (tid == 0) *vote = 0u;  // (published by the prologue's barrier)
        F5_GUARD_COUNT(0, tid == 0);
    }

    // ---- key validity bits of every tile (masked build): one 64-bit word per tile in LDS, written before any DMA is in flight
    unsigned long long* mbits = reinterpret_cast<unsigned long long*>(smem + NBUF * BUF);
    if constexpr (MASKED) {
        for (int i = wave; i < nt; i += WAVES) {
            const int key = i * KT + lane;
            const uint8_t m = key < N ? (mask ? mask[(size_t)b * N + key] : (uint8_t)1) : (uint8_t)0;
            const unsigned long long bits = __ballot(m != 0);
            if (lane == 0) mbits[i] = bits;
        }
    }

    bf16x8 qf[QB][4];
#pragma unroll
    for (int j = 0; j < QB; ++j) {
        int qrow = q0 + 32 * j + r;
        if (qrow >= N) qrow = N - 1;
        const bf16_t* qp = base + (size_t)qrow * ldq + 8 * h;
#pragma unroll
        for (int ds = 0; ds < 4; ++ds) qf[j][ds] = *reinterpret_cast<const bf16x8*>(qp + 16 * ds);
    }

    // ---- K/V tile -> LDS by DMA: a piece is 8 key rows x 128 B (one wave-instruction, 1 KiB); wave w moves pieces w (and w + 4 in the 4-wave build) of K and of V
    const int drow = lane >> 3, dchunk = lane & 7;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const unsigned ldq2 = (unsigned)ldq * 2u;
    unsigned kco[PCS], vco[PCS];  // byte offset of this lane's 16-byte chunk inside the key row, K and V swizzles
#pragma unroll
    for (int pc = 0; pc < PCS; ++pc) {
        const int row = (wv + WAVES * pc) * 8 + drow;
        kco[pc] = (unsigned)((dchunk ^ ((row >> 1) & 7)) << 4);
        vco[pc] = (unsigned)((dchunk ^ (((row >> 1) & 1) << 2)) << 4);
        if constexpr (!MASKED) {  // whole tiles only: the row offset is lane-constant too
            kco[pc] += (unsigned)row * ldq2;
            vco[pc] += (unsigned)row * ldq2;
        }
    }
    auto dma_tile = [&](int k0, int buf) {
        const char* kt = reinterpret_cast<const char*>(kbase) + (MASKED ? (size_t)0 : (size_t)k0 * ldq2);  // wave-uniform
        const char* vt = reinterpret_cast<const char*>(vbase) + (MASKED ? (size_t)0 : (size_t)k0 * ldq2);
#pragma unroll
        for (int pc = 0; pc < PCS; ++pc) {
            const int piece = wv + WAVES * pc;
            unsigned ko = kco[pc], vo = vco[pc];
            if constexpr (MASKED) {  // ragged last tile: rows past the sequence re-read its last key (masked out by the validity bits)
                const unsigned ro = (unsigned)min(k0 + piece * 8 + drow, N - 1) * ldq2;
                ko += ro;
                vo += ro;
            }
            char* dst = smem + buf * BUF + piece * 1024;
            __builtin_amdgcn_global_load_lds((gptr_t)(kt + ko), (lptr_t)dst, 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t)(vt + vo), (lptr_t)(dst + TB), 16, 0, 0);
        }
    };

    // ---- per-lane LDS read addresses (buffer 0; the tile's buffer offset is added per tile)
    const unsigned lds0 = (unsigned)(size_t)(lptr_t)smem;
    // K fragment of d-slice ds: row r, logical 16-byte chunk 2*ds + h at physical chunk (2*ds + h) ^ ((r >> 1) & 7): the address of slice ds
    // is the address of slice 0 with bits 5..6 XORed by ds (the tile buffers are 128-byte aligned), so one register carries all four
    unsigned ka_t = lds0 + r * 128 + ((h ^ ((r >> 1) & 7)) << 4);  // slice 0, buffer of the current tile
    unsigned va[2];
    {
        const int v_row = 4 * h + ((lane & 15) >> 2);
        const int v_colb = (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
        const int sw = ((v_row >> 1) & 1) << 6;
        va[0] = lds0 + TB + v_row * 128 + (v_colb ^ sw);
        va[1] = lds0 + TB + v_row * 128 + ((64 + v_colb) ^ sw);
    }
    unsigned ka[4];
#define F5_KREAD(dst, n) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(ka[(n) & 3]), "n"(((n) >> 2) * 32 * 128))
#define F5_VREAD(dst, s, mb, g) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(va[mb]), "n"((16 * (s) + 8 * (g)) * 128))
#define F5_LWAIT1(cnt, a) asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(cnt))
#define F5_LWAIT2(cnt, a, b2) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b2) : "n"(cnt))
#define F5_LWAIT4(cnt, a, b2, c2, d) asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b2), "+v"(c2), "+v"(d) : "n"(cnt))

    f32x16 o_acc[QB][2];
    float m_run[QB], l_run[QB];
    constexpr int DIST = NBUF - 1;  // tiles requested ahead
    // 2^64 (bf16) / 2^15 (fp16, whose numerators must stay below 65504): per-lane row sums of one tile at or above this take the classic path
    static_assert(!(QS && Elem<EL>::F16), "the reference-free build needs bf16's exponent range");
    constexpr float RANGE_GUARD = Elem<EL>::ATTN_SUM_LOG2 == 64 ? 18446744073709551616.0f : (float)(1u << (Elem<EL>::ATTN_SUM_LOG2 & 31));
    constexpr float LOW_GUARD = 5.421010862427522e-20f;     // 2^-64 (QS): a query's l below this sends the item through the classic loop
#define F5_VMWAIT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
    bool rerun = false;  // QS: the second pass
    int boff = 0, boff2 = DIST * BUF;  // LDS offsets of tile t's buffer and of tile t+DIST's
    for (;;) {  // QS: at most two passes (the second is the low-side re-run); the other build leaves after the first
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            m_run[j] = (QS && !rerun) ? 0.f : -1e30f;
            l_run[j] = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) o_acc[j][0][i] = o_acc[j][1][i] = 0.f;
        }
        // ---- prologue: tiles 0 .. NBUF-2 on their way, tile 0 published
        int k0z = 0;  // laundered (QS): keeps the prologue's DMA addresses from being hoisted out of the pass loop and held across the tile loops
        if constexpr (QS) {
            asm volatile("" : "+s"(k0z));
            asm volatile("" : "+v"(kco[0]), "+v"(kco[1]), "+v"(vco[0]), "+v"(vco[1]), "+v"(ka_t), "+v"(va[0]), "+v"(va[1]));
        }
        dma_tile(k0z, 0);
        if (nt > 1) dma_tile(KT + k0z, 1);
        {
            const int ahead = min(nt, DIST) - 1;  // tiles requested after tile 0
            if (ahead == 0) F5_VMWAIT(0);
            else if (ahead == 1) F5_VMWAIT(2 * PCS);
            else F5_VMWAIT(4 * PCS);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the validity words
        __builtin_amdgcn_s_barrier();

        // one K/V tile; REFD = the numerators subtract m_run (the only form of the other build).  Returns whether the classic step ran.
        auto tile = [&](auto refd_c, const int t) -> bool {
            constexpr bool REFD = decltype(refd_c)::value;
            bool tripped = false;
            if (t + DIST < nt) dma_tile((t + DIST) * KT, boff2 / BUF);
            ka[0] = ka_t;
            ka[1] = ka_t ^ 32u;
            ka[2] = ka_t ^ 64u;
            ka[3] = ka_t ^ 96u;

            // ---- S^T = K . Q^T
            unsigned long long vmv = ~0ull;  // validity of this tile's 64 keys (the same word in every lane)
            if constexpr (MASKED) {
                const unsigned ma = lds0 + NBUF * BUF + 8 * t;
                asm volatile("ds_read_b64 %0, %1" : "=v"(vmv) : "v"(ma));
            }
            bf16x8 kf[4];  // fragments 4..7 reuse the registers of 0..3 as soon as those MFMAs are issued
            F5_KREAD(kf[0], 0); F5_KREAD(kf[1], 1); F5_KREAD(kf[2], 2); F5_KREAD(kf[3], 3);
            f32x16 s[QB][2];
            auto qk = [&](auto& kfr, int n) {
#pragma unroll
                for (int j = 0; j < QB; ++j)
                    s[j][n >> 2] = el_mfma32<EL>(kfr, qf[j][n & 3], (n & 3) ? s[j][n >> 2] : f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f});
            };
            // scheduling fences pin {wait, two MFMAs, next read} groups: left alone the compiler hoists all eight reads (32 registers) above the MFMAs
#define F5_FENCE() __builtin_amdgcn_sched_barrier(0)
            F5_FENCE();
            F5_LWAIT1(3, kf[0]); qk(kf[0], 0); F5_FENCE(); F5_KREAD(kf[0], 4);
            F5_LWAIT1(3, kf[1]); qk(kf[1], 1); F5_FENCE(); F5_KREAD(kf[1], 5);
            F5_LWAIT1(3, kf[2]); qk(kf[2], 2); F5_FENCE(); F5_KREAD(kf[2], 6);
            F5_LWAIT1(3, kf[3]); qk(kf[3], 3); F5_FENCE(); F5_KREAD(kf[3], 7);
            F5_LWAIT1(3, kf[0]); qk(kf[0], 4); F5_FENCE();
            F5_LWAIT1(2, kf[1]); qk(kf[1], 5); F5_FENCE();
            F5_LWAIT1(1, kf[2]); qk(kf[2], 6); F5_FENCE();
            F5_LWAIT1(0, kf[3]); qk(kf[3], 7); F5_FENCE();
            if constexpr (MASKED) F5_LWAIT1(0, vmv);  // ties the validity word to the waits above (it was the oldest read)
            // V^T fragments of the first PV step fly during the softmax
            bf16x4 vf[2][2];  // [mb][g]; the fragments of step s+1 reuse the registers as soon as the MFMAs of step s are issued
            F5_VREAD(vf[0][0], 0, 0, 0); F5_VREAD(vf[0][1], 0, 0, 1); F5_VREAD(vf[1][0], 0, 1, 0); F5_VREAD(vf[1][1], 0, 1, 1);

            auto apply_mask = [&]() {
                if constexpr (MASKED) {
                    if (__builtin_amdgcn_ballot_w64(vmv != ~0ull) != 0ull) {
                        const unsigned long long vmh = h ? (vmv >> 4) : vmv;
#pragma unroll
                        for (int j = 0; j < QB; ++j)
#pragma unroll
                            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                                for (int i = 0; i < 16; ++i) {
                                    const int bit = 32 * kb + (i & 3) + 8 * (i >> 2);
                                    if (!((vmh >> bit) & 1ull)) s[j][kb][i] = -INFINITY;
                                }
                    }
                }
            };
            apply_mask();

            // ---- softmax numerators.  Common path: against the reference the query already has, no maximum.
            float rs[QB] = {0.f, 0.f};
            auto exps0 = [&](int j) {  // QS, reference 0
                float ra = 0.f, rb = 0.f;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; i += 2) {
                        const float x0 = __builtin_amdgcn_exp2f(s[j][kb][i]);
                        const float x1 = __builtin_amdgcn_exp2f(s[j][kb][i + 1]);
                        s[j][kb][i] = x0;
                        s[j][kb][i + 1] = x1;
                        ra += x0;
                        rb += x1;
                    }
                rs[j] = ra + rb;
            };
            auto exps = [&](int j) {
                const float nm = -m_run[j];
                float ra = 0.f, rb = 0.f;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 16; i += 2) {
                        const float x0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[j][kb][i], c, nm));
                        const float x1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s[j][kb][i + 1], c, nm));
                        s[j][kb][i] = x0;
                        s[j][kb][i + 1] = x1;
                        ra += x0;
                        rb += x1;
                    }
                rs[j] = ra + rb;
            };
            auto row_max = [&](int j) {  // scaled maximum of query block j's 64 scores (both half-waves)
                float mx0 = max3_asm(s[j][0][0], s[j][0][1], s[j][0][2]), mx1 = max3_asm(s[j][1][0], s[j][1][1], s[j][1][2]);
#pragma unroll
                for (int i = 3; i < 15; i += 2) {
                    mx0 = max3_asm(mx0, s[j][0][i], s[j][0][i + 1]);
                    mx1 = max3_asm(mx1, s[j][1][i], s[j][1][i + 1]);
                }
                mx0 = max3_asm(mx0, mx1, s[j][0][15]);
                const float mt = max3_asm(mx0, s[j][1][15], s[j][1][15]);
                const auto r2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(mt), __float_as_uint(mt), false, false);
                return fmaxf(__uint_as_float(r2[0]), __uint_as_float(r2[1])) * c;
            };
            if constexpr (!REFD) {
                exps0(0);
                exps0(1);
            } else {
                if (t == 0 && (!QS || rerun)) {  // first tile of the block: the reference is its exact maximum (O and l are still zero: nothing to
                                                 // rescale); -inf (a fully masked tile) leaves the finite start value alone
                    m_run[0] = fmaxf(m_run[0], row_max(0));
                    m_run[1] = fmaxf(m_run[1], row_max(1));
                }
                exps(0);
                exps(1);
            }
            if (__builtin_amdgcn_ballot_w64(!(rs[0] < RANGE_GUARD) || !(rs[1] < RANGE_GUARD)) != 0ull) {
                // some numerator left the guarded range (a score 64 log2 units above its query's reference, inf or NaN): classic step.  The
                // scores were overwritten by the numerators: recompute them (the K tile is still in LDS), move the references to the exact
                // running maxima, rescale O and l
                bf16x8 k2;  // cold path: one fragment at a time
#define F5_REDO(n) F5_KREAD(k2, n); F5_LWAIT1(0, k2); qk(k2, n);
                F5_REDO(0) F5_REDO(1) F5_REDO(2) F5_REDO(3) F5_REDO(4) F5_REDO(5) F5_REDO(6) F5_REDO(7)
#undef F5_REDO
                apply_mask();
#pragma unroll
                for (int j = 0; j < QB; ++j) {
                    const float m_new = fmaxf(m_run[j], row_max(j));
                    const float alpha = __builtin_amdgcn_exp2f(m_run[j] - m_new);
                    m_run[j] = m_new;
                    l_run[j] *= alpha;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        o_acc[j][0][i] *= alpha;
                        o_acc[j][1][i] *= alpha;
                    }
                    exps(j);
                }
                tripped = true;  // (wave-uniform: the ballot decided)
            }
            l_run[0] += rs[0];
            l_run[1] += rs[1];

            // ---- O^T += V^T . P^T: four 16-key steps; each half (32 dims) of the V^T fragment is re-requested for the next step right after
            //      its two MFMAs are issued
            auto pv_half = [&](int st, int mb, const bf16x8 (&pf)[QB]) {
                const bf16x8 vfr = __builtin_shufflevector(vf[mb][0], vf[mb][1], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                for (int j = 0; j < QB; ++j) o_acc[j][mb] = el_mfma32<EL>(vfr, pf[j], o_acc[j][mb]);
            };
#define F5_PV(st, more)                                                                       \
        {                                                                                         \
            bf16x8 pf[QB];                                                                        \
            pf[0] = pack8<EL>(s[0][(st) >> 1], 8 * ((st) & 1));                                       \
            pf[1] = pack8<EL>(s[1][(st) >> 1], 8 * ((st) & 1));                                       \
            F5_FENCE();                                                                           \
            F5_LWAIT2(2, vf[0][0], vf[0][1]);                                                     \
            pv_half(st, 0, pf);                                                                   \
            F5_FENCE();                                                                           \
            if constexpr (more) {                                                                 \
                F5_VREAD(vf[0][0], (st) + 1, 0, 0);                                               \
                F5_VREAD(vf[0][1], (st) + 1, 0, 1);                                               \
            }                                                                                     \
            F5_LWAIT2((more) ? 2 : 0, vf[1][0], vf[1][1]);                                        \
            pv_half(st, 1, pf);                                                                   \
            F5_FENCE();                                                                           \
            if constexpr (more) {                                                                 \
                F5_VREAD(vf[1][0], (st) + 1, 1, 0);                                               \
                F5_VREAD(vf[1][1], (st) + 1, 1, 1);                                               \
            }                                                                                     \
        }
            F5_PV(0, true)
            F5_PV(1, true)
            F5_PV(2, true)
            F5_PV(3, false)
#undef F5_PV

            // ---- publish tile t+1 (requested a whole tile ago) and retire this tile's buffer: every LDS read of this wave has been waited for
            {  // tile t+1 must have landed: the tiles requested after it may stay in flight
                const int ahead = min(nt - 1, t + DIST) - (t + 1);
                if (ahead <= 0) F5_VMWAIT(0);
                else if (ahead == 1) F5_VMWAIT(2 * PCS);
                else F5_VMWAIT(4 * PCS);
            }
            __builtin_amdgcn_s_barrier();
            const int step = boff + BUF == NBUF * BUF ? -(NBUF - 1) * BUF : BUF;  // wave-uniform
            boff += step;
            ka_t += step;
            va[0] += step;
            va[1] += step;
            boff2 = boff2 + BUF == NBUF * BUF ? 0 : boff2 + BUF;
            return tripped;
        };
        // two builds of the loop: reference-free until this wave's first classic step (QS, first pass), subtracting from there on
        int t = 0;
        if constexpr (QS) {
            if (!rerun)
                while (t < nt)
                    if (tile(std::false_type{}, t++)) {
                        F5_GUARD_COUNT(1, lane == 0);
                        break;
                    }
        }
        for (; t < nt; ++t) tile(std::true_type{}, t);
        if constexpr (!QS) {
            break;
        } else {
            if (rerun) break;
            // ---- low-side guard: the loop ended on a barrier with no DMA in flight and every LDS read waited for
            bool low = false;
#pragma unroll
            for (int j = 0; j < QB; ++j) low = low || !(l_run[j] + __shfl_xor(l_run[j], 32, 64) >= LOW_GUARD);
            if (__builtin_amdgcn_ballot_w64(low) != 0ull && lane == 0) *vote = 1u;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (__builtin_amdgcn_readfirstlane(*vote) == 0u) break;
            F5_GUARD_COUNT(2, tid == 0);
            rerun = true;  // the whole item again, classic loop; the ring restarts at buffer 0
            ka_t -= boff;
            va[0] -= boff;
            va[1] -= boff;
            boff = 0;
            boff2 = DIST * BUF;
        }
    }
#undef F5_GUARD_COUNT
#undef F5_KREAD
#undef F5_VREAD
#undef F5_LWAIT1
#undef F5_LWAIT4
#undef F5_VMWAIT
#undef F5_LWAIT2
#undef F5_FENCE

    // ---- normalise; stage the wave's 64 x 64 output block through LDS (the ring is free: the loop ended on a barrier with no DMA in flight)
    //      and store whole 128-byte rows
    int lane_e = lane;  // laundered: keeps the epilogue's lane-constant addresses from being hoisted above the tile loop (and spilled around it)
    asm volatile("" : "+v"(lane_e));
    const int r_e = lane_e & 31, h_e = lane_e >> 5;
    char* stage = smem + wave * (64 * 128);
#pragma unroll
    for (int j = 0; j < QB; ++j) {
        const float l_tot = l_run[j] + __shfl_xor(l_run[j], 32, 64);
        const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const bf16x4 v4 = el_pack4<EL>(o_acc[j][mb][4 * g] * inv, o_acc[j][mb][4 * g + 1] * inv, o_acc[j][mb][4 * g + 2] * inv, o_acc[j][mb][4 * g + 3] * inv);
                const int row = 32 * j + r_e, chunk = (4 * mb + g) ^ (row & 7);
                *reinterpret_cast<bf16x4*>(stage + row * 128 + chunk * 16 + 8 * h_e) = v4;
            }
    }
    {
        bf16_t* obase = out + ((size_t)b * bs + q0) * ldo + head * 64;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int row = 8 * k + (lane_e >> 3), chunk = lane_e & 7;
            const u32x4_t v = *reinterpret_cast<const u32x4_t*>(stage + row * 128 + ((chunk ^ (row & 7)) * 16));
            if (q0 + row < N) *reinterpret_cast<u32x4_t*>(obase + (size_t)row * ldo + chunk * 8) = v;
        }
    }
}


// Compiled as two translation units (build time): attention_fast_f16.hip (#define F5_F16_TU + #include of this file) holds the EL = f16_t
// instantiations of the wide kernel for the fp16 precision mode behind launch_attention_wide_f16(); every host-side rule lives here.
#ifdef F5_F16_TU
#define F5_EL f16_t
#else
#define F5_EL bf16_t
#endif
// the wide kernel's launch for this translation unit's element type
static int launch_wide(bool masked, int B, int N, int H, const void* qkv, int ldq, const uint8_t* mask, void* out, int ldo, hipStream_t stream, int bstride,
                       int qscaled) {
    const float c = qscaled ? 1.0f : F5_ATTN_QSCALE;
    dim3 grid(cdiv(N, 256), H, B);
#define F5_WIDE(M_, Q_) \
    hipLaunchKernelGGL((attn_wide_kernel<M_, Q_, F5_EL>), grid, dim3(256), 0, stream, (const bf16_t*)qkv, ldq, H * 64, mask, (bf16_t*)out, ldo, N, bstride, c)
#ifdef F5_F16_TU
    if (qscaled) return f5_fail(F5_EINVAL, "attention_fast: the fp16 mode takes q as projected");
    if (masked) F5_WIDE(true, false); else F5_WIDE(false, false);
#else
    if (masked) {
        if (qscaled) F5_WIDE(true, true); else F5_WIDE(true, false);
    } else {
        if (qscaled) F5_WIDE(false, true); else F5_WIDE(false, false);
    }
#endif
#undef F5_WIDE
    F5_LAUNCH_CHECK();
    return 0;
}
#ifdef F5_F16_TU
int launch_attention_wide_f16(bool masked, int B, int N, int H, const void* qkv, int ldq, const uint8_t* mask, void* out, int ldo, hipStream_t stream, int bstride,
                              int qscaled) {
    return launch_wide(masked, B, N, H, qkv, ldq, mask, out, ldo, stream, bstride, qscaled);
}
#else

bool attention_fast_supported(int precision, int N, int H) { return (precision == F5_PREC_BF16 || precision == F5_PREC_FP16) && N >= 1 && H >= 1; }

int launch_attention_pipe(int waves, int B, int N, int H, const void* qkv, int ldq, const uint8_t* mask, void* out, int ldo, hipStream_t stream, int bstride,
                          int qscaled);  // attention_pipe.hip

int launch_attention_pipe_segs(bool masked, int nbr, const AttnSegs& segs, int maxN, int H, const void* qkv, int ldq, void* out, int ldo, hipStream_t stream,
                               int bstride, int qscaled);  // attention_pipe.hip
// the fp16 precision mode's instantiations (attention_pipe_f16.hip, attention_fast_f16.hip)
int launch_attention_pipe_f16(int waves, int B, int N, int H, const void* qkv, int ldq, const uint8_t* mask, void* out, int ldo, hipStream_t stream, int bstride,
                              int qscaled);
int launch_attention_pipe_segs_f16(bool masked, int nbr, const AttnSegs& segs, int maxN, int H, const void* qkv, int ldq, void* out, int ldo, hipStream_t stream,
                                   int bstride, int qscaled);
int launch_attention_wide_f16(bool masked, int B, int N, int H, const void* qkv, int ldq, const uint8_t* mask, void* out, int ldo, hipStream_t stream, int bstride,
                              int qscaled);

static int cu_count_cached() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    }
    return cus;
}
// which of the two tuned kernels launch_attention_fast gives a (B, N, H) problem
static bool picks_wide(int B, int N, int H, bool masked, int ldq, int bstride) {
    // 256 queries per workgroup need at least one workgroup per CU to pay; below that (single-utterance serving) the 128-query
    // workgroups of the pipelined kernel fill the chip better (B = 1: 17 vs 23 us)
    bool wide = g_attn_variant == 2 || (g_attn_variant == 0 && (long)B * H * cdiv(N, 256) >= cu_count_cached());
    if (masked && N > 64 * 128) wide = false;  // the wide kernel's table of key validity bits holds 128 tiles
    if ((size_t)N * (size_t)ldq * 2u >= (1ull << 32)) wide = false;  // its per-lane key offsets are 32-bit
    if ((size_t)bstride * (size_t)ldq * 2u >= (1ull << 32)) wide = false;
    return wide;
}

int launch_attention_ragged(int precision, int attn_kernel_opt, const AttnSegs& segs, int H, const void* qkv, int ldq, void* out, int ldo, hipStream_t stream,
                            int bstride, int qscaled, const AttnDropout* drop) {
    if (segs.cnt < 0 || segs.cnt > AttnSegs::MAX || segs.nbr < 1) return f5_fail(F5_EINVAL, "attention_ragged: a table holds at most %d utterances", AttnSegs::MAX);
    const size_t es = precision == F5_PREC_FP32 ? 4 : 2;
    if (drop && drop->prob > 0.0) {  // attention dropout: every utterance its own launch (the shared launches have no dropout build)
        for (int u = 0; u < segs.cnt; ++u) {
            const int nu = segs.n[u];
            const int kind = (attn_kernel_opt != 0 && attention_fast_supported(precision, nu, H)) ? 1 : 0;
            AttnDropout d = *drop;
            d.bw0 = drop->bw0 + (uint32_t)u;
            F5_TRY(launch_attention(precision, kind, segs.nbr, nu, H, (const char*)qkv + (size_t)segs.off[u] * ldq * es, ldq, nullptr,
                                    (char*)out + (size_t)segs.off[u] * ldo * es, ldo, stream, bstride, qscaled, &d));
        }
        return 0;
    }
    AttnSegs grp[2];  // [0] utterances with n % 64 == 0 (unmasked build), [1] the others -- as each one's own launch would pick
    int maxn[2] = {0, 0};
    for (int u = 0; u < segs.cnt; ++u) {
        const int nu = segs.n[u];
        const int kind = (attn_kernel_opt != 0 && attention_fast_supported(precision, nu, H)) ? 1 : 0;
        const bool masked = (nu % 64) != 0;
        if (kind == 1 && (ldq & 7) == 0 && (ldo & 7) == 0 && !picks_wide(segs.nbr, nu, H, masked, ldq, bstride)) {
            AttnSegs& g = grp[masked ? 1 : 0];
            g.nbr = segs.nbr;
            g.off[g.cnt] = segs.off[u];
            g.n[g.cnt++] = nu;
            maxn[masked ? 1 : 0] = std::max(maxn[masked ? 1 : 0], nu);
        } else {  // its own launch: the wide kernel, or the reference kernel
            F5_TRY(launch_attention(precision, kind, segs.nbr, nu, H, (const char*)qkv + (size_t)segs.off[u] * ldq * es, ldq, nullptr,
                                    (char*)out + (size_t)segs.off[u] * ldo * es, ldo, stream, bstride, qscaled));
        }
    }
    for (int k = 0; k < 2; ++k)
        if (grp[k].cnt > 0)
            F5_TRY((precision == F5_PREC_FP16 ? launch_attention_pipe_segs_f16 : launch_attention_pipe_segs)(k == 1, segs.nbr, grp[k], maxn[k], H, qkv, ldq, out, ldo,
                                                                                                             stream, bstride, qscaled));
    return 0;
}

int launch_attention_ragged_all(int precision, int attn_kernel_opt, int nbr, int cnt, const int* off, const int* n, int H, const void* qkv, int ldq, void* out,
                                int ldo, hipStream_t stream, int bstride, int qscaled, const AttnDropout* drop) {
    AttnDropout d;
    if (drop) d = *drop;
    for (int u0 = 0; u0 < cnt; u0 += AttnSegs::MAX) {
        if (drop) d.bw0 = drop->bw0 + (uint32_t)u0;
        AttnSegs sg;
        sg.nbr = nbr;
        for (int u = u0; u < cnt && u < u0 + AttnSegs::MAX; ++u) {
            sg.off[sg.cnt] = off[u];
            sg.n[sg.cnt++] = n[u];
        }
        F5_TRY(launch_attention_ragged(precision, attn_kernel_opt, sg, H, qkv, ldq, out, ldo, stream, bstride, qscaled, drop ? &d : nullptr));
    }
    return 0;
}

int launch_attention_fast(int precision, int B, int N, int H, const void* qkv, int ldq, const uint8_t* mask, void* out, int ldo, hipStream_t stream,
                          int bstride, int qscaled) {
    if ((ldq & 7) || (ldo & 7)) return f5_fail(F5_EINVAL, "attention_fast: ldq and ldo must be multiples of 8");
    const bool h16 = precision == F5_PREC_FP16;
    const bool masked = mask != nullptr || (N % 64) != 0;
    const bool wide = picks_wide(B, N, H, masked, ldq, bstride);
    if (!wide) return (h16 ? launch_attention_pipe_f16 : launch_attention_pipe)(4, B, N, H, qkv, ldq, mask, out, ldo, stream, bstride, qscaled);
    return (h16 ? launch_attention_wide_f16 : launch_wide)(masked, B, N, H, qkv, ldq, mask, out, ldo, stream, bstride, qscaled);
}
#endif
