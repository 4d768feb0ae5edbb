// gemm_w4_probe.hip -- standalone probe of the round-4 "one wave per SIMD" main loop for the block GEMMs (C = A . W^T, bf16, fp32 accumulate):
//   256 x 256 x 64 tiles, 4 waves per workgroup (one per SIMD), 128 x 128 outputs per wave held in 256 AccVGPRs, fragments double-buffered in
//   VGPRs, operands by LDS-DMA (whole 128-byte lines) into TWO 64-KiB stage buffers that are refilled in place two iterations ahead, two
//   barriers per 64-deep iteration, every non-MFMA instruction placed by hand between the MFMAs (inline asm, hand-counted waits).
// The vendor library's best kernel for these shapes has this shape (hipBLASLt "MT256x256x64 ... 4 waves"; measured 17 - 22 % faster than the
// 8-wave staggered kernel of gemm_fast.hip at the four call sites); this file is where the schedule was developed before it moved into the library.
//   hipcc -O3 --offload-arch=gfx950 tools/gemm_w4_probe.hip -o tools/bin/gemm_w4_probe && tools/bin/gemm_w4_probe
// Schedules (template parameter SCHED; main() runs the list in its `for (int sched : {...})`; results under profiles/r4_w4_probe_*.txt):
//    0        first schedule: reads every 3rd MFMA slot, B1 behind 49, requests every 3 from 50, B2 behind 100
//    1 / 3    reads every 2nd slot, B1 behind 40, requests every 3 from 42, B2 behind 86 / 78           (the library's first build)
//    2 / 4    the same with requests every 2 slots                                                     (slower)
//   10 .. 14  timing-only ablations of schedule 1: no requests / no fragment reads / neither / MFMA stream alone / no barriers
//   17 .. 23  store experiments: no stores (17, 20), half-tile start skew of every other workgroup (18, 19), non-temporal stores (22)
//   30 .. 33  read-modify-write epilogue (the in-place residual update): all loads first / with skew / loads only / step-wise
//   40, 41    M0 written one slot ahead of its request (no effect); 41 also requests every 2 slots
//   42 .. 47  sub-step-1 reads in the first 16 slots, requests spread wide (every 4 - 6 slots); 46 = the library's schedule
//   50        deferred stores: half of a tile's packed output leaves during the next tile's first four iterations (slower)
//   60        schedule 46 with the vendor kernel's request form, buffer_load_dwordx4 ... offen lds (no difference)
//   70 .. 73  whole-line epilogue: the MFMA's operand roles swapped (tokens on the row index) and the weight rows permuted on their way into LDS
//             (LDS row 16 i + c of a wave's 128 <- weight row 8 c + i), so that a lane's eight accumulators over i are eight consecutive features of
//             one token and 16 adjacent lanes write 256 contiguous bytes per store.  70: on schedule 46; 71: on schedule 1; 72 / 73: the
//             read-modify-write forms of 30 / 33 in that map (on schedule 1, as they are; 72 loads four token tiles ahead, not all eight)
//   80, 81    the library's in-place residual epilogue IN FULL on schedule 46: C is the fp16 residual stream, x += gate[n] * (acc + bias[n]) with the
//             saturating fp16 pack, bias | gate in LDS, the accumulators started from the bias, the next tile's first fragments read again behind
//             the epilogue, and the LayerNorm fold's partial row statistics (sum (h - pivot), sum (h - pivot)^2 per 64-feature plane) of the values
//             just stored.  80: the library's lane map (resid_tile + emit_stats of csrc/gemm_w4.hip); 81: the whole-line map of 70 for the stream
//             (one 16-byte load and store per lane, token tile and component), the statistics fed in the OLD map through a 4-KiB patch of LDS per
//             wave (ds_write_b128 token-major, chunk c of row t at chunk c ^ t; ds_read_b64 back).  Both produce real values: the error column
//             is against the fp64-free host form of the update on sampled rows, and the statistics of those rows are checked too.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include <type_traits>

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));

template <int N, int I = 0, typename F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}
__device__ __forceinline__ u32x4 pair_swap(bf16x4 a, bf16x4 b) {
    const u32x2 ua = __builtin_bit_cast(u32x2, a), ub = __builtin_bit_cast(u32x2, b);
    const u32x2 s0 = __builtin_amdgcn_permlane16_swap(ua[0], ub[0], false, false);
    const u32x2 s1 = __builtin_amdgcn_permlane16_swap(ua[1], ub[1], false, false);
    return u32x4{s0[0], s1[0], s0[1], s1[1]};
}
__device__ __forceinline__ bf16x4 to_bf16x4(const f32x4& v) { return bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]}; }

// LDS image of one operand of one stage: 256 rows x 128 bytes (64 k), logical 16-byte chunk c of row r at physical chunk c ^ ((r >> 1) & 7):
// every 16-lane group of a ds_read_b128 fragment read (16 rows, chunks q and q ^ 1) then covers the 16 slots of a 256-byte bank row once.
// Layout: [A buffer 0][A buffer 1][W buffer 0][W buffer 1], 32 KiB each, so that the buffer and the 16-row tile are immediate offsets.
constexpr int OPB = 32768;

template <int SCHED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void w4_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W,
                                                                                           bf16_t* __restrict__ C, int M, int N, int K, int lda,
                                                                                           int ldw, int ldc, int tiles_n, int nblocks, int group,
                                                                                           const float* __restrict__ bias, const float* __restrict__ gate,
                                                                                           float* __restrict__ stats, const float* __restrict__ pivot, int stats_ld) {
    constexpr bool RESID = SCHED == 80 || SCHED == 81;                  // the library's in-place epilogue in full
    constexpr bool WLM = (SCHED >= 70 && SCHED <= 73) || SCHED == 81;   // whole-line map: operand roles swapped, weight rows permuted
    constexpr bool L46 = SCHED == 46 || SCHED == 50 || SCHED == 60 || SCHED == 70 || RESID;  // the library's main-loop schedule
    constexpr int EPI_LDS = 4 * OPB, PATCH = EPI_LDS + 16384;           // RESID: bias[N] | gate[N] (N <= 2048), then a 4-KiB patch per wave
    __shared__ __attribute__((aligned(4096))) char smem[4 * OPB + (RESID ? 16384 + 16384 : 0)];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fq = lane >> 4;

    auto tile_mn = [&](int bid, int& tm0, int& tn0) {  // XCD band + L2 patch order of gemm_fast.hip
        const int q = nblocks >> 3, r = nblocks & 7, xcd = bid & 7;
        const int swz = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
        const int gm = group > 0 ? group : 1;
        const int tiles_m_all = nblocks / tiles_n;
        const int grp = swz / (gm * tiles_n);
        const int gsz = min(gm, tiles_m_all - grp * gm);
        const int rin = swz - grp * gm * tiles_n;
        const int tile_n = rin / gsz, tile_m = grp * gm + (rin - tile_n * gsz);
        tm0 = tile_m * 256;
        tn0 = tile_n * 256;
    };
    const int G = gridDim.x;
    const int my_tiles = (nblocks - (int)blockIdx.x + G - 1) / G;
    const int nk = K / 64;
    const int total = my_tiles * nk;

    // ---- DMA: per iteration this wave moves pieces p = wave * 8 + jj (jj = 0..7) of the activation tile and of the weight tile; a piece is 8 rows
    // x 128 bytes (one instruction: lane l -> row l >> 3, physical chunk l & 7).  Constant per-lane byte offsets, the K position sits in the bases.
    unsigned voffA[8], voffW[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        const int row = (wave * 8 + jj) * 8 + (lane >> 3);
        const int logical = (lane & 7) ^ ((row >> 1) & 7);
        voffA[jj] = (unsigned)(row * lda * 2 + logical * 16);
        // whole-line epilogue: LDS row 16 i + c of a wave's 128 features receives weight row 8 c + i (the swizzle stays keyed on the LDS row)
        const int wrow = WLM ? (row & ~127) + 8 * (row & 15) + ((row & 127) >> 4) : row;
        voffW[jj] = (unsigned)(wrow * ldw * 2 + logical * 16);
    }
    const char* baseA;  // DMA front: tile row / feature base at the front's K position
    const char* baseW;
    int f_tile = blockIdx.x, f_k = 0, f_g = 0;
    auto front_tile = [&]() {
        int sm, sn;
        tile_mn(f_tile, sm, sn);
        baseA = reinterpret_cast<const char*>(A) + (size_t)sm * lda * 2;
        baseW = reinterpret_cast<const char*>(W) + (size_t)sn * ldw * 2;
    };
    front_tile();
    const int wdst = wave * 8192;  // this wave's pieces inside an operand buffer
    typedef __attribute__((ext_vector_type(4))) int i32x4;
    auto dma = [&](int ldsdst, unsigned voff, const char* base) {
        if constexpr (SCHED == 60) {  // the vendor kernel's request form: buffer_load ... lds through a raw buffer descriptor (base, no stride, 4 GiB, dword3 0x00020000)
            const unsigned long long b = (unsigned long long)base;
            const i32x4 rsrc = {(int)(unsigned)b, (int)(unsigned)(b >> 32) & 0xffff, -1, 0x00020000};
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(ldsdst), "v"(voff), "s"(rsrc) : "memory");
        } else {
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(ldsdst), "v"(voff), "s"(base) : "memory");
        }
    };
    auto front_advance = [&]() {
        ++f_g;
        baseA += 128;
        baseW += 128;
        if (++f_k == nk) {
            f_k = 0;
            f_tile += G;
            if (f_tile < nblocks) front_tile();
        }
    };
    // ---- fragment read addresses (LDS byte addresses; the 16-row tile index and the buffer are immediate offsets)
    const unsigned lds0 = (unsigned)(size_t)smem;
    const unsigned ra0 = lds0 + (unsigned)((wm * 128 + fr) * 128 + ((fq ^ (fr >> 1)) * 16));  // sub-step 0: chunks 0..3
    const unsigned ra1 = ra0 ^ 64u;                                                             // sub-step 1: chunks 4..7
    const unsigned rw0 = lds0 + 2 * OPB + (unsigned)((wn * 128 + fr) * 128 + ((fq ^ (fr >> 1)) * 16));
    const unsigned rw1 = rw0 ^ 64u;

    f32x4 acc[8][8];  // [feature tile][token tile], AccVGPRs
    f32x4 fw[2][8], fa[2][8];
    auto zero_acc = [&]() {
        static_for<8>([&](auto ic) {
            static_for<8>([&](auto jc) { acc[decltype(ic)::value][decltype(jc)::value] = f32x4{0.f, 0.f, 0.f, 0.f}; });
        });
    };
#define DSR(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
    // read fragment e (0..7: weight tiles, 8..15: token tiles) of sub-step S from buffer X
    auto rd = [&](auto sc, auto xc, auto ec) {
        constexpr int S = decltype(sc)::value, X = decltype(xc)::value, e = decltype(ec)::value;
        (void)fw; (void)fa; (void)ra0; (void)ra1; (void)rw0; (void)rw1;  // (asm operands alone do not capture inside a generic lambda)
        if constexpr (e < 8) {
            if constexpr (S == 0) DSR(fw[0][e], rw0, X * OPB + e * 2048); else DSR(fw[1][e], rw1, X * OPB + e * 2048);
        } else {
            if constexpr (S == 0) DSR(fa[0][e - 8], ra0, X * OPB + (e - 8) * 2048); else DSR(fa[1][e - 8], ra1, X * OPB + (e - 8) * 2048);
        }
    };
    // one 64-deep iteration on buffer X.  ISSUE: the DMA front still has stages to request; WAITV: the next iteration's stage must be waited for
    // (not in a tile's first iteration: everything requested before the epilogue was waited for there).
    // deferred stores (schedules 50 / 51): half of a tile's output stays in 64 registers and leaves during the NEXT tile's first four iterations
    u32x4 dq[16];
    const char* dbase = reinterpret_cast<const char*>(C);
    unsigned doff[4] = {0u, 0u, 0u, 0u};
    auto body = [&](auto xc, auto issuec, auto waitc, auto stc) {
        constexpr int ST = decltype(stc)::value;  // -1: none, 0..3: this iteration stores dq[4 ST .. 4 ST + 3]
        constexpr int X = decltype(xc)::value;
        constexpr bool ISSUE = decltype(issuec)::value, WAITV = decltype(waitc)::value;
        // schedule: RD1 = the 16 fragment reads of sub-step 1 at MFMA slots R1S * k; B1 (lgkmcnt(0) + barrier) behind slot B1P; the 16 DMA requests at
        // slots D0 + DS * k; B2 (counted vmcnt + barrier) behind slot B2P; RD0 = the next iteration's first fragments at slots R0 + R0S * k
        // SCHED >= 10: timing-only ablations of schedule 1 (wrong results): 10 no DMA requests, 11 no fragment reads, 12 neither, 13 neither and no
        // barriers / waits (MFMA stream alone), 14 everything but the barriers
        // 17: MFMA stream alone, epilogue without its stores; 18: MFMA stream alone, half of the workgroups start half a tile late; 19: schedule 1
        // with that start skew; 20: schedule 1 without the stores
        constexpr bool NO_DMA = SCHED == 10 || SCHED == 12 || SCHED == 13 || SCHED == 17 || SCHED == 18, NO_RD = SCHED == 11 || NO_DMA && SCHED != 10, NO_BAR = SCHED == 13 || SCHED == 14 || SCHED == 17 || SCHED == 18;
        constexpr bool M0E = SCHED == 40 || SCHED == 41;
        constexpr bool S42 = (SCHED >= 42 && SCHED <= 47) || SCHED == 50 || SCHED == 51 || SCHED == 60 || SCHED == 70 || RESID;  // family of schedule 42: reads of sub-step 1 in the first 16 slots, requests spread wide
        constexpr int R1S = SCHED == 0 ? 3 : (S42 ? 1 : 2), B1P = SCHED == 0 ? 49 : (S42 ? (L46 ? 20 : 24) : 40), D0 = SCHED == 0 ? 50 : (S42 ? (L46 ? 22 : 26) : 42), DS = (SCHED == 2 || SCHED == 4 || SCHED == 41) ? 2 : (SCHED == 43 ? 5 : (SCHED == 44 || L46 ? 6 : (S42 ? 4 : 3)));
        constexpr int B2P = SCHED == 0 ? 100 : (SCHED == 3 || SCHED == 4 ? 78 : (SCHED == 45 ? 104 : (SCHED == 47 ? 94 : 86))), R0 = B2P + 2, R0S = SCHED == 0 ? 0 : (SCHED == 45 ? 1 : 2);
        static_for<128>([&](auto nc) {
            (void)acc; (void)fw; (void)fa;
            constexpr int n = decltype(nc)::value;
            constexpr int s = n / 64, i = (n % 64) / 8, j = n % 8;
            if constexpr (WLM)  // tokens on the row index: a lane holds tokens 4 fq + r of the feature its LDS row carries
                asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[i][j]) : "v"(fa[s][j]), "v"(fw[s][i]));
            else
                asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[i][j]) : "v"(fw[s][i]), "v"(fa[s][j]));
            if constexpr (!NO_RD && n < 16 * R1S && n % R1S == 0) rd(std::integral_constant<int, 1>{}, xc, std::integral_constant<int, n / R1S>{});
            if constexpr (n == B1P && !NO_BAR) {  // B1: every wave is done with buffer X
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            }
            if constexpr (M0E && ISSUE && n + 1 >= D0 && n + 1 < D0 + 16 * DS && (n + 1 - D0) % DS == 0) {  // M0 one slot ahead of its request
                constexpr int pc = (n + 1 - D0) / DS;
                const int dst = pc < 8 ? X * OPB + wdst + pc * 1024 : 2 * OPB + X * OPB + wdst + (pc - 8) * 1024;
                asm volatile("s_mov_b32 m0, %0" ::"s"(dst));
            }
            if constexpr (M0E && ISSUE && n >= D0 && n < D0 + 16 * DS && (n - D0) % DS == 0) {
                constexpr int pc = (n - D0) / DS;
                if constexpr (pc < 8)
                    asm volatile("global_load_lds_dwordx4 %0, %1" ::"v"(voffA[pc]), "s"(baseA) : "memory");
                else
                    asm volatile("global_load_lds_dwordx4 %0, %1" ::"v"(voffW[pc - 8]), "s"(baseW) : "memory");
            }
            if constexpr (!M0E && ISSUE && !NO_DMA && n >= D0 && n < D0 + 16 * DS && (n - D0) % DS == 0) {
                constexpr int pc = (n - D0) / DS;
                if constexpr (pc < 8)
                    dma(X * OPB + wdst + pc * 1024, voffA[pc], baseA);
                else
                    dma(2 * OPB + X * OPB + wdst + (pc - 8) * 1024, voffW[pc - 8], baseW);
            }
            if constexpr (n == B2P && !NO_BAR) {  // B2: the other buffer (next iteration's stage) has landed for everyone
                constexpr int issued = (!ISSUE || NO_DMA) ? 0 : (B2P < D0 ? 0 : ((B2P - D0) / DS + 1 > 16 ? 16 : (B2P - D0) / DS + 1));  // this iteration's requests so far
                if constexpr (WAITV)
                    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(issued) : "memory");
                else
                    asm volatile("s_barrier" ::: "memory");
            }
            if constexpr (R0S == 0) {
                if constexpr (n >= 102 && n < 126) {
                    constexpr int a = n - 102;  // 24 slots, 16 reads: slots 0,1,3,4,6,7,...
                    if constexpr (a % 3 != 2) rd(std::integral_constant<int, 0>{}, std::integral_constant<int, 1 - X>{}, std::integral_constant<int, a - a / 3>{});
                }
            } else {
                if constexpr (!NO_RD && n >= R0 && n < R0 + 16 * R0S && (n - R0) % R0S == 0)
                    rd(std::integral_constant<int, 0>{}, std::integral_constant<int, 1 - X>{}, std::integral_constant<int, (n - R0) / R0S>{});
            }
            if constexpr (ST >= 0 && n >= 90 && n < 122 && (n - 90) % 8 == 0) {
                constexpr int k = (n - 90) / 8;
                (void)dq; (void)doff; (void)dbase;
                if constexpr (k == 0) asm volatile("global_store_dwordx4 %0, %1, %2" ::"v"(doff[ST]), "v"(dq[4 * ST + 0]), "s"(dbase) : "memory");
                if constexpr (k == 1) asm volatile("global_store_dwordx4 %0, %1, %2 offset:64" ::"v"(doff[ST]), "v"(dq[4 * ST + 1]), "s"(dbase) : "memory");
                if constexpr (k == 2) asm volatile("global_store_dwordx4 %0, %1, %2 offset:128" ::"v"(doff[ST]), "v"(dq[4 * ST + 2]), "s"(dbase) : "memory");
                if constexpr (k == 3) asm volatile("global_store_dwordx4 %0, %1, %2 offset:192" ::"v"(doff[ST]), "v"(dq[4 * ST + 3]), "s"(dbase) : "memory");
            }
            if constexpr (n == 127) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        });
        if constexpr (ISSUE) front_advance();
    };

    // ---- prologue: stages 0 and 1 requested, stage 0 landed, first fragments read
    auto issue_all = [&](int X) {
#pragma unroll
        for (int pc = 0; pc < 8; ++pc) dma(X * OPB + wdst + pc * 1024, voffA[pc], baseA);
#pragma unroll
        for (int pc = 0; pc < 8; ++pc) dma(2 * OPB + X * OPB + wdst + pc * 1024, voffW[pc], baseW);
    };
    if constexpr (SCHED == 18 || SCHED == 19 || SCHED == 31) {
        if ((blockIdx.x >> 3) & 1)
            for (int i = 0; i < K / 340; ++i) __builtin_amdgcn_s_sleep(127);  // 64 x 127 cycles each: about half a tile at K = 1024
    }
    if constexpr (RESID) {  // bias[N] | gate[N] of the launch into LDS (visible to every wave behind the prologue's barrier)
        float* lb = reinterpret_cast<float*>(smem + EPI_LDS);
        for (int i = tid; i < N; i += 256) {
            lb[i] = bias[i];
            lb[N + i] = gate[i];
        }
    }
    issue_all(0);
    front_advance();
    issue_all(1);
    front_advance();
    if constexpr (RESID) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
    static_for<16>([&](auto ec) { rd(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, ec); });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    int m0, n0;
    tile_mn(blockIdx.x, m0, n0);
    [[maybe_unused]] const float* const lds_bias = reinterpret_cast<const float*>(smem + EPI_LDS);
    [[maybe_unused]] const float* const lds_gate = lds_bias + N;
    // RESID: every accumulator starts from its feature's bias, read from the LDS image (lane indices through an opaque asm: the address is
    // otherwise kept across the main loop)
    auto start_acc = [&](int tn0) {
        if constexpr (!RESID) {
            zero_acc();
        } else {
            int lid = lane;
            asm volatile("" : "+v"(lid));
            if constexpr (SCHED == 81) {
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(lds_bias + tn0 + wn * 128 + 8 * (lid & 15));
                const f32x4 b1 = *reinterpret_cast<const f32x4*>(lds_bias + tn0 + wn * 128 + 8 * (lid & 15) + 4);
                asm volatile("" ::"v"(b0), "v"(b1));
                static_for<8>([&](auto ic) {
                    static_for<8>([&](auto jc) {
                        constexpr int i = decltype(ic)::value;
                        const float b = i < 4 ? b0[i & 3] : b1[i & 3];
                        acc[i][decltype(jc)::value] = f32x4{b, b, b, b};
                    });
                });
            } else {
                f32x4 bn[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) bn[i] = *reinterpret_cast<const f32x4*>(lds_bias + tn0 + wn * 128 + i * 16 + 4 * (lid >> 4));
                static_for<8>([&](auto ic) {
                    static_for<8>([&](auto jc) { acc[decltype(ic)::value][decltype(jc)::value] = bn[decltype(ic)::value]; });
                });
            }
        }
    };
    start_acc(n0);
#define W4_ACC(i, j)                                                                         \
    ([&]() -> f32x4 {                                                                        \
        float c0_, c1_, c2_, c3_;                                                            \
        asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(c0_) : "a"(acc[i][j][0]));           \
        asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(c1_) : "a"(acc[i][j][1]));           \
        asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(c2_) : "a"(acc[i][j][2]));           \
        asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(c3_) : "a"(acc[i][j][3]));           \
        return f32x4{c0_, c1_, c2_, c3_};                                                    \
    }())
    // ---- schedules 80 / 81: the in-place epilogues of csrc/gemm_w4.hip (resid_tile / resid_tile_wl there; no row mask here)
    [[maybe_unused]] auto widen_h = [](unsigned lo, unsigned hi) __attribute__((always_inline)) {
        const f16x4_t hv = __builtin_bit_cast(f16x4_t, u32x2{lo, hi});
        return f32x4{(float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]};
    };
    [[maybe_unused]] auto to_h16 = [](const f32x4& v) __attribute__((always_inline)) {  // saturating fp16 store form
        f16x4_t hv;
#pragma unroll
        for (int e = 0; e < 4; ++e) hv[e] = (_Float16)__builtin_amdgcn_fmed3f(v[e], -65504.0f, 65504.0f);
        return hv;
    };
    [[maybe_unused]] auto emit_stats = [&](int fq, int nb, int m /* row inside the wave's 128 */, float pv, const f32x4& h0, const f32x4& h1, const f32x4& h2, const f32x4& h3) {
        const f32x4 npv{-pv, -pv, -pv, -pv};
        const f32x4 d0 = h0 + npv, d1 = h1 + npv, d2 = h2 + npv, d3 = h3 + npv;
        const f32x4 a = (d0 + d1) + (d2 + d3);
        const f32x4 q = __builtin_elementwise_fma(d3, d3, __builtin_elementwise_fma(d2, d2, __builtin_elementwise_fma(d1, d1, d0 * d0)));
        const float s1 = (a[0] + a[1]) + (a[2] + a[3]), s2 = (q[0] + q[1]) + (q[2] + q[3]);
        float a0 = s1, b0 = s2;
        asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a0), "+v"(b0));
        float t = a0 + b0, z = 0.0f;
        asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(t), "+v"(z));
        const float tot = t + z;
        if (fq < 2) {
            char* sb = reinterpret_cast<char*>(stats + ((size_t)(nb >> 6) * stats_ld + (m0 + wm * 128)) * 2);  // (scalar base + 32-bit lane offset)
            *reinterpret_cast<float*>(sb + (unsigned)((m * 2 + fq) * 4)) = tot;
        }
    };
    [[maybe_unused]] auto resid_old = [&]() {  // schedule 80
        int fr = lane & 15, fq = lane >> 4;
        asm volatile("" : "+v"(fr), "+v"(fq));
        char* const sbase = reinterpret_cast<char*>(C) + ((size_t)(m0 + wm * 128) * ldc + n0 + wn * 128) * 2;
        unsigned offj[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) offj[j] = (unsigned)(((fr + 16 * j) * ldc + 16 * (fq & 1) + 8 * (fq >> 1)) * 2);
        float piv[8];
        const float* pbase = pivot + (size_t)(m0 + wm * 128) * 2;
#pragma unroll
        for (int j = 0; j < 8; ++j) piv[j] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(pbase) + (unsigned)((fr + 16 * j) * 8));
        u32x4 xs[2][8][2];
        auto load_step = [&](auto sc) __attribute__((always_inline)) {
            constexpr int h = decltype(sc)::value / 8, j = decltype(sc)::value % 8;
            xs[h][j][0] = *reinterpret_cast<const u32x4*>(sbase + offj[j] + h * 128);
            xs[h][j][1] = *reinterpret_cast<const u32x4*>(sbase + offj[j] + h * 128 + 64);
        };
        constexpr int AHEAD = 4;
        static_for<AHEAD>([&](auto sc) { load_step(sc); });
        __builtin_amdgcn_sched_barrier(0);
        f32x4 g4[4];
        static_for<16>([&](auto sc) __attribute__((always_inline)) {
            constexpr int h = decltype(sc)::value / 8, j = decltype(sc)::value % 8;
            const int nb = n0 + wn * 128 + h * 64;
            if constexpr (j == 0) {
#pragma unroll
                for (int ii = 0; ii < 4; ++ii) g4[ii] = *reinterpret_cast<const f32x4*>(lds_gate + nb + ii * 16 + 4 * fq);
            }
            f32x4 x0, x1, x2, x3;
            {
                const u32x4 q = xs[h][j][0];
                const u32x2 s0 = __builtin_amdgcn_permlane16_swap(q[0], q[2], false, false);
                const u32x2 s1 = __builtin_amdgcn_permlane16_swap(q[1], q[3], false, false);
                x0 = widen_h(s0[0], s1[0]);
                x1 = widen_h(s0[1], s1[1]);
            }
            {
                const u32x4 q = xs[h][j][1];
                const u32x2 s0 = __builtin_amdgcn_permlane16_swap(q[0], q[2], false, false);
                const u32x2 s1 = __builtin_amdgcn_permlane16_swap(q[1], q[3], false, false);
                x2 = widen_h(s0[0], s1[0]);
                x3 = widen_h(s0[1], s1[1]);
            }
            const f32x4 a0 = W4_ACC(h * 4 + 0, j), a1 = W4_ACC(h * 4 + 1, j), a2 = W4_ACC(h * 4 + 2, j), a3 = W4_ACC(h * 4 + 3, j);
            const f32x4 v0 = __builtin_elementwise_fma(a0, g4[0], x0), v1 = __builtin_elementwise_fma(a1, g4[1], x1), v2 = __builtin_elementwise_fma(a2, g4[2], x2),
                        v3 = __builtin_elementwise_fma(a3, g4[3], x3);
            const f16x4_t h0 = to_h16(v0), h1 = to_h16(v1), h2 = to_h16(v2), h3 = to_h16(v3);
            *reinterpret_cast<u32x4*>(sbase + offj[j] + h * 128) = pair_swap(__builtin_bit_cast(bf16x4, h0), __builtin_bit_cast(bf16x4, h1));
            *reinterpret_cast<u32x4*>(sbase + offj[j] + h * 128 + 64) = pair_swap(__builtin_bit_cast(bf16x4, h2), __builtin_bit_cast(bf16x4, h3));
            auto h_f32 = [](const f16x4_t& hv) __attribute__((always_inline)) { return f32x4{(float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]}; };
            emit_stats(fq, nb, fr + 16 * j, piv[j], h_f32(h0), h_f32(h1), h_f32(h2), h_f32(h3));
            if constexpr (decltype(sc)::value + AHEAD < 16) load_step(std::integral_constant<int, decltype(sc)::value + AHEAD>{});
            __builtin_amdgcn_sched_barrier(0);
        });
    };
    [[maybe_unused]] auto resid_wl = [&]() {  // schedule 81
        int lid = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        asm volatile("" : "+v"(lid));
        const int fc = lid & 15, fq = lid >> 4;
        typedef __attribute__((address_space(1))) char gchar;
        typedef __attribute__((address_space(1))) u32x4 gu32x4;
        gchar* sst = (gchar*)(reinterpret_cast<char*>(C) + ((size_t)(m0 + wm * 128) * ldc + n0 + wn * 128) * 2);
        const gchar* sld = sst;
        const size_t jstride = (size_t)ldc * 32;
        unsigned offr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) offr[r] = (unsigned)(((4 * fq + r) * ldc + 8 * fc) * 2);
        float piv[8];
        const char* pbase = reinterpret_cast<const char*>(pivot + (size_t)(m0 + wm * 128) * 2);
#pragma unroll
        for (int j = 0; j < 8; ++j) piv[j] = *reinterpret_cast<const float*>(pbase + (unsigned)((fc + 16 * j) * 8));
        char* const patch = smem + PATCH + wave * 4096;
        const unsigned wof = (unsigned)(4 * fq * 256 + ((fc ^ (4 * fq)) * 16));
        const unsigned rof = (unsigned)(fc * 256 + ((fc >> 1) & 7) * 32 + (((fq >> 1) ^ (fc & 1)) * 16) + (fq & 1) * 8);
        constexpr int AHEAD = 6;
        u32x4 xs[32];
        auto load_step = [&](auto sc) __attribute__((always_inline)) {
            constexpr int r = decltype(sc)::value % 4;
            xs[decltype(sc)::value] = *(const gu32x4*)(sld + offr[r]);
            if constexpr (r == 3) {
                sld += jstride;
                asm volatile("" : "+s"(sld));
            }
        };
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(lds_gate + n0 + wn * 128 + 8 * fc), g1 = *reinterpret_cast<const f32x4*>(lds_gate + n0 + wn * 128 + 8 * fc + 4);
        static_for<AHEAD>([&](auto sc) { load_step(sc); });
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::"v"(g0), "v"(g1));
        u32x2 rb[8];
        auto read_back = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int hi = 0; hi < 8; ++hi) rb[hi] = *reinterpret_cast<const u32x2*>(patch + (rof ^ (unsigned)(hi * 32)));
        };
        auto stats_of = [&](int j) __attribute__((always_inline)) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
                emit_stats(fq, n0 + wn * 128 + h * 64, fc + 16 * j, piv[j], widen_h(rb[h * 4][0], rb[h * 4][1]), widen_h(rb[h * 4 + 1][0], rb[h * 4 + 1][1]),
                           widen_h(rb[h * 4 + 2][0], rb[h * 4 + 2][1]), widen_h(rb[h * 4 + 3][0], rb[h * 4 + 3][1]));
        };
        static_for<8>([&](auto jc) __attribute__((always_inline)) {
            constexpr int j = decltype(jc)::value;
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("" : "+v"(offr[0]), "+v"(offr[1]), "+v"(offr[2]), "+v"(offr[3]));
            f32x4 a[8];
            static_for<8>([&](auto ic) { a[decltype(ic)::value] = W4_ACC(decltype(ic)::value, j); });
            static_for<4>([&](auto rc) __attribute__((always_inline)) {
                constexpr int r = decltype(rc)::value, s = 4 * j + r;
                const u32x4 x = xs[s];
                const f32x4 x0 = widen_h(x[0], x[1]), x1 = widen_h(x[2], x[3]);
                const f32x4 v0 = __builtin_elementwise_fma(f32x4{a[0][r], a[1][r], a[2][r], a[3][r]}, g0, x0),
                            v1 = __builtin_elementwise_fma(f32x4{a[4][r], a[5][r], a[6][r], a[7][r]}, g1, x1);
                const u32x2 q0 = __builtin_bit_cast(u32x2, to_h16(v0)), q1 = __builtin_bit_cast(u32x2, to_h16(v1));
                const u32x4 q{q0[0], q0[1], q1[0], q1[1]};
                *(gu32x4*)(sst + offr[r]) = q;
                *reinterpret_cast<u32x4*>(patch + (wof ^ (unsigned)(16 * r)) + 256 * r) = q;
                if constexpr (s + AHEAD < 32) load_step(std::integral_constant<int, s + AHEAD>{});
            });
            sst += jstride;
            asm volatile("" : "+s"(sst));
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (j > 0) stats_of(j - 1);
            __builtin_amdgcn_sched_barrier(0);
            read_back();
            if constexpr (j == 7) stats_of(j);
            __builtin_amdgcn_sched_barrier(0);
        });
    };
    auto epilogue = [&]() {
        bf16_t* orow = C + (size_t)(m0 + wm * 128 + fr) * ldc + n0 + wn * 128 + 16 * (fq & 1) + 8 * (fq >> 1);
        if constexpr (SCHED == 50 || SCHED == 51) {
            // token tiles 0..3 leave now, 4..7 are kept (already packed) for the next tile's iterations 0..3
            static_for<8>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                __builtin_amdgcn_sched_barrier(0);
                static_for<4>([&](auto hc) {
                    constexpr int i = decltype(hc)::value * 2;
                    asm volatile("" : "+a"(acc[i][j]));
                    asm volatile("" : "+a"(acc[i + 1][j]));
                    const u32x4 q = pair_swap(to_bf16x4(acc[i][j]), to_bf16x4(acc[i + 1][j]));
                    if constexpr (j < 4)
                        *reinterpret_cast<u32x4*>(orow + (size_t)16 * j * ldc + 32 * (i / 2)) = q;
                    else
                        dq[(j - 4) * 4 + i / 2] = q;
                });
            });
            dbase = reinterpret_cast<const char*>(C + (size_t)(m0 + wm * 128) * ldc + n0 + wn * 128);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) doff[jj] = (unsigned)(((fr + 16 * (jj + 4)) * ldc + 16 * (fq & 1) + 8 * (fq >> 1)) * 2);
            return;
        }
        if constexpr (SCHED == 80) {
            resid_old();
            return;
        }
        if constexpr (SCHED == 81) {
            resid_wl();
            return;
        }
        if constexpr (SCHED >= 70 && SCHED <= 73) {
            // whole-line map: lane (fq, fr) holds tokens 16 j + 4 fq + r and features 8 fr + i; per (j, r) one 16-byte store, 16 adjacent lanes
            // cover 256 contiguous bytes, an instruction 4 token rows x 256 bytes.  72: the stream loads four token tiles ahead of their use; 73: step-wise
            bf16_t* wrow = C + (size_t)(m0 + wm * 128 + 4 * fq) * ldc + n0 + wn * 128 + 8 * fr;
            [[maybe_unused]] u32x4 xs[8][4];
            if constexpr (SCHED == 72) {  // (all eight token tiles ahead do not fit beside the 32 unpacked values of a step: four ahead)
                static_for<4>([&](auto jc) {
                    static_for<4>([&](auto rc) {
                        constexpr int j = decltype(jc)::value, r = decltype(rc)::value;
                        xs[j][r] = *reinterpret_cast<const u32x4*>(wrow + (size_t)(16 * j + r) * ldc);
                    });
                });
                __builtin_amdgcn_sched_barrier(0);
            }
            static_for<8>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                __builtin_amdgcn_sched_barrier(0);
                f32x4 v[8];
                static_for<8>([&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    asm volatile("" : "+a"(acc[i][j]));
                    v[i] = acc[i][j];
                });
                static_for<4>([&](auto rc) {
                    constexpr int r = decltype(rc)::value;
                    if constexpr (SCHED == 73) xs[j][r] = *reinterpret_cast<const u32x4*>(wrow + (size_t)(16 * j + r) * ldc);
                    if constexpr (SCHED == 72 && j >= 4) xs[j][r] = xs[j - 4][r];
                    f32x4 a{v[0][r], v[1][r], v[2][r], v[3][r]}, b{v[4][r], v[5][r], v[6][r], v[7][r]};
                    if constexpr (SCHED >= 72) {
                        const u32x4 x = xs[j][r];
                        a[0] += __builtin_bit_cast(float, x[0] << 16); a[1] += __builtin_bit_cast(float, x[0] & 0xffff0000u);
                        a[2] += __builtin_bit_cast(float, x[1] << 16); a[3] += __builtin_bit_cast(float, x[1] & 0xffff0000u);
                        b[0] += __builtin_bit_cast(float, x[2] << 16); b[1] += __builtin_bit_cast(float, x[2] & 0xffff0000u);
                        b[2] += __builtin_bit_cast(float, x[3] << 16); b[3] += __builtin_bit_cast(float, x[3] & 0xffff0000u);
                    }
                    const u32x2 qa = __builtin_bit_cast(u32x2, to_bf16x4(a)), qb = __builtin_bit_cast(u32x2, to_bf16x4(b));
                    *reinterpret_cast<u32x4*>(wrow + (size_t)(16 * j + r) * ldc) = u32x4{qa[0], qa[1], qb[0], qb[1]};
                    if constexpr (SCHED == 72 && j < 4) xs[j][r] = *reinterpret_cast<const u32x4*>(wrow + (size_t)(16 * (j + 4) + r) * ldc);
                });
            });
            return;
        }
        if constexpr (SCHED >= 30 && SCHED <= 34) {
            // read-modify-write of the output tile (the in-place residual update of the library): 30 every load before the first store, 31 the
            // same behind a half-tile start skew of every other workgroup, 32 loads only, 33 each step's loads just ahead of its stores
            u32x4 xs[8][4];
            if constexpr (SCHED != 33) {
                static_for<8>([&](auto jc) {
                    static_for<4>([&](auto hc) {
                        constexpr int j = decltype(jc)::value, hh = decltype(hc)::value;
                        xs[j][hh] = *reinterpret_cast<const u32x4*>(orow + (size_t)16 * j * ldc + 32 * hh);
                    });
                });
                __builtin_amdgcn_sched_barrier(0);
            }
            static_for<8>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                __builtin_amdgcn_sched_barrier(0);
                static_for<4>([&](auto hc) {
                    constexpr int hh = decltype(hc)::value, i = hh * 2;
                    if constexpr (SCHED == 33) xs[j][hh] = *reinterpret_cast<const u32x4*>(orow + (size_t)16 * j * ldc + 32 * hh);
                    asm volatile("" : "+a"(acc[i][j]));
                    asm volatile("" : "+a"(acc[i + 1][j]));
                    const u32x4 x = xs[j][hh];
                    f32x4 a = acc[i][j], b = acc[i + 1][j];
                    a[0] += __builtin_bit_cast(float, x[0] << 16); a[1] += __builtin_bit_cast(float, x[0] & 0xffff0000u);
                    a[2] += __builtin_bit_cast(float, x[1] << 16); a[3] += __builtin_bit_cast(float, x[1] & 0xffff0000u);
                    b[0] += __builtin_bit_cast(float, x[2] << 16); b[1] += __builtin_bit_cast(float, x[2] & 0xffff0000u);
                    b[2] += __builtin_bit_cast(float, x[3] << 16); b[3] += __builtin_bit_cast(float, x[3] & 0xffff0000u);
                    const u32x4 q = pair_swap(to_bf16x4(a), to_bf16x4(b));
                    if constexpr (SCHED == 32)
                        asm volatile("" ::"v"(q));
                    else
                        *reinterpret_cast<u32x4*>(orow + (size_t)16 * j * ldc + 32 * hh) = q;
                });
            });
            return;
        }
        static_for<8>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            __builtin_amdgcn_sched_barrier(0);  // (keeps the accumulator reads of later token tiles from being hoisted: register pressure)
            static_for<4>([&](auto hc) {
                constexpr int i = decltype(hc)::value * 2;
                asm volatile("" : "+a"(acc[i][j]));
                asm volatile("" : "+a"(acc[i + 1][j]));
                const u32x4 q = pair_swap(to_bf16x4(acc[i][j]), to_bf16x4(acc[i + 1][j]));
                if constexpr (SCHED == 17 || SCHED == 20)
                    asm volatile("" ::"v"(q));
                else if constexpr (SCHED == 22 || SCHED == 23)
                    __builtin_nontemporal_store(q, reinterpret_cast<u32x4*>(orow + (size_t)16 * j * ldc + 32 * (i / 2)));
                else
                    *reinterpret_cast<u32x4*>(orow + (size_t)16 * j * ldc + 32 * (i / 2)) = q;
            });
        });
    };
    using T = std::true_type;
    using F = std::false_type;
    using X0 = std::integral_constant<int, 0>;
    using X1 = std::integral_constant<int, 1>;
    // a tile: nk iterations (nk even, >= 4), buffer = kt & 1; only the last two iterations of the last tile request nothing
    using N1 = std::integral_constant<int, -1>;
    if constexpr (SCHED == 50 || SCHED == 51) {
        auto flush = [&]() {  // the kept half leaves at once (after the last tile)
            static_for<16>([&](auto ec) {
                constexpr int e = decltype(ec)::value;
                *reinterpret_cast<u32x4*>(const_cast<char*>(dbase) + doff[e / 4] + 64 * (e % 4)) = dq[e];
            });
        };
        for (int t = 0; t < my_tiles; ++t) {
            const bool last = t + 1 == my_tiles;
            if (t == 0) {
                body(X0{}, T{}, T{}, N1{});
                body(X1{}, T{}, T{}, N1{});
                body(X0{}, T{}, T{}, N1{});
                body(X1{}, T{}, T{}, N1{});
            } else {
                body(X0{}, T{}, F{}, std::integral_constant<int, 0>{});
                body(X1{}, T{}, T{}, std::integral_constant<int, 1>{});
                body(X0{}, T{}, T{}, std::integral_constant<int, 2>{});
                body(X1{}, T{}, T{}, std::integral_constant<int, 3>{});
            }
            const int kend = last ? nk - 2 : nk;
            for (int kt = 4; kt < kend; kt += 2) {
                body(X0{}, T{}, T{}, N1{});
                body(X1{}, T{}, T{}, N1{});
            }
            if (last) {
                body(X0{}, F{}, T{}, N1{});
                body(X1{}, F{}, T{}, N1{});
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            epilogue();
            zero_acc();
            if (!last) tile_mn(blockIdx.x + (t + 1) * G, m0, n0);
        }
        flush();
        return;
    }
    for (int t = 0; t < my_tiles; ++t) {
        const bool last = t + 1 == my_tiles;
        if (t == 0)
            body(X0{}, T{}, T{}, N1{});  // (the very first iteration waits: stage 1 was requested just now)
        else
            body(X0{}, T{}, F{}, N1{});
        body(X1{}, T{}, T{}, N1{});
        const int kend = last ? nk - 2 : nk;
        for (int kt = 2; kt < kend; kt += 2) {
            body(X0{}, T{}, T{}, N1{});
            body(X1{}, T{}, T{}, N1{});
        }
        if (last) {
            body(X0{}, F{}, T{}, N1{});
            body(X1{}, F{}, T{}, N1{});
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stages requested ahead have landed; only stores follow
        if constexpr (RESID) __builtin_amdgcn_sched_barrier(0);
        epilogue();
        if constexpr (RESID) __builtin_amdgcn_sched_barrier(0);
        if (!last) tile_mn(blockIdx.x + (t + 1) * G, m0, n0);
        start_acc(n0);
        if constexpr (RESID) {  // as the library: the next tile's first fragments are read AGAIN behind the epilogue, which frees their registers inside it
            if (!last) {
                static_for<16>([&](auto ec) { rd(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, ec); });
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        }
    }
#undef W4_ACC
}

__global__ void ref_rows(const bf16_t* A, const bf16_t* W, float* out, const int* rows, int nrows, int N, int K, int lda, int ldw) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (n >= N || r >= nrows) return;
    const bf16_t* a = A + (size_t)rows[r] * lda;
    const bf16_t* w = W + (size_t)n * ldw;
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += (float)a[k] * (float)w[k];
    out[(size_t)r * N + n] = s;
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

static float bf2f(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }
static uint16_t f2bf(float f) { uint32_t u; memcpy(&u, &f, 4); u += 0x7fff + ((u >> 16) & 1); return (uint16_t)(u >> 16); }

struct ResidArgs { const float* bias; const float* gate; float* stats; const float* pivot; int stats_ld; };  // schedules 80 / 81
static ResidArgs g_resid = {nullptr, nullptr, nullptr, nullptr, 0};
static void launch(int sched, dim3 grid, const bf16_t* dA, const bf16_t* dW, bf16_t* dC, int M, int N, int K, int tiles_n, int nblocks) {
#define W4_CASE(S) case S: hipLaunchKernelGGL(w4_kernel<S>, grid, dim3(256), 0, 0, dA, dW, dC, M, N, K, K, K, N, tiles_n, nblocks, 8, g_resid.bias, g_resid.gate, g_resid.stats, g_resid.pivot, g_resid.stats_ld); break;
    switch (sched) { W4_CASE(0) W4_CASE(1) W4_CASE(3) W4_CASE(10) W4_CASE(11) W4_CASE(12) W4_CASE(13) W4_CASE(14) W4_CASE(17) W4_CASE(18) W4_CASE(19) W4_CASE(20) W4_CASE(21) W4_CASE(22) W4_CASE(23) W4_CASE(30) W4_CASE(31) W4_CASE(32) W4_CASE(33) W4_CASE(40) W4_CASE(41) W4_CASE(42) W4_CASE(43) W4_CASE(44) W4_CASE(45) W4_CASE(46) W4_CASE(47) W4_CASE(50) W4_CASE(60) W4_CASE(70) W4_CASE(71) W4_CASE(72) W4_CASE(73) W4_CASE(80) W4_CASE(81) }
}

int main(int argc, char** argv) {
    struct Shape { const char* name; int M, N, K; };
    const Shape shapes[] = {{"small", 1024, 512, 512}, {"qkv", 65536, 3072, 1024}, {"ff1", 65536, 2048, 1024}, {"ff2", 65536, 1024, 2048}, {"out", 65536, 1024, 1024}, {"cube", 8192, 8192, 8192}};
    int ncu = 256;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    ncu = prop.multiProcessorCount & ~7;
    // (a list of schedules on the command line replaces the default one)
    std::vector<int> scheds = {1, 20, 46, 70, 71, 30, 33, 72, 73, 1, 20, 70, 71, 80, 81, 80, 81};
    if (argc > 1) {
        scheds.clear();
        for (int i = 1; i < argc; ++i) scheds.push_back(atoi(argv[i]));
    }
    for (int sched : scheds)
    for (const Shape& sh : shapes) {
        const int M = sh.M, N = sh.N, K = sh.K;
        const bool resid = sched == 80 || sched == 81;
        if (resid && N > 2048) continue;  // (bias | gate live in 16 KiB of LDS; the in-place call sites have N = 1024)
        std::vector<uint16_t> hA((size_t)M * K), hW((size_t)N * K);
        uint32_t st = 12345u;
        auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) & 0xffff) / 65536.0f - 0.5f; };
        for (auto& v : hA) v = f2bf(rnd());
        for (auto& v : hW) v = f2bf(rnd());
        bf16_t *dA, *dW, *dC;
        CK(hipMalloc(&dA, hA.size() * 2));
        CK(hipMalloc(&dW, hW.size() * 2));
        CK(hipMalloc(&dC, (size_t)M * N * 2));
        CK(hipMemcpy(dA, hA.data(), hA.size() * 2, hipMemcpyHostToDevice));
        CK(hipMemcpy(dW, hW.data(), hW.size() * 2, hipMemcpyHostToDevice));
        CK(hipMemset(dC, 0xff, (size_t)M * N * 2));
        // schedules 80 / 81: C is the fp16 stream x0[m][n] = ((131 m + 7 n) % 1024 - 512) / 64 (exact in fp16), bias / gate per feature, a pivot per row
        float *dBias = nullptr, *dGate = nullptr, *dStats = nullptr, *dPivot = nullptr;
        auto x0_of = [](long long m, int n) { return (float)((131 * m + 7 * n) % 1024 - 512) / 64.0f; };
        auto bias_of = [](int n) { return (float)(n % 13 - 6) * 0.125f; };
        auto gate_of = [](int n) { return (float)(n % 7 - 3) * 0.25f; };
        auto pivot_of = [](int m) { return (float)(m % 5 - 2) * 0.5f; };
        if (resid) {
            std::vector<_Float16> hx((size_t)M * N);
            for (int m = 0; m < M; ++m)
                for (int n = 0; n < N; ++n) hx[(size_t)m * N + n] = (_Float16)x0_of(m, n);
            CK(hipMemcpy(dC, hx.data(), hx.size() * 2, hipMemcpyHostToDevice));
            std::vector<float> hb(N), hg(N), hp((size_t)M * 2);
            for (int n = 0; n < N; ++n) { hb[n] = bias_of(n); hg[n] = gate_of(n); }
            for (int m = 0; m < M; ++m) { hp[2 * m] = pivot_of(m); hp[2 * m + 1] = 1.0f; }
            CK(hipMalloc(&dBias, N * 4)); CK(hipMalloc(&dGate, N * 4)); CK(hipMalloc(&dPivot, (size_t)M * 8)); CK(hipMalloc(&dStats, (size_t)(N / 64) * M * 8));
            CK(hipMemcpy(dBias, hb.data(), N * 4, hipMemcpyHostToDevice));
            CK(hipMemcpy(dGate, hg.data(), N * 4, hipMemcpyHostToDevice));
            CK(hipMemcpy(dPivot, hp.data(), (size_t)M * 8, hipMemcpyHostToDevice));
            CK(hipMemset(dStats, 0xff, (size_t)(N / 64) * M * 8));
            g_resid = ResidArgs{dBias, dGate, dStats, dPivot, M};
        }
        const int tiles_m = M / 256, tiles_n = N / 256, nblocks = tiles_m * tiles_n;
        const int grid = nblocks < ncu ? nblocks : ncu;
        launch(sched, dim3(grid), dA, dW, dC, M, N, K, tiles_n, nblocks);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        // check sampled rows
        const int nrows = 24;
        std::vector<int> rows(nrows);
        for (int r = 0; r < nrows; ++r) rows[r] = (int)(((long long)r * 2654435761LL) % M);
        rows[0] = 0; rows[1] = M - 1; rows[2] = 255; rows[3] = 256 % M;
        int* dRows; float* dRef;
        CK(hipMalloc(&dRows, nrows * 4));
        CK(hipMalloc(&dRef, (size_t)nrows * N * 4));
        CK(hipMemcpy(dRows, rows.data(), nrows * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(ref_rows, dim3((N + 255) / 256, nrows), dim3(256), 0, 0, dA, dW, dRef, dRows, nrows, N, K, K, K);
        CK(hipDeviceSynchronize());
        std::vector<float> ref((size_t)nrows * N);
        std::vector<uint16_t> got(N);
        CK(hipMemcpy(ref.data(), dRef, ref.size() * 4, hipMemcpyDeviceToHost));
        double maxerr = 0, maxref = 0, staterr = 0;
        for (int r = 0; r < nrows; ++r) {
            CK(hipMemcpy(got.data(), (uint16_t*)dC + (size_t)rows[r] * N, N * 2, hipMemcpyDeviceToHost));
            if (resid) {  // the stream against x0 + gate (A . W + bias); the statistics against the sums of the STORED values
                std::vector<float> st((size_t)(N / 64) * 2);
                for (int pl = 0; pl < N / 64; ++pl) CK(hipMemcpy(&st[2 * pl], dStats + ((size_t)pl * M + rows[r]) * 2, 8, hipMemcpyDeviceToHost));
                for (int pl = 0; pl < N / 64; ++pl) {
                    double s1 = 0, s2 = 0;
                    for (int n = 64 * pl; n < 64 * pl + 64; ++n) {
                        _Float16 hv; memcpy(&hv, &got[n], 2);
                        const double v = (double)(float)hv, want = (double)x0_of(rows[r], n) + (double)gate_of(n) * ((double)ref[(size_t)r * N + n] + bias_of(n));
                        const double e = fabs(v - want);
                        if (!(e <= maxerr)) maxerr = e;
                        if (fabs(want) > maxref) maxref = fabs(want);
                        s1 += v - pivot_of(rows[r]); s2 += (v - pivot_of(rows[r])) * (v - pivot_of(rows[r]));
                    }
                    const double e1 = fabs(st[2 * pl] - s1) / (1 + fabs(s1)), e2 = fabs(st[2 * pl + 1] - s2) / (1 + fabs(s2));
                    if (!(e1 <= staterr)) staterr = e1;
                    if (!(e2 <= staterr)) staterr = e2;
                }
                continue;
            }
            for (int n = 0; n < N; ++n) {
                const double e = fabs((double)bf2f(got[n]) - ref[(size_t)r * N + n]);
                if (!(e <= maxerr)) maxerr = e;
                if (fabs(ref[(size_t)r * N + n]) > maxref) maxref = fabs(ref[(size_t)r * N + n]);
            }
        }
        if (resid) printf("[sched %d] %s: statistics of the sampled rows, max rel err %.3g%s\n", sched, sh.name, staterr, staterr <= 1e-4 ? "" : "  <-- MISMATCH");
        // timing
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        float best = 1e9f;
        for (int rnd2 = 0; rnd2 < 3; ++rnd2) {
            CK(hipEventRecord(e0));
            for (int it = 0; it < 10; ++it) launch(sched, dim3(grid), dA, dW, dC, M, N, K, tiles_n, nblocks);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            if (ms / 10 < best) best = ms / 10;
        }
        printf("[sched %d] %s M=%d N=%d K=%d: %.1f us = %.0f TF | max abs err %.4g (max |ref| %.3g)%s\n", sched, sh.name, M, N, K, best * 1e3, 2.0 * M * N * K / best / 1e9, maxerr, maxref,
               ((sched >= 10 && sched != 22 && sched < 40) || sched == 72 || sched == 73) ? "  (timing only)" : (maxerr <= 0.02 * maxref + 1e-3 ? "" : "  <-- MISMATCH"));
        fflush(stdout);
        (void)hipFree(dA); (void)hipFree(dW); (void)hipFree(dC); (void)hipFree(dRows); (void)hipFree(dRef);
        if (resid) { (void)hipFree(dBias); (void)hipFree(dGate); (void)hipFree(dStats); (void)hipFree(dPivot); g_resid = ResidArgs{nullptr, nullptr, nullptr, nullptr, 0}; }
    }
    return 0;
}
