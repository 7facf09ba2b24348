// Implicit-GEMM convolution on the bf16 matrix cores over "bf16-plane" tensors.
//
// A tensor is stored as NP bf16 planes [NP][B,H,W,C]:
//   NP = 1  plain bf16 activations / weights (bf16 MFMA, fp32 accumulate)
//   NP = 3  an EXACT 3-way split of fp32 values, v = p0 + p1 + p2 (8+8+8 mantissa bits).  Every fp32
//           product is then evaluated as the six leading partial products
//               a0*b0 + a0*b1 + a1*b0 + a0*b2 + a1*b1 + a2*b0      (dropped terms <= 2^-26 |a*b|)
//           with fp32 accumulation: fp32-class error at 512/192 = 2.7x the fp32-MFMA rate
//           (six v_mfma_f32_32x32x16_bf16 @32 cycles instead of eight v_mfma_f32_32x32x2_f32 @64).
//
// Because both operands already live in memory as bf16 planes, tiles go HBM/L2 -> LDS by DMA
// (global_load_lds_dwordx4, 1 KiB per wave instruction) with no VGPR staging and no VALU work: a
// 3-stage LDS ring, counted s_waitcnt vmcnt(N) (never 0 in the loop) and ONE raw s_barrier per
// 16-deep K chunk.  The LDS image is lane-linear (DMA constraint), so the bank-conflict swizzle is
// applied to the per-lane SOURCE address and undone in the fragment reads (slot ^= (row>>3)&1 for
// 32-byte rows).  Halo / tail rows source a 64-byte zero page.  Weights are pre-arranged at pack time
// in exactly the LDS image order.  MFMA roles are swapped (A operand = weights, B operand = pixels)
// so each lane ends up with 4 consecutive output channels of one pixel: the epilogue (BN scale/shift,
// LeakyReLU, residual, re-split into planes) stores 8 bytes per plane per lane.
//
// Replaces the same reference call sites as conv_igemm_f32.hip (darknet.py:43-44, :52-53, :118,
// :161-162).
//
// This header holds the kernel, its launcher and the weight / layout kernels as templates over the plane count NP and the element type EL
// (conv_planes_common.h); conv_planes.hip instantiates them for the bf16 planes and the fp16 hi+lo planes, conv_planes_f16.hip for one
// fp16 plane (YV3_F16), conv_planes_i8.hip for int8 (YV3_I8: two elements per 16-bit unit, v_mfma_i32_32x32x32_i8, a quantising epilogue).
#pragma once
#include <stdlib.h>
#include <type_traits>
#include "conv_planes_common.h"

namespace {

// s_waitcnt lgkmcnt(N) as the BUILTIN (vmcnt / expcnt left at their maxima): hipcc's own wait insertion understands it, so after it the
// compiler knows those LDS reads have returned.  Behind an inline-asm wait it does not -- and then puts a full lgkmcnt(0) in front of
// the next use of the registers, AFTER younger reads were issued (the second k-step's fragments requested at the start of a compute
// segment: ~320 exposed cycles per chunk, round 4).
template <int N> __device__ __forceinline__ void wait_lgkmcnt() { __builtin_amdgcn_s_waitcnt(0xC07F | (N << 8)); }

#ifndef YV3_PP_GRP
#define YV3_PP_GRP(wid) ((wid) >> 2)
#endif
// Every compile-time measurement switch below (timeline dumps that overwrite alpha[], ablations with INVALID results, schedule
// experiments) exists only in measurement builds: the shipped libyv3.so is compiled without any of them.
#if !defined(YV3_MEASURE) && (defined(YV3_TIMELINE) || defined(YV3_ABLATE) || defined(YV3_WABL) || defined(YV3_PPX) || defined(YV3_PRIO) || \
                              defined(YV3_EXP_BF16MFMA) || defined(YV3_AB_NO_TWO_LANES_RULE) || defined(YV3_WINO_ROLL))
#error "measurement switches need -DYV3_MEASURE (make measure / tools/build_variant.sh); the shipped library has none"
#endif
// Measurement switches.  Run time: yv3_conv_desc.tune[] (conv_select.h names the codes; tune[3], measurement builds only: epilogue IO ablations).
// Compile time (A/B builds through tools/build_variant.sh):
// YV3_WABL (timing ablations of the Winograd GEMM stage's ping-pong loop, results INVALID; tools/timeline.py --kernel wino):
//   1 no DMA pieces in the compute segment   2 both k-steps' fragments read in the load segment (no SPLIT)
//   4 no fold at the end of a position       8 no MFMAs (fragments kept alive)
//   16 every DMA source is the tile's FIRST chunk (L1/L2-hot lines: no memory-system bandwidth / latency in the loop)
//   32 pixel-side rows paired into full 128-byte lines (row r reads half (r & 1) of line r >> 1: the traffic of 128-byte rows)
#ifndef YV3_WABL
#define YV3_WABL 0
#endif
// YV3_PPX (schedule experiments of the ping-pong loop, results valid): 1 s_setprio(1) around the compute segment's MFMAs
//   2 Winograd stage: both k-steps' fragments in the load segment (no SPLIT)   4 the same for every 32x64-wave-tile kernel
#ifndef YV3_PPX
#define YV3_PPX 0
#endif
// YV3_WINO_EPI4: the Winograd tile's four outputs through epilogue_store_wino4 (1) or four epilogue_store passes (0; A/B builds)
#ifndef YV3_WINO_EPI4
#define YV3_WINO_EPI4 1
#endif

// PP ("ping-pong"): the 8 waves of the workgroup form two groups of four (one wave per SIMD each) that run
// half a chunk out of phase: while one group issues a chunk's 24 MFMAs from registers, the other reads its
// fragments of the next chunk from LDS and issues its share of the DMA, then they swap at an s_barrier.
// Each SIMD's matrix pipe is thereby fed by one wave while its partner wave loads, instead of both
// waves stalling on LDS / DMA / barrier at the same time.
// MINW = 2 (4-wave workgroups only): two workgroups per CU (<= 256 registers per wave); their barriers are independent, so
// one workgroup's waves feed the matrix pipes while the other's wait for DMA / run their epilogue.
// MTG (0 = whole wave tile): 32-row blocks per epilogue round (conv_planes_common.h) -- 128-row wave tiles use 2.
// WINO (ping-pong kernels, NP = 2): Winograd F(2x2,3x3) GEMM stage (csrc/winograd.hip): the K loop walks the 16 transform
// positions (Cin/32 chunks each, operand matrix xi * xi_stride into the V planes); at the end of a position the product
// accumulators are folded into the tile's four outputs with the coefficients of A^T x A^T (0 / +-1: exact) and cleared.
// ROLL (single-phase kernels, ring of >= 3 stages): the chunk's ONE barrier sits between its two k-steps, and the first k-step's
// fragments of chunk k+1 are read under the second k-step's MFMAs of chunk k -- a rolling software pipeline over the chunk
// boundary, so that no LDS read latency is ever exposed behind a barrier (the plain loop reads a chunk's first fragments right
// after its barrier and waits for them before the first MFMA).
template <int NP, int BM, int BN, int WM, int WN, int NSTAGE, bool K3, bool DUAL, bool OUT_F32, bool PP = false, bool SK = false, int MINW = 1, int MTG = 0,
          bool WINO = false, bool ROLL = false, int EL = plane_elem(NP)>
__global__ __launch_bounds__(64 * WM * WN, MINW) void conv_planes_kernel(const ConvParamsP p) {
    static_assert(!WINO || ((PP || ROLL) && !K3 && !DUAL && !OUT_F32 && NP == 2), "Winograd stage: ping-pong or rolling fp16-plane kernel");
    static_assert(!ROLL || (!PP && !SK && NSTAGE >= 3), "rolling loop: single-phase kernel with a ring of >= 3 stages");
    constexpr int NW = WM * WN;
    constexpr int WTM = BM / WM, WTN = BN / WN;          // wave tile: WTM pixels x WTN channels
    constexpr int MT = WTM / 32, NT = WTN / 32;
    constexpr int EMTG = MTG ? MTG : MT;
    constexpr int A_PLANE = BM * ROWB;                    // bytes
    constexpr int B_PLANE = BN * ROWB;
    constexpr int STAGE = NP * (A_PLANE + B_PLANE);
    constexpr int AROWS = BM / NW;                        // pixel rows staged per wave (multiple of 16)
    constexpr int AQ = (AROWS + RPG - 1) / RPG;           // global_load_lds per plane per wave, A side
    constexpr int ATAIL = AROWS % RPG;                    // rows of the last one when it is partial (192-row tiles on 8 waves: 24 = 16 + 8)
    constexpr int BROWS = BN / NW;                        // weight rows staged per wave
    constexpr int BQ = BROWS > RPG ? BROWS / RPG : 1;     // global_load_lds per plane per wave, weight side
    constexpr int G = NP * (AQ + BQ);                     // DMA instructions per chunk per wave
    constexpr int D = NSTAGE - 1;                         // prefetch distance in chunks
    static_assert((BROWS <= RPG || BROWS % RPG == 0) && MT >= 1 && NT >= 1, "tile/wave layout");

    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
#ifdef YV3_TIMELINE
    const unsigned long long tl_entry = __builtin_amdgcn_s_memtime();
#endif

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid / WN, wn = wid % WN;

    // ---- staging, pixel side: wave w moves rows [AROWS*w, AROWS*(w+1)) of every plane, RPG rows per DMA.
    // lane -> (row = lane/4 within the group, physical slot = lane%4); the source is the un-swizzled slot.
    // (the swizzle follows the row's position in the TILE: a wave's first row is a multiple of 16 except with a partial last piece)
    const int sslot = ((lane & (SLOTS - 1)) ^ (((lane >> 4) + (ATAIL ? (AROWS * wid) >> 2 : 0)) & (SLOTS - 1))) * 8;
    long long aoff[AQ], aoff2[DUAL ? AQ : 1];
    int ahi[K3 ? AQ : 1], awi[K3 ? AQ : 1];
    bool aok[AQ];
    const int HoWo = p.Ho * p.Wo;
    // ---- staging, weight side: the packed tile is already in LDS-image (swizzled) order
    const bool bact = lane < (BROWS < RPG ? BROWS : RPG) * SLOTS;
    int m0 = 0, n0 = 0, bin = 0;
    long long btile = 0;
    int kh = 0, kw = 0, c0 = 0;
    bool tapinit = true;
    // index math of one workgroup tile (logical id `bid`), positioned at K chunk k0
    auto setup_tile = [&](int bid, int k0) {
        n0 = (bid % p.ntiles) * BN;
        m0 = (bid / p.ntiles) * BM;
#pragma unroll
        for (int q = 0; q < AQ; ++q) {
            const int m = m0 + AROWS * wid + q * RPG + (lane >> 2);
            aok[q] = m < p.M;
            const int mm = aok[q] ? m : 0;
            const int b = mm / HoWo;
            const int rem = mm - b * HoWo;
            const int ho = rem / p.Wo;
            const int wo = rem - ho * p.Wo;
            if (K3) {
                ahi[q] = ho * p.stride - 1; awi[q] = wo * p.stride - 1;
                aoff[q] = (((long long)b * p.H + ahi[q]) * p.W + awi[q]) * p.Cin + sslot;
            } else if (DUAL) {
                aoff[q] = (((long long)b * (p.H >> 1) + (ho >> 1)) * (p.W >> 1) + (wo >> 1)) * p.Cup + sslot;
                aoff2[q] = (((long long)b * p.H + ho) * p.W + wo) * (p.Cin - p.Cup) + sslot;
            } else {
                aoff[q] = (((long long)b * p.H + ho * p.stride) * p.W + wo * p.stride) * p.Cin + sslot;
                if constexpr (WINO && (YV3_WABL & 32)) aoff[q] = (long long)(mm >> 1) * p.Cin + (mm & 1) * 32 + sslot;
            }
        }
        const int n0w = n0 + BROWS * wid;                      // first weight row of this wave (a wave's rows never straddle a packed tile)
        const int brow = n0w % p.tb + (lane >> 2);
        btile = (long long)(n0w / p.tb) * p.nk;
        bin = brow * PBK + (lane & (SLOTS - 1)) * 8;
        const int cpt = p.Cin / PBK;                           // chunks per filter tap
        const int tap = (K3 || WINO) ? k0 / cpt : 0;
        kh = WINO ? 0 : tap / 3; kw = tap - kh * 3; c0 = (k0 - tap * cpt) * PBK;      // (WINO: kw = transform position)
        tapinit = true;
    };
    if (!(PP && SK)) setup_tile(yv3_xcd_remap(blockIdx.x, gridDim.x), 0);

    // ---- DMA of one K chunk = G wave instructions ("pieces").  dma_prepare computes this lane's source
    // pointers once per chunk; dma_piece(idx) issues one global_load_lds, so that the pieces can be spread
    // between the MFMAs of the previous chunk instead of being issued as one burst behind the barrier.
    // The per-lane source pointer only changes shape when the filter tap changes (every Cin/32 chunks): bounds
    // test, base pointer and plane stride are recomputed there; inside a tap a chunk is one 64-bit add.
    const u16* ap[AQ];
    long long aps[AQ];
    int ainc[AQ];
    const u16* wbp = p.w;
    unsigned char* dst = lds;
    auto dma_prepare = [&](int kc, int stage) {
        dst = lds + stage * STAGE;
        if (DUAL) {
#pragma unroll
            for (int q = 0; q < AQ; ++q) {
                const bool ok = aok[q];
                const u16* src = p.x;
                long long off, ps = p.xs;
                if (c0 < p.Cup) off = aoff[q] + c0;
                else { src = p.x2; off = aoff2[q] + (c0 - p.Cup); ps = p.x2s; }
                ap[q] = ok ? src + off : g_zero_page;
                aps[q] = ok ? ps : 0;
            }
        } else if (c0 == 0 || tapinit) {                       // wave-uniform: first chunk of a tap / of the tile
            tapinit = false;
#pragma unroll
            for (int q = 0; q < AQ; ++q) {
                bool ok = aok[q];
                long long off = aoff[q] + c0;
                if (K3) {
                    ok = ok && (unsigned)(ahi[q] + kh) < (unsigned)p.H && (unsigned)(awi[q] + kw) < (unsigned)p.W;
                    off += ((long long)kh * p.W + kw) * p.Cin;
                }
                if (WINO) off += (long long)kw * p.xi_stride;
                ap[q] = ok ? p.x + off : g_zero_page;
                aps[q] = ok ? p.xs : 0;
                ainc[q] = ok ? PBK : 0;
            }
        } else {
#pragma unroll
            for (int q = 0; q < AQ; ++q) ap[q] += ainc[q];
        }
        wbp = p.w + ((btile + kc) * NP) * (long long)(p.tb * PBK) + bin;
        if constexpr (WINO && (YV3_WABL & 16)) {
            wbp = p.w + (btile * NP) * (long long)(p.tb * PBK) + bin;
#pragma unroll
            for (int q = 0; q < AQ; ++q) { ap[q] = p.x + aoff[q]; aps[q] = p.xs; }
        }
        c0 += PBK;
        if (c0 == p.Cin) { c0 = 0; if (WINO) ++kw; else if (++kw == 3) { kw = 0; ++kh; } }
    };
    auto dma_piece = [&](int idx) {
        if (idx < AQ * NP) {
            const int q = idx / NP, pl = idx % NP;
            // (a partial last piece: the lanes of the rows beyond this wave's share stay out -- they would land in the next wave's rows)
            if (ATAIL == 0 || q < AQ - 1 || (lane >> 2) < ATAIL)
                __builtin_amdgcn_global_load_lds(GPTR(ap[q] + pl * aps[q]),
                                                 LPTR(dst + pl * A_PLANE + (AROWS * wid + q * RPG) * ROWB), 16, 0, 0);
        } else if (bact) {
            const int q = (idx - AQ * NP) / NP, pl = (idx - AQ * NP) % NP;
            __builtin_amdgcn_global_load_lds(GPTR(wbp + (long long)pl * (p.tb * PBK) + q * (RPG * PBK)),
                                             LPTR(dst + NP * A_PLANE + pl * B_PLANE + (wid * BROWS + q * RPG) * ROWB), 16, 0, 0);
        }
    };

    f32x16 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    f32x16 yac[WINO ? 4 : 1][NT][MT];          // WINO: the tile's four outputs Y[wi][wj] (index 2*wi + wj)
    if constexpr (WINO) {
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) yac[o][i][j][e] = 0.f;
    }
    int wleft = WINO ? p.Cin / PBK : 0, wxi = 0;   // chunks left in the current transform position, its index

    const int l31 = lane & 31, lhi = lane >> 5;
    const int x_row = (wm * WTM + l31) * ROWB;                                  // pixel fragments (B operand)
    const int w_row = NP * A_PLANE + (wn * WTN + l31) * ROWB;                   // weight fragments (A operand)
    const int fsw = swz(l31);

    if constexpr (!PP) {
#pragma unroll
        for (int d = 0; d < D; ++d)
            if (d < p.nk) {
                dma_prepare(d, d);
#pragma unroll
                for (int g = 0; g < G; ++g) dma_piece(g);
            }
    }

    constexpr int KS = PBK / 16;              // MFMA k-steps per chunk
    constexpr int NF = (NT + MT) * NP;        // fragments (ds_read_b128) per k-step
    constexpr int NU = NT * MT;               // MFMA units (6 or 1 MFMAs each) per k-step
    bf16x8v frag[KS][NF];                     // [0, NT*NP): weights (i, plane); then pixels (j, plane)
    const unsigned char* st = lds;
    auto read_frag = [&](int ks, int f) {
        const int fslot = ((ks * 2 + lhi) ^ fsw) * 16;
        if (f < NT * NP) frag[ks][f] = *reinterpret_cast<const bf16x8v*>(st + w_row + fslot + (f / NP) * 32 * ROWB + (f % NP) * B_PLANE);
        else { const int g = f - NT * NP;
               frag[ks][f] = *reinterpret_cast<const bf16x8v*>(st + x_row + fslot + (g / NP) * 32 * ROWB + (g % NP) * A_PLANE); }
    };

    if constexpr (PP) {
        static_assert(!PP || (NW == 8 && NSTAGE >= 3 && NP <= 2), "ping-pong: 8 waves, 3-deep ring, one or two planes");
        constexpr int NMF = NP == 2 ? 3 : 1;      // MFMAs per (weight tile, pixel tile, k-step)
        const int grp = YV3_PP_GRP(wid);
        // 32x64 wave tiles (128x128 workgroup tile): the compute segment is only 12 MFMAs per k-step, so the second
        // k-step's fragments are fetched under the first k-step's MFMAs; measured +5 % there, -5 % on 64x64 wave tiles
        // (round 4: NOT for the Winograd stage -- with its 4-deep ring both k-steps' fragments in the load segment are 2-4 % faster per
        // layer, profiles/r04c_pp_schedule_*.log)
        constexpr bool SPLIT = MT == 1 && !(YV3_PPX & 4);
        // ordered SPLIT (fp16 planes): the second k-step's fragments are requested in the order its MFMAs consume them (x_hi, w_lo..,
        // x_lo, w_hi..) and hipcc waits for them one by one (partial lgkmcnt: it can, now that the load segment's wait is the builtin):
        // a wave's ds_read_b128 return 1 KB per ~36 cycles (tools/probes/lds_read_rate.hip), so six of them take ~320 cycles -- longer
        // than the first k-step's six MFMAs
        constexpr bool OSPLIT = SPLIT && NP == 2 && !(YV3_PPX & 8);
        // ... the first OS_EARLY of them already in the load segment (then the load segment's 8 reads take about as long as the partner's 12
        // MFMAs, and the 4 left for the compute segment have returned before the second k-step starts)
        constexpr int OS_EARLY = 2;
        auto os_order = [](int q) -> int {          // fragment index (read_frag) of the q-th operand in consumption order
            if (q < MT) return NT * NP + q * NP;                       // x_hi[j]
            q -= MT;
            if (q < NT) return q * NP + 1;                             // w_lo[i]
            q -= NT;
            if (q < MT) return NT * NP + q * NP + 1;                   // x_lo[j]
            q -= MT;
            return q * NP;                                             // w_hi[i]
        };
#ifdef YV3_TIMELINE
        unsigned long long tl_load = 0, tl_b1 = 0, tl_comp = 0, tl_b2 = 0, tl_pro = 0, tl_epi = 0, tl_t = tl_entry;
        int tl_items = 0, tl_chunks = 0;
#define TL_MARK(acc_) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); acc_ += t_ - tl_t; tl_t = t_; } while (0)
#else
#define TL_MARK(acc_) do {} while (0)
#endif
        // ---- work list.  One tile, all of K, per workgroup -- or (SK, "stream-K") a persistent workgroup per CU that
        // owns a contiguous range [it, it_end) of (tile, K chunk) iterations of ITS XCD's tile range, so that every CU
        // gets the same number of chunks whatever the tile count (no idle CUs in a last partial round).  A range starts
        // with the TAIL part [k0, nk) of a tile (accumulators dumped to the workspace) and ends with the HEAD part
        // [0, k1) of another, whose tail the next workgroup of the same XCD dumped at ITS start, long ago: head + tail
        // are added in that fixed order and the epilogue runs once.  Ranges are >= nk chunks (host guarantees tiles >=
        // workgroups), so a tile is never split three ways.
        // The schedulable unit of the stream-K ranges is one K chunk -- or (WINO) one whole transform position (UC chunks): a
        // Winograd tile is only split between positions, where the product accumulators are zero and a part is the four
        // partial outputs.
        const int UC = WINO ? p.Cin / PBK : 1;                                    // chunks per unit
        const int UN = WINO ? 16 : p.nk;                                          // units per tile
        int it = 0, it_end = UN, tile_base = 0;
        const int jb = blockIdx.x >> 3, nj = gridDim.x >> 3;                     // (SK) this workgroup's slot in its XCD
        long long tx = 0;                                                        // (SK) unit iterations of this XCD
        if constexpr (SK) {
            const int xcd = blockIdx.x & 7;
            const int t0 = (int)((long long)xcd * p.total / 8), t1 = (int)((long long)(xcd + 1) * p.total / 8);
            tx = (long long)(t1 - t0) * UN;
            it = (int)(tx * jb / nj); it_end = (int)(tx * (jb + 1) / nj); tile_base = t0;
        }
        bool first_item = true;
        while (it < it_end) {
            int u0 = 0, u1 = UN;
            if constexpr (SK) {
                const int tl = it / UN;
                u0 = it - tl * UN;
                u1 = it_end - it < UN - u0 ? u0 + (it_end - it) : UN;
                setup_tile(tile_base + tl, u0 * UC);
                if (!first_item) __syncthreads();                                 // the previous item's epilogue tiles are dead
            }
            const int k0 = u0 * UC, k1 = u1 * UC;
            if constexpr (WINO) {
                wleft = UC; wxi = u0;
#pragma unroll
                for (int o = 0; o < 4; ++o)
#pragma unroll
                    for (int i = 0; i < NT; ++i)
#pragma unroll
                        for (int j = 0; j < MT; ++j)
#pragma unroll
                            for (int e = 0; e < 16; ++e) yac[o][i][j][e] = 0.f;
            }
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < MT; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
#pragma unroll
            for (int d = 0; d < D; ++d)
                if (k0 + d < k1) {
                    dma_prepare(k0 + d, d);
#pragma unroll
                    for (int g = 0; g < G; ++g) dma_piece(g);
                }
            // chunk k0 has landed.  After an epilogue its stores sit behind these pieces in the (load/store-mixed) vmcnt
            // queue, so later items drain it completely.
            if (first_item && k0 + D <= k1) wait_vmcnt<(D - 1) * G>(); else wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
            if (grp == 1) __builtin_amdgcn_s_barrier();                           // group 1 runs one segment behind
            TL_MARK(tl_pro);
            int cur = 0, nxt = D % NSTAGE;
            for (int kc = k0; kc < k1; ++kc) {
                // ---- load segment: fragments of chunk kc -> registers; addresses of chunk kc+D (VALU, off the matrix
                // pipe's critical path).  My pieces of chunk kc+1 (issued D-1 compute segments ago) must have landed.
                st = lds + cur * STAGE;
#pragma unroll
                for (int ks = 0; ks < (SPLIT ? 1 : KS); ++ks)
#pragma unroll
                    for (int f = 0; f < NF; ++f) read_frag(ks, f);
                if constexpr (OSPLIT) {                                            // the second k-step's first operands: x_hi, w_lo of weight tile 0
#pragma unroll
                    for (int q = 0; q < OS_EARLY; ++q) read_frag(1, os_order(q));
                }
                const bool more = kc + D < k1;
                if (more) dma_prepare(kc + D, nxt);
                if (kc + D - 1 < k1) wait_vmcnt<(D - 2) * G>(); else wait_vmcnt<0>();
                wait_lgkmcnt<0>();
                __builtin_amdgcn_sched_barrier(0);
                TL_MARK(tl_load);
                __builtin_amdgcn_s_barrier();
                TL_MARK(tl_b1);
                __builtin_amdgcn_sched_barrier(0);
                // ---- compute segment: MFMAs from registers, the DMA pieces of chunk kc+D between them
                // (SPLIT: plus the second k-step's fragment reads)
                if constexpr ((YV3_PPX & 1) != 0) __builtin_amdgcn_s_setprio(1);
                if constexpr (OSPLIT) {
                    static_assert(!OSPLIT || KS == 2, "ordered SPLIT: two k-steps");
#pragma unroll
                    for (int q = OS_EARLY; q < NF; ++q) { read_frag(1, os_order(q)); __builtin_amdgcn_sched_barrier(0); }
                } else if constexpr (SPLIT) {
#pragma unroll
                    for (int ks = 1; ks < KS; ++ks)
#pragma unroll
                        for (int f = 0; f < NF; ++f) read_frag(ks, f);
                }
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    if (SPLIT && !OSPLIT && ks == 1) { wait_lgkmcnt<0>(); __builtin_amdgcn_sched_barrier(0); }
#pragma unroll
                    for (int t = 0; t < NMF; ++t)                                  // rotate over the accumulators: no back-to-back RAW
#pragma unroll
                        for (int u = 0; u < NU; ++u) {
                            const int i = u / MT, j = u % MT;
                            const bf16x8v* wf = &frag[ks][i * NP];
                            const bf16x8v* xf = &frag[ks][NT * NP + j * NP];
                            if constexpr (WINO && (YV3_WABL & 8)) { asm volatile("" :: "v"(wf[t == 0 ? 1 : 0]), "v"(xf[t == 1 ? 1 : 0])); }
                            else if constexpr (NP == 2) acc[i][j] = PlaneOps<2>::mfma(wf[t == 0 ? 1 : 0], xf[t == 1 ? 1 : 0], acc[i][j]);
                            else acc[i][j] = ElemOps<EL>::mfma(wf[0], xf[0], acc[i][j]);
                            constexpr int TOT = KS * NMF * NU;                     // one DMA piece after every (TOT / G)-th MFMA
                            const int mi = (ks * NMF + t) * NU + u;
                            if (more && !(WINO && (YV3_WABL & 1)) && (mi * G) / TOT != ((mi + 1) * G) / TOT) dma_piece((mi * G) / TOT);
                        }
                }
                __builtin_amdgcn_sched_barrier(0);
                if constexpr ((YV3_PPX & 1) != 0) __builtin_amdgcn_s_setprio(0);
                if constexpr (WINO) {
                    if (--wleft == 0 && !(YV3_WABL & 4)) {                         // end of a transform position: Y += (A^T x A^T)[.][xi] * M
                        wleft = p.Cin / PBK;
                        const int xr = wxi >> 2, xc = wxi & 3;
                        ++wxi;
                        const float r0 = xr < 3 ? 1.f : 0.f, r1 = xr == 0 ? 0.f : (xr == 1 ? 1.f : -1.f);
                        const float q0 = xc < 3 ? 1.f : 0.f, q1 = xc == 0 ? 0.f : (xc == 1 ? 1.f : -1.f);
                        const float sc[4] = {r0 * q0, r0 * q1, r1 * q0, r1 * q1};
#pragma unroll
                        for (int i = 0; i < NT; ++i)
#pragma unroll
                            for (int j = 0; j < MT; ++j)
#pragma unroll
                                for (int e = 0; e < 16; ++e) {
                                    const float mv = acc[i][j][e];
#pragma unroll
                                    for (int o = 0; o < 4; ++o) yac[o][i][j][e] = fmaf(mv, sc[o], yac[o][i][j][e]);
                                    acc[i][j][e] = 0.f;
                                }
                    }
                }
                TL_MARK(tl_comp);
                // both groups pass the same number of barriers; group 1 skips its last one so that group 0 can start the
                // epilogue early -- except with SPLIT, where group 1 still reads fragments from LDS in its last segment
                if (SPLIT || !(grp == 1 && kc + 1 == k1)) __builtin_amdgcn_s_barrier();
                TL_MARK(tl_b2);
                __builtin_amdgcn_sched_barrier(0);
                cur = cur + 1 == NSTAGE ? 0 : cur + 1;
                nxt = nxt + 1 == NSTAGE ? 0 : nxt + 1;
            }
            // group 0 gets here one segment before group 1 (which reads no LDS in its last segment; the epilogue's LDS
            // tiles are per wave)
            if (SPLIT && grp == 0) __builtin_amdgcn_s_barrier();
            if constexpr (SK) {
                constexpr int NO = WINO ? 4 : 1;                                 // accumulator sets of a part (WINO: the four outputs)
                constexpr int PART = NO * NT * MT * 16 * 64;                     // floats of one wave's part
                if (u0 > 0) {                                                    // tail / middle part: hand the accumulators over
                    float* w = p.ws + ((size_t)blockIdx.x * NW + wid) * PART + lane * 4;
#pragma unroll
                    for (int o = 0; o < NO; ++o)
#pragma unroll
                        for (int i = 0; i < NT; ++i)
#pragma unroll
                            for (int j = 0; j < MT; ++j)
#pragma unroll
                                for (int g = 0; g < 4; ++g) {
                                    const f32x16& a_ = WINO ? yac[o][i][j] : acc[i][j];
                                    *reinterpret_cast<f32x4*>(w + (((o * NT + i) * MT + j) * 4 + g) * 256) =
                                        f32x4{a_[4 * g], a_[4 * g + 1], a_[4 * g + 2], a_[4 * g + 3]};
                                }
                    // The two halves of a split tile run on the SAME XCD (workgroups b and b+8), i.e. behind the same L2:
                    // once the stores have been acknowledged (vmcnt 0: the vector L1 is write-through) the partner can
                    // read them -- no L2 write-back / invalidate (an agent-scope release/acquire pair costs ~60 us per
                    // launch here).  The XCC id travels with the flag and is checked by the reader.
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                    if (tid == 0) __hip_atomic_store(p.wsflags + blockIdx.x, 1 + (int)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 15),
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    it += u1 - u0; first_item = false;
                    continue;
                }
                if (u1 < UN) {
                    // head part: add, in workgroup order, what the following workgroups of this XCD accumulated for the
                    // rest of this tile (one tail part, preceded by middle parts when a range is shorter than a tile)
                    const long long tile_end = (long long)(it / UN + 1) * UN;
                    for (int k = 1; jb + k < nj; ++k) {
                        const long long s_k = tx * (jb + k) / nj, e_k = tx * (jb + k + 1) / nj;
                        if (s_k >= tile_end) break;
                        if (e_k == s_k) continue;
                        const int partner = blockIdx.x + 8 * k;
                        if (tid == 0) {
                            int n = 0, f;
                            while ((f = __hip_atomic_load(p.wsflags + partner, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0 && ++n < (1 << 22))
                                __builtin_amdgcn_s_sleep(2);
                            // never expected (reported by the host as an error): hand-over timed out, or the partner ran
                            // on another XCD, whose L2 this one is not coherent with
                            if ((f == 0 || f != 1 + (int)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 15)) && p.flags) atomicOr(p.flags, 2);
                            __hip_atomic_store(p.wsflags + partner, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                        __syncthreads();
                        const float* w = p.ws + ((size_t)partner * NW + wid) * PART + lane * 4;
#pragma unroll
                        for (int o = 0; o < NO; ++o)
#pragma unroll
                            for (int i = 0; i < NT; ++i)
#pragma unroll
                                for (int j = 0; j < MT; ++j)
#pragma unroll
                                    for (int g = 0; g < 4; ++g) {
                                        const f32x4 t = *reinterpret_cast<const f32x4*>(w + (((o * NT + i) * MT + j) * 4 + g) * 256);
                                        f32x16& a_ = WINO ? yac[o][i][j] : acc[i][j];
#pragma unroll
                                        for (int q = 0; q < 4; ++q) a_[4 * g + q] += t[q];
                                    }
                    }
                }
            }
            if constexpr (WINO) {
                if constexpr (MT == 1 && NP == 2 && YV3_WINO_EPI4) epilogue_store_wino4<BM, BN, WM, WN>(yac, p, lds, m0, n0, wid, lane);
                else {
#pragma unroll
                    for (int o = 0; o < 4; ++o)
                        epilogue_store<NP, BM, BN, WM, WN, false, false, EMTG, true>(yac[o], p, lds, m0, n0, wid, lane, o >> 1, o & 1);
                }
            } else epilogue_store<NP, BM, BN, WM, WN, OUT_F32, false, EMTG, false, EL>(acc, p, lds, m0, n0, wid, lane);
            TL_MARK(tl_epi);
#ifdef YV3_TIMELINE
            ++tl_items; tl_chunks += k1 - k0;
#endif
            it += u1 - u0; first_item = false;
        }
#ifdef YV3_TIMELINE
        if (blockIdx.x == 100 && lane == 0 && p.alpha) {     // debug build only: cycle split of one workgroup -> alpha[0..]
            float* dbg = const_cast<float*>(p.alpha) + wid * 8;
            dbg[0] = (float)tl_pro / tl_items; dbg[1] = (float)tl_load / tl_chunks; dbg[2] = (float)tl_b1 / tl_chunks;
            dbg[3] = (float)tl_comp / tl_chunks; dbg[4] = (float)tl_b2 / tl_chunks; dbg[5] = (float)tl_epi / tl_items;
            dbg[6] = (float)tl_items; dbg[7] = (float)(tl_t - tl_entry);
        }
#endif
        return;
    }
    if constexpr (ROLL) {
        static_assert(KS == 2, "rolling loop: two k-steps per chunk");
        // chunk 0 has landed and is visible; its first k-step's fragments go to registers
        if (D <= p.nk) wait_vmcnt<(D - 1) * G>(); else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int f = 0; f < NF; ++f) read_frag(0, f);
        static_assert(NP <= 2, "rolling loop: one or two planes");
        constexpr int NMF = NP == 2 ? 3 : 1;          // MFMAs per (weight tile, pixel tile, k-step)
        constexpr int TOT = NMF * NU;                 // MFMAs of one k-step block
        constexpr int RH = TOT >= 4 ? TOT / 2 : TOT;  // the other buffer's NF fragment reads follow the first RH of them
        // MFMAs of k-step `ks` (registers frag[ks]), rotating over the accumulators; `rd`: fragment reads into frag[ko] from `st`
        // behind them; `pieces`: this chunk's DMA pieces too
        auto kstep_block = [&](auto ks_c, auto ko_c, bool rd, bool pieces) {
            constexpr int ks = decltype(ks_c)::value, ko = decltype(ko_c)::value;
#pragma unroll
            for (int t = 0; t < NMF; ++t)
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int i = u / MT, j = u % MT;
                    const bf16x8v* wf = &frag[ks][i * NP];
                    const bf16x8v* xf = &frag[ks][NT * NP + j * NP];
                    if constexpr (NP == 2) acc[i][j] = PlaneOps<2>::mfma(wf[t == 0 ? 1 : 0], xf[t == 1 ? 1 : 0], acc[i][j]);
                    else acc[i][j] = ElemOps<EL>::mfma(wf[0], xf[0], acc[i][j]);
                    const int mi = t * NU + u;
                    if (rd && mi < RH) {
#pragma unroll
                        for (int f = mi * NF / RH; f < (mi + 1) * NF / RH; ++f) read_frag(ko, f);
                    }
                    if (pieces) {
#pragma unroll
                        for (int g = mi * G / TOT; g < (mi + 1) * G / TOT; ++g) dma_piece(g);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
        };
#ifdef YV3_TIMELINE
        unsigned long long rl_prep = 0, rl_b0 = 0, rl_wait = 0, rl_bar = 0, rl_b1 = 0, rl_fold = 0, rl_t = __builtin_amdgcn_s_memtime();
        const unsigned long long rl_t0 = rl_t;       // loop entry (everything before: prologue)
#define RL_MARK(acc_) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); acc_ += t_ - rl_t; rl_t = t_; } while (0)
#else
#define RL_MARK(acc_) do {} while (0)
#endif
        int cur = 0, nxt = D % NSTAGE;
        for (int kc = 0; kc < p.nk; ++kc) {
            const bool more = kc + D < p.nk;
            const bool next = kc + 1 < p.nk;
            st = lds + cur * STAGE;
            if (more) dma_prepare(kc + D, nxt);
            __builtin_amdgcn_sched_barrier(0);
            RL_MARK(rl_prep);
            // ---- first k-step: MFMAs on frag[0]; behind the first half of them the second k-step's fragment reads, behind all of
            // them the DMA pieces of chunk kc+D.  (Reads go out AFTER an MFMA, never before the block's first one: the wait
            // hipcc puts in front of a block's first MFMA is lgkmcnt(0), which must not catch reads issued for the next block.)
            kstep_block(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, true, more);
            RL_MARK(rl_b0);
            // ---- the chunk's barrier: my pieces of chunk kc+1 have landed, my reads of this chunk's stage are complete
            if (next) {
                if (more) wait_vmcnt<(D - 1) * G>(); else wait_vmcnt<0>();
                wait_lgkmcnt<0>();
                __builtin_amdgcn_sched_barrier(0);
                RL_MARK(rl_wait);
                __builtin_amdgcn_s_barrier();
                RL_MARK(rl_bar);
                __builtin_amdgcn_sched_barrier(0);
                st = lds + (cur + 1 == NSTAGE ? 0 : cur + 1) * STAGE;
            }
            // ---- second k-step: MFMAs on frag[1]; behind the first half of them the NEXT chunk's first-k-step fragment reads
            kstep_block(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}, next, false);
            RL_MARK(rl_b1);
            if constexpr (WINO) {
                if (--wleft == 0) {                                                // end of a transform position: Y += (A^T x A^T)[.][xi] * M
                    wleft = p.Cin / PBK;
                    const int xr = wxi >> 2, xc = wxi & 3;
                    ++wxi;
                    const float r0 = xr < 3 ? 1.f : 0.f, r1 = xr == 0 ? 0.f : (xr == 1 ? 1.f : -1.f);
                    const float q0 = xc < 3 ? 1.f : 0.f, q1 = xc == 0 ? 0.f : (xc == 1 ? 1.f : -1.f);
                    const float sc[4] = {r0 * q0, r0 * q1, r1 * q0, r1 * q1};
#pragma unroll
                    for (int i = 0; i < NT; ++i)
#pragma unroll
                        for (int j = 0; j < MT; ++j)
#pragma unroll
                            for (int e = 0; e < 16; ++e) {
                                const float mv = acc[i][j][e];
#pragma unroll
                                for (int o = 0; o < 4; ++o) yac[o][i][j][e] = fmaf(mv, sc[o], yac[o][i][j][e]);
                                acc[i][j][e] = 0.f;
                            }
                }
            }
            RL_MARK(rl_fold);
            cur = cur + 1 == NSTAGE ? 0 : cur + 1;
            nxt = nxt + 1 == NSTAGE ? 0 : nxt + 1;
        }
#ifdef YV3_TIMELINE
        if (blockIdx.x == 100 && lane == 0 && p.alpha && WINO) {     // debug build only: cycle split of one workgroup -> alpha[0..]
            float* dbg = const_cast<float*>(p.alpha) + wid * 8;
            const float n_ = (float)p.nk;
            dbg[0] = rl_prep / n_; dbg[1] = rl_b0 / n_; dbg[2] = rl_wait / n_; dbg[3] = rl_bar / n_; dbg[4] = rl_b1 / n_; dbg[5] = rl_fold / n_;
            dbg[6] = n_; dbg[7] = (float)(rl_t - tl_entry);
        }
#endif
        if constexpr (WINO) {
            __syncthreads();                                                       // every wave is done with the last stage
            if constexpr (MT == 1 && NP == 2 && YV3_WINO_EPI4) epilogue_store_wino4<BM, BN, WM, WN>(yac, p, lds, m0, n0, wid, lane);
            else {
#pragma unroll
                for (int o = 0; o < 4; ++o)
                    epilogue_store<NP, BM, BN, WM, WN, false, false, EMTG, true>(yac[o], p, lds, m0, n0, wid, lane, o >> 1, o & 1);
            }
        } else epilogue_store<NP, BM, BN, WM, WN, OUT_F32, true, EMTG, false, EL>(acc, p, lds, m0, n0, wid, lane);
#ifdef YV3_TIMELINE
        if (blockIdx.x == (unsigned)(p.tune[2] > 0 ? p.tune[2] : 100) && lane == 0 && p.alpha && !WINO && NW * 10 <= p.Cout) {   // non-Winograd rolling tiles (bf16): + prologue / epilogue
            const unsigned long long t_end = __builtin_amdgcn_s_memtime();
            float* dbg = const_cast<float*>(p.alpha) + wid * 10;
            const float n_ = (float)p.nk;
            dbg[0] = rl_prep / n_; dbg[1] = rl_b0 / n_; dbg[2] = rl_wait / n_; dbg[3] = rl_bar / n_; dbg[4] = rl_b1 / n_; dbg[5] = n_;
            dbg[6] = (float)(rl_t0 - tl_entry); dbg[7] = (float)(t_end - rl_t); dbg[8] = (float)(t_end - tl_entry); dbg[9] = 0.f;
        }
#endif
        return;
    }
#ifdef YV3_TIMELINE
    unsigned long long tl_wait = 0, tl_bar = 0, tl_body = 0, tl_prev = 0, tl_dma = 0;
#endif
#if defined(YV3_PRIO) && YV3_PRIO == 1
    // the second-dispatched half of an 8-wave workgroup loses issue arbitration (age) to the first half on
    // every segment and the first half then idles at the barrier; static priority for the younger half
    if (NW == 8 && wid >= 4) __builtin_amdgcn_s_setprio(1);
#elif defined(YV3_PRIO) && YV3_PRIO == 2
    if (NW == 8 && wid < 4) __builtin_amdgcn_s_setprio(1);
#endif
    int cur = 0, nxt = D % NSTAGE;
    for (int kc = 0; kc < p.nk; ++kc) {
        // chunk kc must have landed; up to D-1 younger chunks may stay in flight (never a full drain mid-loop)
#ifdef YV3_TIMELINE
        const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
        if (kc + D - 1 < p.nk) wait_vmcnt<(D - 1) * G>(); else wait_vmcnt<0>();
#ifdef YV3_TIMELINE
        const unsigned long long t1 = __builtin_amdgcn_s_memtime();
#endif
        __builtin_amdgcn_s_barrier();
#ifdef YV3_TIMELINE
        const unsigned long long t2 = __builtin_amdgcn_s_memtime();
        tl_wait += t1 - t0; tl_bar += t2 - t1;
        if (kc > 0) tl_body += t0 - tl_prev;
        tl_prev = t2;
#endif
        st = lds + cur * STAGE;
#if !defined(YV3_ABLATE) || (YV3_ABLATE != 1)
        const bool more = kc + D < p.nk;
#else
        const bool more = false;
#endif
#if !defined(YV3_ABLATE) || (YV3_ABLATE != 2)
#pragma unroll
        for (int f = 0; f < NF; ++f) read_frag(0, f);
#endif
        if (more) dma_prepare(kc + D, nxt);
        __builtin_amdgcn_sched_barrier(0);
        // Units of MFMAs with the remaining LDS reads and the DMA pieces of chunk kc+D spread between
        // them: every non-MFMA instruction issues while the matrix pipe is busy with the previous unit.
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int gu = ks * NU + u;                              // unit index within the chunk
#if !defined(YV3_ABLATE) || (YV3_ABLATE != 2)
                if (ks + 1 < KS) {
#pragma unroll
                    for (int f = u * NF / NU; f < (u + 1) * NF / NU; ++f) read_frag(ks + 1, f);
                }
#endif
                if (more) {
                    // all pieces go out during the FIRST k-step's units: the DMA then has the rest of this chunk's
                    // MFMAs to land before the wait at the top of the next iteration
                    constexpr int DU = YV3_DMA_UNITS < KS * NU ? YV3_DMA_UNITS : KS * NU;
#pragma unroll
                    for (int g = (gu < DU ? gu * G / DU : G); g < (gu < DU ? (gu + 1) * G / DU : G); ++g) {
#ifdef YV3_TIMELINE
                        const unsigned long long ta = __builtin_amdgcn_s_memtime();
                        dma_piece(g);
                        tl_dma += __builtin_amdgcn_s_memtime() - ta;
#else
                        dma_piece(g);
#endif
                    }
                }
#if defined(YV3_ABLATE) && (YV3_ABLATE == 3)
                {   // keep the fragment reads alive, skip the MFMAs: DMA + LDS-read path only
                    const int i = u / MT, j = u % MT;
#pragma unroll
                    for (int pl = 0; pl < NP; ++pl) {
                        asm volatile("" :: "v"(frag[ks][i * NP + pl]));
                        asm volatile("" :: "v"(frag[ks][NT * NP + j * NP + pl]));
                    }
                }
#elif !defined(YV3_ABLATE) || (YV3_ABLATE != 2)
                const int i = u / MT, j = u % MT;
                f32x16 c = acc[i][j];
                const bf16x8v* wf = &frag[ks][i * NP];
                const bf16x8v* xf = &frag[ks][NT * NP + j * NP];
                c = mfma_unit<NP, EL>(wf, xf, c);
                acc[i][j] = c;
#endif
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        cur = cur + 1 == NSTAGE ? 0 : cur + 1;
        nxt = nxt + 1 == NSTAGE ? 0 : nxt + 1;
    }

#ifdef YV3_TIMELINE
    if (blockIdx.x == 17 && lane == 0 && p.alpha) {      // debug build only: dump cycle split of one block into alpha[0..]
        float* dbg = const_cast<float*>(p.alpha);
        dbg[wid * 4 + 0] = (float)tl_wait; dbg[wid * 4 + 1] = (float)tl_bar; dbg[wid * 4 + 2] = (float)tl_body; dbg[wid * 4 + 3] = (float)tl_dma;
    }
#endif
    epilogue_store<NP, BM, BN, WM, WN, OUT_F32, true, EMTG, false, EL>(acc, p, lds, m0, n0, wid, lane);
}

// Launches the instantiation the choice names: tile / waves / ring are the template arguments (the switch of yv3_conv2d_planes), main loop
// and schedule are c.loop / c.stream_k.  The `if constexpr`s only keep combinations that do not exist from being instantiated; a choice
// that asks for one is an error of the selector.
template <int NP, int BM, int BN, int WM, int WN, int NSTAGE, int MINW = 1, int MTG = 0, bool ROLL = false, int EL = plane_elem(NP)>
int launch_cfg(const ConvParamsP& p, bool k3, bool dual, bool out_f32, const yv3_planes_choice& c, hipStream_t s) {
    const int mtiles = (p.M + BM - 1) / BM;
    const dim3 grid((unsigned)(mtiles * p.ntiles));
    const dim3 block(64 * WM * WN);
    const size_t pipe = (size_t)NSTAGE * NP * (BM + BN) * ROWB;
    const size_t epi = (size_t)WM * WN * (MTG ? MTG * 32 : BM / WM) * (BN / WN + 4) * 4;   // WM*WN waves x rows per round x (BN/WN + 4) floats
    const size_t lds = pipe > epi ? pipe : epi;
    ConvParamsP q = p;
    q.total = (int)grid.x;
    const dim3 sgrid((unsigned)c.grid);
    const bool pp = c.loop == YV3_LOOP_PINGPONG;
    if ((c.loop == YV3_LOOP_ROLLING) != ROLL || (c.stream_k && (!pp || c.grid <= 0))) return YV3_EINVAL;
#define YV3_LAUNCH(K3_, DUAL_, OF_) do { \
    if constexpr (NP == 1 && WM * WN == 8 && NSTAGE >= 3 && !ROLL) { \
        if (pp && !c.stream_k) { hipLaunchKernelGGL((conv_planes_kernel<NP, BM, BN, WM, WN, NSTAGE, K3_, DUAL_, OF_, true, false, 1, MTG, false, false, EL>), grid, block, lds, s, q); break; } \
    } \
    if constexpr (NP == 2 && WM * WN == 8 && NSTAGE >= 3 && !ROLL) { \
        if (c.stream_k) { hipLaunchKernelGGL((conv_planes_kernel<NP, BM, BN, WM, WN, NSTAGE, K3_, DUAL_, OF_, true, true>), sgrid, block, lds, s, q); break; } \
        if (pp) { hipLaunchKernelGGL((conv_planes_kernel<NP, BM, BN, WM, WN, NSTAGE, K3_, DUAL_, OF_, true>), grid, block, lds, s, q); break; } \
    } \
    if (pp) return YV3_EINVAL; \
    hipLaunchKernelGGL((conv_planes_kernel<NP, BM, BN, WM, WN, NSTAGE, K3_, DUAL_, OF_, false, false, MINW, MTG, false, ROLL, EL>), grid, block, lds, s, q); } while (0)
    if (out_f32) {
        if (k3 || dual) return YV3_ESHAPE;                   // fp32 outputs are the 1x1 head convs
        if constexpr (EL == YV3_EL_I8) return YV3_EDTYPE;    // (int8 layers write int8 or bf16; the head convs are YV3_BF16 launches)
        else YV3_LAUNCH(false, false, true);
    } else if (k3) YV3_LAUNCH(true, false, false);
    else if (dual) YV3_LAUNCH(false, true, false);
    else YV3_LAUNCH(false, false, false);
#undef YV3_LAUNCH
    YV3_CHECK_LAUNCH();
    return 0;
}

// OIHW fp32 -> NP bf16 planes in LDS-image order:
//   [n / tb][k / PBK][plane][n % tb][physical slot][8],  physical slot = (k % PBK)/8 ^ swz(n % tb),
//   k = (kh*3+kw)*cin + c
template <int NP, int EL = plane_elem(NP)>
__global__ void pack_weight_planes_kernel(const float* __restrict__ in, u16* __restrict__ out,
                                          int cout, int cin, int k, int tb, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;    // over [cout_pad][K]
    if (i >= total) return;
    const int kk = k * k;
    const int K = kk * cin;
    const int n = (int)(i / K);
    const int kidx = (int)(i - (long long)n * K);
    const int tap = kidx / cin, c = kidx - tap * cin;
    float v = 0.f;
    if (n < cout) v = in[((long long)n * cin + c) * kk + tap];
    const int nk = K / PBK;
    const int r = n % tb, ke = kidx % PBK;
    const int slot = (ke >> 3) ^ swz(r);
    const long long base = (((long long)(n / tb) * nk + kidx / PBK) * NP) * (long long)(tb * PBK) + r * PBK + slot * 8 + (ke & 7);
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) {
        const u16 h = ElemOps<EL>::cvt(v);
        out[base + (long long)pl * tb * PBK] = h;
        v -= ElemOps<EL>::back(h);
    }
}

// fp32 [n] -> NP planes (RN split); used for layout conversion of whole tensors
template <int NP, int EL = plane_elem(NP)>
__global__ void split_planes_kernel(const float* __restrict__ in, u16* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = in[i];
    if constexpr (NP == 1 && EL == YV3_EL_F16) {         // (one fp16 plane: NaN stays NaN -- the saturating min / max would make it -65504)
        if (v != v) { out[i] = 0x7e00; return; }
    }
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) {
        const u16 h = ElemOps<EL>::cvt(v);
        out[i + pl * n] = h;
        v -= ElemOps<EL>::back(h);
    }
}

template <int NP, int EL = plane_elem(NP)>
__global__ void merge_planes_kernel(const u16* __restrict__ in, float* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = 0.f;
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) v += ElemOps<EL>::back(in[i + pl * n]);
    out[i] = v;
}

// yv3_conv2d_planes' / yv3_conv2d_planes_f16's kernel parameters: the descriptor and the selector's choice, nothing decided here.
inline ConvParamsP conv_planes_params(const yv3_conv_desc* d, const yv3_planes_choice& c) {
    ConvParamsP p;
    p.x = (const u16*)d->x; p.x2 = (const u16*)d->x2; p.w = (const u16*)d->w;
    p.alpha = d->alpha; p.beta = d->beta; p.res = (const u16*)d->residual; p.y = d->y;
    p.H = d->H; p.W = d->W; p.Cin = d->cin; p.Cup = d->cin_up; p.Cout = d->cout;
    p.stride = d->stride; p.act = d->act; p.flags = d->flags;
    for (int i = 0; i < 4; ++i) p.tune[i] = d->tune[i];            // (the measurement builds' hooks inside the kernels)
    p.dec_out = nullptr;
    if (d->dec_out) {
        p.dec_out = d->dec_out; p.dec_bs = d->dec_out_batch_stride; p.dec_stride = d->dec_stride;
        for (int i = 0; i < 6; ++i) p.dec_an[i] = d->dec_anchors[i] / d->dec_stride;     // float32 division, as torch does
    }
    p.ws = (float*)d->workspace; p.ws_bytes = d->workspace ? d->workspace_bytes : 0;
    p.wsflags = d->workspace ? (int*)((char*)d->workspace + (size_t)YV3_SK_MAX_WG * YV3_SK_PART_BYTES) : nullptr;
    p.Ho = c.Ho; p.Wo = c.Wo; p.M = c.M;
    p.K = d->k * d->k * d->cin;
    p.nk = p.K / PBK;
    if (d->cin_up) {
        p.xs = (long long)d->B * (d->H / 2) * (d->W / 2) * d->cin_up;
        p.x2s = (long long)d->B * d->H * d->W * (d->cin - d->cin_up);
    } else {
        p.xs = (long long)d->B * d->H * d->W * d->cin;
        p.x2s = 0;
    }
    p.ys = (long long)c.M * d->cout;
    if (d->x_plane_stride > 0) p.xs = d->x_plane_stride;            // batch slices of larger plane tensors
    if (d->x2_plane_stride > 0) p.x2s = d->x2_plane_stride;
    if (d->y_plane_stride > 0) p.ys = d->y_plane_stride;
    p.tb = d->cout_pad < 128 ? d->cout_pad : 128;
    p.ntiles = c.ntiles;
    p.s_res = 0.f; p.inv_s_out = 0.f; p.out_bf16 = 0;               // (YV3_I8 launches set them: conv_planes_i8.hip)
    return p;
}

// The one-plane tiles (YV3_BF16 and YV3_F16: the same kernels with another element type): the ONE table from a kernel of the choice to
// its instantiation -- rows x channels, waves WM x WN, ring, workgroups per CU, epilogue rounds, rolling loop.  YV3_EINVAL: not a
// one-plane tile of this file (the k3s1 kernels are conv_planes_k3s1.hip's; the Winograd stages and the w4 tile are never chosen for one plane).
template <int EL>
int launch_one_plane(const ConvParamsP& p, bool k3, bool dual, bool out_f32, const yv3_planes_choice& c, hipStream_t s) {
#define YV3_T1(...) launch_cfg<1, __VA_ARGS__, EL>(p, k3, dual, out_f32, c, s)
    switch (c.kernel) {
        case YV3_PK_256x128_W8:      return YV3_T1(256, 128, 4, 2, 2, 1, 0, false);
        case YV3_PK_128x128_W8:      return YV3_T1(128, 128, 4, 2, 3, 1, 0, false);
        case YV3_PK_128x128_W4:      return YV3_T1(128, 128, 2, 2, 2, 2, 0, false);
        case YV3_PK_128x64:          return YV3_T1(128, 64, 2, 2, 2, 1, 0, false);
        case YV3_PK_128x32:          return YV3_T1(128, 32, 4, 1, 2, 1, 0, false);
        case YV3_PK_256x128_W8_PP6:  return YV3_T1(256, 128, 4, 2, 6, 1, 0, false);
        case YV3_PK_256x128_W4:      return YV3_T1(256, 128, 2, 2, 3, 2, 2, false);
        case YV3_PK_256x128_W4_ROLL: return YV3_T1(256, 128, 2, 2, 3, 2, 2, true);
        case YV3_PK_256x256:         return YV3_T1(256, 256, 2, 4, 3, 1, 1, false);
        case YV3_PK_256x256_ROLL:    return YV3_T1(256, 256, 2, 4, 3, 1, 1, true);
        case YV3_PK_256x256_ROLL4:   return YV3_T1(256, 256, 2, 4, 4, 1, 1, true);
        case YV3_PK_256x256_PP3:     return YV3_T1(256, 256, 2, 4, 3, 1, 1, false);
        case YV3_PK_256x256_PP4:     return YV3_T1(256, 256, 2, 4, 4, 1, 1, false);
        case YV3_PK_192x256_ROLL:    return YV3_T1(192, 256, 2, 4, 3, 1, 1, true);
        case YV3_PK_192x256_PP3:     return YV3_T1(192, 256, 2, 4, 3, 1, 1, false);
        case YV3_PK_192x256_PP4:     return YV3_T1(192, 256, 2, 4, 4, 1, 1, false);
        default: return YV3_EINVAL;
    }
#undef YV3_T1
}

}  // namespace
