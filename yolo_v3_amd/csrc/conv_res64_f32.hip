// The first residual block of Darknet-53 as ONE kernel, EXACT-fp32 mode (YV3_F32):
//     feature.mlist.2 = res_layer(64):  x + conv_bn_relu(32 -> 64, 3x3)(conv_bn_relu(64 -> 32, 1x1)(x))    reference darknet.py:46-53
// The fp32 twin of conv_res64.hip.  Unfused, the two launches cost 0.23 + 1.09 ms of the exact-fp32 mode's 27 ms step at 416x416 bs=64
// -- 1.4 GB of fp32 activations through HBM for 0.11 TFLOP -- against 0.72 ms of fp32 MFMA time.  A persistent workgroup per CU walks
// 8x16-pixel output tiles, two barriers per tile:
//   1. the 10 x 18 x 64-channel region of x the tile needs is DMA-ed into LDS (global_load_lds, issued a tile ahead): 192 rows of 256 B,
//      16-byte slots XOR-swizzled by the row (slot ^ row & 15) so that the fragment reads of 16 consecutive rows are conflict-free;
//   2. the 1x1 conv runs on the matrix cores for those 180 pixels, all eight waves busy: 12 blocks of 16 pixels x 2 blocks of 16
//      channels, three blocks per wave, v_mfma_f32_16x16x4_f32 with the weights as the A operand (in registers) -- so that a lane's
//      D fragment is 4 consecutive channels of one pixel: BN + LeakyReLU, one ds_write_b128 into an LDS-resident fp32 image (zero
//      outside the picture: the 3x3 conv's padding), pitch 20 pixels, rows of 128 B swizzled by the image column (slot ^ (col >> 1) & 7);
//   3. the 3x3 conv (M = 64 channels, N = 128 pixels, K = 9 x 32; v_mfma_f32_32x32x2_f32, weights as the A operand) runs entirely out of
//      LDS -- its weights (72 KB of fp32) are resident for the whole launch -- no global traffic, no barrier inside;
//   4. epilogue straight from the accumulators (a lane holds 4 groups of 4 consecutive channels of one pixel): BN + LeakyReLU + residual
//      (x rows re-read from L2, requested before step 3) -> 16-byte stores.  It is DEFERRED into the next tile's step 2: waves 0-3 run it
//      behind their share of the 1x1, waves 4-7 (their SIMD partners) in front of theirs, so that on every SIMD one wave has matrix work
//      while the other stores.  The last tile's epilogue runs after the loop.
// Same products in the same K order as conv_igemm_f32_kernel (an f32 MFMA is a k-ordered fmaf chain over its k slots, whichever operand
// is A): per group of 8 k, k = 0, 4, 1, 5, 2, 6, 3, 7 -- the 32x32x2 pairing (8 kk + t, 8 kk + 4 + t) laid out over the 16x16x4 MFMA's
// four slots for the 1x1 -- same epilogue operations: BIT-IDENTICAL to yv3_conv2d (1x1) followed by yv3_conv2d (3x3 + residual) in
// YV3_F32 (tests/test_gpu_kernels.py::test_fused_res64_f32_equals_two_launches_bitwise).  HBM traffic: x once (+ 41 % halo) + y once.
#include "yv3_common.h"

namespace {

constexpr int QT_R = 8, QT_C = 16;                        // output tile (rows x cols)
constexpr int QR_COLS = QT_C + 2, QR_PX = (QT_R + 2) * QR_COLS;   // region 10 x 18 = 180 pixels
constexpr int QR_ROWS = 192;                              // padded to 12 blocks of 16 pixels
constexpr int QX_ROWB = 64 * 4;                           // bytes per x-region row (64 channels)
constexpr int QX_BYTES = QR_ROWS * QX_ROWB;               // 49 152
constexpr int QI_RP = 20;                                 // image pitch (pixels per row; even: pixel parity == column parity)
constexpr int QI_ROWB = 32 * 4;                           // bytes per image pixel (32 channels)
constexpr int QI_BYTES = (QT_R + 2) * QI_RP * QI_ROWB;    // 25 600
constexpr int QW_BYTES = 9 * 64 * QI_ROWB;                // 73 728: [tap][64 channel rows][32 k]
constexpr int Q_X_OFF = 0, Q_I_OFF = QX_BYTES, Q_W_OFF = Q_I_OFF + QI_BYTES, Q_LDS = Q_W_OFF + QW_BYTES;   // 148 480
static_assert(Q_LDS <= 160 * 1024, "LDS budget");

#define QGPTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define QLPTR(p) ((__attribute__((address_space(3))) void*)(p))

__device__ __attribute__((aligned(64))) float g_zero_f32_res[16];      // zero-initialised: source of out-of-picture region rows

struct Res64F32Params {
    const float* x;          // [B,H,W,64]
    const float* w1; const float* alpha1; const float* beta1;      // 1x1 64 -> 32: [32][64]
    const float* w2; const float* alpha2; const float* beta2;      // 3x3 32 -> 64: [64][3][3][32]
    float* y;                // [B,H,W,64]
    int H, W, B, tiles_x, tiles_y, total;
};

__global__ __launch_bounds__(512) void conv_res64_f32_kernel(const Res64F32Params p) {
#pragma clang fp contract(off)                            // (the epilogue's LeakyReLU and residual add stay two roundings)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lhi = lane >> 5, l15 = lane & 15, q4 = lane >> 4;
    const int wm = wid >> 1, wn = wid & 1;                // 3x3 wave tile: 32 channels (wn) x 32 pixels (tile rows 2wm, 2wm+1)

    // ---- 3x3 weights: resident in LDS for the launch.  72 wave instructions of 8 rows x 128 B; lane -> (row, physical slot)
    for (int pc = wid; pc < QW_BYTES / 1024; pc += 8) {
        const int r = pc * 8 + (lane >> 3);               // tap * 64 + channel row
        const int tap = r >> 6, n = r & 63;
        const int ls = (lane & 7) ^ ((n >> 1) & 7);       // logical 16-byte slot this lane carries
        __builtin_amdgcn_global_load_lds(QGPTR(p.w2 + (long long)n * 288 + tap * 32 + ls * 4), QLPTR(lds + Q_W_OFF + pc * 1024), 16, 0, 0);
    }
    // ---- 1x1 weights: this lane's A operands, resident in registers.  Channel block cb = wid & 1 (row l15 of the A fragment), k slot q4;
    // MFMA m = 2 g + h of the 16 carries k = 8 g + 2 h + (q4 >> 1) + 4 (q4 & 1): slots 0..3 = k 8g + {0,4,1,5} (h = 0), {2,6,3,7} (h = 1)
    const int cb = wid & 1, kq = (q4 >> 1) + 4 * (q4 & 1);
    float w1a[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) w1a[m] = p.w1[(cb * 16 + l15) * 64 + 8 * (m >> 1) + 2 * (m & 1) + kq];
    const f32x4 al1 = *reinterpret_cast<const f32x4*>(p.alpha1 + cb * 16 + 4 * q4);
    const f32x4 be1 = *reinterpret_cast<const f32x4*>(p.beta1 + cb * 16 + 4 * q4);
    f32x4 al2[4], be2[4];                                 // 3x3 epilogue: channels wn * 32 + 8 g + 4 lhi + (0..3)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        al2[g] = *reinterpret_cast<const f32x4*>(p.alpha2 + wn * 32 + 8 * g + 4 * lhi);
        be2[g] = *reinterpret_cast<const f32x4*>(p.beta2 + wn * 32 + 8 * g + 4 * lhi);
    }

    // ---- x-region DMA: 48 wave instructions per tile (4 rows of 256 B each); this wave issues i = wid + 8k.  Per lane: region pixel of
    // its row, logical slot (the swizzle is applied on the source side), all tile-independent.
    constexpr int DK = 6;
    int drr[DK], dcc[DK], dls[DK];
#pragma unroll
    for (int k = 0; k < DK; ++k) {
        const int row = (wid + 8 * k) * 4 + (lane >> 4);
        drr[k] = row < QR_PX ? row / QR_COLS : -100;      // rows 180..191: never inside the picture -> zero page
        dcc[k] = row - (row / QR_COLS) * QR_COLS;
        dls[k] = ((lane & 15) ^ (row & 15)) * 4;          // floats
    }
    auto x_dma = [&](int tile) {
        const int b = tile / (p.tiles_x * p.tiles_y);
        const int rem = tile - b * (p.tiles_x * p.tiles_y);
        const int ty = rem / p.tiles_x, tx = rem - ty * p.tiles_x;
#pragma unroll
        for (int k = 0; k < DK; ++k) {
            const int gy = QT_R * ty - 1 + drr[k], gx = QT_C * tx - 1 + dcc[k];
            const bool ok = (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            const float* src = ok ? p.x + (((long long)b * p.H + gy) * p.W + gx) * 64 + dls[k] : g_zero_f32_res;
            __builtin_amdgcn_global_load_lds(QGPTR(src), QLPTR(lds + Q_X_OFF + (wid + 8 * k) * 1024), 16, 0, 0);
        }
    };

    // ---- 1x1: this wave's three pixel blocks rb = (wid >> 1) + 4 j (B operand: region pixel 16 rb + l15, k slot q4), both k of a lane
    // in one logical slot 2 g + (q4 & 1) of the row (physical slot ^ row & 15 == l15), floats q4 >> 1 and + 2.  D: channels
    // cb * 16 + 4 q4 + (0..3) of that pixel -> image byte address (-1: no pixel) and (row << 8 | col)
    constexpr int NJ = 3;
    int xrow[NJ], himg[NJ], hpos[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int ridx = ((wid >> 1) + 4 * j) * 16 + l15;
        const bool live = ridx < QR_PX;
        const int rr = live ? ridx / QR_COLS : 0, cc = live ? ridx - (ridx / QR_COLS) * QR_COLS : 0;
        xrow[j] = Q_X_OFF + ridx * QX_ROWB + (q4 >> 1) * 4;
        himg[j] = live ? Q_I_OFF + (rr * QI_RP + cc) * QI_ROWB + (((4 * cb + q4) ^ ((cc >> 1) & 7)) * 16) : -1;
        hpos[j] = (rr << 8) | cc;
    }

    // ---- 3x3 fragment addresses: pixel side (B) per column tap (the swizzle follows the image column), weight side (A)
    const int pr = l31 >> 4, pcx = l31 & 15;
    const int pbase = (2 * wm + pr) * QI_RP + pcx;
    int xa[3], xsw[3];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) { xa[kw] = Q_I_OFF + (pbase + kw) * QI_ROWB; xsw[kw] = ((pcx + kw) >> 1) & 7; }
    const int wa = Q_W_OFF + (wn * 32 + l31) * QI_ROWB, wsw = (l31 >> 1) & 7;          // ((wn * 32 + l31) >> 1) & 7 == (l31 >> 1) & 7

    // ---- deferred epilogue of the previous tile: sums, residual, output offset of this lane's pixel (+ wn * 32 + 4 lhi)
    f32x16 pacc;
    f32x4 pres[4];
    long long porow = 0;
    bool pend = false;
    auto epilogue = [&]() {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float t = fmaf(pacc[4 * g + i], al2[g][i], be2[g][i]);
                t = t > 0.f ? t : 0.1f * t;                   // (conv_igemm_f32.hip's form of LeakyReLU(0.1))
                v[i] = t + pres[g][i];
            }
            *reinterpret_cast<f32x4*>(p.y + porow + 8 * g) = v;
        }
    };

#if defined(YV3_MEASURE) && defined(YV3_TIMELINE)        // cycle split of workgroup 17 -> the first floats of y (results INVALID)
    unsigned long long tl_s[5] = {0, 0, 0, 0, 0}, tl_t = 0;   // [top barrier (+ waits), deferred epilogue, 1x1, mid barrier, 3x3]
    int tl_n = 0;
#define R64_MARK(i_) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); tl_s[i_] += t_ - tl_t; tl_t = t_; } while (0)
    const unsigned long long tl_entry = __builtin_amdgcn_s_memtime();
    tl_t = tl_entry;
#else
#define R64_MARK(i_) do {} while (0)
#endif
    if ((int)blockIdx.x < p.total) x_dma(blockIdx.x);
    for (int tile = blockIdx.x; tile < p.total; tile += gridDim.x) {
        const int b = tile / (p.tiles_x * p.tiles_y);
        const int rem = tile - b * (p.tiles_x * p.tiles_y);
        const int ty = rem / p.tiles_x, tx = rem - ty * p.tiles_x;
        const int r0 = QT_R * ty, c0 = QT_C * tx;

        // my share of this tile's x region (first tile: and of the weights) has landed, with the residual rows of the pending epilogue;
        // the previous epilogue's stores were acknowledged a whole 3x3 ago
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                          // the x region is complete; every wave is past its 3x3 reads of the image
        R64_MARK(0);

        // ---- 2. 1x1 conv (64 -> 32) for the region pixels -> image; the pending epilogue behind (waves 0-3) or in front (4-7) of it
        if (wid >= 4 && pend) { epilogue(); R64_MARK(1); }
        {
            f32x4 acc[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int g = 0; g < 8; ++g) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const float* xs = reinterpret_cast<const float*>(lds + xrow[j] + (((2 * g + (q4 & 1)) ^ l15) * 16));
                    const float b0 = xs[0], b1 = xs[2];
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1a[2 * g], b0, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1a[2 * g + 1], b1, acc[j], 0, 0, 0);
                }
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (himg[j] >= 0) {
                    const int gy = r0 - 1 + (hpos[j] >> 8), gx = c0 - 1 + (hpos[j] & 255);
                    const bool inpic = (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
                    f32x4 o;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float v = fmaf(acc[j][i], al1[i], be1[i]);
                        v = v > 0.f ? v : 0.1f * v;
                        o[i] = inpic ? v : 0.f;                   // outside the picture: the 3x3 conv's zero padding
                    }
                    *reinterpret_cast<f32x4*>(lds + himg[j]) = o;
                }
            }
        }
        R64_MARK(2);
        if (wid < 4 && pend) { epilogue(); R64_MARK(1); }
        __syncthreads();                                          // image complete; the x region is free again
        R64_MARK(3);
        if (tile + (int)gridDim.x < p.total) x_dma(tile + gridDim.x);          // lands during step 3

        // residual of this lane's pixel, 4 x 4 channels (L2-warm: the region DMA just read them), requested before the 3x3
        porow = (((long long)b * p.H + r0 + 2 * wm + pr) * p.W + c0 + pcx) * 64 + wn * 32 + 4 * lhi;
#pragma unroll
        for (int g = 0; g < 4; ++g) pres[g] = *reinterpret_cast<const f32x4*>(p.x + porow + 8 * g);

        // ---- 3. 3x3 conv out of LDS: 9 taps x 4 groups of 8 k, K order (kh, kw, c)
        f32x16 acc2;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc2[e] = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int kh = tap / 3, kw = tap % 3;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const f32x4 xf = *reinterpret_cast<const f32x4*>(lds + xa[kw] + kh * (QI_RP * QI_ROWB) + (((kk * 2 + lhi) ^ xsw[kw]) * 16));
                const f32x4 wf = *reinterpret_cast<const f32x4*>(lds + wa + tap * (64 * QI_ROWB) + (((kk * 2 + lhi) ^ wsw) * 16));
#pragma unroll
                for (int t = 0; t < 4; ++t) acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[t], xf[t], acc2, 0, 0, 0);
            }
        }
        pacc = acc2;
        pend = true;
        R64_MARK(4);
#if defined(YV3_MEASURE) && defined(YV3_TIMELINE)
        ++tl_n;
#endif
    }
    if (pend) {                                                   // the last tile's epilogue
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        epilogue();
        R64_MARK(1);
    }
#if defined(YV3_MEASURE) && defined(YV3_TIMELINE)
    if (blockIdx.x == 17 && lane == 0) {
        float* dbg = p.y + wid * 8;
        for (int i = 0; i < 5; ++i) dbg[i] = (float)tl_s[i] / (tl_n > 0 ? tl_n : 1);
        dbg[5] = (float)(tl_t - tl_entry); dbg[6] = (float)tl_n;
    }
#endif
#undef R64_MARK
}

}  // namespace

extern "C" int yv3_res_block64_f32(const float* x, const float* w1_packed, const float* alpha1, const float* beta1,
                                   const float* w2_packed, const float* alpha2, const float* beta2, float* y,
                                   int B, int H, int W, void* stream) {
    if (!x || !w1_packed || !alpha1 || !beta1 || !w2_packed || !alpha2 || !beta2 || !y || B <= 0 || H <= 0 || W <= 0) return YV3_EINVAL;
    if ((H % QT_R) || (W % QT_C)) return YV3_ESHAPE;                    // whole 8 x 16 tiles only
    Res64F32Params p;
    p.x = x; p.w1 = w1_packed; p.alpha1 = alpha1; p.beta1 = beta1;
    p.w2 = w2_packed; p.alpha2 = alpha2; p.beta2 = beta2; p.y = y;
    p.H = H; p.W = W; p.B = B;
    p.tiles_x = W / QT_C; p.tiles_y = H / QT_R;
    const long long total = (long long)B * p.tiles_x * p.tiles_y;
    if (total > 0x7fffffffLL) return YV3_ESHAPE;
    p.total = (int)total;
    const int ncu = yv3_num_cu();
    const int grid = p.total < ncu ? p.total : ncu;                    // persistent: one workgroup per CU
    hipLaunchKernelGGL(conv_res64_f32_kernel, dim3(grid), dim3(512), Q_LDS, (hipStream_t)stream, p);
    YV3_CHECK_LAUNCH();
    return 0;
}
