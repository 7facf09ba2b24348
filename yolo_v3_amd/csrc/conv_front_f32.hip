// The first two layers of Darknet-53 as ONE kernel, EXACT-fp32 mode (YV3_F32) -- the fp32 twin of conv_front.hip:
//     feature.mlist.0  conv_bn_relu(3 -> 32, 3x3, s1)   reference darknet.py:76, :43-44
//     feature.mlist.1  conv_bn_relu(32 -> 64, 3x3, s2)  reference darknet.py:68-70 (make_res_stack's down-sampling conv)
// Unfused, the first layer writes a [B,H,W,32] fp32 activation (1.42 GB at 416x416 bs=64) that the second immediately re-reads:
// 0.68 + 1.04 ms of the mode's 26.5 ms step.  Here it never leaves the CU: a persistent workgroup walks 8x16-pixel tiles of the
// SECOND layer's output, two barriers per tile, and for each tile
//   1. stages the 19 x 35 x 3 input patch (NCHW fp32, zero halo) in LDS                  (prefetched one tile ahead in registers)
//   2. computes the 17 x 33 first-layer pixels the tile needs on the matrix cores: 36 blocks of 16 pixels x 2 blocks of 16 channels,
//      K = 27 taps (c, kh, kw) + one zero slot in FRONT = 7 x v_mfma_f32_16x16x4_f32, the weights as the A operand (in registers), the
//      B fragments gathered from the patch (im2col by LDS address).  An f32 MFMA is a k-ordered fmaf chain, so this is conv0.hip's
//      conv0_kernel<0> chain fma for fma: acc = fma(x, w, acc) over (c, kh, kw) from +0 (the zero slot leaves the +0 start a +0).
//      BN + LeakyReLU, one ds_write_b128 of 4 channels per block into an LDS-resident fp32 image, zero where the pixel lies outside
//      the picture (the second conv's padding), stored by column parity [parity][17 rows][18] so that the stride-2 taps read
//      CONSECUTIVE 128-byte rows, XOR-swizzled by the half-column (slot ^ (colh >> 1) & 7): conflict-free ds_read_b128 for all nine taps;
//   3. runs the second conv (M = 64 channels, N = 128 pixels, K = 9 taps x 32; v_mfma_f32_32x32x2_f32, weights as the A operand)
//      entirely out of LDS: its weights (72 KB of fp32) are DMA-ed once per workgroup and stay resident -- no global traffic, no barrier;
//   4. BN + LeakyReLU straight from the accumulators (a lane holds 4 groups of 4 consecutive channels of one pixel) -> 16-byte stores,
//      DEFERRED into the next tile's step 2: waves 0-3 run it behind their first-layer blocks, waves 4-7 (their SIMD partners) in front,
//      so that on every SIMD one wave has matrix work while the other stores.  The last tile's epilogue runs after the loop.
// Same operations in the same order as yv3_conv0(YV3_F32) followed by yv3_conv2d(YV3_F32) (k pairs 8 kk + t / 8 kk + 4 + t per
// MFMA, as conv_igemm_f32_kernel): BIT-IDENTICAL to the two launches (tests/test_gpu_kernels.py::
// test_fused_front_f32_equals_two_launches_bitwise).  HBM traffic: 12 B in + 256 B out per second-layer pixel.
// LDS: 78 336 (image) + 73 728 (weights) + 8 208 (patch) = 160 272 B: one workgroup per CU.
#include "yv3_common.h"

namespace {

constexpr int GT_R = 8, GT_C = 16;                        // output tile of the second conv (rows x cols)
constexpr int GR_COLS = 2 * GT_C + 1;                     // first-layer region: 17 rows x 33 cols
constexpr int GR_PX = (2 * GT_R + 1) * GR_COLS;           // 561
constexpr int GR_BLK = (GR_PX + 15) / 16;                 // 36 blocks of 16 pixels
constexpr int GP_ROWS = 2 * GT_R + 3, GP_COLS = 2 * GT_C + 3;   // input patch 19 x 35
constexpr int GP_PITCH = 36, GP_CH = GP_ROWS * GP_PITCH;  // floats
constexpr int GA_RP = 18, GA_PB = (2 * GT_R + 1) * GA_RP; // image row pitch (pixels), parity block (306 pixels; even)
constexpr int G_ROWB = 32 * 4;                            // bytes per image pixel / per weight row (32 fp32)
constexpr int GA_BYTES = 2 * GA_PB * G_ROWB;              // 78 336
constexpr int GW_BYTES = 9 * 64 * G_ROWB;                 // 73 728: [tap][64 channel rows][32 k]
constexpr int G_A_OFF = 0, G_W_OFF = GA_BYTES, G_P_OFF = G_W_OFF + GW_BYTES, G_LDS = G_P_OFF + 3 * GP_CH * 4;     // 160 272
static_assert(G_LDS <= 160 * 1024, "LDS budget");

#define GGPTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define GLPTR(p) ((__attribute__((address_space(3))) void*)(p))

struct FrontF32Params {
    const float* x;          // [B,3,H,W] fp32
    const float* w0;         // first layer weights [27][32] fp32 (tap-major: ((c*3 + kh)*3 + kw)*32 + n)
    const float* alpha0; const float* beta0;
    const float* w1;         // second layer [64][3][3][32] fp32
    const float* alpha1; const float* beta1;
    float* y;                // [B,H/2,W/2,64]
    int H, W, B, tiles_x, tiles_y, total;
};

__global__ __launch_bounds__(512) void conv_front_f32_kernel(const FrontF32Params p, const float* __restrict__ w0) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    float* const patch = reinterpret_cast<float*>(lds + G_P_OFF);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);                // 8 waves: two per SIMD
    const int l31 = lane & 31, lhi = lane >> 5, l15 = lane & 15, q4 = lane >> 4;
    const int wm = wid >> 1, wn = wid & 1;                // second conv: wave tile 32 channels (wn) x 32 pixels (tile rows 2wm, 2wm+1)
    const int Ho = p.H >> 1, Wo = p.W >> 1;

    // ---- second-layer weights: resident in LDS for the launch.  72 wave instructions of 8 rows x 128 B; lane -> (row, physical slot)
    for (int pc = wid; pc < GW_BYTES / 1024; pc += 8) {
        const int r = pc * 8 + (lane >> 3);               // tap * 64 + channel row
        const int tap = r >> 6, n = r & 63;
        const int ls = (lane & 7) ^ ((n >> 1) & 7);       // logical 16-byte slot this lane carries
        __builtin_amdgcn_global_load_lds(GGPTR(p.w1 + (long long)n * 288 + tap * 32 + ls * 4), GLPTR(lds + G_W_OFF + pc * 1024), 16, 0, 0);
    }
    // ---- first layer: k slot q4 of MFMA m carries tap k = 4 m + q4 - 1 (k = -1: the zero slot).  A operand: weight of channel
    // 16 cb + l15; B operand: patch float at koff[m] from the pixel's corner
    float w0a[2][7];
    int koff[7];
#pragma unroll
    for (int m = 0; m < 7; ++m) {
        const int k = 4 * m + q4 - 1, kc = k < 0 ? 0 : k;
        const int c = kc / 9, kh = (kc % 9) / 3, kw = kc % 3;
        koff[m] = (c * GP_CH + kh * GP_PITCH + kw) * 4;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) w0a[cb][m] = k < 0 ? 0.f : w0[k * 32 + cb * 16 + l15];
    }
    const bool kzero = q4 == 0;                           // this lane's slot of MFMA 0 is the zero slot
    f32x4 al0[2], be0[2];                                 // D of block cb: channels 16 cb + 4 q4 + (0..3)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        al0[cb] = *reinterpret_cast<const f32x4*>(p.alpha0 + cb * 16 + 4 * q4);
        be0[cb] = *reinterpret_cast<const f32x4*>(p.beta0 + cb * 16 + 4 * q4);
    }
    f32x4 al1[4], be1[4];                                 // second conv epilogue: channels wn * 32 + 8 g + 4 lhi + (0..3)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        al1[g] = *reinterpret_cast<const f32x4*>(p.alpha1 + wn * 32 + 8 * g + 4 * lhi);
        be1[g] = *reinterpret_cast<const f32x4*>(p.beta1 + wn * 32 + 8 * g + 4 * lhi);
    }

    // ---- first-layer blocks of this wave (pb = wid + 8 j; the fifth only for waves 0-3): the pixel's patch corner (LDS byte address),
    // its image pixel (byte address, -1: no pixel; swizzle key (col >> 2) & 7), and (row << 8 | col) in the region -- tile-independent
    constexpr int FJ = (GR_BLK + 7) / 8;                  // 5
    static_assert(GR_BLK == 8 * (FJ - 1) + 4, "waves 0-3 take FJ blocks, waves 4-7 FJ - 1");
    int fpo[FJ], fimg[FJ], fpos[FJ];
#pragma unroll
    for (int j = 0; j < FJ; ++j) {
        const int idx = (wid + 8 * j) * 16 + l15;
        const bool live = idx < GR_PX;
        const int ii = live ? idx : 0;
        const int row = ii / GR_COLS, col = ii - row * GR_COLS, colh = col >> 1;
        fpo[j] = G_P_OFF + (row * GP_PITCH + col) * 4;
        fimg[j] = live ? G_A_OFF + ((col & 1) * GA_PB + row * GA_RP + colh) * G_ROWB : -1;
        fpos[j] = (row << 8) | col;
    }

    // ---- fragment addresses of the second conv (constant over tiles).  Pixel side: lane -> (tile row, tile col) of its output pixel;
    // image pixel of tap (kh,kw): parity = kw&1, row 2r+kh, half-column c + (kw>>1); the swizzle key follows the half-column
    const int pr = l31 >> 4, pcx = l31 & 15;
    int xa[2], xsw[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) { xa[q] = G_A_OFF + ((2 * (2 * wm + pr)) * GA_RP + pcx + q) * G_ROWB; xsw[q] = ((pcx + q) >> 1) & 7; }
    const int wa = G_W_OFF + (wn * 32 + l31) * G_ROWB, wsw = (l31 >> 1) & 7;

    // ---- patch elements of this thread (i = tid + 512*k of 3 x 19 x 35): LDS index, offset in the picture, position -- tile-independent
    constexpr int PN = 3 * GP_ROWS * GP_COLS;             // 1995
    constexpr int PK = (PN + 511) / 512;                  // 4
    int plds[PK], prr[PK], pcc[PK];
    long long pgo[PK];
#pragma unroll
    for (int k = 0; k < PK; ++k) {
        const int i = tid + 512 * k;
        const int c = i / (GP_ROWS * GP_COLS);
        const int r2 = i - c * (GP_ROWS * GP_COLS);
        prr[k] = r2 / GP_COLS; pcc[k] = r2 - prr[k] * GP_COLS;
        plds[k] = i < PN ? c * GP_CH + prr[k] * GP_PITCH + pcc[k] : -1;
        pgo[k] = ((long long)c * p.H + prr[k] - 2) * p.W + pcc[k] - 2;
    }
    float pre[PK];
    auto patch_fetch = [&](int tile) {
        const int b = tile / (p.tiles_x * p.tiles_y);
        const int rem = tile - b * (p.tiles_x * p.tiles_y);
        const int ty = rem / p.tiles_x, tx = rem - ty * p.tiles_x;
        const float* xb = p.x + (size_t)b * 3 * p.H * p.W + (long long)(2 * GT_R * ty) * p.W + 2 * GT_C * tx;
#pragma unroll
        for (int k = 0; k < PK; ++k) {
            const int gy = 2 * GT_R * ty - 2 + prr[k], gx = 2 * GT_C * tx - 2 + pcc[k];
            float v = 0.f;
            if (plds[k] >= 0 && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) v = xb[pgo[k]];
            pre[k] = v;
        }
    };

    // ---- deferred epilogue of the previous tile: sums and the output offset of this lane's pixel (+ wn * 32 + 4 lhi)
    f32x16 pacc;
    long long pm = 0;
    bool pend = false;
    auto epilogue = [&]() {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float t = fmaf(pacc[4 * g + i], al1[g][i], be1[g][i]);
                v[i] = t > 0.f ? t : 0.1f * t;
            }
            *reinterpret_cast<f32x4*>(p.y + pm + 8 * g) = v;
        }
    };

#if defined(YV3_MEASURE) && defined(YV3_TIMELINE)        // cycle split of workgroup 17 -> the first floats of y (results INVALID)
    unsigned long long tl_s[5] = {0, 0, 0, 0, 0}, tl_t = 0;   // [top barrier (+ waits), deferred epilogue, first layer, mid barrier, 3x3]
    int tl_n = 0;
#define FR_MARK(i_) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); tl_s[i_] += t_ - tl_t; tl_t = t_; } while (0)
    const unsigned long long tl_entry = __builtin_amdgcn_s_memtime();
    tl_t = tl_entry;
#else
#define FR_MARK(i_) do {} while (0)
#endif
    if ((int)blockIdx.x < p.total) patch_fetch(blockIdx.x);

    for (int tile = blockIdx.x; tile < p.total; tile += gridDim.x) {
        const int b = tile / (p.tiles_x * p.tiles_y);
        const int rem = tile - b * (p.tiles_x * p.tiles_y);
        const int ty = rem / p.tiles_x, tx = rem - ty * p.tiles_x;
        const int r0 = GT_R * ty, c0 = GT_C * tx;

        // ---- 1. patch -> LDS.  Every wave is past the previous tile's first layer here (its patch reads are done).
#pragma unroll
        for (int k = 0; k < PK; ++k)
            if (plds[k] >= 0) patch[plds[k]] = pre[k];
        if (tile == (int)blockIdx.x) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // my share of the weight DMA has landed
        __syncthreads();                                          // patch complete; every wave is past its reads of the image
        if (tile + (int)gridDim.x < p.total) patch_fetch(tile + gridDim.x);       // lands during steps 2-3
        FR_MARK(0);

        // ---- 2. first layer for the 561 region pixels: blocks pb = wid + 8 j (waves 0-3: five, 4-7: four), in two batches (j < 3,
        // j >= 3): a batch's fragment reads up front, then 7 rounds of independent MFMAs, then BN + LeakyReLU + image writes; the pending
        // epilogue behind (waves 0-3) or in front (4-7) of them
        if (wid >= 4 && pend) { epilogue(); FR_MARK(1); }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            constexpr int NB = 3;
            const int j0 = h ? NB : 0, nj = h ? FJ - NB : NB;
            float xv[NB][7];
            f32x4 acc[NB][2];
#pragma unroll
            for (int jj = 0; jj < NB; ++jj) {
                const int j = j0 + jj;
                if (jj < nj && (j < FJ - 1 || wid < 4)) {                      // (compile-time / wave-uniform)
#pragma unroll
                    for (int m = 0; m < 7; ++m) xv[jj][m] = *reinterpret_cast<const float*>(lds + fpo[j] + koff[m]);
                    if (kzero) xv[jj][0] = 0.f;
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) acc[jj][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
#pragma unroll
            for (int m = 0; m < 7; ++m)
#pragma unroll
                for (int jj = 0; jj < NB; ++jj)
                    if (jj < nj && (j0 + jj < FJ - 1 || wid < 4))
#pragma unroll
                        for (int cb = 0; cb < 2; ++cb)
                            acc[jj][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0a[cb][m], xv[jj][m], acc[jj][cb], 0, 0, 0);
#pragma unroll
            for (int jj = 0; jj < NB; ++jj) {
                const int j = j0 + jj;
                if (jj < nj && (j < FJ - 1 || wid < 4) && fimg[j] >= 0) {
                    const int gy = 2 * r0 - 1 + (fpos[j] >> 8), gx = 2 * c0 - 1 + (fpos[j] & 255);
                    const bool inimg = (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) {
                        f32x4 o;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            float v = fmaf(acc[jj][cb][i], al0[cb][i], be0[cb][i]);
                            v = v > 0.f ? v : 0.1f * v;                          // (conv0_kernel's form of LeakyReLU(0.1))
                            o[i] = inimg ? v : 0.f;                             // outside the picture: the second conv's zero padding
                        }
                        *reinterpret_cast<f32x4*>(lds + fimg[j] + (((4 * cb + q4) ^ ((fpos[j] >> 2) & 7)) * 16)) = o;
                    }
                }
            }
        }
        FR_MARK(2);
        if (wid < 4 && pend) { epilogue(); FR_MARK(1); }
        __syncthreads();                                                          // image complete
        FR_MARK(3);

        // ---- 3. second conv out of LDS: 9 taps x 4 groups of 8 k, K order (kh, kw, c)
        f32x16 acc2;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc2[e] = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int kh = tap / 3, kw = tap % 3;
            const int aoff = ((kw & 1) * GA_PB + kh * GA_RP) * G_ROWB;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const f32x4 xf = *reinterpret_cast<const f32x4*>(lds + xa[kw >> 1] + aoff + (((kk * 2 + lhi) ^ xsw[kw >> 1]) * 16));
                const f32x4 wf = *reinterpret_cast<const f32x4*>(lds + wa + tap * (64 * G_ROWB) + (((kk * 2 + lhi) ^ wsw) * 16));
#pragma unroll
                for (int t = 0; t < 4; ++t) acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[t], xf[t], acc2, 0, 0, 0);
            }
        }
        pacc = acc2;
        pm = (((long long)b * Ho + r0 + 2 * wm + pr) * Wo + c0 + pcx) * 64 + wn * 32 + 4 * lhi;
        pend = true;
        FR_MARK(4);
#if defined(YV3_MEASURE) && defined(YV3_TIMELINE)
        ++tl_n;
#endif
    }
    if (pend) { epilogue(); FR_MARK(1); }                             // the last tile's epilogue
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#if defined(YV3_MEASURE) && defined(YV3_TIMELINE)
    if (blockIdx.x == 17 && lane == 0) {
        float* dbg = p.y + wid * 8;
        for (int i = 0; i < 5; ++i) dbg[i] = (float)tl_s[i] / (tl_n > 0 ? tl_n : 1);
        dbg[5] = (float)(tl_t - tl_entry); dbg[6] = (float)tl_n;
    }
#endif
#undef FR_MARK
}

}  // namespace

extern "C" int yv3_conv_front_f32(const float* x_nchw, const float* w0_tap_major, const float* alpha0, const float* beta0,
                                  const float* w1_packed, const float* alpha1, const float* beta1, float* y,
                                  int B, int H, int W, void* stream) {
    if (!x_nchw || !w0_tap_major || !alpha0 || !beta0 || !w1_packed || !alpha1 || !beta1 || !y || B <= 0 || H <= 0 || W <= 0)
        return YV3_EINVAL;
    if ((H % (2 * GT_R)) || (W % (2 * GT_C))) return YV3_ESHAPE;          // whole 8 x 16 output tiles only (network inputs are multiples of 32)
    FrontF32Params p;
    p.x = x_nchw; p.w0 = w0_tap_major; p.alpha0 = alpha0; p.beta0 = beta0;
    p.w1 = w1_packed; p.alpha1 = alpha1; p.beta1 = beta1; p.y = y;
    p.H = H; p.W = W; p.B = B;
    p.tiles_x = (W / 2) / GT_C; p.tiles_y = (H / 2) / GT_R;
    const long long total = (long long)B * p.tiles_x * p.tiles_y;
    if (total > 0x7fffffffLL) return YV3_ESHAPE;
    p.total = (int)total;
    const int ncu = yv3_num_cu();
    const int grid = p.total < ncu ? p.total : ncu;                      // persistent: one workgroup per CU
    hipLaunchKernelGGL(conv_front_f32_kernel, dim3(grid), dim3(512), G_LDS, (hipStream_t)stream, p, w0_tap_major);
    YV3_CHECK_LAUNCH();
    return 0;
}
