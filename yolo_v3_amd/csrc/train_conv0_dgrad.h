// dL/dx of the first layer (3x3, stride 1, pad 1, cin = 3) into the caller's NCHW image layout: the input gradient of the training
// step (yv3_train_conv0_dgrad in train.hip, yv3_train_conv0_dgrad_bf16 in train_bf16.hip; one kernel, the dz element type a
// template argument).
//
//   dx[b][ci][y][x] = sum over (kh, kw, co) of dz[b][y + 1 - kh][x + 1 - kw][co] * w[co][ci][kh][kw]
//
// As a GEMM this is N = 3, K = 9 cout: the 64x64 MFMA dgrad tile would run 61 of its 64 columns empty and write NHWC.  It is a
// memory-bound direct kernel instead: dz must be read once (cout elements per pixel) and three floats per pixel written.
//   * A tile is TH x TW pixels, one image row per wave.  Its dz with the one-pixel halo is staged in LDS as fp32 (a bf16 dz is
//     widened on the way in) by 16-byte loads that run along the NHWC rows; the halo re-reads hit L2.
//   * Eight lanes share a pixel: lane q of the eight owns channels 4q .. 4q+3 of the CC = 32 channel chunk, so one ds_read_b128 per
//     tap feeds 12 FMAs, and its 27 x 4 weights stay in registers for the whole launch (rounded to bf16 for the bf16 kernel, as
//     yv3_train_to_bf16 rounds) -- no weight traffic in the loop.  A 16-lane group of a ds_read_b128 reads 2 x 128 contiguous bytes:
//     conflict-free without padding.  The eight partial sums meet in a three-step xor butterfly.
//   * A wave takes its row in 8 steps of 8 pixels; lane (p, q) keeps the sum of step q, so after the row each lane holds one pixel
//     and every plane is stored as 64 consecutive floats per wave.
//   * Workgroups are persistent: each walks tiles blockIdx.x, + gridDim.x, ..., and loads the next tile's dz into registers before
//     it computes the current one, so the global loads fly under the FMAs.
//   * A launch covers CC channels; a wider cout (not the network's) takes one launch per chunk, each adding to dx after the first.
//     Each lane sums in the fixed order (tap, channel), the butterfly and the chunks in a fixed order too, all in fp32 and
//     independent of the grid.  No atomics: identical calls give identical bits.
#pragma once
#include "yv3_common.h"

namespace conv0dg {

constexpr int TW = 64, TH = 4, NT = TW * TH;
constexpr int CC = 32;
constexpr int HALO_W = TW + 2, HALO_H = TH + 2, HALO_P = HALO_W * HALO_H;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float round_bf16(float f) {                 // RNE, NaN -> the canonical quiet NaN (train_bf16.hip rne_bf16)
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u);
}

struct Args {
    const void* dz;        // BF16 ? bf16 : fp32, [B][H][W][ld]
    const float* w;        // [cout][3][3][3]
    float* dx;             // [B][3][H][W]
    int H, W, cout, ld;    // ld: channels per pixel in memory (cout; coutp for bf16)
    int tiles_x, tiles_y, n_tiles;
    int c0;                // this launch: channels c0 .. c0 + CC - 1, added to dx when c0 > 0
};

template <bool BF16>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv0_dgrad(const Args a) {
    constexpr int PER = BF16 ? 8 : 4, Q = CC / PER;                    // channels per 16-byte load, loads per pixel
    constexpr int NPRE = (HALO_P * Q + NT - 1) / NT;                   // staging loads per thread
    __shared__ __attribute__((aligned(16))) float tile[HALO_P * CC];
    const int tid = threadIdx.x, row = tid >> 6, p = (tid & 63) >> 3, q = tid & 7;

    f32x4 wr[27];                                                      // wr[tap * 3 + ci] = w[c0 + 4q .. + 3][ci][tap]
#pragma unroll
    for (int r = 0; r < 27; ++r) {
        const int tap = r / 3, ci = r - tap * 3;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int co = a.c0 + 4 * q + k;
            v[k] = co < a.cout ? a.w[(long long)co * 27 + ci * 9 + tap] : 0.f;
            if (BF16) v[k] = round_bf16(v[k]);
        }
        wr[r] = f32x4{v[0], v[1], v[2], v[3]};
    }

    u32x4 pre[NPRE];                                                   // the next tile's dz, on its way to LDS
    auto prefetch = [&](int t) {
        const int tx = t % a.tiles_x, ty = (t / a.tiles_x) % a.tiles_y, b = t / (a.tiles_x * a.tiles_y);
#pragma unroll
        for (int n = 0; n < NPRE; ++n) {
            const int i = tid + n * NT, hp = i / Q, hq = i - hp * Q;
            const int r = hp / HALO_W, c = hp - r * HALO_W;
            const int y = ty * TH - 1 + r, x = tx * TW - 1 + c, ch = a.c0 + hq * PER;
            const bool in = i < HALO_P * Q && y >= 0 && y < a.H && x >= 0 && x < a.W && ch < a.ld;
            const long long off = (((long long)b * a.H + y) * a.W + x) * a.ld + ch;
            pre[n] = u32x4{0u, 0u, 0u, 0u};
            if (in) pre[n] = BF16 ? *(const u32x4*)((const u16*)a.dz + off) : *(const u32x4*)((const float*)a.dz + off);
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int n = 0; n < NPRE; ++n) {
            const int i = tid + n * NT;
            if (i >= HALO_P * Q) break;
            const u32x4 v = pre[n];
            if (BF16) {
                *(u32x4*)(tile + i * 8) = u32x4{v.x << 16, v.x & 0xffff0000u, v.y << 16, v.y & 0xffff0000u};
                *(u32x4*)(tile + i * 8 + 4) = u32x4{v.z << 16, v.z & 0xffff0000u, v.w << 16, v.w & 0xffff0000u};
            } else {
                *(u32x4*)(tile + i * 4) = v;
            }
        }
    };

    if ((int)blockIdx.x < a.n_tiles) prefetch(blockIdx.x);
    for (int t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        __syncthreads();                                               // the previous tile's reads of the LDS image are done
        commit();
        __syncthreads();
        if (t + (int)gridDim.x < a.n_tiles) prefetch(t + gridDim.x);
        float out[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
        for (int s = 0; s < 8; ++s) {
            float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int kh = tap / 3, kw = tap - kh * 3;
                const f32x4 d = *(const f32x4*)(tile + ((row + 2 - kh) * HALO_W + (s * 8 + p + 2 - kw)) * CC + 4 * q);
#pragma unroll
                for (int ci = 0; ci < 3; ++ci) {
                    const f32x4 wv = wr[tap * 3 + ci];
                    acc[ci] = fmaf(d.x, wv.x, acc[ci]);
                    acc[ci] = fmaf(d.y, wv.y, acc[ci]);
                    acc[ci] = fmaf(d.z, wv.z, acc[ci]);
                    acc[ci] = fmaf(d.w, wv.w, acc[ci]);
                }
            }
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                float v = acc[ci];
                v += __shfl_xor(v, 1);
                v += __shfl_xor(v, 2);
                v += __shfl_xor(v, 4);
                out[ci] = q == s ? v : out[ci];
            }
        }
        const int tx = t % a.tiles_x, ty = (t / a.tiles_x) % a.tiles_y, b = t / (a.tiles_x * a.tiles_y);
        const int y = ty * TH + row, x = tx * TW + q * 8 + p;          // lane (p, q) kept step q's pixel p
        if (y < a.H && x < a.W)
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                float* dst = a.dx + (((long long)b * 3 + ci) * a.H + y) * a.W + x;
                *dst = a.c0 ? *dst + out[ci] : out[ci];
            }
    }
}

// (the callers have checked the pointers and that the sizes are positive)
template <bool BF16>
int launch(const void* dz, const float* w, float* dx, int B, int H, int W, int cout, int ld, hipStream_t st) {
    Args a;
    a.dz = dz; a.w = w; a.dx = dx; a.H = H; a.W = W; a.cout = cout; a.ld = ld;
    a.tiles_x = (W + TW - 1) / TW; a.tiles_y = (H + TH - 1) / TH;
    const long long n = (long long)B * a.tiles_x * a.tiles_y;
    if (n > 0x7fffffffLL - 65536) return YV3_ESHAPE;                   // (tile indices are ints, one grid stride past the end included)
    a.n_tiles = (int)n;
    const long long slots = 2LL * yv3_num_cu();                        // two workgroups per CU (registers, 50 KiB of LDS each)
    for (a.c0 = 0; a.c0 < cout; a.c0 += CC) {
        hipLaunchKernelGGL(conv0_dgrad<BF16>, dim3((unsigned)(n < slots ? n : slots)), dim3(NT), 0, st, a);
        YV3_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace conv0dg
