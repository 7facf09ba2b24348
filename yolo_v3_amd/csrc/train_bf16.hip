// The convolutions of net.backprop_math = BF16 and BF16_ACT (yolo_v3_amd/backprop.py's table MATH names each mode's entry points): the
// forward / dgrad / wgrad of csrc/train.hip with both operands rounded to bf16 (round to nearest even) and the products accumulated in
// fp32 on v_mfma_f32_32x32x16_bf16.  The rest of the step stays on the fp32 kernels of train.hip (BF16) or runs on train_bf16_act.hip's
// (BF16_ACT).  train_conv.h holds what the entry points share with train.hip's; the kernels, GeoB and the split rule are this file's.
//
// The three products are those of train.hip's conv_gemm:
//   FWD   z[p][co]       = sum_{tap,ci} x(p, tap, ci) * w[co][ci][tap]         M = B*Ho*Wo, N = cout, K = k*k*cin
//   DGRAD dx[q][ci]      = sum_{tap,co} dz(q, tap, co) * w[co][ci][tap]        M = B*H*W,   N = cin,  K = k*k*coutp
//   WGRAD dw[co][tap,ci] = sum_p dz[p][co] * x(p, tap, ci)                      M = cout,    N = k*k*cin, K = B*Ho*Wo (split)
// Operands (all bf16 bits):
//   x     NHWC [B][H][W][cin] (layer 0: the caller's NCHW image), or cat(up2x(x2), x) read in place when cin_up > 0;
//   dz    NHWC [B][Ho][Wo][coutp], coutp = cout rounded up to a multiple of 8 (the heads' 255 -> 256), padding channels zero;
//   wf    [coutp][k*k*cin]  (row n = output channel, K index tap*cin + ci; rows >= cout zero)      -- yv3_train_pack_weight_bf16
//   wd    [cin][k*k*coutp]  (row n = input channel, K index tap*coutp + co; columns co >= cout zero)
// so that both operands of FWD and DGRAD run along K in groups of 8 consecutive channels of one pixel and tap: one 16-byte load each
// (every layer but the first has cin % 8 == 0; the first, K = 27 over an NCHW image, takes the scalar gather path VEC = false).
//
// Kernel (conv_bf16): 256 threads = 4 waves, each wave a 64x64 block of the C tile (2x2 MFMA 32x32x16 accumulators); the waves are
// arranged 2x2 (128x128 tile), 4x1 (256x64, for N <= 64) or 1x4 (64x256, for M <= 64) so that the narrow layers (cout = 32 / 64 at
// the full resolution) do not run three quarters empty.  K step 32.  The LDS holds both operands row-major with K contiguous
// ([row][32 + 8] bf16: an 80-byte row stride makes the ds_read_b128 fragment reads of 16 consecutive rows conflict-free), so an A or B
// fragment is one 16-byte read.  The next K step's global loads are issued before the MFMAs of the current one (one LDS buffer,
// register staging).  WGRAD runs K over pixels while both operands are contiguous in M / N (channels), so its loads (8 channels of
// one pixel, 16 bytes) are transposed in the register-to-LDS write (8 2-byte LDS writes).
// Measured (tools/train_bench.py --math f32 bf16, 416x416, bs=16): conv fwd 238, dgrad 148, wgrad 149 TFLOP/s -- against 32 / 24 / 32
// on train.hip's 64x64 fp32 tile; the BF16 step is 0.32x the F32 step, and BatchNorm / activation is now its largest class (DESIGN.md
// section 8d.1).  The tile arrangement above is the first design, not the result of a sweep.
//
// Determinism: no atomics.  The MFMA k-chain runs in a fixed order, and the wgrad split partials are summed in split order in fp64.
#include "yv3_common.h"
#include "train_conv0_dgrad.h"
#include "train_bf16_round.h"
#include "train_conv.h"

namespace {

constexpr int TK = 32, LDK = TK + 8;   // (NT = 256 threads: train_conv.h)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct GeoB {
    const u16* x;     // input (tail of the concatenation when cin_up > 0)
    const u16* x2;    // cin_up > 0: [B][H/2][W/2][cin_up]
    const u16* dz;    // DGRAD / WGRAD: [B][Ho][Wo][coutp]
    const u16* wp;    // FWD: wf [coutp][K]; DGRAD: wd [cin][K]
    const float* bias;
    float* out;       // FWD z [M][cout], DGRAD dx [M][cin], WGRAD partials [split][cout][k*k*cin]
    u16* out_b;       // FWD with a bf16 result (OUT_B16): zb [M][cout], out unused
    int B, H, W, cin, cin_up, cout, coutp, k, stride, pad, Ho, Wo, nchw, accumulate;
    long long M, N, K, kchunk;
};

__device__ __forceinline__ u16 load_x1(const GeoB& g, int n, int ih, int iw, int ci) {
    if (ih < 0 || iw < 0 || ih >= g.H || iw >= g.W) return 0;
    if (g.nchw) return g.x[(((long long)n * g.cin + ci) * g.H + ih) * g.W + iw];
    if (ci < g.cin_up) return g.x2[(((long long)n * (g.H >> 1) + (ih >> 1)) * (g.W >> 1) + (iw >> 1)) * g.cin_up + ci];
    return g.x[(((long long)n * g.H + ih) * g.W + iw) * (g.cin - g.cin_up) + (ci - g.cin_up)];
}

// 8 consecutive channels ci .. ci+7 (ci % 8 == 0, NHWC) of the input at (n, ih, iw); 0 outside the image
__device__ __forceinline__ u32x4 load_x8(const GeoB& g, int n, int ih, int iw, int ci) {
    if (ih < 0 || iw < 0 || ih >= g.H || iw >= g.W) return u32x4{0u, 0u, 0u, 0u};
    const u16* p;
    if (ci < g.cin_up) p = g.x2 + (((long long)n * (g.H >> 1) + (ih >> 1)) * (g.W >> 1) + (iw >> 1)) * g.cin_up + ci;
    else p = g.x + (((long long)n * g.H + ih) * g.W + iw) * (g.cin - g.cin_up) + (ci - g.cin_up);
    return *(const u32x4*)p;
}

// dz channels co .. co+7 at input pixel (n, ih, iw) through tap (kh, kw): the output pixel that read it, or 0
__device__ __forceinline__ u32x4 load_dz8(const GeoB& g, int n, int ih, int iw, int kh, int kw, int co) {
    int oh = ih + g.pad - kh, ow = iw + g.pad - kw;
    const u32x4 zero{0u, 0u, 0u, 0u};
    if (oh < 0 || ow < 0) return zero;
    if (g.stride == 2) {
        if ((oh | ow) & 1) return zero;
        oh >>= 1; ow >>= 1;
    }
    if (oh >= g.Ho || ow >= g.Wo) return zero;
    return *(const u32x4*)(g.dz + (((long long)n * g.Ho + oh) * g.Wo + ow) * g.coutp + co);
}

__device__ __forceinline__ u32x4 pack8(const u16* v) {
    return u32x4{v[0] | ((unsigned)v[1] << 16), v[2] | ((unsigned)v[3] << 16), v[4] | ((unsigned)v[5] << 16), v[6] | ((unsigned)v[7] << 16)};
}

// WAVES_M x WAVES_N waves, each a 64x64 block of the (64 WAVES_M) x (64 WAVES_N) C tile; WGRAD: blockIdx.z is the K split.
// OUT_B16 (FWD, N % 8 == 0, no bias): the same accumulators stored once as bf16 in g.out_b -- BF16_ACT's zb
template <int MODE, bool VEC, int WAVES_M, int WAVES_N, bool OUT_B16 = false>
__global__ __launch_bounds__(NT) void conv_bf16(GeoB g) {
    constexpr int TM = 64 * WAVES_M, TN = 64 * WAVES_N;
    constexpr int A_PER = TM * TK / 8 / NT, B_PER = TN * TK / 8 / NT;     // 16-byte chunks per thread and K step
    __shared__ __attribute__((aligned(16))) u16 As[TM][LDK];
    __shared__ __attribute__((aligned(16))) u16 Bs[TN][LDK];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const long long m0 = (long long)blockIdx.x * TM, n0 = (long long)blockIdx.y * TN;
    long long k_lo = 0, k_hi = g.K;
    if (MODE == WGRAD) {
        k_lo = (long long)blockIdx.z * g.kchunk;
        k_hi = k_lo + g.kchunk < g.K ? k_lo + g.kchunk : g.K;
    }
    const int kk2 = g.k * g.k;
    // FWD / DGRAD: chunk i of this thread is row (t >> 2) + 64 i, K quad t & 3.  WGRAD: K index t & 31, 8-channel group (t >> 5) + 8 i.
    const int kq = t & 3, wk = t & 31;
    int pn[A_PER], ph[A_PER], pw[A_PER];
    bool pok[A_PER];
    int w_tap[B_PER], w_ci[B_PER];
    if (MODE != WGRAD) {
        const int HH = MODE == FWD ? g.Ho : g.H, WW = MODE == FWD ? g.Wo : g.W;
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const long long m = m0 + (t >> 2) + 64 * i;
            pok[i] = m < g.M;
            pn[i] = ph[i] = pw[i] = 0;
            if (pok[i]) {
                pn[i] = (int)(m / ((long long)HH * WW));
                const int r = (int)(m - (long long)pn[i] * HH * WW);
                ph[i] = r / WW; pw[i] = r - ph[i] * WW;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const long long nb = n0 + 8 * ((t >> 5) + 8 * i);
            w_tap[i] = (int)(nb / g.cin);
            w_ci[i] = (int)(nb - (long long)w_tap[i] * g.cin);
        }
    }
    u32x4 ra[A_PER], rb[B_PER];

    auto load = [&](long long k0) {
        const u32x4 zero{0u, 0u, 0u, 0u};
        if (MODE == WGRAD) {
            const long long p = k0 + wk;
            const bool pin = p < k_hi;
            int n_img = 0, oh = 0, ow = 0;
            if (pin) {
                n_img = (int)(p / ((long long)g.Ho * g.Wo));
                const int r = (int)(p - (long long)n_img * g.Ho * g.Wo);
                oh = r / g.Wo; ow = r - oh * g.Wo;
            }
            // A(m = co, k = p) = dz[p][co]: 8 consecutive co (coutp % 8 == 0: a group lies wholly inside or outside the row)
#pragma unroll
            for (int i = 0; i < A_PER; ++i) {
                const long long m = m0 + 8 * ((t >> 5) + 8 * i);
                ra[i] = (pin && m < g.coutp) ? *(const u32x4*)(g.dz + p * g.coutp + m) : zero;
            }
            // B(k = p, n = tap*cin + ci) = x(p, tap, ci)
#pragma unroll
            for (int i = 0; i < B_PER; ++i) {
                const long long nb = n0 + 8 * ((t >> 5) + 8 * i);
                if (!pin || nb >= g.N) { rb[i] = zero; continue; }
                if (VEC) {
                    const int kh = w_tap[i] / g.k, kw = w_tap[i] - (w_tap[i] / g.k) * g.k;
                    rb[i] = load_x8(g, n_img, oh * g.stride - g.pad + kh, ow * g.stride - g.pad + kw, w_ci[i]);
                } else {
                    u16 v[8];
                    int tap = w_tap[i], ci = w_ci[i];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        v[j] = 0;
                        if (nb + j < g.N) {
                            const int kh = tap / g.k, kw = tap - kh * g.k;
                            v[j] = load_x1(g, n_img, oh * g.stride - g.pad + kh, ow * g.stride - g.pad + kw, ci);
                        }
                        if (++ci == g.cin) { ci = 0; ++tap; }
                    }
                    rb[i] = pack8(v);
                }
            }
        } else {
            const long long kb = k0 + 8 * kq;
            const int cred = MODE == FWD ? g.cin : g.coutp;           // channels per tap along K
            const int tap = (int)(kb / cred), c = (int)(kb - (long long)tap * cred);
            const int kh = tap / g.k, kw = tap - (tap / g.k) * g.k;
#pragma unroll
            for (int i = 0; i < A_PER; ++i) {
                if (VEC) {
                    ra[i] = zero;
                    if (pok[i] && kb < k_hi) {
                        ra[i] = MODE == FWD ? load_x8(g, pn[i], ph[i] * g.stride - g.pad + kh, pw[i] * g.stride - g.pad + kw, c)
                                            : load_dz8(g, pn[i], ph[i], pw[i], kh, kw, c);
                    }
                } else {                                                 // FWD of the NCHW first layer
                    u16 v[8];
                    int tp = tap, cc = c;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        v[j] = 0;
                        if (pok[i] && kb + j < k_hi && tp < kk2) {
                            const int h2 = tp / g.k, w2 = tp - h2 * g.k;
                            v[j] = load_x1(g, pn[i], ph[i] * g.stride - g.pad + h2, pw[i] * g.stride - g.pad + w2, cc);
                        }
                        if (++cc == cred) { cc = 0; ++tp; }
                    }
                    ra[i] = pack8(v);
                }
            }
#pragma unroll
            for (int i = 0; i < B_PER; ++i) {
                const long long n = n0 + (t >> 2) + 64 * i;
                if (VEC) {
                    rb[i] = (n < g.N && kb < k_hi) ? *(const u32x4*)(g.wp + n * g.K + kb) : zero;
                } else {
                    u16 v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = (n < g.N && kb + j < k_hi) ? g.wp[n * g.K + kb + j] : (u16)0;
                    rb[i] = pack8(v);
                }
            }
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    load(k_lo);
    for (long long k0 = k_lo; k0 < k_hi; k0 += TK) {
        __syncthreads();
        if (MODE == WGRAD) {
#pragma unroll
            for (int i = 0; i < A_PER; ++i) {
                const int row = 8 * ((t >> 5) + 8 * i);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    As[row + 2 * j][wk] = (u16)(ra[i][j] & 0xffffu);
                    As[row + 2 * j + 1][wk] = (u16)(ra[i][j] >> 16);
                }
            }
#pragma unroll
            for (int i = 0; i < B_PER; ++i) {
                const int row = 8 * ((t >> 5) + 8 * i);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    Bs[row + 2 * j][wk] = (u16)(rb[i][j] & 0xffffu);
                    Bs[row + 2 * j + 1][wk] = (u16)(rb[i][j] >> 16);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < A_PER; ++i) *(u32x4*)&As[(t >> 2) + 64 * i][8 * kq] = ra[i];
#pragma unroll
            for (int i = 0; i < B_PER; ++i) *(u32x4*)&Bs[(t >> 2) + 64 * i][8 * kq] = rb[i];
        }
        __syncthreads();
        if (k0 + TK < k_hi) load(k0 + TK);
#pragma unroll
        for (int kk = 0; kk < TK; kk += 16) {
            bf16x8 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = *(const bf16x8*)&As[wm * 64 + i * 32 + (lane & 31)][kk + 8 * (lane >> 5)];
                b[i] = *(const bf16x8*)&Bs[wn * 64 + i * 32 + (lane & 31)][kk + 8 * (lane >> 5)];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    // C/D map of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    if (OUT_B16) {
        // A lane holds one column, so the memory neighbour of its element sits in lane ^ 1.  The two lanes of a pair trade: the even
        // lane keeps the even rows r and gets its neighbour's, the odd lane the odd rows, and each stores both columns of its rows in
        // one 4-byte store (N % 8 == 0 and an even column: a pair lies wholly inside or outside the row).  Every lane takes part
        // in the exchange; only the store is guarded.
        const bool odd = lane & 1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long long n = n0 + wn * 64 + j * 32 + (lane & 30);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const unsigned own0 = rne_bf16(acc[i][j][r]), own1 = rne_bf16(acc[i][j][r + 1]);
                    const unsigned got = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(odd ? own0 : own1), 0xB1, 0xf, 0xf, true);  // quad_perm [1,0,3,2]
                    const unsigned v = odd ? (got | (own1 << 16)) : (own0 | (got << 16));
                    const int rr = r + (odd ? 1 : 0);
                    const long long m = m0 + wm * 64 + i * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * (lane >> 5);
                    if (m < g.M && n < g.N) *(unsigned*)(g.out_b + m * g.N + n) = v;
                }
        }
        return;
    }
    float* out = g.out + (MODE == WGRAD ? (long long)blockIdx.z * g.M * g.N : 0);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const long long n = n0 + wn * 64 + j * 32 + (lane & 31);
        if (n >= g.N) continue;
        const float bias = (MODE == FWD && g.bias) ? g.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m < g.M) {
                    float v = acc[i][j][r];
                    if (MODE == FWD) v += bias;
                    if (MODE == DGRAD && g.accumulate) v += out[m * g.N + n];
                    out[m * g.N + n] = v;
                }
            }
    }
}

// wf[n][tap*cin + ci] (n < coutp) and wd[ci][tap*coutp + co] (co < coutp), zero where the channel is padding
__global__ void pack_weight_bf16(const float* __restrict__ w, u16* __restrict__ wf, u16* __restrict__ wd, int cout, int coutp, int cin,
                                 int kk2) {
    const long long n = (long long)coutp * cin * kk2;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    YV3_WEIGHT_INDEX(i, cin, kk2);
    const u16 v = co < cout ? rne_bf16(w[i]) : (u16)0;
    if (wf) wf[(long long)co * cin * kk2 + (long long)tap * cin + ci] = v;
    if (wd) wd[(long long)ci * kk2 * coutp + (long long)tap * coutp + co] = v;
}

// dst[r][c] = bf16(src[r][c]) for c < C, 0 for C <= c < ld
__global__ void to_bf16(const float* __restrict__ src, u16* __restrict__ dst, long long rows, int C, int ld) {
    const long long n = rows * ld;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (ld == C) { dst[i] = rne_bf16(src[i]); continue; }
        const long long r = i / ld;
        const int c = (int)(i - r * ld);
        dst[i] = c < C ? rne_bf16(src[r * C + c]) : (u16)0;
    }
}

// ---- host side
int round8(int c) { return (c + 7) & ~7; }

// train_conv.h's geometry with the padded channel count of dz
GeoB make_geo(int B, int H, int W, int cin, int cin_up, int cout, int k, int stride, int nchw) {
    GeoB g = make_geo<GeoB>(B, H, W, cin, cin_up, cout, k, stride, nchw);
    g.coutp = round8(cout);
    return g;
}

// the 16-byte gathers need whole groups of 8 channels in an NHWC input
bool vec8_ok(int cin, int cin_up, int x_nchw) { return x_nchw || !((cin & 7) || (cin_up & 7)); }

// the tile arrangement (waves along M x along N): 1x4 when M is small, 4x1 when N is, else 2x2 -- a function of the shape only
void pick_tile(long long M, long long N, int* wm, int* wn) {
    if (N <= 64) { *wm = 4; *wn = 1; }
    else if (M <= 64) { *wm = 1; *wn = 4; }
    else { *wm = 2; *wn = 2; }
}

// the wgrad split over output pixels: a function of the shape only, so that the summation order never changes
void wgrad_split(long long M, long long N, long long K, int* split, long long* chunk) {
    int wm, wn;
    pick_tile(M, N, &wm, &wn);
    const long long tiles = ((M + 64 * wm - 1) / (64 * wm)) * ((N + 64 * wn - 1) / (64 * wn));
    long long s = 1024 / tiles;
    if (s < 1) s = 1;
    const long long smax = (K + 511) / 512;
    if (s > smax) s = smax;
    long long c = (K + s - 1) / s;
    c = (c + TK - 1) / TK * TK;
    *chunk = c;
    *split = (int)((K + c - 1) / c);
}

template <int MODE, bool VEC, bool OUT_B16 = false>
int launch_conv(const GeoB& g, int split, hipStream_t st) {
    int wm, wn;
    pick_tile(g.M, g.N, &wm, &wn);
    dim3 grid((unsigned)((g.M + 64 * wm - 1) / (64 * wm)), (unsigned)((g.N + 64 * wn - 1) / (64 * wn)), (unsigned)split);
    if (grid.x > 0x7fffffffu || grid.y > 65535u) return YV3_ESHAPE;
    if (wm == 4) hipLaunchKernelGGL((conv_bf16<MODE, VEC, 4, 1, OUT_B16>), grid, dim3(NT), 0, st, g);
    else if (wm == 1) hipLaunchKernelGGL((conv_bf16<MODE, VEC, 1, 4, OUT_B16>), grid, dim3(NT), 0, st, g);
    else hipLaunchKernelGGL((conv_bf16<MODE, VEC, 2, 2, OUT_B16>), grid, dim3(NT), 0, st, g);
    YV3_CHECK_LAUNCH();
    return 0;
}

// the forward into fp32 z [+ bias], or (OUT_B16: whole groups of 8 output channels, no bias) into bf16 zb
template <bool OUT_B16>
int conv_fwd(const void* x, const void* x2, const void* wf, const float* bias, void* z, int B, int H, int W, int cin, int cin_up, int cout,
             int k, int stride, int x_nchw, hipStream_t st) {
    if (int rc = conv_check(x && wf && z && (cin_up <= 0 || x2), B, H, W, cin, cin_up, cout, k, stride, x_nchw)) return rc;
    if ((OUT_B16 && (cout & 7)) || !vec8_ok(cin, cin_up, x_nchw)) return YV3_ESHAPE;
    GeoB g = make_geo(B, H, W, cin, cin_up, cout, k, stride, x_nchw);
    g.x = (const u16*)x; g.x2 = (const u16*)x2; g.wp = (const u16*)wf; g.bias = bias;
    g.out = OUT_B16 ? nullptr : (float*)z; g.out_b = OUT_B16 ? (u16*)z : nullptr;
    g.M = (long long)B * g.Ho * g.Wo; g.N = cout; g.K = (long long)k * k * cin;
    return x_nchw ? launch_conv<FWD, false, OUT_B16>(g, 1, st) : launch_conv<FWD, true, OUT_B16>(g, 1, st);
}

}  // namespace

extern "C" {

int yv3_train_to_bf16(const float* src, void* dst, long long rows, int C, int ld, void* stream) {
    if (!src || !dst || rows <= 0 || C <= 0 || ld < C) return YV3_EINVAL;
    hipLaunchKernelGGL(to_bf16, dim3(grid1(rows * ld)), dim3(NT), 0, (hipStream_t)stream, src, (u16*)dst, rows, C, ld);
    YV3_CHECK_LAUNCH();
    return 0;
}

int yv3_train_pack_weight_bf16(const float* w, void* wf, void* wd, int cout, int cin, int k, void* stream) {
    if (!w || (!wf && !wd)) return YV3_EINVAL;
    if (cout <= 0 || cin <= 0) return YV3_EINVAL;
    if (!(k == 1 || k == 3)) return YV3_ESHAPE;
    const long long n = (long long)round8(cout) * cin * k * k;
    hipLaunchKernelGGL(pack_weight_bf16, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, w, (u16*)wf, (u16*)wd,
                       cout, round8(cout), cin, k * k);
    YV3_CHECK_LAUNCH();
    return 0;
}

int yv3_train_conv_fwd_bf16(const void* x, const void* x2, const void* wf, const float* bias, float* z,
                            int B, int H, int W, int cin, int cin_up, int cout, int k, int stride, int x_nchw, void* stream) {
    return conv_fwd<false>(x, x2, wf, bias, z, B, H, W, cin, cin_up, cout, k, stride, x_nchw, (hipStream_t)stream);
}

int yv3_train_conv_fwd_bf16o(const void* x, const void* x2, const void* wf, void* zb, int B, int H, int W, int cin, int cin_up, int cout,
                             int k, int stride, int x_nchw, void* stream) {
    return conv_fwd<true>(x, x2, wf, nullptr, zb, B, H, W, cin, cin_up, cout, k, stride, x_nchw, (hipStream_t)stream);
}

int yv3_train_conv_dgrad_bf16(const void* dz, const void* wd, float* dx, int B, int H, int W, int cin, int cout, int k, int stride,
                              int accumulate, void* stream) {
    if (int rc = conv_check(dz && wd && dx, B, H, W, cin, 0, cout, k, stride, 0)) return rc;
    GeoB g = make_geo(B, H, W, cin, 0, cout, k, stride, 0);
    g.dz = (const u16*)dz; g.wp = (const u16*)wd; g.out = dx; g.accumulate = accumulate;
    g.M = (long long)B * H * W; g.N = cin; g.K = (long long)k * k * g.coutp;
    return launch_conv<DGRAD, true>(g, 1, (hipStream_t)stream);
}

int yv3_train_conv0_dgrad_bf16(const void* dz, const float* w, float* dx_nchw, int B, int H, int W, int cout, void* stream) {
    if (!dz || !w || !dx_nchw || B <= 0 || H <= 0 || W <= 0 || cout <= 0) return YV3_EINVAL;
    return conv0dg::launch<true>(dz, w, dx_nchw, B, H, W, cout, round8(cout), (hipStream_t)stream);
}

size_t yv3_train_conv_wgrad_bf16_workspace_bytes(int B, int H, int W, int cin, int cout, int k, int stride) {
    return wgrad_workspace_bytes(wgrad_split, B, H, W, cin, cout, k, stride);
}

int yv3_train_conv_wgrad_bf16(const void* x, const void* x2, const void* dz, float* dw, int B, int H, int W, int cin, int cin_up,
                              int cout, int k, int stride, int x_nchw, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = conv_check(x && dz && dw && ws && (cin_up <= 0 || x2), B, H, W, cin, cin_up, cout, k, stride, x_nchw)) return rc;
    if (!vec8_ok(cin, cin_up, x_nchw)) return YV3_ESHAPE;
    if (ws_bytes < yv3_train_conv_wgrad_bf16_workspace_bytes(B, H, W, cin, cout, k, stride)) return YV3_EWORKSPACE;
    GeoB g = make_geo(B, H, W, cin, cin_up, cout, k, stride, x_nchw);
    g.x = (const u16*)x; g.x2 = (const u16*)x2; g.dz = (const u16*)dz; g.out = (float*)ws;
    g.M = cout; g.N = (long long)k * k * cin; g.K = (long long)B * g.Ho * g.Wo;
    int split;
    wgrad_split(g.M, g.N, g.K, &split, &g.kchunk);
    hipStream_t st = (hipStream_t)stream;
    const int rc = x_nchw ? launch_conv<WGRAD, false>(g, split, st) : launch_conv<WGRAD, true>(g, split, st);
    if (rc) return rc;
    const long long n = g.M * g.N;
    hipLaunchKernelGGL(wgrad_reduce, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, (const float*)ws, dw, cout, cin, k * k,
                       split);
    YV3_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
