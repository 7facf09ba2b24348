// Training step of YoloNet (reference train.py: loss = net(inp, labels); loss.backward()): the train-mode BatchNorm forward, the
// BN + LeakyReLU backward, and convolution forward / dgrad / wgrad in exact fp32 on v_mfma_f32_32x32x2_f32.
//
// One implicit-GEMM kernel serves the three convolution products (conv_gemm below); they differ only in how the two operands and the
// result are addressed:
//   FWD   z[p][co]       = sum_{tap,ci} x(p, tap, ci) * w[co][ci][tap]         M = B*Ho*Wo, N = cout, K = k*k*cin
//   DGRAD dx[q][ci]      = sum_{tap,co} dz(q, tap, co) * w[co][ci][tap]        M = B*H*W,   N = cin,  K = k*k*cout
//   WGRAD dw[co][tap,ci] = sum_p dz[p][co] * x(p, tap, ci)                      M = cout,    N = k*k*cin, K = B*Ho*Wo (split)
// x(p, tap, ci) is the input gathered at output pixel p and filter tap (zero outside the image); the input is NHWC, or NCHW for
// the first layer, or -- for the convs after an upsample -- the concatenation [up2x(x2), x] read in place.
//
// Determinism: no atomics.  Every sum runs in a fixed order (the MFMA k-chain, then the wgrad split partials and the per-channel
// partials summed in index order in fp64), so identical inputs give identical bits.
// These are net.backprop_math = F32's entry points (yolo_v3_amd/backprop.py's table MATH names each mode's).  train_conv.h holds
// what the conv entry points share with train_bf16.hip's, train_channel.h the finalize kernels shared with train_bf16_act.hip.
#include "yv3_common.h"
#include "train_conv0_dgrad.h"
#include "train_channel.h"
#include "train_conv.h"

namespace {

constexpr int BM = 64, BN = 64, BK = 32;   // (NT = 256 threads: train_conv.h)

struct Geo {
    const float* x;    // input (tail of the concatenation when cin_up > 0)
    const float* x2;   // cin_up > 0: low-resolution NHWC [B][H/2][W/2][cin_up], channels [0, cin_up) of the concatenation
    const float* dz;   // DGRAD / WGRAD: NHWC [B][Ho][Wo][cout]
    const float* wp;   // FWD: [k*k*cin][cout]; DGRAD: [k*k*cout][cin]
    const float* bias; // FWD: optional [cout]
    float* out;        // FWD z, DGRAD dx (NHWC), WGRAD partials [split][cout][k*k*cin]
    int B, H, W, cin, cin_up, cout, k, stride, pad, Ho, Wo, nchw, accumulate;
    long long M, N, K, kchunk;
};

// element of the (possibly concatenated / NCHW) input at image n, row ih, column iw, channel ci; 0 outside the image
__device__ __forceinline__ float load_x(const Geo& g, int n, int ih, int iw, int ci) {
    if (ih < 0 || iw < 0 || ih >= g.H || iw >= g.W) return 0.f;
    if (g.nchw) return g.x[(((long long)n * g.cin + ci) * g.H + ih) * g.W + iw];
    if (ci < g.cin_up)
        return g.x2[(((long long)n * (g.H >> 1) + (ih >> 1)) * (g.W >> 1) + (iw >> 1)) * g.cin_up + ci];
    const int ct = g.cin - g.cin_up;
    return g.x[(((long long)n * g.H + ih) * g.W + iw) * ct + (ci - g.cin_up)];
}

// dz at input pixel (n, ih, iw) through filter tap (kh, kw): the output pixel that read it, or 0
__device__ __forceinline__ float load_dz(const Geo& g, int n, int ih, int iw, int kh, int kw, int co) {
    int oh = ih + g.pad - kh, ow = iw + g.pad - kw;
    if (oh < 0 || ow < 0) return 0.f;
    if (g.stride == 2) {
        if ((oh | ow) & 1) return 0.f;
        oh >>= 1; ow >>= 1;
    }
    if (oh >= g.Ho || ow >= g.Wo) return 0.f;
    return g.dz[(((long long)n * g.Ho + oh) * g.Wo + ow) * g.cout + co];
}

// one 64x64 tile of C = A * B per workgroup (4 waves, each one 32x32 MFMA accumulator); WGRAD: blockIdx.z is the K split
template <int MODE>
__global__ __launch_bounds__(NT) void conv_gemm(Geo g) {
    __shared__ float As[BK][BM + 4];
    __shared__ float Bs[BK][BN + 4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const long long m0 = (long long)blockIdx.x * BM, n0 = (long long)blockIdx.y * BN;
    long long k_lo = 0, k_hi = g.K;
    if (MODE == WGRAD) {
        k_lo = (long long)blockIdx.z * g.kchunk;
        k_hi = k_lo + g.kchunk < g.K ? k_lo + g.kchunk : g.K;
    }
    const int kk2 = g.k * g.k;
    // A loader: FWD / DGRAD read 8 consecutive k of one row m (channels are contiguous), WGRAD 8 consecutive m of one k
    // B loader: 8 consecutive n of one k
    const int a_m = (MODE == WGRAD) ? (t & 7) * 8 : t >> 2, a_k = (MODE == WGRAD) ? t >> 3 : (t & 3) * 8;
    const int b_k = t >> 3, b_n = (t & 7) * 8;
    // pixel of this thread's A row (FWD / DGRAD)
    int pn = 0, ph = 0, pw = 0;
    bool a_row_ok = false;
    if (MODE != WGRAD) {
        const long long m = m0 + a_m;
        a_row_ok = m < g.M;
        const int HH = MODE == FWD ? g.Ho : g.H, WW = MODE == FWD ? g.Wo : g.W;
        if (a_row_ok) {
            pn = (int)(m / ((long long)HH * WW));
            const int r = (int)(m - (long long)pn * HH * WW);
            ph = r / WW; pw = r - ph * WW;
        }
    }
    f32x16 acc;
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;

    for (long long k0 = k_lo; k0 < k_hi; k0 += BK) {
        float av[8], bv[8];
        if (MODE == WGRAD) {
            // A(m = co, k = p) = dz[p][co]
            const long long p = k0 + a_k;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const long long m = m0 + a_m + j;
                av[j] = (p < k_hi && m < g.M) ? g.dz[p * g.cout + m] : 0.f;
            }
            // B(k = p, n = tap*cin + ci) = x(p, tap, ci)
            const long long pb = k0 + b_k;
            const long long nb = n0 + b_n;
            if (pb < k_hi && nb < g.N) {
                const int n_img = (int)(pb / ((long long)g.Ho * g.Wo));
                const int r = (int)(pb - (long long)n_img * g.Ho * g.Wo);
                const int oh = r / g.Wo, ow = r - (r / g.Wo) * g.Wo;
                int tap = (int)(nb / g.cin), ci = (int)(nb - (long long)tap * g.cin);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float v = 0.f;
                    if (nb + j < g.N) {
                        const int kh = tap / g.k, kw = tap - kh * g.k;
                        v = load_x(g, n_img, oh * g.stride - g.pad + kh, ow * g.stride - g.pad + kw, ci);
                    }
                    bv[j] = v;
                    if (++ci == g.cin) { ci = 0; ++tap; }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) bv[j] = 0.f;
            }
        } else {
            const long long kb = k0 + a_k;
            const int cred = MODE == FWD ? g.cin : g.cout;        // channels per tap along K
            int tap = (int)(kb / cred), c = (int)(kb - (long long)tap * cred);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float v = 0.f;
                if (a_row_ok && kb + j < k_hi && tap < kk2) {
                    const int kh = tap / g.k, kw = tap - kh * g.k;
                    v = MODE == FWD ? load_x(g, pn, ph * g.stride - g.pad + kh, pw * g.stride - g.pad + kw, c)
                                    : load_dz(g, pn, ph, pw, kh, kw, c);
                }
                av[j] = v;
                if (++c == cred) { c = 0; ++tap; }
            }
            const long long kbb = k0 + b_k;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const long long n = n0 + b_n + j;
                bv[j] = (kbb < k_hi && n < g.N) ? g.wp[kbb * g.N + n] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (MODE == WGRAD) As[a_k][a_m + j] = av[j];
            else As[a_k + j][a_m] = av[j];
            Bs[b_k][b_n + j] = bv[j];
        }
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < BK; kb += 2) {
            const float a = As[kb + (lane >> 5)][wm * 32 + (lane & 31)];
            const float b = Bs[kb + (lane >> 5)][wn * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
    // C/D map of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const long long n = n0 + wn * 32 + (lane & 31);
    if (n >= g.N) return;
    float* out = g.out + (MODE == WGRAD ? (long long)blockIdx.z * g.M * g.N : 0);
    const float bias = (MODE == FWD && g.bias) ? g.bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < g.M) {
            float v = acc[r];
            if (MODE == FWD) v += bias;
            if (MODE == DGRAD && g.accumulate) v += out[m * g.N + n];
            out[m * g.N + n] = v;
        }
    }
}

__global__ void pack_weight(const float* __restrict__ w, float* __restrict__ wf, float* __restrict__ wd, int cout, int cin, int kk2) {
    const long long n = (long long)cout * cin * kk2;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    YV3_WEIGHT_INDEX(i, cin, kk2);
    const float v = w[i];
    if (wf) wf[((long long)tap * cin + ci) * cout + co] = v;
    if (wd) wd[((long long)tap * cout + co) * cin + ci] = v;
}

// ---- per-channel reductions over the P rows of a [P][C] tensor: fp64 partials per (channel block, row chunk), summed in order
constexpr int RC = 64, RR = NT / RC;   // 64 channels x 4 row lanes per workgroup
enum { R_STATS = 0, R_BNBWD = 1, R_COLSUM = 2 };

struct Red {
    const float* z; const float* dy; const float* mean; const float* invstd; const float* gamma; const float* beta;
    long long P; int C; long long chunk; int split;
    double* part;     // [split][2][C]
};

template <int MODE>
__global__ __launch_bounds__(NT) void channel_partials(Red r) {
    __shared__ double s0[RR][RC], s1[RR][RC];
    const int cl = threadIdx.x % RC, rl = threadIdx.x / RC;
    const int c = blockIdx.x * RC + cl;
    const long long p_lo = (long long)blockIdx.y * r.chunk;
    const long long p_hi = p_lo + r.chunk < r.P ? p_lo + r.chunk : r.P;
    double a = 0.0, b = 0.0;
    if (c < r.C) {
        float mu = 0.f, is = 0.f, ga = 0.f, be = 0.f;
        if (MODE == R_BNBWD) { mu = r.mean[c]; is = r.invstd[c]; ga = r.gamma[c]; be = r.beta[c]; }
        for (long long p = p_lo + rl; p < p_hi; p += RR) {
            const float v = r.z[p * r.C + c];
            if (MODE == R_STATS) { a += (double)v; b += (double)v * (double)v; }
            else if (MODE == R_COLSUM) { a += (double)v; }
            else {
                const float xh = (v - mu) * is;
                const float du = leaky_grad(ga * xh + be, r.dy[p * r.C + c]);
                a += (double)du; b += (double)du * (double)xh;
            }
        }
    }
    s0[rl][cl] = a; s1[rl][cl] = b;
    __syncthreads();
    if (rl == 0 && c < r.C) {
        for (int j = 1; j < RR; ++j) { a += s0[j][cl]; b += s1[j][cl]; }
        r.part[((long long)blockIdx.y * 2 + 0) * r.C + c] = a;
        r.part[((long long)blockIdx.y * 2 + 1) * r.C + c] = b;
    }
}

__global__ void eval_stats(const float* run_mean, const float* run_var, float eps, float* mean, float* invstd, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    mean[c] = run_mean[c];
    invstd[c] = (float)(1.0 / sqrt((double)run_var[c] + (double)eps));
}

// y = leaky(gamma (z - mean) invstd + beta) [+ residual]     (reference darknet.py:41-44, 53)
__global__ void bn_act_fwd(const float* __restrict__ z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                           const float* __restrict__ res, float* __restrict__ y, long long n, int C) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const float u = gamma[c] * ((z[i] - mean[c]) * invstd[c]) + beta[c];
        float v = u > 0.f ? u : u * 0.1f;
        if (res) v += res[i];
        y[i] = v;
    }
}

// dz = gamma invstd (du - dbeta / P - xhat dgamma / P)   (train; eval: the last two terms are 0)
__global__ void bn_act_bwd_dz(const float* __restrict__ z, const float* __restrict__ dy, const float* mean, const float* invstd,
                              const float* gamma, const float* beta, const float* coef, float* __restrict__ dz, long long n, int C) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const float xh = (z[i] - mean[c]) * invstd[c];
        const float du = leaky_grad(gamma[c] * xh + beta[c], dy[i]);
        dz[i] = coef[c] * ((du - coef[C + c]) - xh * coef[2 * C + c]);
    }
}

__global__ void scale_copy(const float* __restrict__ src, const float* scale, float* __restrict__ dst, long long n) {
    const float s = scale ? *scale : 1.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dst[i] = src[i] * s;
}

__global__ void add_into(const float* __restrict__ src, float* __restrict__ dst, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dst[i] += src[i];
}

// d[up2x(low), tail] -> d low (the 2x2 sum, in raster order) and d tail
__global__ void upcat_bwd(const float* __restrict__ dcat, float* __restrict__ dlow, float* __restrict__ dtail,
                          int B, int H, int W, int cu, int ct, int acc_low, int acc_tail) {
    const int C = cu + ct;
    const long long nlow = (long long)B * (H / 2) * (W / 2) * cu, ntail = (long long)B * H * W * ct;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nlow + ntail; i += (long long)gridDim.x * blockDim.x) {
        if (i < nlow) {
            if (!dlow) continue;
            const int c = (int)(i % cu);
            long long q = i / cu;
            const int x = (int)(q % (W / 2)); q /= (W / 2);
            const int y = (int)(q % (H / 2));
            const int n = (int)(q / (H / 2));
            float s = 0.f;
            for (int dy = 0; dy < 2; ++dy)
                for (int dx = 0; dx < 2; ++dx)
                    s += dcat[(((long long)n * H + 2 * y + dy) * W + 2 * x + dx) * C + c];
            dlow[i] = acc_low ? dlow[i] + s : s;
        } else {
            if (!dtail) continue;
            const long long j = i - nlow;
            const int c = (int)(j % ct);
            const float v = dcat[(j / ct) * C + cu + c];
            dtail[j] = acc_tail ? dtail[j] + v : v;
        }
    }
}

// ---- host side
// the wgrad split over output pixels: a function of the shape only, so that the summation order never changes
void wgrad_split(long long M, long long N, long long K, int* split, long long* chunk) {
    const long long tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    long long s = 2048 / tiles;
    if (s < 1) s = 1;
    const long long smax = (K + 255) / 256;
    if (s > smax) s = smax;
    long long c = (K + s - 1) / s;
    c = (c + BK - 1) / BK * BK;
    *chunk = c;
    *split = (int)((K + c - 1) / c);
}

long long red_split(long long P, int C, long long* chunk) {
    const long long cb = (C + RC - 1) / RC;
    long long s = 1024 / cb;
    if (s < 1) s = 1;
    const long long smax = (P + 63) / 64;
    if (s > smax) s = smax;
    long long c = (P + s - 1) / s;
    *chunk = c;
    return (P + c - 1) / c;
}

int launch_red(int mode, Red r, hipStream_t st) {
    dim3 grid((r.C + RC - 1) / RC, r.split);
    if (mode == R_STATS) hipLaunchKernelGGL(channel_partials<R_STATS>, grid, dim3(NT), 0, st, r);
    else if (mode == R_BNBWD) hipLaunchKernelGGL(channel_partials<R_BNBWD>, grid, dim3(NT), 0, st, r);
    else hipLaunchKernelGGL(channel_partials<R_COLSUM>, grid, dim3(NT), 0, st, r);
    YV3_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" {

int yv3_train_pack_weight(const float* w, float* wf, float* wd, int cout, int cin, int k, void* stream) {
    if (!w || (!wf && !wd)) return YV3_EINVAL;
    if (cout <= 0 || cin <= 0) return YV3_EINVAL;
    if (!(k == 1 || k == 3)) return YV3_ESHAPE;
    const long long n = (long long)cout * cin * k * k;
    hipLaunchKernelGGL(pack_weight, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, w, wf, wd, cout, cin, k * k);
    YV3_CHECK_LAUNCH();
    return 0;
}

int yv3_train_conv_fwd(const float* x, const float* x2, const float* wf, const float* bias, float* z,
                       int B, int H, int W, int cin, int cin_up, int cout, int k, int stride, int x_nchw, void* stream) {
    if (int rc = conv_check(x && wf && z && (cin_up <= 0 || x2), B, H, W, cin, cin_up, cout, k, stride, x_nchw)) return rc;
    Geo g = make_geo<Geo>(B, H, W, cin, cin_up, cout, k, stride, x_nchw);
    g.x = x; g.x2 = x2; g.wp = wf; g.bias = bias; g.out = z;
    g.M = (long long)B * g.Ho * g.Wo; g.N = cout; g.K = (long long)k * k * cin;
    dim3 grid((unsigned)((g.M + BM - 1) / BM), (unsigned)((g.N + BN - 1) / BN));
    hipLaunchKernelGGL(conv_gemm<FWD>, grid, dim3(NT), 0, (hipStream_t)stream, g);
    YV3_CHECK_LAUNCH();
    return 0;
}

int yv3_train_conv_dgrad(const float* dz, const float* wd, float* dx, int B, int H, int W, int cin, int cout, int k, int stride,
                         int accumulate, void* stream) {
    if (int rc = conv_check(dz && wd && dx, B, H, W, cin, 0, cout, k, stride, 0)) return rc;
    Geo g = make_geo<Geo>(B, H, W, cin, 0, cout, k, stride, 0);
    g.dz = dz; g.wp = wd; g.out = dx; g.accumulate = accumulate;
    g.M = (long long)B * H * W; g.N = cin; g.K = (long long)k * k * cout;
    dim3 grid((unsigned)((g.M + BM - 1) / BM), (unsigned)((g.N + BN - 1) / BN));
    hipLaunchKernelGGL(conv_gemm<DGRAD>, grid, dim3(NT), 0, (hipStream_t)stream, g);
    YV3_CHECK_LAUNCH();
    return 0;
}

int yv3_train_conv0_dgrad(const float* dz, const float* w, float* dx_nchw, int B, int H, int W, int cout, void* stream) {
    if (!dz || !w || !dx_nchw || B <= 0 || H <= 0 || W <= 0 || cout <= 0) return YV3_EINVAL;
    if (cout & 3) return YV3_ESHAPE;                                   // (16-byte loads of dz)
    return conv0dg::launch<false>(dz, w, dx_nchw, B, H, W, cout, cout, (hipStream_t)stream);
}

size_t yv3_train_conv_wgrad_workspace_bytes(int B, int H, int W, int cin, int cout, int k, int stride) {
    return wgrad_workspace_bytes(wgrad_split, B, H, W, cin, cout, k, stride);
}

int yv3_train_conv_wgrad(const float* x, const float* x2, const float* dz, float* dw, int B, int H, int W, int cin, int cin_up,
                         int cout, int k, int stride, int x_nchw, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = conv_check(x && dz && dw && ws && (cin_up <= 0 || x2), B, H, W, cin, cin_up, cout, k, stride, x_nchw)) return rc;
    if (ws_bytes < yv3_train_conv_wgrad_workspace_bytes(B, H, W, cin, cout, k, stride)) return YV3_EWORKSPACE;
    Geo g = make_geo<Geo>(B, H, W, cin, cin_up, cout, k, stride, x_nchw);
    g.x = x; g.x2 = x2; g.dz = dz; g.out = (float*)ws;
    g.M = cout; g.N = (long long)k * k * cin; g.K = (long long)B * g.Ho * g.Wo;
    int split;
    wgrad_split(g.M, g.N, g.K, &split, &g.kchunk);
    dim3 grid((unsigned)((g.M + BM - 1) / BM), (unsigned)((g.N + BN - 1) / BN), (unsigned)split);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(conv_gemm<WGRAD>, grid, dim3(NT), 0, st, g);
    YV3_CHECK_LAUNCH();
    const long long n = g.M * g.N;
    hipLaunchKernelGGL(wgrad_reduce, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, (const float*)ws, dw, cout, cin, k * k, split);
    YV3_CHECK_LAUNCH();
    return 0;
}

size_t yv3_train_channel_workspace_bytes(long long P, int C) {
    if (P <= 0 || C <= 0) return 0;
    long long chunk;
    const long long split = red_split(P, C, &chunk);
    return (size_t)split * 2 * C * sizeof(double) + (size_t)3 * C * sizeof(float);
}

int yv3_train_bn_stats(const float* z, long long P, int C, float eps, float momentum, const float* run_mean, const float* run_var,
                       float* run_mean_out, float* run_var_out, float* mean, float* invstd, void* ws, size_t ws_bytes, void* stream) {
    if (!z || !mean || !invstd || !ws || P <= 0 || C <= 0) return YV3_EINVAL;
    if ((run_mean_out != nullptr) != (run_var_out != nullptr)) return YV3_EINVAL;
    if (run_mean_out && (!run_mean || !run_var)) return YV3_EINVAL;
    if (ws_bytes < yv3_train_channel_workspace_bytes(P, C)) return YV3_EWORKSPACE;
    Red r = {};
    r.z = z; r.P = P; r.C = C; r.split = (int)red_split(P, C, &r.chunk); r.part = (double*)ws;
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_red(R_STATS, r, st);
    if (rc) return rc;
    hipLaunchKernelGGL(stats_finalize, dim3((C + NT - 1) / NT), dim3(NT), 0, st, (const double*)ws, r.split, C, P, eps, momentum,
                       run_mean, run_var, run_mean_out, run_var_out, mean, invstd);
    YV3_CHECK_LAUNCH();
    return 0;
}

int yv3_train_bn_eval_stats(const float* run_mean, const float* run_var, float eps, float* mean, float* invstd, int C, void* stream) {
    if (!run_mean || !run_var || !mean || !invstd || C <= 0) return YV3_EINVAL;
    hipLaunchKernelGGL(eval_stats, dim3((C + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, run_mean, run_var, eps, mean, invstd, C);
    YV3_CHECK_LAUNCH();
    return 0;
}

int yv3_train_bn_act_fwd(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                         const float* residual, float* y, long long P, int C, void* stream) {
    if (!z || !mean || !invstd || !gamma || !beta || !y || P <= 0 || C <= 0) return YV3_EINVAL;
    const long long n = P * C;
    hipLaunchKernelGGL(bn_act_fwd, dim3(grid1(n)), dim3(NT), 0, (hipStream_t)stream, z, mean, invstd, gamma, beta, residual, y, n, C);
    YV3_CHECK_LAUNCH();
    return 0;
}

int yv3_train_bn_act_bwd(const float* z, const float* dy, const float* mean, const float* invstd, const float* gamma, const float* beta,
                         float* dz, float* dgamma, float* dbeta, long long P, int C, int train, void* ws, size_t ws_bytes, void* stream) {
    if (!z || !dy || !mean || !invstd || !gamma || !beta || !dz || !dgamma || !dbeta || !ws || P <= 0 || C <= 0) return YV3_EINVAL;
    if (ws_bytes < yv3_train_channel_workspace_bytes(P, C)) return YV3_EWORKSPACE;
    Red r = {};
    r.z = z; r.dy = dy; r.mean = mean; r.invstd = invstd; r.gamma = gamma; r.beta = beta;
    r.P = P; r.C = C; r.split = (int)red_split(P, C, &r.chunk); r.part = (double*)ws;
    float* coef = (float*)((char*)ws + (size_t)r.split * 2 * C * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    int rc = launch_red(R_BNBWD, r, st);
    if (rc) return rc;
    hipLaunchKernelGGL(bnbwd_finalize, dim3((C + NT - 1) / NT), dim3(NT), 0, st, (const double*)ws, r.split, C, P, train, gamma, invstd,
                       dgamma, dbeta, coef);
    YV3_CHECK_LAUNCH();
    const long long n = P * C;
    hipLaunchKernelGGL(bn_act_bwd_dz, dim3(grid1(n)), dim3(NT), 0, st, z, dy, mean, invstd, gamma, beta, (const float*)coef, dz, n, C);
    YV3_CHECK_LAUNCH();
    return 0;
}

int yv3_train_bias_bwd(const float* dlogits, const float* scale, float* dout, float* dbias, long long P, int C, void* ws, size_t ws_bytes,
                       void* stream) {
    if (!dlogits || !dout || !dbias || !ws || P <= 0 || C <= 0) return YV3_EINVAL;
    if (ws_bytes < yv3_train_channel_workspace_bytes(P, C)) return YV3_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long long n = P * C;
    hipLaunchKernelGGL(scale_copy, dim3(grid1(n)), dim3(NT), 0, st, dlogits, scale, dout, n);
    YV3_CHECK_LAUNCH();
    Red r = {};
    r.z = dout; r.P = P; r.C = C; r.split = (int)red_split(P, C, &r.chunk); r.part = (double*)ws;
    int rc = launch_red(R_COLSUM, r, st);
    if (rc) return rc;
    hipLaunchKernelGGL(colsum_finalize, dim3((C + NT - 1) / NT), dim3(NT), 0, st, (const double*)ws, r.split, C, dbias);
    YV3_CHECK_LAUNCH();
    return 0;
}

int yv3_train_add(const float* src, float* dst, long long n, void* stream) {
    if (!src || !dst || n <= 0) return YV3_EINVAL;
    hipLaunchKernelGGL(add_into, dim3(grid1(n)), dim3(NT), 0, (hipStream_t)stream, src, dst, n);
    YV3_CHECK_LAUNCH();
    return 0;
}

int yv3_train_upcat_bwd(const float* dcat, float* dlow, float* dtail, int B, int H, int W, int cin_up, int ctail,
                        int acc_low, int acc_tail, void* stream) {
    if (!dcat || (!dlow && !dtail) || B <= 0 || H <= 0 || W <= 0 || cin_up <= 0 || ctail <= 0) return YV3_EINVAL;
    if ((H & 1) || (W & 1)) return YV3_ESHAPE;
    const long long n = (long long)B * (H / 2) * (W / 2) * cin_up + (long long)B * H * W * ctail;
    hipLaunchKernelGGL(upcat_bwd, dim3(grid1(n)), dim3(NT), 0, (hipStream_t)stream, dcat, dlow, dtail, B, H, W, cin_up, ctail,
                       acc_low, acc_tail);
    YV3_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
