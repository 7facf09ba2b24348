// The per-channel kernels of net.backprop_math = BF16_ACT (yolo_v3_amd/backprop.py's table MATH names each mode's entry points): the
// BatchNorm / activation / bias kernels of train.hip on activations that exist in bf16 only.  The conv forward (train_bf16.hip,
// OUT_B16) stores zb = bf16(z32); here
//   bn_stats_bf16     reads zb                       -> mean, invstd, running statistics (fp32, fp64 sums)
//   bn_act_fwd_bf16   reads zb [, bf16 res]          -> y = bf16(leaky(bn(zb)) [+ res])
//   bn_act_bwd_bf16   reads zb, fp32 dy              -> dgamma, dbeta (fp32), dz = bf16(...)
//   bias_bwd_bf16     reads fp32 dy (C = 255)        -> dbias (fp32), dz = bf16(dy * scale) in rows of round8(C), padding zero
// The arithmetic per element is that of train.hip's kernels, in fp32, in the same order; a value is rounded once, where it is stored
// (rne_bf16: nearest even, NaN -> 0x7fc0, subnormals kept).
//
// These are bandwidth kernels.  A [P][C] bf16 tensor with C % 8 == 0 is a row of G = C / 8 groups of 16 bytes, and a thread owns one
// group (`gl` group lanes along the row, `nrl` row lanes, gl * nrl <= 256): it loads its 8 channels' constants once, then walks down
// the rows with one 16-byte load per bf16 operand (two for a fp32 one) and one 16-byte store.  For C <= 256 a workgroup's lanes cover
// whole rows, so its accesses are contiguous.  bias_bwd reads fp32 rows of 255 (4-byte aligned only): a thread owns two channels
// and stores them as one 4-byte pair.
//
// Determinism: no atomics.  A thread sums its rows in order in fp64, the row lanes of a workgroup are summed in lane order, and the
// row chunks in chunk order (train_channel.h) -- the split is a function of (P, C) only.
#include "yv3_common.h"
#include "train_bf16_round.h"
#include "train_channel.h"

namespace {

constexpr int NT = 256;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// how a workgroup's 256 threads lie over rows of `units` thread-sized pieces: gl along the row, nrl rows at a time, bx workgroups per row
struct Lay { int units, gl, nrl, bx; };

Lay make_lay(int units, int max_gl) {
    Lay l;
    l.units = units;
    l.gl = units < max_gl ? units : max_gl;
    l.nrl = NT / l.gl;
    l.bx = (units + l.gl - 1) / l.gl;
    return l;
}
Lay lay8(int C) { return make_lay(C / 8, 32); }              // 8 bf16 channels per thread
Lay lay2(int C) { return make_lay((C + 7) / 8 * 4, 128); }   // 2 channels per thread over round8(C)

// the row split of a reduction: about 1024 workgroups, at least 4 rows per thread.  The finalize kernels add the chunks serially per
// channel, so their time grows with the split: measured at bs=16 they take 19 of the step's 23 ms of BN / act
long long red_split(long long P, const Lay& l, long long* chunk) {
    long long s = 1024 / l.bx;
    if (s < 1) s = 1;
    const long long smax = (P + 4 * l.nrl - 1) / (4 * l.nrl);
    if (s > smax) s = smax;
    const long long c = (P + s - 1) / s;
    *chunk = c;
    return (P + c - 1) / c;
}

// row workgroups of an elementwise pass: about 4 rows per thread, at most about 2048 workgroups (the threads stride on)
int row_blocks(long long P, const Lay& l) {
    long long by = (P + 4 * l.nrl - 1) / (4 * l.nrl);
    const long long cap = 2048 / l.bx > 0 ? 2048 / l.bx : 1;
    return (int)(by < cap ? by : cap);
}

__device__ __forceinline__ void unpack8(const u32x4 v, float* f) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[2 * j] = __uint_as_float(v[j] << 16);
        f[2 * j + 1] = __uint_as_float(v[j] & 0xffff0000u);
    }
}

__device__ __forceinline__ u32x4 round8_pack(const float* f) {
    u32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (unsigned)rne_bf16(f[2 * j]) | ((unsigned)rne_bf16(f[2 * j + 1]) << 16);
    return v;
}

__device__ __forceinline__ void load8(const float* p, float* f) {
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[j] = a[j]; f[4 + j] = b[j]; }
}

// the sums a[U], b[U] of every thread (channels c0 + g_l U + j of row lane rl) -> part[chunk][2][C], row lanes added in lane order
// through the kernel's LDS arrays s0, s1 (NT * U doubles each: gl * nrl <= NT threads write U values)
template <int U>
__device__ __forceinline__ void reduce_rows(double* s0, double* s1, const double* a, const double* b, int gl, int nrl, int g_l, int rl,
                                            int c0, int C, double* part) {
    if (rl < nrl) {
#pragma unroll
        for (int j = 0; j < U; ++j) { s0[(rl * gl + g_l) * U + j] = a[j]; s1[(rl * gl + g_l) * U + j] = b[j]; }
    }
    __syncthreads();
    const int t = threadIdx.x, c = c0 + t;
    if (t < gl * U && c < C) {
        double x = 0.0, y = 0.0;
        for (int r = 0; r < nrl; ++r) { x += s0[r * gl * U + t]; y += s1[r * gl * U + t]; }
        part[c] = x;
        part[C + c] = y;
    }
}

struct RedB {
    const u16* z; const float* dy; const float* mean; const float* invstd; const float* gamma; const float* beta;
    long long P, chunk; int C, gl, nrl;
    double* part;     // [split][2][C]
};

// BWD = false: sum z, sum z^2.  BWD = true: sum du, sum du xhat (du = dy act'(u)).  blockIdx.y is the row chunk.
template <bool BWD>
__global__ __launch_bounds__(NT) void channel_partials_b(RedB r) {
    __shared__ double s0[NT * 8], s1[NT * 8];      // 32 KB: at most 5 workgroups per CU
    const int g_l = threadIdx.x % r.gl, rl = threadIdx.x / r.gl;
    const int c = (blockIdx.x * r.gl + g_l) * 8;
    const long long p_lo = (long long)blockIdx.y * r.chunk;
    const long long p_hi = p_lo + r.chunk < r.P ? p_lo + r.chunk : r.P;
    double a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = b[j] = 0.0;
    if (rl < r.nrl && c < r.C) {
        float mu[8], is[8], ga[8], be[8];
        if (BWD) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { mu[j] = r.mean[c + j]; is[j] = r.invstd[c + j]; ga[j] = r.gamma[c + j]; be[j] = r.beta[c + j]; }
        }
        for (long long p = p_lo + rl; p < p_hi; p += r.nrl) {
            float v[8], d[8];
            unpack8(*(const u32x4*)(r.z + p * r.C + c), v);
            if (BWD) load8(r.dy + p * r.C + c, d);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (!BWD) { a[j] += (double)v[j]; b[j] += (double)v[j] * (double)v[j]; }
                else {
                    const float xh = (v[j] - mu[j]) * is[j];
                    const float du = leaky_grad(ga[j] * xh + be[j], d[j]);
                    a[j] += (double)du; b[j] += (double)du * (double)xh;
                }
            }
        }
    }
    reduce_rows<8>(s0, s1, a, b, r.gl, r.nrl, g_l, rl, blockIdx.x * r.gl * 8, r.C, r.part + (long long)blockIdx.y * 2 * r.C);
}

// y = bf16(leaky(gamma (z - mean) invstd + beta) [+ res])
__global__ __launch_bounds__(NT) void bn_act_fwd_b(const u16* __restrict__ z, const float* mean, const float* invstd, const float* gamma,
                                                   const float* beta, const u16* __restrict__ res, u16* __restrict__ y, long long P, int C,
                                                   int gl, int nrl) {
    const int g_l = threadIdx.x % gl, rl = threadIdx.x / gl;
    const int c = (blockIdx.x * gl + g_l) * 8;
    if (rl >= nrl || c >= C) return;
    float mu[8], is[8], ga[8], be[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { mu[j] = mean[c + j]; is[j] = invstd[c + j]; ga[j] = gamma[c + j]; be[j] = beta[c + j]; }
    for (long long p = (long long)blockIdx.y * nrl + rl; p < P; p += (long long)gridDim.y * nrl) {
        float v[8], rs[8];
        unpack8(*(const u32x4*)(z + p * C + c), v);
        if (res) unpack8(*(const u32x4*)(res + p * C + c), rs);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float u = ga[j] * ((v[j] - mu[j]) * is[j]) + be[j];
            v[j] = u > 0.f ? u : u * 0.1f;
            if (res) v[j] += rs[j];
        }
        *(u32x4*)(y + p * C + c) = round8_pack(v);
    }
}

// dz = bf16(gamma invstd (du - dbeta / P - xhat dgamma / P)); coef as bnbwd_finalize leaves it
__global__ __launch_bounds__(NT) void bn_act_bwd_dz_b(const u16* __restrict__ z, const float* __restrict__ dy, const float* mean,
                                                      const float* invstd, const float* gamma, const float* beta, const float* coef,
                                                      u16* __restrict__ dz, long long P, int C, int gl, int nrl) {
    const int g_l = threadIdx.x % gl, rl = threadIdx.x / gl;
    const int c = (blockIdx.x * gl + g_l) * 8;
    if (rl >= nrl || c >= C) return;
    float mu[8], is[8], ga[8], be[8], k0[8], k1[8], k2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mu[j] = mean[c + j]; is[j] = invstd[c + j]; ga[j] = gamma[c + j]; be[j] = beta[c + j];
        k0[j] = coef[c + j]; k1[j] = coef[C + c + j]; k2[j] = coef[2 * C + c + j];
    }
    for (long long p = (long long)blockIdx.y * nrl + rl; p < P; p += (long long)gridDim.y * nrl) {
        float v[8], d[8];
        unpack8(*(const u32x4*)(z + p * C + c), v);
        load8(dy + p * C + c, d);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float xh = (v[j] - mu[j]) * is[j];
            const float du = leaky_grad(ga[j] * xh + be[j], d[j]);
            v[j] = k0[j] * ((du - k1[j]) - xh * k2[j]);
        }
        *(u32x4*)(dz + p * C + c) = round8_pack(v);
    }
}

// dz[p][c] = bf16(dy[p][c] * scale) for c < C, 0 for C <= c < ld; the fp32 products summed per channel.  blockIdx.y is the row chunk.
__global__ __launch_bounds__(NT) void bias_bwd_b(const float* __restrict__ dy, const float* scale, u16* __restrict__ dz, long long P, int C,
                                                 int ld, long long chunk, int gl, int nrl, double* part) {
    __shared__ double s0[NT * 2], s1[NT * 2];
    const int g_l = threadIdx.x % gl, rl = threadIdx.x / gl;
    const int c = (blockIdx.x * gl + g_l) * 2;
    const long long p_lo = (long long)blockIdx.y * chunk;
    const long long p_hi = p_lo + chunk < P ? p_lo + chunk : P;
    double a[2] = {0.0, 0.0}, b[2] = {0.0, 0.0};
    if (rl < nrl && c < ld) {
        const float s = scale ? *scale : 1.f;
        for (long long p = p_lo + rl; p < p_hi; p += nrl) {
            float v[2] = {0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (c + j < C) {
                    v[j] = dy[p * C + c + j];
                    if (scale) v[j] *= s;
                    a[j] += (double)v[j];
                }
            *(unsigned*)(dz + p * ld + c) = (unsigned)rne_bf16(v[0]) | ((unsigned)rne_bf16(v[1]) << 16);
        }
    }
    reduce_rows<2>(s0, s1, a, b, gl, nrl, g_l, rl, blockIdx.x * gl * 2, C, part + (long long)blockIdx.y * 2 * C);
}

size_t ws_bytes_for(long long split, int C) { return (size_t)split * 2 * C * sizeof(double) + (size_t)3 * C * sizeof(float); }

}  // namespace

extern "C" {

size_t yv3_train_channel_bf16_workspace_bytes(long long P, int C) {
    if (P <= 0 || C <= 0) return 0;
    long long chunk;
    long long split = red_split(P, lay2(C), &chunk);
    if (!(C & 7)) {
        const long long s8 = red_split(P, lay8(C), &chunk);
        if (s8 > split) split = s8;
    }
    return ws_bytes_for(split, C);
}

int yv3_train_bn_stats_bf16(const void* z, long long P, int C, float eps, float momentum, const float* run_mean, const float* run_var,
                            float* run_mean_out, float* run_var_out, float* mean, float* invstd, void* ws, size_t ws_bytes, void* stream) {
    if (!z || !mean || !invstd || !ws || P <= 0 || C <= 0) return YV3_EINVAL;
    if ((run_mean_out != nullptr) != (run_var_out != nullptr)) return YV3_EINVAL;
    if (run_mean_out && (!run_mean || !run_var)) return YV3_EINVAL;
    if (C & 7) return YV3_ESHAPE;
    if (ws_bytes < yv3_train_channel_bf16_workspace_bytes(P, C)) return YV3_EWORKSPACE;
    const Lay l = lay8(C);
    RedB r = {};
    r.z = (const u16*)z; r.P = P; r.C = C; r.gl = l.gl; r.nrl = l.nrl; r.part = (double*)ws;
    const int split = (int)red_split(P, l, &r.chunk);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(channel_partials_b<false>, dim3(l.bx, split), dim3(NT), 0, st, r);
    YV3_CHECK_LAUNCH();
    hipLaunchKernelGGL(stats_finalize, dim3((C + NT - 1) / NT), dim3(NT), 0, st, (const double*)ws, split, C, P, eps, momentum,
                       run_mean, run_var, run_mean_out, run_var_out, mean, invstd);
    YV3_CHECK_LAUNCH();
    return 0;
}

int yv3_train_bn_act_fwd_bf16(const void* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                              const void* residual, void* y, long long P, int C, void* stream) {
    if (!z || !mean || !invstd || !gamma || !beta || !y || P <= 0 || C <= 0) return YV3_EINVAL;
    if (C & 7) return YV3_ESHAPE;
    const Lay l = lay8(C);
    hipLaunchKernelGGL(bn_act_fwd_b, dim3(l.bx, row_blocks(P, l)), dim3(NT), 0, (hipStream_t)stream, (const u16*)z, mean, invstd, gamma,
                       beta, (const u16*)residual, (u16*)y, P, C, l.gl, l.nrl);
    YV3_CHECK_LAUNCH();
    return 0;
}

int yv3_train_bn_act_bwd_bf16(const void* z, const float* dy, const float* mean, const float* invstd, const float* gamma,
                              const float* beta, void* dz, float* dgamma, float* dbeta, long long P, int C, int train, void* ws,
                              size_t ws_bytes, void* stream) {
    if (!z || !dy || !mean || !invstd || !gamma || !beta || !dz || !dgamma || !dbeta || !ws || P <= 0 || C <= 0) return YV3_EINVAL;
    if (C & 7) return YV3_ESHAPE;
    if (ws_bytes < yv3_train_channel_bf16_workspace_bytes(P, C)) return YV3_EWORKSPACE;
    const Lay l = lay8(C);
    RedB r = {};
    r.z = (const u16*)z; r.dy = dy; r.mean = mean; r.invstd = invstd; r.gamma = gamma; r.beta = beta;
    r.P = P; r.C = C; r.gl = l.gl; r.nrl = l.nrl; r.part = (double*)ws;
    const int split = (int)red_split(P, l, &r.chunk);
    float* coef = (float*)((char*)ws + (size_t)split * 2 * C * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(channel_partials_b<true>, dim3(l.bx, split), dim3(NT), 0, st, r);
    YV3_CHECK_LAUNCH();
    hipLaunchKernelGGL(bnbwd_finalize, dim3((C + NT - 1) / NT), dim3(NT), 0, st, (const double*)ws, split, C, P, train, gamma, invstd,
                       dgamma, dbeta, coef);
    YV3_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_act_bwd_dz_b, dim3(l.bx, row_blocks(P, l)), dim3(NT), 0, st, (const u16*)z, dy, mean, invstd, gamma, beta,
                       (const float*)coef, (u16*)dz, P, C, l.gl, l.nrl);
    YV3_CHECK_LAUNCH();
    return 0;
}

int yv3_train_bias_bwd_bf16(const float* dlogits, const float* scale, void* dout, float* dbias, long long P, int C, void* ws,
                            size_t ws_bytes, void* stream) {
    if (!dlogits || !dout || !dbias || !ws || P <= 0 || C <= 0) return YV3_EINVAL;
    if (ws_bytes < yv3_train_channel_bf16_workspace_bytes(P, C)) return YV3_EWORKSPACE;
    const Lay l = lay2(C);
    long long chunk;
    const int split = (int)red_split(P, l, &chunk);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bias_bwd_b, dim3(l.bx, split), dim3(NT), 0, st, dlogits, scale, (u16*)dout, P, C, (C + 7) & ~7, chunk, l.gl, l.nrl,
                       (double*)ws);
    YV3_CHECK_LAUNCH();
    hipLaunchKernelGGL(colsum_finalize, dim3((C + NT - 1) / NT), dim3(NT), 0, st, (const double*)ws, split, C, dbias);
    YV3_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
