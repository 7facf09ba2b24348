// The per-channel finalize kernels of the training step, shared by train.hip (fp32 activations) and train_bf16_act.hip (bf16 activations):
// both reduce a [P][C] tensor into fp64 partials part[split][2][C] and finish them here, in split order.
#pragma once
#include "yv3_common.h"

namespace {

__device__ __forceinline__ float leaky_grad(float u, float d) { return u > 0.f ? d : d * 0.1f; }

__device__ __forceinline__ void sum_partials(const double* part, int split, int C, int c, double* a, double* b) {
    double x = 0.0, y = 0.0;
    for (int s = 0; s < split; ++s) { x += part[((long long)s * 2) * C + c]; y += part[((long long)s * 2 + 1) * C + c]; }
    *a = x; *b = y;
}

// batch statistics -> mean, 1/sqrt(var_biased + eps); running stats (momentum, unbiased variance) written to run_*_out
__global__ void stats_finalize(const double* part, int split, int C, long long P, float eps, float momentum,
                               const float* run_mean, const float* run_var, float* run_mean_out, float* run_var_out,
                               float* mean, float* invstd) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s, q;
    sum_partials(part, split, C, c, &s, &q);
    const double mu = s / (double)P;
    double var = q / (double)P - mu * mu;
    if (var < 0.0) var = 0.0;
    mean[c] = (float)mu;
    invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (run_mean_out) {
        const double unb = P > 1 ? var * (double)P / (double)(P - 1) : var;
        run_mean_out[c] = (float)((1.0 - momentum) * (double)run_mean[c] + momentum * mu);
        run_var_out[c] = (float)((1.0 - momentum) * (double)run_var[c] + momentum * unb);
    }
}

// per-channel coefficients of the backward: dgamma, dbeta out; coef[0] = gamma invstd, coef[1] = dbeta / P, coef[2] = dgamma / P
__global__ void bnbwd_finalize(const double* part, int split, int C, long long P, int train, const float* gamma, const float* invstd,
                               float* dgamma, float* dbeta, float* coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double a, b;
    sum_partials(part, split, C, c, &a, &b);
    dbeta[c] = (float)a;
    dgamma[c] = (float)b;
    coef[c] = gamma[c] * invstd[c];
    coef[C + c] = train ? (float)(a / (double)P) : 0.f;
    coef[2 * C + c] = train ? (float)(b / (double)P) : 0.f;
}

__global__ void colsum_finalize(const double* part, int split, int C, float* out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double a, b;
    sum_partials(part, split, C, c, &a, &b);
    out[c] = (float)a;
}

}  // namespace
