// What the two convolution files of the training step (train.hip: fp32 operands, train_bf16.hip: bf16 operands) have in common: the
// shape rules and argument checks of their entry points, the output geometry, the index arithmetic of a weight, the kernel that sums
// the wgrad split partials and the wgrad workspace size.  Each file keeps its kernels, its Geo struct and its split rule (wgrad_split).
#pragma once
#include "yv3_common.h"

namespace {

constexpr int NT = 256;
enum { FWD = 0, DGRAD = 1, WGRAD = 2 };

// element i of the parameter w[cout][cin][k][k]: declares its output channel `co`, input channel `ci` and `tap`.  (A macro, not a
// function: the compiler simplifies a function on its own before inlining it, which reorders the instructions of its three kernels.)
#define YV3_WEIGHT_INDEX(i, cin, kk2)                            \
    const int co = (int)((i) / ((long long)(cin) * (kk2)));      \
    const int r = (int)((i) - (long long)co * (cin) * (kk2));    \
    const int ci = r / (kk2), tap = r - ci * (kk2)

// dw[co][ci][kh][kw] = sum over the splits of part[split][co][tap][ci], in split order (fp64)
__global__ void wgrad_reduce(const float* __restrict__ part, float* __restrict__ dw, int cout, int cin, int kk2, int split) {
    const long long MN = (long long)cout * cin * kk2;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= MN) return;
    YV3_WEIGHT_INDEX(i, cin, kk2);
    const long long src = (long long)co * cin * kk2 + (long long)tap * cin + ci;
    double s = 0.0;
    for (int z = 0; z < split; ++z) s += (double)part[z * MN + src];
    dw[i] = (float)s;
}

// ---- host side
int grid1(long long n) { long long b = (n + NT - 1) / NT; return (int)(b < 65536 ? (b > 0 ? b : 1) : 65536); }

bool conv_shape_ok(int B, int H, int W, int cin, int cin_up, int cout, int k, int stride) {
    if (B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || cin_up < 0) return false;
    if (!(k == 1 || k == 3) || !(stride == 1 || stride == 2)) return false;
    if (cin_up > 0 && (cin_up >= cin || (H & 1) || (W & 1))) return false;
    return true;
}

// the checks of a conv entry point in the ABI's order: the pointers (ptrs_ok: the entry's own) and sizes (YV3_EINVAL), then the shape
// (YV3_ESHAPE).  dgrad passes cin_up = 0, x_nchw = 0
int conv_check(bool ptrs_ok, int B, int H, int W, int cin, int cin_up, int cout, int k, int stride, int x_nchw) {
    if (!ptrs_ok) return YV3_EINVAL;
    if (B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0) return YV3_EINVAL;
    if (!conv_shape_ok(B, H, W, cin, cin_up, cout, k, stride) || (x_nchw && cin_up)) return YV3_ESHAPE;
    return 0;
}

int conv_out(int n, int k, int stride) { return (n + 2 * ((k - 1) / 2) - k) / stride + 1; }

// G: the file's Geo -- the sizes and the output geometry; the caller sets the pointers and M, N, K
template <class G>
G make_geo(int B, int H, int W, int cin, int cin_up, int cout, int k, int stride, int nchw) {
    G g = {};
    g.B = B; g.H = H; g.W = W; g.cin = cin; g.cin_up = cin_up; g.cout = cout; g.k = k; g.stride = stride; g.nchw = nchw;
    g.pad = (k - 1) / 2;
    g.Ho = conv_out(H, k, stride); g.Wo = conv_out(W, k, stride);
    return g;
}

// bytes of the wgrad partials [split][cout][k*k*cin] under `rule`, a file's split over the K = B*Ho*Wo output pixels of the
// M x N = cout x k*k*cin product; 0: the shape is out of range
size_t wgrad_workspace_bytes(void (*rule)(long long M, long long N, long long K, int* split, long long* chunk),
                             int B, int H, int W, int cin, int cout, int k, int stride) {
    if (!conv_shape_ok(B, H, W, cin, 0, cout, k, stride)) return 0;
    int split; long long chunk;
    const long long M = cout, N = (long long)k * k * cin, K = (long long)B * conv_out(H, k, stride) * conv_out(W, k, stride);
    rule(M, N, K, &split, &chunk);
    return (size_t)split * M * N * sizeof(float);
}

}  // namespace
