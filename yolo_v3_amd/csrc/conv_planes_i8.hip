// YV3_I8: calibrated int8 convolutions on v_mfma_i32_32x32x32_i8 -- the one-plane tile templates of conv_planes_kernel.h
// instantiated with the one-byte element type, in a translation unit of their own: conv_planes.hip's and conv_planes_f16.hip's
// instantiations stay what they were.
// Byte for byte an int8 layer of C channels is a bf16 layer of C/2: a 64-deep int8 K chunk is the 64-byte LDS row (ROWB) the plane kernels
// stage with 16-byte global_load_lds, a lane's fragment of a k-step is 16 bytes either way (row = lane & 31, K half = lane >> 5, the same for
// both operands -- the product only needs the two operands to agree on which byte is which k), and the i32 result tile has the fp32 tile's
// lane map.  So the kernel parameters count the input channels in 16-bit units (Cin / 2, Cup / 2, K / 2) and everything up to the epilogue
// runs unchanged; the accumulator registers hold int32 bit patterns, which the epilogue converts, scales, adds the residual to and quantises
// (conv_planes_common.h, EL == YV3_EL_I8).
// Not here: Winograd, stream-K, the k3s1 and w4 kernels (yv3_select_planes_i8 never chooses them) and fp32 outputs (the head convs are
// YV3_BF16 launches that read the integers as bf16).
#include "conv_planes_kernel.h"

namespace {

constexpr int KB = 2 * PBK;        // int8 K elements per chunk = bytes per LDS row

// OIHW fp32 holding integers in [-127, 127] -> int8 in the LDS-image order of pack_weight_planes_kernel, in bytes:
//   [n / tb][k / 64][n % tb][physical slot][16],  physical slot = (k % 64) / 16 ^ swz(n % tb),  k = (kh*3+kw)*cin + c
__global__ void pack_weight_i8_kernel(const float* __restrict__ in, signed char* __restrict__ out, int cout, int cin, int k, int tb, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;    // over [cout_pad][K]
    if (i >= total) return;
    const int kk = k * k;
    const int K = kk * cin;
    const int n = (int)(i / K);
    const int kidx = (int)(i - (long long)n * K);
    const int tap = kidx / cin, c = kidx - tap * cin;
    float v = 0.f;
    if (n < cout) v = in[((long long)n * cin + c) * kk + tap];
    const int nk = K / KB;
    const int r = n % tb, ke = kidx % KB;
    const int slot = (ke >> 4) ^ swz(r);
    const long long base = ((long long)(n / tb) * nk + kidx / KB) * (long long)(tb * KB) + r * KB + slot * 16 + (ke & 15);
    out[base] = (signed char)(int)__builtin_amdgcn_fmed3f(__builtin_rintf(v), -127.f, 127.f);
}

// one bf16 plane -> int8, 8 elements per thread: q = clip(rint(x * inv_s), -127, 127), NaN -> 0
__global__ void quantize_bf16_i8_kernel(const u32x4* __restrict__ in, u32x2* __restrict__ out, long long n8, float inv_s) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    const u32x4 q = in[i];
    float v[8];
#pragma unroll
    for (int h = 0; h < 4; ++h) { v[2 * h] = ElemOps<YV3_EL_BF16>::lo(q[h]); v[2 * h + 1] = ElemOps<YV3_EL_BF16>::hi(q[h]); }
#pragma unroll
    for (int h = 0; h < 8; ++h) v[h] = v[h] == v[h] ? ElemOps<YV3_EL_I8>::quant(v[h] * inv_s) : 0.f;
    out[i] = u32x2{ElemOps<YV3_EL_I8>::pack4(v[0], v[1], v[2], v[3]), ElemOps<YV3_EL_I8>::pack4(v[4], v[5], v[6], v[7])};
}

}  // namespace

int yv3_pack_weight_i8(const float* w_oihw, void* w_packed, int cout, int cin, int k, int cout_pad, hipStream_t s) {
    const long long total = (long long)cout_pad * k * k * cin;
    const int tb = cout_pad < 128 ? cout_pad : 128;
    if (cout_pad % tb || cin % KB || cout_pad % 32) return YV3_ESHAPE;
    hipLaunchKernelGGL(pack_weight_i8_kernel, dim3(yv3_ceil_div(total, 256)), dim3(256), 0, s, w_oihw, (signed char*)w_packed, cout, cin, k, tb, total);
    YV3_CHECK_LAUNCH();
    return 0;
}

extern "C" int yv3_quantize_bf16_i8(const void* in, void* out, long long n, float inv_s, void* stream) {
    if (!in || !out || n < 0 || !(inv_s > 0.f)) return YV3_EINVAL;
    if (n % 8 || ((size_t)in & 15) || ((size_t)out & 7)) return YV3_ESHAPE;
    if (n == 0) return 0;
    hipLaunchKernelGGL(quantize_bf16_i8_kernel, dim3(yv3_ceil_div(n / 8, 256)), dim3(256), 0, (hipStream_t)stream, (const u32x4*)in, (u32x2*)out, n / 8, inv_s);
    YV3_CHECK_LAUNCH();
    return 0;
}

// Launches what the selector chose for a YV3_I8 descriptor (yv3_select_planes_i8: the one-bf16-plane choice for the layer's bytes).
int yv3_conv2d_planes_i8(const yv3_conv_desc* d, const yv3_planes_choice& c, hipStream_t s) {
    ConvParamsP p = conv_planes_params(d, c);
    p.Cin = d->cin / 2; p.Cup = d->cin_up / 2;                     // 16-bit units: what the staging code counts
    p.K = d->k * d->k * p.Cin;
    p.nk = p.K / PBK;
    p.dec_out = nullptr; p.ws = nullptr; p.wsflags = nullptr; p.ws_bytes = 0; p.flags = nullptr;      // (nothing here saturates or hands over)
    p.s_res = d->s_res; p.inv_s_out = d->inv_s_out; p.out_bf16 = d->out_dtype == YV3_BF16;
    return launch_one_plane<YV3_EL_I8>(p, d->k == 3, d->cin_up > 0, false, c, s);
}
