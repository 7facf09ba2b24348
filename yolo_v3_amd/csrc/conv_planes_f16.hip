// YV3_F16: one fp16 plane (11 significant bits, saturated to +-65504) on the tile set of the one-bf16-plane mode -- the instantiations of
// conv_planes_kernel.h with NP = 1 and the fp16 element type (conversion with saturation + status bit, v_mfma_f32_32x32x16_f16), in a
// translation unit of their own: they build beside conv_planes.hip's, which stay what they were.
// Not here: the Winograd stage (a transformed operand rounded to 11 bits is another precision class), stream-K and the four-wave 192x128
// tile (conv_planes_w4.hip) -- rules of the fp16 hi+lo mode that yv3_select_planes never applies to one plane.
#include "conv_planes_kernel.h"

int yv3_conv2d_planes_k3s1_f16(const ConvParamsP& p, yv3_planes_kernel kernel, hipStream_t s);

// OIHW fp32 -> one fp16 plane (round to nearest even, subnormals kept) in the LDS-image order of pack_weight_planes_kernel
int yv3_pack_weight_plane_f16(const float* w_oihw, void* w_packed, int cout, int cin, int k, int cout_pad, hipStream_t s) {
    const long long total = (long long)cout_pad * k * k * cin;
    const int tb = cout_pad < 128 ? cout_pad : 128;
    if (cout_pad % tb) return YV3_ESHAPE;
    hipLaunchKernelGGL((pack_weight_planes_kernel<1, YV3_EL_F16>), dim3(yv3_ceil_div(total, 256)), dim3(256), 0, s, w_oihw, (u16*)w_packed, cout, cin, k, tb, total);
    YV3_CHECK_LAUNCH();
    return 0;
}

extern "C" int yv3_split_plane_f16(const float* in, void* out, long long n, void* stream) {
    if (!in || !out || n < 0) return YV3_EINVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL((split_planes_kernel<1, YV3_EL_F16>), dim3(yv3_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, in, (u16*)out, n);
    YV3_CHECK_LAUNCH();
    return 0;
}

extern "C" int yv3_merge_plane_f16(const void* in, float* out, long long n, void* stream) {
    if (!in || !out || n < 0) return YV3_EINVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL((merge_planes_kernel<1, YV3_EL_F16>), dim3(yv3_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, (const u16*)in, out, n);
    YV3_CHECK_LAUNCH();
    return 0;
}

// Launches what the selector chose for a YV3_F16 descriptor: yv3_select_planes(d, 1, ncu), i.e. the one-bf16-plane mode's choice.
int yv3_conv2d_planes_f16(const yv3_conv_desc* d, const yv3_planes_choice& c, hipStream_t s) {
    const ConvParamsP p = conv_planes_params(d, c);
    const bool k3 = d->k == 3, dual = d->cin_up > 0, out_f32 = d->out_dtype == YV3_F32;
    switch (c.kernel) {
        case YV3_PK_K3S1_256x128: case YV3_PK_K3S1_128x128: case YV3_PK_K3S1_128x64: return yv3_conv2d_planes_k3s1_f16(p, c.kernel, s);
        default: return launch_one_plane<YV3_EL_F16>(p, k3, dual, out_f32, c, s);      // (conv_planes_kernel.h: the table YV3_BF16 uses)
    }
}
