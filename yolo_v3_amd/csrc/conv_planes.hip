// The bf16-plane (one or three planes) and fp16 hi+lo instantiations of conv_planes_kernel.h and the entry points over them.
#include "conv_planes_kernel.h"

int yv3_pack_weight_planes(const float* w_oihw, void* w_packed, int cout, int cin, int k, int cout_pad, int np, hipStream_t s) {
    const long long total = (long long)cout_pad * k * k * cin;
    const int tb = cout_pad < 128 ? cout_pad : 128;
    if (cout_pad % tb) return YV3_ESHAPE;
    const dim3 grid(yv3_ceil_div(total, 256));
    if (np == 3)      hipLaunchKernelGGL(pack_weight_planes_kernel<3>, grid, dim3(256), 0, s, w_oihw, (u16*)w_packed, cout, cin, k, tb, total);
    else if (np == 2) hipLaunchKernelGGL(pack_weight_planes_kernel<2>, grid, dim3(256), 0, s, w_oihw, (u16*)w_packed, cout, cin, k, tb, total);
    else              hipLaunchKernelGGL(pack_weight_planes_kernel<1>, grid, dim3(256), 0, s, w_oihw, (u16*)w_packed, cout, cin, k, tb, total);
    YV3_CHECK_LAUNCH();
    return 0;
}

extern "C" int yv3_split_planes(const float* in, void* out, long long n, int np, void* stream) {
    if (!in || !out || n < 0 || np < 1 || np > 3) return YV3_EINVAL;
    if (n == 0) return 0;
    const dim3 grid(yv3_ceil_div(n, 256));
    if (np == 3)      hipLaunchKernelGGL(split_planes_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, in, (u16*)out, n);
    else if (np == 2) hipLaunchKernelGGL(split_planes_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, in, (u16*)out, n);
    else              hipLaunchKernelGGL(split_planes_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, in, (u16*)out, n);
    YV3_CHECK_LAUNCH();
    return 0;
}

extern "C" int yv3_merge_planes(const void* in, float* out, long long n, int np, void* stream) {
    if (!in || !out || n < 0 || np < 1 || np > 3) return YV3_EINVAL;
    if (n == 0) return 0;
    const dim3 grid(yv3_ceil_div(n, 256));
    if (np == 3)      hipLaunchKernelGGL(merge_planes_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, (const u16*)in, out, n);
    else if (np == 2) hipLaunchKernelGGL(merge_planes_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, (const u16*)in, out, n);
    else              hipLaunchKernelGGL(merge_planes_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (const u16*)in, out, n);
    YV3_CHECK_LAUNCH();
    return 0;
}

int yv3_conv2d_planes_k3s1(const ConvParamsP& p, int np, yv3_planes_kernel kernel, hipStream_t s);
int yv3_conv2d_planes_w4(const ConvParamsP& p, hipStream_t s);
int yv3_wino_input_transform(const u16* x, long long xs, u16* v, int B, int H, int W, int C, hipStream_t s);

// Winograd F(2x2,3x3) form of a 3x3 / stride-1 fp16-plane layer: input transform (winograd.hip) + the 16-position GEMM with the
// output transform folded into the main loop.  `p` = the direct launch's parameters (x, res, y, strides, Cout, act, flags).
static int launch_wino(const yv3_conv_desc* d, ConvParamsP p, const yv3_planes_choice& c, hipStream_t s) {
    const int th = (d->H + 1) / 2, tw = (d->W + 1) / 2;
    const long long T = (long long)d->B * th * tw;
    u16* v = (u16*)d->wino_ws;
    int rc = yv3_wino_input_transform(p.x, p.xs, v, d->B, d->H, d->W, d->cin, s);
    if (rc) return rc;
    p.x = v; p.xs = 16 * T * d->cin; p.xi_stride = T * d->cin;
    p.w = (const u16*)d->w_wino; p.alpha = d->alpha_wino;
    p.wH = d->H; p.wW = d->W; p.wth = th; p.wtw = tw;
    p.H = 1; p.W = (int)T; p.Ho = 1; p.Wo = (int)T; p.M = (int)T; p.stride = 1;
    p.K = 16 * d->cin; p.nk = p.K / PBK;
    p.tb = 128;
    constexpr int BM = 128, BN = 128, NS = 4;
    const dim3 grid((unsigned)(((T + BM - 1) / BM) * p.ntiles));
    p.total = (int)grid.x;
    const size_t pipe = (size_t)NS * 2 * (BM + BN) * ROWB, epi = (size_t)8 * 32 * (BN / 2 + 4) * 4;
    const size_t lds = pipe > epi ? pipe : epi;
    if (c.kernel == YV3_PK_WINO_EVEN) {
        if (c.grid <= 0) return YV3_EINVAL;
        const size_t vbytes = (size_t)2 * 16 * T * d->cin * sizeof(u16);
        p.ws = (float*)((char*)d->wino_ws + ((vbytes + 255) & ~(size_t)255));
        p.wsflags = (int*)((char*)p.ws + (size_t)YV3_WINO_SK_MAX_WG * YV3_WINO_SK_PART_BYTES);
        p.ws_bytes = yv3_wino_sk_bytes();
        hipLaunchKernelGGL((conv_planes_kernel<2, BM, BN, 4, 2, NS, false, false, false, true, true, 1, 0, true>), dim3((unsigned)c.grid), dim3(512), lds, s, p);
    } else {
        p.ws = nullptr; p.wsflags = nullptr; p.ws_bytes = 0;
        if (c.kernel == YV3_PK_WINO_ROLL)
            hipLaunchKernelGGL((conv_planes_kernel<2, BM, BN, 4, 2, NS, false, false, false, false, false, 1, 0, true, true>), grid, dim3(512), lds, s, p);
        else
            hipLaunchKernelGGL((conv_planes_kernel<2, BM, BN, 4, 2, NS, false, false, false, true, false, 1, 0, true>), grid, dim3(512), lds, s, p);
    }
    YV3_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t yv3_conv_workspace_bytes(void) { return yv3_sk_bytes(); }

static_assert(PBK == YV3_SEL_CHUNK, "conv_select.cpp counts K chunks of PBK elements");
static_assert(YV3_SK_PART_BYTES == 256 * 128 * sizeof(float), "a stream-K part holds the accumulators of the largest tile with a stream-K instantiation, 256x128");

// Launches what the selector chose (conv_select.cpp: yv3_select_planes) for a descriptor that passed its checks.
int yv3_conv2d_planes(const yv3_conv_desc* d, int np, const yv3_planes_choice& c, hipStream_t s) {
    const ConvParamsP p = conv_planes_params(d, c);
    const bool k3 = d->k == 3, dual = d->cin_up > 0, out_f32 = d->out_dtype == YV3_F32;
    switch (c.kernel) {
        case YV3_PK_K3S1_256x128: case YV3_PK_K3S1_128x128: case YV3_PK_K3S1_128x64: return yv3_conv2d_planes_k3s1(p, np, c.kernel, s);
        case YV3_PK_WINO_PINGPONG: case YV3_PK_WINO_ROLL: case YV3_PK_WINO_EVEN: return launch_wino(d, p, c, s);
        case YV3_PK_W4_192x128:     return yv3_conv2d_planes_w4(p, s);
        default: break;
    }
    if (np == 1) return launch_one_plane<YV3_EL_BF16>(p, k3, dual, out_f32, c, s);      // (conv_planes_kernel.h: the table YV3_F16 uses too)
    // two fp16 planes / three bf16 planes: the eight-wave tiles' ring is one deeper for two planes
#define YV3_CFG(N2_, N3_, ...) (np == 2 ? launch_cfg<2, __VA_ARGS__, N2_>(p, k3, dual, out_f32, c, s) : launch_cfg<3, __VA_ARGS__, N3_>(p, k3, dual, out_f32, c, s))
    switch (c.kernel) {
        case YV3_PK_256x128_W8:     return YV3_CFG(3, 2, 256, 128, 4, 2);
        case YV3_PK_128x128_W8:     return YV3_CFG(4, 3, 128, 128, 4, 2);
        case YV3_PK_128x128_W4:     return np == 2 ? launch_cfg<2, 128, 128, 2, 2, 2, 2>(p, k3, dual, out_f32, c, s) : YV3_EINVAL;
        case YV3_PK_128x64:         return YV3_CFG(2, 2, 128, 64, 2, 2);
        case YV3_PK_128x32:         return YV3_CFG(2, 2, 128, 32, 4, 1);
        default: break;             // (the other tiles are one-plane tiles)
    }
#undef YV3_CFG
    return YV3_EINVAL;
}
