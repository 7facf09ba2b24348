// YOLO head decode (reference yololayer.py:31-59,97-105, inference branch) as one fused
// elementwise kernel.  With NHWC logits [B,H,W,3*(5+C)] the reference's final row order
// (y*W + x)*3 + a (yololayer.py:104) IS the input order, so the decode is a pure streaming map:
// one read, one write, no permute.  HBM-bound: 2 * 4 bytes per element.
//
// Op order follows the reference so that results agree to the rounding of exp/sigmoid:
//   xy  : (sigmoid(t) + grid) * stride                yololayer.py:45,58,98
//   wh  : (exp(t) * (anchor / stride)) * stride       yololayer.py:37,59,98
//   conf, cls : sigmoid(t)                            yololayer.py:47-48
#include "yv3_common.h"

namespace {

struct DecodeArgs {
    const float* logits;
    float* out;
    long long out_batch_stride;
    int ld;            // NHWC: floats per pixel; NCHW: unused
    int H, W, attrib;
    float stride;
    float aw[3], ah[3];   // anchor / stride (float32 division, as torch does)
};

// One workgroup iteration = PPB consecutive pixels; thread -> channel ca of the 3*(5+C) per pixel (no
// per-element integer division: anchor / attribute come from two compares, grid x/y once per pixel).
constexpr int PPB = 4;

template <bool NCHW>
__global__ __launch_bounds__(256) void decode_kernel(const DecodeArgs a) {
    const int b = blockIdx.y;
    const int HW = a.H * a.W;
    const int ch = 3 * a.attrib;
    const float* src = a.logits + (NCHW ? (long long)b * HW * ch : (long long)b * HW * a.ld);
    float* dst = a.out + (long long)b * a.out_batch_stride;
    for (int ca = threadIdx.x; ca < ch; ca += 256) {
        const int anc = (ca >= a.attrib) + (ca >= 2 * a.attrib);
        const int attr = ca - anc * a.attrib;
        const float an = attr == 2 ? a.aw[anc] : a.ah[anc];
        for (int p0 = blockIdx.x * PPB; p0 < HW; p0 += gridDim.x * PPB) {
            float t[PPB];
#pragma unroll
            for (int k = 0; k < PPB; ++k) {
                const int pix = p0 + k < HW ? p0 + k : HW - 1;
                t[k] = NCHW ? src[(long long)ca * HW + pix] : src[(long long)pix * a.ld + ca];
            }
#pragma unroll
            for (int k = 0; k < PPB; ++k) {
                const int pix = p0 + k;
                if (pix >= HW) break;
                dst[(long long)pix * ch + ca] = yv3_decode_value(t[k], attr, an, (float)(pix % a.W), (float)(pix / a.W), a.stride);
            }
        }
    }
}

// Backward of decode_kernel<true>: dlogits[ca][pix] = dout[pix][ca] * d(decoded value)/d(logit), the derivative recomputed from the
// logit by the forward's own yv3_decode_value: the decoded w / h itself for tw / th (e^t is its own derivative), s (1 - s) for conf and the
// classes, stride s (1 - s) for tx / ty (s = sigmoid(t), taken as the forward's value of a conf attribute).
__global__ __launch_bounds__(256) void decode_bwd_kernel(const DecodeArgs a, const float* __restrict__ dout, float* __restrict__ dlogits) {
    const int b = blockIdx.y;
    const int HW = a.H * a.W;
    const int ch = 3 * a.attrib;
    const float* src = a.logits + (long long)b * HW * ch;
    const float* dsrc = dout + (long long)b * HW * ch;
    float* dst = dlogits + (long long)b * HW * ch;
    for (int ca = threadIdx.x; ca < ch; ca += 256) {
        const int anc = (ca >= a.attrib) + (ca >= 2 * a.attrib);
        const int attr = ca - anc * a.attrib;
        const float an = attr == 2 ? a.aw[anc] : a.ah[anc];
        const bool wh = attr == 2 || attr == 3;
        for (int pix = blockIdx.x; pix < HW; pix += gridDim.x) {
            const float v = yv3_decode_value(src[(long long)ca * HW + pix], attr < 2 ? 4 : attr, an, 0.f, 0.f, a.stride);
            const float sd = v * (1.f - v);
            const float d = wh ? v : (attr < 2 ? a.stride * sd : sd);
            dst[(long long)ca * HW + pix] = dsrc[(long long)pix * ch + ca] * d;
        }
    }
}

int run(const float* logits, int ld, const float* anchors, float stride, float* out, long long obs,
        int B, int H, int W, int C, bool nchw, void* stream) {
    if (!logits || !anchors || !out || B <= 0 || H <= 0 || W <= 0 || C < 0 || stride <= 0.f) return YV3_EINVAL;
    DecodeArgs a;
    a.logits = logits; a.out = out; a.out_batch_stride = obs; a.ld = ld;
    a.H = H; a.W = W; a.attrib = 5 + C; a.stride = stride;
    if (!nchw && ld < 3 * a.attrib) return YV3_ESHAPE;
    for (int i = 0; i < 3; ++i) { a.aw[i] = anchors[2 * i] / stride; a.ah[i] = anchors[2 * i + 1] / stride; }
    const int groups = (H * W + PPB - 1) / PPB;
    const dim3 grid((unsigned)(groups < 1024 ? groups : 1024), (unsigned)B);
    if (nchw) hipLaunchKernelGGL(decode_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else      hipLaunchKernelGGL(decode_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    YV3_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int yv3_decode(const float* logits, int ld_logits, const float* anchors_host, float stride,
                          float* out, long long out_batch_stride, int B, int H, int W, int num_class, void* stream) {
    return run(logits, ld_logits, anchors_host, stride, out, out_batch_stride, B, H, W, num_class, false, stream);
}

extern "C" int yv3_decode_nchw(const float* logits_nchw, const float* anchors_host, float stride,
                               float* out, long long out_batch_stride, int B, int H, int W, int num_class, void* stream) {
    return run(logits_nchw, 0, anchors_host, stride, out, out_batch_stride, B, H, W, num_class, true, stream);
}

extern "C" int yv3_decode_bwd_nchw(const float* logits_nchw, const float* dout, const float* anchors_host, float stride,
                                   float* dlogits_nchw, int B, int H, int W, int num_class, void* stream) {
    if (!logits_nchw || !dout || !anchors_host || !dlogits_nchw || B <= 0 || H <= 0 || W <= 0 || num_class < 0 || stride <= 0.f)
        return YV3_EINVAL;
    if (B > 65535) return YV3_ESHAPE;
    DecodeArgs a = {};
    a.logits = logits_nchw; a.H = H; a.W = W; a.attrib = 5 + num_class; a.stride = stride;
    for (int i = 0; i < 3; ++i) { a.aw[i] = anchors_host[2 * i] / stride; a.ah[i] = anchors_host[2 * i + 1] / stride; }
    const long long hw = (long long)H * W;
    const dim3 grid((unsigned)(hw < 4096 ? hw : 4096), (unsigned)B);
    hipLaunchKernelGGL(decode_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, a, dout, dlogits_nchw);
    YV3_CHECK_LAUNCH();
    return 0;
}
