// Affine training augmentation (rotate, scale, shear, shift) for a whole batch of packed uint8 RGB images of any sizes: one
// program per image (include/yv3.h: yv3_affine_program; yolo_v3_amd/affine_augment.py samples them) holding two 2x3 float64
// matrices computed on the host -- fwd (source -> output) for the labels, inv (output -> source) for the pixels.  The output has
// the source's size.  tests/affine_aug_ref.py is the definition both kernels are held to, bit for bit.
//   affine_pixels_kernel   grid (workgroups per image, B) x 256: a workgroup reads its image's program, branches uniformly on
//                          `active` and walks the image in tiles of AF_TH x AF_TW pixels, a wave per tile row, a thread per output
//                          pixel: Pillow's Image.transform(AFFINE, BILINEAR, fillcolor 128) in float64 -- the centre of the output
//                          pixel through inv, 128 outside [0, W) x [0, H), otherwise two horizontal lerps and a vertical one on
//                          clamped neighbours, truncated.  Neighbouring lanes read neighbouring source pixels; the sources are
//                          byte gathers served by the caches (DESIGN.md section 8e.2 has the measurements), no LDS.  An inactive image (or one whose program fails the
//                          checks) is copied through.
//   affine_labels_kernel   a wave per image, rows strided over lanes, float64: the four corners of a box through fwd, their
//                          axis-aligned hull, bbs_clip, bbs_remove_cut_out(0.1); kept rows stay in place, dropped rows are zeros,
//                          so a row depends on itself alone and labels_out may be labels.
// (compiled with -ffp-contract=off: every float64 op rounds as the restatement's separate operations do)
#include "yv3_common.h"

namespace {

constexpr int AF_TH = 4, AF_TW = 64, AF_NT = AF_TH * AF_TW;

// python's min(a, b) / max(a, b): the second argument only where it is strictly smaller / larger (NaN and -0.0 as numpy scalars)
__device__ inline double af_min(double a, double b) { return b < a ? b : a; }
__device__ inline double af_max(double a, double b) { return b > a ? b : a; }

// The checks yolo_v3_amd/affine_augment.py:check_affine_programs restates on the host, in the same order.
__device__ inline int af_check_program(const yv3_affine_program* __restrict__ P, int H, int W) {
    if (H <= 0 || W <= 0) return YV3_EINVAL;
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (!isfinite(P->fwd[k]) || !isfinite(P->inv[k])) return YV3_EINVAL;
    if (P->active != 0 && P->active != 1) return YV3_EINVAL;
    return 0;
}

// Image b's source range [so, so + n3) inside src_bytes and its output range [oo, oo + n3) inside out_bytes, in 64 bits
__device__ inline bool af_in_bounds(int H, int W, long long so, long long src_bytes, long long oo, long long out_bytes) {
    if (H <= 0 || W <= 0) return false;
    const long long px = (long long)H * W;                     // < 2^62
    if (px > src_bytes / 3 || px > out_bytes / 3) return false;
    const long long n3 = px * 3;
    return so >= 0 && so <= src_bytes && n3 <= src_bytes - so && oo >= 0 && oo <= out_bytes && n3 <= out_bytes - oo;
}

__global__ __launch_bounds__(AF_NT) void affine_pixels_kernel(const unsigned char* __restrict__ src, long long src_bytes,
                                                              const long long* __restrict__ src_offsets, const int* __restrict__ hw,
                                                              const yv3_affine_program* __restrict__ programs,
                                                              unsigned char* __restrict__ out, long long out_bytes,
                                                              const long long* __restrict__ out_offsets, int* __restrict__ status) {
    const int b = blockIdx.y, t = threadIdx.x;
    const yv3_affine_program* P = programs + b;
    const int H = hw[2 * b], W = hw[2 * b + 1];
    const long long so = src_offsets[b], oo = out_offsets[b];
    const bool in_bounds = af_in_bounds(H, W, so, src_bytes, oo, out_bytes);
    const int code = in_bounds ? af_check_program(P, H, W) : YV3_EINVAL;
    if (blockIdx.x == 0 && t == 0) status[b] = code;
    if (!in_bounds) return;
    const bool active = !code && P->active == 1;
    const double i0 = P->inv[0], i1 = P->inv[1], i2 = P->inv[2], i3 = P->inv[3], i4 = P->inv[4], i5 = P->inv[5];
    const unsigned char* img = src + so;
    unsigned char* dst = out + oo;
    const int lx = t & (AF_TW - 1), ly = t / AF_TW;

    const int tiles_x = (W + AF_TW - 1) / AF_TW, tiles_y = (H + AF_TH - 1) / AF_TH;
    const long long n_tiles = (long long)tiles_x * tiles_y;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int ty = (int)(tile / tiles_x), tx = (int)(tile - (long long)ty * tiles_x);
        const int x = tx * AF_TW + lx, y = ty * AF_TH + ly;
        if (x >= W || y >= H) continue;
        unsigned char* d = dst + ((long long)y * W + x) * 3;
        if (!active) {
            const unsigned char* p = img + ((long long)y * W + x) * 3;
            d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
            continue;
        }
        const double xc = (double)x + 0.5, yc = (double)y + 0.5;
        double xin = i0 * xc + i1 * yc + i2;
        double yin = i3 * xc + i4 * yc + i5;
        if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) {
            d[0] = 128; d[1] = 128; d[2] = 128;
            continue;
        }
        xin = xin - 0.5; yin = yin - 0.5;                      // in [-0.5, W - 0.5) x [-0.5, H - 0.5)
        const double fx = floor(xin), fy = floor(yin);
        const double dx = xin - fx, dy = yin - fy;
        const int x0 = (int)fx, y0 = (int)fy;                  // -1 .. W - 1, -1 .. H - 1
        const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1), ya = min(max(y0, 0), H - 1);
        const bool second = y0 + 1 >= 0 && y0 + 1 < H;
        const int yb = second ? y0 + 1 : ya;
        const unsigned char* ra = img + (long long)ya * W * 3;
        const unsigned char* rb = img + (long long)yb * W * 3;
        const unsigned char *paa = ra + (long long)xa * 3, *pab = ra + (long long)xb * 3;
        const unsigned char *pba = rb + (long long)xa * 3, *pbb = rb + (long long)xb * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double a0 = (double)paa[c], a1 = (double)pab[c];
            const double v1 = a0 + (a1 - a0) * dx;
            double v2 = v1;
            if (second) {
                const double b0 = (double)pba[c], b1 = (double)pbb[c];
                v2 = b0 + (b1 - b0) * dx;
            }
            d[c] = (unsigned char)(int)(v1 + (v2 - v1) * dy);
        }
    }
}

__global__ __launch_bounds__(64) void affine_labels_kernel(const double* labels, int T, const int* __restrict__ hw,
                                                           const yv3_affine_program* __restrict__ programs, double* labels_out,
                                                           int* __restrict__ status) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const yv3_affine_program* P = programs + b;
    const int H = hw[2 * b], W = hw[2 * b + 1];
    const int code = af_check_program(P, H, W);
    if (lane == 0) status[b] = code;
    const bool active = !code && P->active == 1;
    const double f0 = P->fwd[0], f1 = P->fwd[1], f2 = P->fwd[2], f3 = P->fwd[3], f4 = P->fwd[4], f5 = P->fwd[5];
    const double Wd = (double)W, Hd = (double)H;
    // bbs_clip's bound, in float64: W - float64(np.finfo(np.float32).eps)
    const double xmax = Wd - 1.1920928955078125e-07, ymax = Hd - 1.1920928955078125e-07;
    for (int r = lane; r < T; r += 64) {
        const double* L = labels + ((size_t)b * T + r) * 5;
        double* O = labels_out + ((size_t)b * T + r) * 5;
        const double cls = L[0], cx = L[1], cy = L[2], w = L[3], h = L[4];
        double o0 = cls, o1 = cx, o2 = cy, o3 = w, o4 = h;
        if (active) {
            o0 = o1 = o2 = o3 = o4 = 0.0;
            if (!(w <= 0.0 || h <= 0.0)) {                                     // label_np_to_bbs drops such rows
                // BoundingBoxConverter.convert: relative cxcywh -> x1y1x2y2, then * (W, H)
                const double x1 = (cx - w / 2) * Wd, x2 = (cx + w / 2) * Wd;
                const double y1 = (cy - h / 2) * Hd, y2 = (cy + h / 2) * Hd;
                // the four corners through fwd, in the order (x1,y1) (x2,y1) (x2,y2) (x1,y2)
                const double ax = f0 * x1 + f1 * y1 + f2, ay = f3 * x1 + f4 * y1 + f5;
                const double bx = f0 * x2 + f1 * y1 + f2, by = f3 * x2 + f4 * y1 + f5;
                const double cx2 = f0 * x2 + f1 * y2 + f2, cy2 = f3 * x2 + f4 * y2 + f5;
                const double dx = f0 * x1 + f1 * y2 + f2, dy = f3 * x1 + f4 * y2 + f5;
                const double hx1 = af_min(af_min(ax, bx), af_min(cx2, dx)), hx2 = af_max(af_max(ax, bx), af_max(cx2, dx));
                const double hy1 = af_min(af_min(ay, by), af_min(cy2, dy)), hy2 = af_max(af_max(ay, by), af_max(cy2, dy));
                const double area = (hy2 - hy1) * (hx2 - hx1);                 // bbs_remove_cut_out(., 0.1)
                if (area > 0.0) {
                    const double c1 = af_min(af_max(hx1, 0.0), xmax), c2 = af_min(af_max(hx2, 0.0), xmax);
                    const double d1 = af_min(af_max(hy1, 0.0), ymax), d2 = af_min(af_max(hy2, 0.0), ymax);
                    if ((c2 - c1) * (d2 - d1) / area > 0.1) {                   // x1y1x2y2 -> relative cxcywh
                        const double bw = c2 - c1, bh = d2 - d1;
                        o0 = cls;
                        o1 = (c1 + bw / 2) / Wd;
                        o2 = (d1 + bh / 2) / Hd;
                        o3 = bw / Wd;
                        o4 = bh / Hd;
                    }
                }
            }
        }
        O[0] = o0; O[1] = o1; O[2] = o2; O[3] = o3; O[4] = o4;
    }
}

}  // namespace

extern "C" int yv3_affine_augment(const unsigned char* src, long long src_bytes, const long long* src_offsets, const int* hw,
                                  const void* programs, int B, unsigned char* out, long long out_bytes, const long long* out_offsets,
                                  int* status, void* stream) {
    if (!src || !src_offsets || !hw || !programs || !out || !out_offsets || !status) return YV3_EINVAL;
    if (src_bytes <= 0 || out_bytes <= 0 || B <= 0 || B > 65535) return YV3_EINVAL;
    // a workgroup per two or three 4 x 64 tiles of a 640 x 480 source at batch 16, more tiles per workgroup beyond
    const int per_image = max(1, min(4096, yv3_num_cu() * 32 / B));
    hipLaunchKernelGGL(affine_pixels_kernel, dim3(per_image, B), dim3(AF_NT), 0, (hipStream_t)stream, src, src_bytes, src_offsets,
                       hw, (const yv3_affine_program*)programs, out, out_bytes, out_offsets, status);
    YV3_CHECK_LAUNCH();
    return 0;
}

extern "C" int yv3_affine_labels(const double* labels, int B, int T, const int* hw, const void* programs, double* labels_out,
                                 int* status, void* stream) {
    if (((!labels || !labels_out) && T > 0) || !hw || !programs || !status) return YV3_EINVAL;
    if (B <= 0 || T < 0) return YV3_EINVAL;
    hipLaunchKernelGGL(affine_labels_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, labels, T, hw,
                       (const yv3_affine_program*)programs, labels_out, status);
    YV3_CHECK_LAUNCH();
    return 0;
}
