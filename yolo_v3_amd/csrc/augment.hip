// The reference's training augmentation (custom_data_train.ipynb getTransforms(aug=True), transforms.py):
//   Compose([IaaAugmentations([iaa_hsv_aug(hue, sat, exp), iaa_random_crop(jitter), iaa.Fliplr(0.5), IaaLetterbox(dim)]), ToTensor()])
// for a whole batch of packed uint8 RGB sources of any sizes, with the per-image random draws given as parameters
// [B][8] float64 = dhue, dsat, dexp, top, right, bottom, left, flip (yolo_v3_amd/augment.py samples them):
//   hsv_kernel       step 1, iaa_hsv_aug: OpenCV 8-bit RGB2HSV (integer path), h + dhue, s * dsat, v * dexp, 8-bit HSV2RGB ->
//                    the caller's workspace, image b read at src + src_offsets[b] and written at ws + ws_offsets[b] (the packed
//                    entry point passes one array for both; the gathering one reads a resident arena and writes compactly)
//   resample_kernel  steps 2-4: CropAndPad (pad 128, after the colour step), Fliplr, IaaLetterbox (cv2 INTER_CUBIC fixed point,
//                    replicated border at the edges of the cropped / padded / flipped intermediate, which is never materialised),
//                    128 canvas, /255, fp32 CHW straight into the [B,3,h,w] network input
//   labels_kernel    the label side of the same steps, in float64: rows (cls, cx, cy, w, h) relative to the source ->
//                    rows relative to the canvas, bbs_remove_cut_out(0.1), ToTensor's zero-filled [B][max_rows][5] fp32 target
// Per-image argument errors (a parameter or a source the reference cannot process) are found on the device: every launch writes
// status[b] (0 or a YV3_E* code) for each image, and an image with a non-zero status gets zeros in place of its outputs.
// (compiled with -ffp-contract=off: every float op rounds as the reference's separate float32 / float64 operations do)
#include "yv3_common.h"

namespace {

#include "cv_resize.h"

struct AugGeom {
    int H, W, top, left, H1, W1, flip;
    int rw, rh, xp, yp;                  // IaaLetterbox._compute_height_width_pad((H1, W1), OH, OW)
    double scale_x, scale_y;             // cv::resize scales of the (H1, W1) -> (rh, rw) resample
};

__device__ inline bool aug_is_int(double v) { return v == rint(v) && fabs(v) <= (double)(1 << 30); }

// The checks yolo_v3_amd/augment.py:check_params restates on the host, in the same order.
__device__ inline int aug_geometry(const double* __restrict__ p, int H, int W, int OH, int OW, AugGeom& g) {
    if (H <= 0 || W <= 0) return YV3_EINVAL;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (!isfinite(p[k])) return YV3_EINVAL;
    if (p[1] < 0.0 || p[2] < 0.0) return YV3_EINVAL;
    if (!aug_is_int(p[3]) || !aug_is_int(p[4]) || !aug_is_int(p[5]) || !aug_is_int(p[6])) return YV3_EINVAL;
    if (p[7] != 0.0 && p[7] != 1.0) return YV3_EINVAL;
    const long long H1 = (long long)H + (long long)p[3] + (long long)p[5];
    const long long W1 = (long long)W + (long long)p[6] + (long long)p[4];
    if (H1 < 1 || W1 < 1 || H1 > (1 << 30) || W1 > (1 << 30)) return YV3_ESHAPE;
    g.H = H; g.W = W; g.top = (int)p[3]; g.left = (int)p[6]; g.H1 = (int)H1; g.W1 = (int)W1; g.flip = p[7] != 0.0;
    const double rw = (double)OW / g.W1, rh = (double)OH / g.H1;         // transforms.py:200-204: python floats, int() truncation
    const double ratio = rw < rh ? rw : rh;
    g.rw = (int)(g.W1 * ratio); g.rh = (int)(g.H1 * ratio);
    if (g.rw <= 0 || g.rh <= 0) return YV3_ESHAPE;
    g.xp = (OW - g.rw) / 2; g.yp = (OH - g.rh) / 2;
    g.scale_x = 1.0 / ((double)g.rw / g.W1); g.scale_y = 1.0 / ((double)g.rh / g.H1);
    return 0;
}

// ---- step 1 ------------------------------------------------------------------------------------------------------------------
// OpenCV RGB2HSV_b (hsv_shift = 12, hue range 180): sdiv[v] = round((255 << 12) / v), hdiv[d] = round((180 << 12) / (6 d)),
// entry 0 = 0 (no ties occur for 1..255: cvRound's half-to-even never matters).  HSV2RGB_b: h, s * (1/255.f), v * (1/255.f) as
// float32, h * (6.f/180) wrapped into [0, 6) (hue bytes 180..255 wrap here, as in the reference), sector table, saturate_cast<uchar>.
// Image b's source range [off, off + n3) inside src_bytes and its colour copy's range [wo, wo + n3) inside ws_span, in 64 bits.
__device__ inline bool aug_in_bounds(long long off, long long src_bytes, long long wo, long long ws_span, long long n3) {
    return off >= 0 && off <= src_bytes && n3 <= src_bytes - off && wo >= 0 && wo <= ws_span && n3 <= ws_span - wo;
}

__global__ __launch_bounds__(256) void hsv_kernel(const unsigned char* __restrict__ src, long long src_bytes,
                                                  const long long* __restrict__ src_offsets,
                                                  const long long* __restrict__ ws_offsets, long long ws_span,
                                                  const int* __restrict__ hw, const double* __restrict__ params, int OH, int OW,
                                                  unsigned char* __restrict__ ws) {
    __shared__ int sdiv[256], hdiv[256];
    const int t = threadIdx.x;
    sdiv[t] = t ? (int)rint(1044480.0 / t) : 0;
    hdiv[t] = t ? (int)rint(737280.0 / (6.0 * t)) : 0;
    __syncthreads();
    const int b = blockIdx.y;
    const double* p = params + 8 * (size_t)b;
    AugGeom g;
    if (aug_geometry(p, hw[2 * b], hw[2 * b + 1], OH, OW, g)) return;
    const long long off = src_offsets[b], wo = ws_offsets[b], n = (long long)g.H * g.W;
    if (!aug_in_bounds(off, src_bytes, wo, ws_span, n * 3)) return;
    const float dhue = (float)p[0], dsat = (float)p[1], dexp = (float)p[2];
    const unsigned char* s = src + off;
    unsigned char* d = ws + wo;
    const float hscale = 6.f / 180.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + t; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int r = s[3 * i], gg = s[3 * i + 1], bb = s[3 * i + 2];
        // RGB2HSV_b (blue index 2)
        const int v = max(max(bb, gg), r), vmin = min(min(bb, gg), r);
        const int diff = v - vmin;
        const int vr = v == r ? -1 : 0, vg = v == gg ? -1 : 0;
        const int sat = (diff * sdiv[v] + (1 << 11)) >> 12;
        int h = (vr & (gg - bb)) + (~vr & ((vg & (bb - r + 2 * diff)) + (~vg & (r - gg + 4 * diff))));
        h = (h * hdiv[diff] + (1 << 11)) >> 12;
        h += h < 0 ? 180 : 0;
        // iaa_hsv_aug's Add / Multiply: float32, clipped to the byte range, truncated
        const int h2 = (int)fminf(fmaxf((float)h + dhue, 0.f), 255.f);
        const int s2 = (int)fminf(fmaxf((float)sat * dsat, 0.f), 255.f);
        const int v2 = (int)fminf(fmaxf((float)v * dexp, 0.f), 255.f);
        // HSV2RGB_b
        const float sf = (float)s2 * (1.f / 255.f), vf = (float)v2 * (1.f / 255.f);
        float R = vf, G = vf, Bc = vf;
        if (sf != 0.f) {
            float hf = (float)h2 * hscale;
            if (hf >= 6.f) hf -= 6.f;                                       // h2 <= 255: hf < 8.5, one step wraps it
            int sector = (int)floorf(hf);
            hf -= (float)sector;
            if ((unsigned)sector >= 6u) { sector = 0; hf = 0.f; }
            float tab[4];
            tab[0] = vf;
            tab[1] = vf * (1.f - sf);
            tab[2] = vf * (1.f - sf * hf);
            tab[3] = vf * (1.f - sf * (1.f - hf));
            // sector_data = {{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}} (b, g, r)
            // nibble `sector` of each constant, lowest nibble = sector 0
            const int kb = (0x200311 >> (4 * sector)) & 15;
            const int kg = (0x112003 >> (4 * sector)) & 15;
            const int kr = (0x031120 >> (4 * sector)) & 15;
            Bc = tab[kb]; G = tab[kg]; R = tab[kr];
        }
        d[3 * i]     = (unsigned char)min(max((int)rintf(R * 255.f), 0), 255);
        d[3 * i + 1] = (unsigned char)min(max((int)rintf(G * 255.f), 0), 255);
        d[3 * i + 2] = (unsigned char)min(max((int)rintf(Bc * 255.f), 0), 255);
    }
}

// ---- steps 2-4 ---------------------------------------------------------------------------------------------------------------
// One thread per canvas pixel of one image (grid.y = image).  A tap (x, y) of the (H1, W1) intermediate, border-replicated, is
// source pixel (x' - left, y - top) with x' = flip ? W1 - 1 - x : x, or the 128 pad when that falls outside the source.
__global__ __launch_bounds__(256) void resample_kernel(const unsigned char* __restrict__ ws, long long src_bytes,
                                                       const long long* __restrict__ src_offsets,
                                                       const long long* __restrict__ ws_offsets, long long ws_span,
                                                       const int* __restrict__ hw, const double* __restrict__ params,
                                                       float* __restrict__ out, int OH, int OW, int* __restrict__ status) {
    const int b = blockIdx.y;
    const int px = blockIdx.x * blockDim.x + threadIdx.x;
    AugGeom g;
    int code = aug_geometry(params + 8 * (size_t)b, hw[2 * b], hw[2 * b + 1], OH, OW, g);
    const long long wo = ws_offsets[b];
    if (!code && !aug_in_bounds(src_offsets[b], src_bytes, wo, ws_span, (long long)g.H * g.W * 3)) code = YV3_EINVAL;
    if (blockIdx.x == 0 && threadIdx.x == 0) status[b] = code;
    if (px >= OH * OW) return;
    const size_t plane = (size_t)OH * OW;
    float* o = out + (size_t)b * 3 * plane + px;
    if (code) { o[0] = 0.f; o[plane] = 0.f; o[2 * plane] = 0.f; return; }
    const int oy = px / OW, ox = px - oy * OW;
    int rgb[3] = {128, 128, 128};
    const int bx = ox - g.xp, by = oy - g.yp;
    if (bx >= 0 && bx < g.rw && by >= 0 && by < g.rh) {
        const unsigned char* img = ws + wo;
        int ix, iy, ax[4], ay[4];
        float fx, fy;
        cv_coord(bx, g.scale_x, ix, fx);
        cv_coord(by, g.scale_y, iy, fy);
        cv_cubic_coeffs(fx, ax);
        cv_cubic_coeffs(fy, ay);
        int sx[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int xx = min(max(ix - 1 + i, 0), g.W1 - 1);
            sx[i] = (g.flip ? g.W1 - 1 - xx : xx) - g.left;
        }
        int acc[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int sy = min(max(iy - 1 + j, 0), g.H1 - 1) - g.top;
            const bool row_in = sy >= 0 && sy < g.H;
            int row[3] = {0, 0, 0};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int q[3] = {128, 128, 128};
                if (row_in && sx[i] >= 0 && sx[i] < g.W) {
                    const unsigned char* pp = img + ((size_t)sy * g.W + sx[i]) * 3;
                    q[0] = pp[0]; q[1] = pp[1]; q[2] = pp[2];
                }
                row[0] += ax[i] * q[0]; row[1] += ax[i] * q[1]; row[2] += ax[i] * q[2];
            }
            acc[0] += ay[j] * row[0]; acc[1] += ay[j] * row[1]; acc[2] += ay[j] * row[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = min(max((acc[c] + (1 << 21)) >> 22, 0), 255);   // FixedPtCast<int,uchar,22>
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = (float)rgb[c] / 255.f;                       // ToTensor: .float() / 255.0
}

// ---- labels ------------------------------------------------------------------------------------------------------------------
// One wave per image.  Rows are taken 64 at a time; a ballot orders the kept rows of a chunk, so the target keeps input order.
__global__ __launch_bounds__(64) void labels_kernel(const double* __restrict__ labels, int T, const int* __restrict__ hw,
                                                    const double* __restrict__ params, float* __restrict__ target, int max_rows,
                                                    int OH, int OW, int* __restrict__ status) {
    const int b = blockIdx.x, lane = threadIdx.x;
    AugGeom g;
    const int code = aug_geometry(params + 8 * (size_t)b, hw[2 * b], hw[2 * b + 1], OH, OW, g);
    if (lane == 0) status[b] = code;
    float* tg = target + (size_t)b * max_rows * 5;
    int count = 0;
    // bbs_clip's bound: `width - np.finfo(np.float32).eps` with a python int width is a float32 scalar operation
    const double xmax = (double)((float)OW - 1.1920928955078125e-07f), ymax = (double)((float)OH - 1.1920928955078125e-07f);
    for (int base = 0; !code && base < T && count < max_rows; base += 64) {
        const int r = base + lane;
        bool keep = false;
        double x1 = 0, y1 = 0, x2 = 0, y2 = 0, cls = 0;
        if (r < T) {
            const double* L = labels + ((size_t)b * T + r) * 5;
            cls = L[0];
            const double cx = L[1], cy = L[2], w = L[3], h = L[4];
            // BoundingBoxConverter.convert: relative cxcywh -> x1y1x2y2, then * (W, H)
            x1 = (cx - w / 2) * g.W; x2 = (cx + w / 2) * g.W;
            y1 = (cy - h / 2) * g.H; y2 = (cy + h / 2) * g.H;
            if (x2 > x1 && y2 > y1) {                                       // label_np_to_bbs
                x1 += g.left; x2 += g.left; y1 += g.top; y2 += g.top;       // CropAndPad
                if (g.flip) {                                               // Fliplr: (width - 1) - x, corners swapped
                    const double f1 = (double)(g.W1 - 1) - x2, f2 = (double)(g.W1 - 1) - x1;
                    x1 = f1; x2 = f2;
                }
                x1 = x1 * g.rw / g.W1 + g.xp; x2 = x2 * g.rw / g.W1 + g.xp;  // IaaLetterbox
                y1 = y1 * g.rh / g.H1 + g.yp; y2 = y2 * g.rh / g.H1 + g.yp;
                const double area = (y2 - y1) * (x2 - x1);                   // bbs_remove_cut_out(., 0.1)
                const double c1 = fmin(fmax(x1, 0.0), xmax), c2 = fmin(fmax(x2, 0.0), xmax);
                const double d1 = fmin(fmax(y1, 0.0), ymax), d2 = fmin(fmax(y2, 0.0), ymax);
                keep = (c2 - c1) * (d2 - d1) / area > 0.1;
                x1 = c1; x2 = c2; y1 = d1; y2 = d2;
            }
        }
        const unsigned long long m = __ballot(keep);
        const int slot = count + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && slot < max_rows) {                                      // x1y1x2y2 -> cxcywh, / (OW, OH) (ToTensor's fill)
            const double bw = x2 - x1, bh = y2 - y1;
            float* o = tg + (size_t)slot * 5;
            o[0] = (float)cls;
            o[1] = (float)((x1 + bw / 2) / OW);
            o[2] = (float)((y1 + bh / 2) / OH);
            o[3] = (float)(bw / OW);
            o[4] = (float)(bh / OH);
        }
        count += __popcll(m);
    }
    count = min(count, max_rows);
    for (int i = count * 5 + lane; i < max_rows * 5; i += 64) tg[i] = 0.f;
}

}  // namespace

extern "C" size_t yv3_augment_workspace_bytes(long long src_bytes) {
    return src_bytes > 0 ? (size_t)src_bytes : 0;
}

extern "C" int yv3_augment_images_from(const unsigned char* src, long long src_bytes, const long long* src_offsets,
                                       const long long* ws_offsets, long long ws_span, const int* hw, const double* params, int B,
                                       float* out, int out_h, int out_w, void* workspace, size_t workspace_bytes, int* status,
                                       void* stream) {
    if (!src || !src_offsets || !ws_offsets || !hw || !params || !out || !workspace || !status) return YV3_EINVAL;
    if (src_bytes <= 0 || ws_span <= 0 || B <= 0 || out_h <= 0 || out_w <= 0 || B > 65535) return YV3_EINVAL;
    if ((long long)out_h * out_w > (1LL << 30)) return YV3_ESHAPE;
    if (workspace_bytes < (size_t)ws_span) return YV3_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    // ~4 waves of work per CU in all, at most one block per 256 source pixels of a 640x480 image
    const int per_image = max(1, min(1200, yv3_num_cu() * 8 / B));
    hipLaunchKernelGGL(hsv_kernel, dim3(per_image, B), dim3(256), 0, s, src, src_bytes, src_offsets, ws_offsets, ws_span, hw, params,
                       out_h, out_w, (unsigned char*)workspace);
    YV3_CHECK_LAUNCH();
    hipLaunchKernelGGL(resample_kernel, dim3(yv3_ceil_div((long long)out_h * out_w, 256), B), dim3(256), 0, s,
                       (const unsigned char*)workspace, src_bytes, src_offsets, ws_offsets, ws_span, hw, params, out, out_h, out_w,
                       status);
    YV3_CHECK_LAUNCH();
    return 0;
}

// The packed form: the colour copy of image b lives at its source's own offset, in a workspace as large as the sources.
extern "C" int yv3_augment_images(const unsigned char* src, long long src_bytes, const long long* offsets, const int* hw,
                                  const double* params, int B, float* out, int out_h, int out_w,
                                  void* workspace, size_t workspace_bytes, int* status, void* stream) {
    return yv3_augment_images_from(src, src_bytes, offsets, offsets, src_bytes, hw, params, B, out, out_h, out_w, workspace,
                                   workspace_bytes, status, stream);
}

extern "C" int yv3_augment_labels(const double* labels, int B, int T, const int* hw, const double* params,
                                  float* target, int max_rows, int out_h, int out_w, int* status, void* stream) {
    if ((!labels && T > 0) || !hw || !params || !target || !status) return YV3_EINVAL;
    if (B <= 0 || T < 0 || max_rows <= 0 || out_h <= 0 || out_w <= 0) return YV3_EINVAL;
    hipLaunchKernelGGL(labels_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, labels, T, hw, params, target, max_rows,
                       out_h, out_w, status);
    YV3_CHECK_LAUNCH();
    return 0;
}
