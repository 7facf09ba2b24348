// YOLO training loss of one head and its gradient with respect to the head logits (reference yololayer.py:64-95 with
// build_target_tensor, yololayer.py:107-172), all on the device.  The reference builds nine mask / target tensors on the CPU
// with a Python loop over images and GT rows; here that loop is three launches that read the logits once:
//
//   rows_kernel   one workgroup per image: the valid-row prefix, per-row validation, grid cell, best of the nine anchors,
//                 target offsets, nCorrect / nGT, and a per-cell "last row" map (atomicMax of the row index: the last row on a
//                 cell wins whatever the thread order, as the reference's sequential overwrites do)
//   cells_kernel  one thread per (image, anchor, pixel): ignore mask against every valid GT of the image (in LDS) and the six
//                 loss terms, reading the 5 box / conf logits of every cell and the class logits of object cells only; then,
//                 optionally, dL/dlogits for all 5+C channels of the workgroup's cells, written cooperatively in the order of the
//                 unit stride (channel-fastest for NHWC rows, cell-fastest for NCHW planes); per-workgroup fp64 partial sums
//   final_kernel  one workgroup: the partials, counts and status bits in a fixed order
//
// Arithmetic restates torch's fp32 CPU kernels op for op (this file is compiled with -ffp-contract=off): MSELoss(sum)/2 and its
// backward 2*(p-t)*0.5, BCELoss(sum) with each log clamped at -100 and its backward (x-y)/max((1-x)*x, 1e-12), sigmoid's
// backward (g*(1-y))*y.  Nothing is simplified to "sigmoid - target": the two differ once a logit saturates.  Sums are fp64,
// per thread in channel order, per workgroup in a fixed tree, then over workgroups in a fixed order: two identical calls give
// identical bits, and no float atomics are used.  fp32 denormals are kept (a saturated component can be ~1e-39).
#include "yv3_common.h"

namespace {

constexpr int TPB = 256;
constexpr int ST_EINVAL = 1, ST_ELIMIT = 2;     // per-image status bits (workspace)

struct RowRec {
    float gx, gy, gw, gh;        // the GT box in this scale's grid units (NaN for an invalid row: it then matches nothing)
    int cell;                    // (anchor*H + gj)*W + gi when the best anchor is in this head's mask, else -1
    int cls;
    float m, tx, ty, tw, th;     // box_coord_mask and the target offsets (cell >= 0 only)
    int pad[2];
};

struct Args {
    const float* x;
    float* grad;
    long long sb, sp, sc;
    const float* target;
    int B, H, W, T, C, Tc;
    float aw_all[9], ah_all[9];  // the nine anchors / stride, fp32 (torch: FloatTensor(anchors) / stride)
    int mask[3];
    RowRec* rows;                // [B][Tc]
    int* nrows;                  // [B]
    int* img;                    // [B][3]: status bits, nCorrect, nGT
    int* cellmap;                // [B][3*H*W]
    double* partials;            // [nblk][6]
    int nblk;
    double* sums;
    int* counts;
    int* status;
};

__device__ inline float sigmoid(float t) { return 1.f / (1.f + expf(-t)); }

// bbox_iou(b1, b2, mode="cxcywh") of the reference (utils.py), one pair, fp32 in its operation order
__device__ inline float iou_cxcywh(float ax, float ay, float aw, float ah, float bx, float by, float bw, float bh) {
    const float ax1 = ax - aw / 2, ax2 = ax + aw / 2, ay1 = ay - ah / 2, ay2 = ay + ah / 2;
    const float bx1 = bx - bw / 2, bx2 = bx + bw / 2, by1 = by - bh / 2, by2 = by + bh / 2;
    const float ix1 = fmaxf(ax1, bx1), iy1 = fmaxf(ay1, by1), ix2 = fminf(ax2, bx2), iy2 = fminf(ay2, by2);
    const float inter = fmaxf(ix2 - ix1, 0.f) * fmaxf(iy2 - iy1, 0.f);
    const float a1 = (ax2 - ax1) * (ay2 - ay1), a2 = (bx2 - bx1) * (by2 - by1);
    return inter / (a1 + a2 - inter);
}

__device__ inline float clamp_log(float v) { return v < -100.f ? -100.f : v; }          // std::max(v, -100.f)

// torch's binary_cross_entropy element and its input gradient (grad_output 1)
__device__ inline float bce(float x, float y) { return (y - 1.f) * clamp_log(log1pf(-x)) - y * clamp_log(logf(x)); }
__device__ inline float bce_grad(float x, float y) {
    const float d = (1.f - x) * x;
    return (x - y) / (d < 1e-12f ? 1e-12f : d);
}

__global__ __launch_bounds__(TPB) void rows_kernel(const Args a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int HW = a.H * a.W;
    int* cmap = a.cellmap + (long long)b * 3 * HW;
    for (int i = tid; i < 3 * HW; i += TPB) cmap[i] = -1;

    // valid rows: the prefix before the first row whose sum is 0 (yololayer.py:127-128, `break`)
    __shared__ int s_first, s_bits, s_correct, s_gt;
    if (tid == 0) { s_first = a.T; s_bits = 0; s_correct = 0; s_gt = 0; }
    __syncthreads();
    const float* tg = a.target + (long long)b * a.T * 5;
    for (int t = tid; t < a.T; t += TPB) {
        const float* r = tg + (long long)t * 5;
        if ((((r[0] + r[1]) + r[2]) + r[3]) + r[4] == 0.f) atomicMin(&s_first, t);
    }
    __syncthreads();
    int n = s_first;
    if (n > a.Tc) {                                       // more valid rows than YV3_YOLO_LOSS_MAX_ROWS
        if (tid == 0) { a.nrows[b] = 0; a.img[3 * b] = ST_ELIMIT; a.img[3 * b + 1] = 0; a.img[3 * b + 2] = 0; }
        return;
    }
    const float fW = (float)a.W, fH = (float)a.H;
    RowRec* recs = a.rows + (long long)b * a.Tc;
    for (int t = tid; t < n; t += TPB) {
        const float* r = tg + (long long)t * 5;
        const float cls = r[0], cx = r[1], cy = r[2], w = r[3], h = r[4];
        RowRec rec;
        rec.cell = -1; rec.cls = 0; rec.m = rec.tx = rec.ty = rec.tw = rec.th = 0.f; rec.pad[0] = rec.pad[1] = 0;
        const float gx = cx * fW, gy = cy * fH, gw = w * fW, gh = h * fH;
        const float m2 = 2.f - w * h;
        // the reference fails on these rows (IndexError, a wrapped index, or math.sqrt of a negative number)
        const bool bad = !(cls >= 0.f && cx >= 0.f && cy >= 0.f && w >= 0.f && h >= 0.f) || !(cls < (float)a.C) ||
                         !(gx < fW) || !(gy < fH) || !(m2 >= 0.f) || !(gw < 3.0e38f) || !(gh < 3.0e38f);
        if (bad) {
            atomicOr(&s_bits, ST_EINVAL);
            rec.gx = rec.gy = rec.gw = rec.gh = __builtin_nanf("");
            recs[t] = rec;
            continue;
        }
        rec.gx = gx; rec.gy = gy; rec.gw = gw; rec.gh = gh;
        rec.cls = (int)cls;
        // best of all nine anchors by zero-centred IoU, first index on ties (yololayer.py:141-144)
        int best = 0;
        float best_iou = iou_cxcywh(0.f, 0.f, a.aw_all[0], a.ah_all[0], 0.f, 0.f, gw, gh);
        for (int k = 1; k < 9; ++k) {
            const float v = iou_cxcywh(0.f, 0.f, a.aw_all[k], a.ah_all[k], 0.f, 0.f, gw, gh);
            if (v > best_iou) { best_iou = v; best = k; }
        }
        const int an = best == a.mask[0] ? 0 : best == a.mask[1] ? 1 : best == a.mask[2] ? 2 : -1;
        if (an >= 0) {
            const int gi = (int)gx, gj = (int)gy;
            rec.cell = (an * a.H + gj) * a.W + gi;
            rec.m = sqrtf(m2);
            rec.tx = gx - (float)gi;
            rec.ty = gy - (float)gj;
            rec.tw = logf(gw / a.aw_all[best] + 1e-16f);
            rec.th = logf(gh / a.ah_all[best] + 1e-16f);
            // nCorrect: the prediction at that cell against this GT (yololayer.py:150-155)
            const float* px = a.x + (long long)b * a.sb + (long long)(gj * a.W + gi) * a.sp + (long long)an * (5 + a.C) * a.sc;
            const float bx = sigmoid(px[0]) + (float)gi, by = sigmoid(px[a.sc]) + (float)gj;
            const float bw = expf(px[2 * a.sc]) * a.aw_all[best], bh = expf(px[3 * a.sc]) * a.ah_all[best];
            if (iou_cxcywh(gx, gy, gw, gh, bx, by, bw, bh) > 0.5f) atomicAdd(&s_correct, 1);
            atomicAdd(&s_gt, 1);
        }
        recs[t] = rec;
    }
    __syncthreads();                                      // (the cell map's -1 fill is complete before any row claims a cell)
    for (int t = tid; t < n; t += TPB) {
        const int c = recs[t].cell;
        if (c >= 0) atomicMax(&cmap[c], t);
    }
    if (tid == 0) { a.nrows[b] = n; a.img[3 * b] = s_bits; a.img[3 * b + 1] = s_correct; a.img[3 * b + 2] = s_gt; }
}

// tcls of an object cell: 1 when any row on the cell (all have indices <= last) has class k (the union of their classes).
// c0 / nm: the class of the cell's first row and the number of its rows (one row, the common case, needs no search)
__device__ inline float class_target(const int* s_cell, const int* s_cls, int last, int idx, int k, int c0, int nm) {
    if (nm == 1) return k == c0 ? 1.f : 0.f;
    for (int r = 0; r <= last; ++r)
        if (s_cell[r] == idx && s_cls[r] == k) return 1.f;
    return 0.f;
}

template <bool GRAD>
__global__ __launch_bounds__(TPB) void cells_kernel(const Args a) {
    __shared__ float4 s_box[YV3_YOLO_LOSS_MAX_ROWS];
    __shared__ int s_cell[YV3_YOLO_LOSS_MAX_ROWS];
    __shared__ int s_cls[YV3_YOLO_LOSS_MAX_ROWS];
    __shared__ double s_red[6][TPB];
    __shared__ float s_g[5][GRAD ? TPB : 1];      // dL/d(x, y, w, h, conf logits) of the workgroup's cells
    __shared__ int s_last[TPB];                   // their last row, -1: no object (or no cell)
    __shared__ int s_c0[TPB], s_nm[TPB];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int HW = a.H * a.W;
    const int n = a.nrows[b];
    const RowRec* recs = a.rows + (long long)b * a.Tc;
    for (int t = tid; t < n; t += TPB) {
        const RowRec r = recs[t];
        s_box[t] = make_float4(r.gx, r.gy, r.gw, r.gh);
        s_cell[t] = r.cell;
        s_cls[t] = r.cls;
    }
    __syncthreads();

    double acc[6] = {0, 0, 0, 0, 0, 0};
    const int idx = blockIdx.x * TPB + tid;
    s_last[tid] = -1;
    if (idx < 3 * HW) {
        const int an = idx / HW, p = idx - an * HW;
        const int gi = p % a.W, gj = p / a.W;
        const long long off = (long long)b * a.sb + (long long)p * a.sp + (long long)an * (5 + a.C) * a.sc;
        const float* xp = a.x + off;
        const float t0 = xp[0], t1 = xp[a.sc], t2 = xp[2 * a.sc], t3 = xp[3 * a.sc], t4 = xp[4 * a.sc];
        const float sx = sigmoid(t0), sy = sigmoid(t1), conf = sigmoid(t4);
        const float aw = a.aw_all[a.mask[an]], ah = a.ah_all[a.mask[an]];
        const float bx = sx + (float)gi, by = sy + (float)gj, bw = expf(t2) * aw, bh = expf(t3) * ah;
        // ignore mask: IoU > 0.7 with any valid GT of the image, whichever head that GT belongs to (yololayer.py:135-139)
        float noobj = 1.f;
        for (int r = 0; r < n; ++r) {
            const float4 g = s_box[r];
            if (iou_cxcywh(bx, by, bw, bh, g.x, g.y, g.z, g.w) > 0.7f) { noobj = 0.f; break; }
        }
        const int last = a.cellmap[(long long)b * 3 * HW + idx];
        const float obj = last >= 0 ? 1.f : 0.f;
        float m = 0.f, tx = 0.f, ty = 0.f, tw = 0.f, th = 0.f;
        int c0 = 0, nm = 0;
        if (last >= 0) {
            const RowRec& r = recs[last]; m = r.m; tx = r.tx; ty = r.ty; tw = r.tw; th = r.th;
            for (int q = 0; q <= last; ++q)
                if (s_cell[q] == idx) { if (nm == 0) c0 = s_cls[q]; ++nm; }
        }
        // loss_x .. loss_h: sum((p*m - t*m)^2) / 2 (the halving is applied to the sums); backward 2*d*0.5, times m
        const float dx = sx * m - tx * m, dy = sy * m - ty * m, dw = t2 * m - tw * m, dh = t3 * m - th * m;
        acc[0] = (double)(dx * dx); acc[1] = (double)(dy * dy); acc[2] = (double)(dw * dw); acc[3] = (double)(dh * dh);
        // loss_conf: BCE(conf*obj, obj) + BCE(conf*noobj, 0)
        const float x1 = conf * obj, x2 = conf * noobj;
        acc[4] = (double)bce(x1, obj) + (double)bce(x2, 0.f);
        s_last[tid] = last;
        s_c0[tid] = c0;
        s_nm[tid] = nm;
        if (GRAD) {
            s_g[0][tid] = (((dx * 2.f) * 0.5f) * m * (1.f - sx)) * sx;
            s_g[1][tid] = (((dy * 2.f) * 0.5f) * m * (1.f - sy)) * sy;
            s_g[2][tid] = ((dw * 2.f) * 0.5f) * m;
            s_g[3][tid] = ((dh * 2.f) * 0.5f) * m;
            const float gc = bce_grad(x1, obj) * obj + bce_grad(x2, 0.f) * noobj;
            s_g[4][tid] = (gc * (1.f - conf)) * conf;
        }
    }
    __syncthreads();
    // loss_cls, BCE(cls, tcls) over object cells, and (GRAD) the gradient of every channel: the workgroup's (cell, channel)
    // items in the order of the unit stride, so that one object cell's classes are spread over the lanes
    {
        const int cell0 = blockIdx.x * TPB;
        const int ncell = 3 * HW - cell0 < TPB ? 3 * HW - cell0 : TPB;
        const int A = 5 + a.C;
        const int c_lo = GRAD ? 0 : 5, nch = A - c_lo;
        const bool chan_fast = a.sc == 1;
        for (int i = tid; i < ncell * nch; i += TPB) {
            const int cl = chan_fast ? i / nch : i % ncell;
            const int c = c_lo + (chan_fast ? i - cl * nch : i / ncell);
            const int last = s_last[cl];
            if (!GRAD && last < 0) continue;
            const int cidx = cell0 + cl;
            const int an = cidx / HW, p = cidx - an * HW;
            const long long off = (long long)b * a.sb + (long long)p * a.sp + (long long)(an * A + c) * a.sc;
            float g = 0.f;
            if (c < 5) {
                g = s_g[GRAD ? c : 0][GRAD ? cl : 0];
            } else if (last >= 0) {
                const float s = sigmoid(a.x[off]);
                const float y = class_target(s_cell, s_cls, last, cidx, c - 5, s_c0[cl], s_nm[cl]);
                acc[5] += (double)bce(s, y);
                g = (bce_grad(s, y) * (1.f - s)) * s;
            }
            if (GRAD) a.grad[off] = g;
        }
    }
    // fixed-order workgroup reduction
    for (int j = 0; j < 6; ++j) s_red[j][tid] = acc[j];
    __syncthreads();
    for (int w = TPB / 2; w > 0; w >>= 1) {
        if (tid < w)
            for (int j = 0; j < 6; ++j) s_red[j][tid] += s_red[j][tid + w];
        __syncthreads();
    }
    if (tid < 6) a.partials[(long long)(blockIdx.y * gridDim.x + blockIdx.x) * 6 + tid] = s_red[tid][0];
}

__global__ __launch_bounds__(TPB) void final_kernel(const Args a) {
    __shared__ double s_red[6][TPB];
    __shared__ int s_cnt[3][TPB];
    const int tid = threadIdx.x;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int i = tid; i < a.nblk; i += TPB)
        for (int j = 0; j < 6; ++j) acc[j] += a.partials[(long long)i * 6 + j];
    int bits = 0, nc = 0, ng = 0;
    for (int i = tid; i < a.B; i += TPB) { bits |= a.img[3 * i]; nc += a.img[3 * i + 1]; ng += a.img[3 * i + 2]; }
    for (int j = 0; j < 6; ++j) s_red[j][tid] = acc[j];
    s_cnt[0][tid] = bits; s_cnt[1][tid] = nc; s_cnt[2][tid] = ng;
    __syncthreads();
    for (int w = TPB / 2; w > 0; w >>= 1) {
        if (tid < w) {
            for (int j = 0; j < 6; ++j) s_red[j][tid] += s_red[j][tid + w];
            s_cnt[0][tid] |= s_cnt[0][tid + w];
            s_cnt[1][tid] += s_cnt[1][tid + w];
            s_cnt[2][tid] += s_cnt[2][tid + w];
        }
        __syncthreads();
    }
    if (tid < 6) a.sums[tid] = s_red[tid][0] * (tid < 4 ? 0.5 : 1.0);
    if (tid == 0) {
        a.counts[0] = s_cnt[1][0];
        a.counts[1] = s_cnt[2][0];
        a.status[0] = (s_cnt[0][0] & ST_EINVAL) ? YV3_EINVAL : (s_cnt[0][0] & ST_ELIMIT) ? YV3_ELIMIT : 0;
    }
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Layout {
    size_t rows, nrows, img, cellmap, partials, total;
    int Tc, nblk_x;
};

bool layout(int B, int H, int W, int T, Layout* L) {
    if (B <= 0 || H <= 0 || W <= 0 || T < 0) return false;
    const long long cells = 3LL * H * W;
    if (cells * B >= (1LL << 31)) return false;
    L->Tc = T < YV3_YOLO_LOSS_MAX_ROWS ? T : YV3_YOLO_LOSS_MAX_ROWS;
    L->nblk_x = (int)((cells + TPB - 1) / TPB);
    size_t o = 0;
    L->rows = o;     o = align256(o + (size_t)B * (L->Tc > 0 ? L->Tc : 1) * sizeof(RowRec));
    L->nrows = o;    o = align256(o + (size_t)B * sizeof(int));
    L->img = o;      o = align256(o + (size_t)B * 3 * sizeof(int));
    L->cellmap = o;  o = align256(o + (size_t)B * cells * sizeof(int));
    L->partials = o; o = align256(o + (size_t)B * L->nblk_x * 6 * sizeof(double));
    L->total = o + 256;                                   // (room to align an unaligned base)
    return true;
}

// the element offsets (b, p, c) -> b*sb + p*sp + c*sc of a [B][P][Cc] index space address distinct elements
bool injective(long long B, long long P, long long Cc, long long sb, long long sp, long long sc) {
    long long st[3] = {sb, sp, sc}, ex[3] = {B, P, Cc};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if ((ex[j] > 1 && st[j] < st[i]) || ex[i] == 1) { long long t = st[i]; st[i] = st[j]; st[j] = t; t = ex[i]; ex[i] = ex[j]; ex[j] = t; }
    long long span = 1;
    for (int i = 0; i < 3; ++i) {
        if (ex[i] == 1) continue;
        if (st[i] < span) return false;
        span = st[i] * ex[i];
    }
    return true;
}

}  // namespace

extern "C" size_t yv3_yolo_loss_workspace_bytes(int B, int H, int W, int T) {
    Layout L;
    return layout(B, H, W, T, &L) ? L.total : 0;
}

extern "C" int yv3_yolo_loss(const yv3_yolo_loss_desc* d, void* ws, size_t ws_bytes, void* stream) {
    if (!d || !d->logits || !d->sums || !d->counts || !d->status || !ws) return YV3_EINVAL;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->T < 0 || d->num_class <= 0) return YV3_EINVAL;
    if (d->T > 0 && !d->target) return YV3_EINVAL;
    if (!(d->img_dim_h > 0.f) || !(d->img_dim_h < 3.0e38f)) return YV3_EINVAL;
    for (int i = 0; i < 18; ++i)
        if (!(d->anchors[i] > 0.f) || !(d->anchors[i] < 3.0e38f)) return YV3_EINVAL;
    for (int i = 0; i < 3; ++i)
        if (d->mask[i] < 0 || d->mask[i] >= 9) return YV3_EINVAL;
    const long long P = (long long)d->H * d->W, Cc = 3LL * (5 + d->num_class);
    if (d->stride_b <= 0 || d->stride_p <= 0 || d->stride_c <= 0) return YV3_ESHAPE;
    if (!injective(d->B, P, Cc, d->stride_b, d->stride_p, d->stride_c)) return YV3_ESHAPE;
    Layout L;
    if (!layout(d->B, d->H, d->W, d->T, &L)) return YV3_ESHAPE;
    if (ws_bytes < L.total) return YV3_EWORKSPACE;

    Args a;
    a.x = d->logits; a.grad = d->grad;
    a.sb = d->stride_b; a.sp = d->stride_p; a.sc = d->stride_c;
    a.target = d->target;
    a.B = d->B; a.H = d->H; a.W = d->W; a.T = d->T; a.C = d->num_class; a.Tc = L.Tc;
    const float stride = d->img_dim_h / (float)d->H;      // yololayer.py:36; anchors: FloatTensor / stride, fp32
    for (int k = 0; k < 9; ++k) { a.aw_all[k] = d->anchors[2 * k] / stride; a.ah_all[k] = d->anchors[2 * k + 1] / stride; }
    for (int i = 0; i < 3; ++i) a.mask[i] = d->mask[i];
    char* base = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    a.rows = (RowRec*)(base + L.rows);
    a.nrows = (int*)(base + L.nrows);
    a.img = (int*)(base + L.img);
    a.cellmap = (int*)(base + L.cellmap);
    a.partials = (double*)(base + L.partials);
    a.nblk = d->B * L.nblk_x;
    a.sums = d->sums; a.counts = d->counts; a.status = d->status;

    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(rows_kernel, dim3(d->B), dim3(TPB), 0, s, a);
    YV3_CHECK_LAUNCH();
    if (d->grad) hipLaunchKernelGGL(cells_kernel<true>, dim3(L.nblk_x, d->B), dim3(TPB), 0, s, a);
    else         hipLaunchKernelGGL(cells_kernel<false>, dim3(L.nblk_x, d->B), dim3(TPB), 0, s, a);
    YV3_CHECK_LAUNCH();
    hipLaunchKernelGGL(final_kernel, dim3(1), dim3(TPB), 0, s, a);
    YV3_CHECK_LAUNCH();
    return 0;
}
