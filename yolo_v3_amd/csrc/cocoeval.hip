// COCO bbox evaluation (pycocotools 2.0.x COCOeval.evaluate + accumulate, iouType 'bbox', useCats 1) on the GPU.
//
// Stages, all on the caller's stream ("COCO bbox mAP"):
//   1. cc_count / cc_scan / cc_scatter : GTs and dets grouped by g = cat * n_img + img (category-major, so a category's
//      groups are one contiguous range).  The scatter takes slots with atomics, so the order INSIDE a group is arbitrary;
//      every later stage orders a group's members by keys that include the original index, which makes the result
//      independent of that order.
//   2. cc_match : one wave per group.  GTs in file order; dets ranked by (-score, file position) = pycocotools' stable
//      mergesort; the first maxDets[-1] of them run the greedy matching of evaluateImg, lane L = (t, a) = (L / A, L % A),
//      IoUs recomputed in float64 exactly as maskApi bbIou.  Per kept det: ballot masks "dtm != 0" and "dtIgnore" over
//      (t, a); per (category, area): the count of non-ignored GTs.
//   3. cc_order : the kept dets of each category ranked by (score desc, group position), i.e. (score desc, image, in-group
//      rank): pycocotools' stable sort of the per-image concatenation.  maxDet only filters by in-group rank, so this one
//      order serves every (t, a, m).
//   4. cc_accum : one wave per (t, k, a, m): masked prefix counts, float64 rc / pr in pycocotools' operation order, the
//      suffix-max envelope and searchsorted(rc, recThrs, 'left').
// The file is compiled with -ffp-contract=off: every float64 operation rounds separately, as numpy's do.
#include "yv3_common.h"

#define CC_MAX_GT 256            // GTs per (image, category) group held by one wave
#define CC_MAX_DET 1024          // maxDets[-1]
#define CC_MAX_TA 64             // len(iouThrs) * len(areaRng): one lane each
#define CC_MAX_REC 128           // len(recThrs)
#define CC_NOT_KEPT 0x7fffffff   // rank of a det past maxDets[-1]

static inline size_t cc_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct cc_ws {
    int *gcnt, *dcnt, *goff, *doff, *gperm, *dperm, *npig, *prank, *srank;
    double *pscore, *sscore;
    unsigned long long *pmm, *pig, *smm, *sig;
};

static size_t cc_layout(long long n_gt, long long n_det, long long n_groups, long long n_ka, char* base, cc_ws* w) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += cc_align(bytes); return p; };
    cc_ws t;
    t.gcnt = (int*)take(sizeof(int) * n_groups);
    t.dcnt = (int*)take(sizeof(int) * n_groups);
    t.npig = (int*)take(sizeof(int) * n_ka);
    const size_t zeroed = off;                                   // the counters above start at 0
    t.goff = (int*)take(sizeof(int) * (n_groups + 1));
    t.doff = (int*)take(sizeof(int) * (n_groups + 1));
    t.gperm = (int*)take(sizeof(int) * n_gt);
    t.dperm = (int*)take(sizeof(int) * n_det);
    t.prank = (int*)take(sizeof(int) * n_det);
    t.srank = (int*)take(sizeof(int) * n_det);
    t.pscore = (double*)take(sizeof(double) * n_det);
    t.sscore = (double*)take(sizeof(double) * n_det);
    t.pmm = (unsigned long long*)take(8 * n_det);
    t.pig = (unsigned long long*)take(8 * n_det);
    t.smm = (unsigned long long*)take(8 * n_det);
    t.sig = (unsigned long long*)take(8 * n_det);
    if (w) *w = t;
    return base ? zeroed : off;
}

__global__ void cc_zero(int* p, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = 0;
}

// An entry takes part when 0 <= img < n_img and 0 <= cat < n_cat; anything else is dropped (never indexes out of range).
__device__ static inline bool cc_in(int img, int cat, int n_img, int n_cat) {
    return img >= 0 && cat >= 0 && img < n_img && cat < n_cat;
}

__global__ void cc_count(const int* gimg, const int* gcat, int n_gt, const int* dimg, const int* dcat, int n_det, int n_img,
                         int n_cat, int* gcnt, int* dcnt) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i < n_gt) {
        if (cc_in(gimg[i], gcat[i], n_img, n_cat)) atomicAdd(&gcnt[(long long)gcat[i] * n_img + gimg[i]], 1);
    } else if (i < (long long)n_gt + n_det) {
        const long long j = i - n_gt;
        if (cc_in(dimg[j], dcat[j], n_img, n_cat)) atomicAdd(&dcnt[(long long)dcat[j] * n_img + dimg[j]], 1);
    }
}

// Exclusive scan of cnt[0..n) into off[0..n] (one 1024-thread block per array: blockIdx.x 0 = GTs, 1 = dets); cnt becomes
// the scatter cursor (= off).
__global__ void __launch_bounds__(1024) cc_scan(int* gcnt, int* goff, int* dcnt, int* doff, int n) {
    int* cnt = blockIdx.x ? dcnt : gcnt;
    int* off = blockIdx.x ? doff : goff;
    __shared__ int part[1024];
    const int per = (n + 1023) / 1024, lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += cnt[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {                         // Hillis-Steele inclusive scan of the 1024 partial sums
        const int v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int i = lo; i < hi; ++i) {
        const int c = cnt[i];
        off[i] = run;
        cnt[i] = run;
        run += c;
    }
    if (threadIdx.x == 1023) off[n] = part[1023];
}

__global__ void cc_scatter(const int* gimg, const int* gcat, int n_gt, const int* dimg, const int* dcat, int n_det, int n_img,
                           int n_cat, int* gcur, int* dcur, int* gperm, int* dperm) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i < n_gt) {
        if (cc_in(gimg[i], gcat[i], n_img, n_cat)) gperm[atomicAdd(&gcur[(long long)gcat[i] * n_img + gimg[i]], 1)] = (int)i;
    } else if (i < (long long)n_gt + n_det) {
        const int j = (int)(i - n_gt);
        if (cc_in(dimg[j], dcat[j], n_img, n_cat)) dperm[atomicAdd(&dcur[(long long)dcat[j] * n_img + dimg[j]], 1)] = j;
    }
}

struct cc_params {
    int n_img, n_iou, n_area, max_det;
    long long n_groups;
};

// maskApi bbIou for one (det, gt) pair, float64, same operations in the same order.
__device__ static inline double cc_iou(const double* d, double da, const double* g, double ga, int crowd) {
    const double w = fmin(d[2] + d[0], g[2] + g[0]) - fmax(d[0], g[0]);
    if (w <= 0) return 0.0;
    const double h = fmin(d[3] + d[1], g[3] + g[1]) - fmax(d[1], g[1]);
    if (h <= 0) return 0.0;
    const double i = w * h;
    const double u = crowd ? da : da + ga - i;
    return i / u;
}

__global__ void __launch_bounds__(64) cc_match(cc_params P, const double* gbox, const double* garea, const int* gcrowd,
                                               const long long* gid, const double* dbox, const double* dscore,
                                               const double* iou_thrs, const double* area_rng, cc_ws W, int* status) {
    const long long g = blockIdx.x;
    const int lane = threadIdx.x;
    const int g0 = W.goff[g], ng = W.goff[g + 1] - g0;
    const int d0 = W.doff[g], nd = W.doff[g + 1] - d0;
    if (ng == 0 && nd == 0) return;                              // evaluateImg returns None: no contribution
    if (ng > CC_MAX_GT) {                                        // the caller gets YV3_ELIMIT through *status
        for (int j = lane; j < nd; j += 64) W.prank[d0 + j] = CC_NOT_KEPT;
        if (lane == 0) atomicMin(status, YV3_ELIMIT);
        return;
    }
    __shared__ double sg_box[CC_MAX_GT][4];
    __shared__ double sg_area[CC_MAX_GT];
    __shared__ double sg_ga[CC_MAX_GT];
    __shared__ int sg_crowd[CC_MAX_GT];
    __shared__ int sg_id0[CC_MAX_GT];
    __shared__ double sd_box[CC_MAX_DET][4];
    __shared__ unsigned long long gtm[CC_MAX_GT / 64][64];       // per lane: GTs already matched at its (t, a)

    // GTs in file order: slot = number of the group's GTs with a smaller original index
    for (int j = lane; j < ng; j += 64) {
        const int e = W.gperm[g0 + j];
        int r = 0;
        for (int q = 0; q < ng; ++q) r += W.gperm[g0 + q] < e;
        for (int c = 0; c < 4; ++c) sg_box[r][c] = gbox[4 * (long long)e + c];
        sg_area[r] = garea[e];
        sg_ga[r] = gbox[4 * (long long)e + 2] * gbox[4 * (long long)e + 3];
        sg_crowd[r] = gcrowd[e] != 0;
        sg_id0[r] = gid[e] == 0;
    }
    // dets ranked by (-score, original index); the first max_det are kept, the rest marked past maxDets[-1]
    for (int j = lane; j < nd; j += 64) {
        const int e = W.dperm[d0 + j];
        const double s = dscore[e];
        int r = 0;
        for (int q = 0; q < nd; ++q) {
            const int f = W.dperm[d0 + q];
            const double sf = dscore[f];
            r += sf > s || (sf == s && f < e);
        }
        if (r < P.max_det) {
            for (int c = 0; c < 4; ++c) sd_box[r][c] = dbox[4 * (long long)e + c];
            W.pscore[d0 + r] = s;
            W.prank[d0 + r] = r;
        } else {
            W.prank[d0 + r] = CC_NOT_KEPT;
        }
    }
    for (int w = 0; w < CC_MAX_GT / 64; ++w) gtm[w][lane] = 0;
    __syncthreads();

    const int TA = P.n_iou * P.n_area;
    const bool active = lane < TA;
    const int t = active ? lane / P.n_area : 0, a = active ? lane % P.n_area : 0;
    const double thr = fmin(iou_thrs[t], 1 - 1e-10);
    const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    const int k = (int)(g / P.n_img);
    if (lane < P.n_area) {
        int c = 0;
        for (int j = 0; j < ng; ++j) c += !(sg_crowd[j] || sg_area[j] < lo || sg_area[j] > hi);
        if (c) atomicAdd(&W.npig[k * P.n_area + lane], c);
    }
    const int nkeep = min(nd, P.max_det);
    for (int d = 0; d < nkeep; ++d) {
        const double* db = sd_box[d];
        const double da = db[2] * db[3];
        bool dtm_nz = false, dt_ig = false;
        if (active) {
            double best = thr;
            int m = -1, m_ig = 0;
            // GTs stably sorted by _ignore: the non-ignored ones in file order, then the ignored ones
            for (int pass = 0; pass < 2; ++pass) {
                if (pass == 1 && m > -1 && !m_ig) break;         // a non-ignored match stops at the first ignored GT
                for (int j = 0; j < ng; ++j) {
                    const int ig = sg_crowd[j] || sg_area[j] < lo || sg_area[j] > hi;
                    if (ig != pass) continue;
                    if (((gtm[j >> 6][lane] >> (j & 63)) & 1ull) && !sg_crowd[j]) continue;
                    const double iou = cc_iou(db, da, sg_box[j], sg_ga[j], sg_crowd[j]);
                    if (iou < best) continue;
                    best = iou;
                    m = j;
                    m_ig = ig;
                }
            }
            if (m > -1) {
                dt_ig = m_ig;
                dtm_nz = !sg_id0[m];
                gtm[m >> 6][lane] |= 1ull << (m & 63);
            }
            if (!dtm_nz && (da < lo || da > hi)) dt_ig = true;
        }
        const unsigned long long mm = __ballot(dtm_nz), ig = __ballot(dt_ig);
        if (lane == 0) {
            W.pmm[d0 + d] = mm;
            W.pig[d0 + d] = ig;
        }
    }
}

// Position of every grouped det inside its category's (score desc, position) order; kept dets first.
__global__ void __launch_bounds__(256) cc_order(int n_img, int n_cat, cc_ws W) {
    const int n_total = W.doff[(long long)n_cat * n_img];        // grouped dets; the dropped ones are past this
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 >= n_total) return;
    __shared__ double ts[256];
    __shared__ int tk[256];
    auto cat_of = [&](int q) {                                    // largest k with doff[k * n_img] <= q
        int lo = 0, hi = n_cat - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (W.doff[(long long)mid * n_img] <= q) lo = mid; else hi = mid - 1;
        }
        return lo;
    };
    const int first = blockIdx.x * 256, last = min(n_total, first + 256) - 1;
    const int r0 = W.doff[(long long)cat_of(first) * n_img], r1 = W.doff[(long long)(cat_of(last) + 1) * n_img];
    const bool mine = p < n_total;
    int cs = 0, ce = 0, kept = 0;
    double s = 0;
    if (mine) {
        const int k = cat_of(p);
        cs = W.doff[(long long)k * n_img];
        ce = W.doff[(long long)(k + 1) * n_img];
        kept = W.prank[p] != CC_NOT_KEPT;
        s = W.pscore[p];
    }
    int before = 0;
    for (int b = r0; b < r1; b += 256) {
        const int q = b + threadIdx.x;
        __syncthreads();
        if (q < r1) {
            tk[threadIdx.x] = W.prank[q] != CC_NOT_KEPT;
            ts[threadIdx.x] = W.pscore[q];
        }
        __syncthreads();
        if (mine) {
            const int n = min(256, r1 - b);
            for (int j = 0; j < n; ++j) {
                const int y = b + j;
                if (y < cs || y >= ce) continue;
                const int ky = tk[j];
                bool bef;
                if (ky != kept) bef = ky;
                else if (!kept) bef = y < p;
                else bef = ts[j] > s || (ts[j] == s && y < p);
                before += bef;
            }
        }
    }
    if (mine) {
        const int o = cs + before;
        W.srank[o] = W.prank[p];
        W.sscore[o] = s;
        W.smm[o] = kept ? W.pmm[p] : 0;
        W.sig[o] = kept ? W.pig[p] : 0;
    }
}

__global__ void __launch_bounds__(64) cc_accum(int n_img, int n_cat, int n_iou, int n_area, int n_rec, yv3_cocoeval_desc D,
                                               const double* rec_thrs, cc_ws W) {
    const int lane = threadIdx.x;
    long long id = blockIdx.x;
    const int M = D.n_maxdet;
    const int m = (int)(id % M); id /= M;
    const int a = (int)(id % n_area); id /= n_area;
    const int k = (int)(id % n_cat);
    const int t = (int)(id / n_cat);
    const long long rstride = (long long)n_cat * n_area * M;     // precision / scores [T, R, K, A, M]
    const long long base = (((long long)t * n_rec) * n_cat + k) * n_area * M + (long long)a * M + m;
    const long long rbase = (((long long)t * n_cat + k) * n_area + a) * M + m;   // recall [T, K, A, M]
    const int npig = W.npig[k * n_area + a];
    if (npig == 0) {
        for (int r = lane; r < n_rec; r += 64) D.precision[base + r * rstride] = -1.0, D.scores[base + r * rstride] = -1.0;
        if (lane == 0) D.recall[rbase] = -1.0;
        return;
    }
    const int cs = W.doff[(long long)k * n_img], ce = W.doff[(long long)(k + 1) * n_img];
    const int md = D.max_dets[m];
    const int bit = t * n_area + a;
    const unsigned long long lt = (1ull << lane) - 1ull;
    // pass 1: totals (tps = dtm != 0 & !dtIg, fps = dtm == 0 & !dtIg over the dets within maxDets[m] of their group)
    int nd = 0, TP = 0, FP = 0;
    for (int b = cs; b < ce; b += 64) {
        const int q = b + lane;
        bool v = false, tp = false, fp = false;
        if (q < ce) {
            v = W.srank[q] < md;
            const bool mm = (W.smm[q] >> bit) & 1ull, ig = (W.sig[q] >> bit) & 1ull;
            tp = v && mm && !ig;
            fp = v && !mm && !ig;
        }
        nd += __popcll(__ballot(v));
        TP += __popcll(__ballot(tp));
        FP += __popcll(__ballot(fp));
    }
    if (lane == 0) D.recall[rbase] = nd ? (double)TP / (double)npig : 0.0;
    // pass 2, backwards: rc / pr per position, running suffix max of pr, first position with rc >= recThrs[r]
    __shared__ double c_rc[64], c_env[64], c_sc[64];
    double q0 = 0.0, q1 = 0.0, s0 = 0.0, s1 = 0.0;
    const double thr0 = lane < n_rec ? rec_thrs[lane] : 0.0, thr1 = lane + 64 < n_rec ? rec_thrs[lane + 64] : 0.0;
    double carry = -1.0;
    int tp_after = 0, fp_after = 0;
    const int nchunk = (ce - cs + 63) / 64;
    for (int c = nchunk - 1; c >= 0; --c) {
        const int q = cs + c * 64 + lane;
        bool v = false, tp = false, fp = false;
        double sc = 0.0;
        if (q < ce) {
            v = W.srank[q] < md;
            const bool mm = (W.smm[q] >> bit) & 1ull, ig = (W.sig[q] >> bit) & 1ull;
            tp = v && mm && !ig;
            fp = v && !mm && !ig;
            sc = W.sscore[q];
        }
        const unsigned long long vm = __ballot(v), tm = __ballot(tp), fm = __ballot(fp);
        const int nv = __popcll(vm);
        const int tp_before = TP - tp_after - __popcll(tm), fp_before = FP - fp_after - __popcll(fm);
        const int tpc = tp_before + __popcll(tm & (lt | (1ull << lane)));
        const int fpc = fp_before + __popcll(fm & (lt | (1ull << lane)));
        const int o = __popcll(vm & lt);                          // compact offset inside the chunk
        double pr = -1.0, rc = 0.0;
        if (v) {
            const double tpd = (double)tpc, fpd = (double)fpc;
            rc = tpd / (double)npig;
            pr = tpd / (fpd + tpd + 0x1p-52);
        }
        double env = pr;                                          // suffix max over the chunk's lanes >= this one
        for (int sft = 1; sft < 64; sft <<= 1) {
            const double other = __shfl_down(env, sft, 64);
            if (lane + sft < 64 && other > env) env = other;
        }
        if (carry > env) env = carry;
        __syncthreads();
        if (v) {
            c_rc[o] = rc;
            c_env[o] = env;
            c_sc[o] = sc;
        }
        __syncthreads();
        carry = __shfl(env, 0, 64);
        if (nv) {
            if (lane < n_rec && c_rc[nv - 1] >= thr0) {
                int j = 0;
                while (c_rc[j] < thr0) ++j;
                q0 = c_env[j];
                s0 = c_sc[j];
            }
            if (lane + 64 < n_rec && c_rc[nv - 1] >= thr1) {
                int j = 0;
                while (c_rc[j] < thr1) ++j;
                q1 = c_env[j];
                s1 = c_sc[j];
            }
        }
        tp_after += __popcll(tm);
        fp_after += __popcll(fm);
    }
    if (lane < n_rec) D.precision[base + lane * rstride] = q0, D.scores[base + lane * rstride] = s0;
    if (lane + 64 < n_rec) D.precision[base + (lane + 64) * rstride] = q1, D.scores[base + (lane + 64) * rstride] = s1;
}

static int cc_check(const yv3_cocoeval_desc* d) {
    if (!d) return YV3_EINVAL;
    if (d->n_gt < 0 || d->n_det < 0 || d->n_img <= 0 || d->n_cat <= 0) return YV3_EINVAL;
    if (d->n_iou <= 0 || d->n_rec <= 0 || d->n_area <= 0 || d->n_maxdet <= 0 || d->n_maxdet > YV3_COCO_MAX_MAXDETS) return YV3_EINVAL;
    if (d->n_iou * d->n_area > CC_MAX_TA || d->n_rec > CC_MAX_REC) return YV3_ELIMIT;
    for (int m = 0; m < d->n_maxdet; ++m) {
        if (d->max_dets[m] <= 0) return YV3_EINVAL;
        if (m && d->max_dets[m] < d->max_dets[m - 1]) return YV3_EINVAL;   // COCOeval.evaluate sorts maxDets
    }
    if (d->max_dets[d->n_maxdet - 1] > CC_MAX_DET) return YV3_ELIMIT;
    if ((long long)d->n_img * d->n_cat >= (1ll << 31) - 1) return YV3_ELIMIT;
    if ((d->n_gt && (!d->gt_img || !d->gt_cat || !d->gt_box || !d->gt_area || !d->gt_crowd || !d->gt_id)) ||
        (d->n_det && (!d->det_img || !d->det_cat || !d->det_box || !d->det_score)) ||
        !d->iou_thrs || !d->rec_thrs || !d->area_rng || !d->precision || !d->recall || !d->scores || !d->status)
        return YV3_EINVAL;
    return 0;
}

extern "C" size_t yv3_cocoeval_workspace_bytes(int n_gt, int n_det, int n_img, int n_cat, int n_area) {
    if (n_gt < 0 || n_det < 0 || n_img <= 0 || n_cat <= 0 || n_area <= 0) return 0;
    return cc_layout(n_gt, n_det, (long long)n_img * n_cat, (long long)n_cat * n_area, nullptr, nullptr);
}

extern "C" int yv3_cocoeval(const yv3_cocoeval_desc* d, void* ws, size_t ws_bytes, void* stream) {
    const int rc = cc_check(d);
    if (rc) return rc;
    const long long G = (long long)d->n_img * d->n_cat;
    if (!ws || ws_bytes < yv3_cocoeval_workspace_bytes(d->n_gt, d->n_det, d->n_img, d->n_cat, d->n_area)) return YV3_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    cc_ws W;
    const size_t zeroed = cc_layout(d->n_gt, d->n_det, G, (long long)d->n_cat * d->n_area, (char*)ws, &W);
    cc_zero<<<256, 256, 0, s>>>((int*)ws, (long long)(zeroed / sizeof(int)));
    cc_zero<<<1, 64, 0, s>>>(d->status, 1);
    YV3_CHECK_LAUNCH();
    const long long n_all = (long long)d->n_gt + d->n_det;
    if (n_all) {
        const int blocks = yv3_ceil_div(n_all, 256);
        cc_count<<<blocks, 256, 0, s>>>(d->gt_img, d->gt_cat, d->n_gt, d->det_img, d->det_cat, d->n_det, d->n_img, d->n_cat, W.gcnt,
                                          W.dcnt);
        YV3_CHECK_LAUNCH();
    }
    cc_scan<<<2, 1024, 0, s>>>(W.gcnt, W.goff, W.dcnt, W.doff, (int)G);
    YV3_CHECK_LAUNCH();
    if (n_all) {
        cc_scatter<<<yv3_ceil_div(n_all, 256), 256, 0, s>>>(d->gt_img, d->gt_cat, d->n_gt, d->det_img, d->det_cat, d->n_det, d->n_img,
                                                           d->n_cat, W.gcnt, W.dcnt, W.gperm, W.dperm);
        YV3_CHECK_LAUNCH();
    }
    cc_params P;
    P.n_img = d->n_img;
    P.n_iou = d->n_iou;
    P.n_area = d->n_area;
    P.max_det = d->max_dets[d->n_maxdet - 1];
    P.n_groups = G;
    cc_match<<<(unsigned)G, 64, 0, s>>>(P, d->gt_box, d->gt_area, d->gt_crowd, d->gt_id, d->det_box, d->det_score, d->iou_thrs,
                                        d->area_rng, W, d->status);
    YV3_CHECK_LAUNCH();
    if (d->n_det) {
        cc_order<<<yv3_ceil_div(d->n_det, 256), 256, 0, s>>>(d->n_img, d->n_cat, W);
        YV3_CHECK_LAUNCH();
    }
    const long long waves = (long long)d->n_iou * d->n_cat * d->n_area * d->n_maxdet;
    cc_accum<<<(unsigned)waves, 64, 0, s>>>(d->n_img, d->n_cat, d->n_iou, d->n_area, d->n_rec, *d, d->rec_thrs, W);
    YV3_CHECK_LAUNCH();
    return 0;
}
