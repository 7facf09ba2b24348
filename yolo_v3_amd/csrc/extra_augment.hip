// The reference's ExtraAugmentations (transforms.py:292-329) for a whole batch of packed uint8 RGB images of any sizes: one
// program of at most six steps per image (include/yv3.h: yv3_extra_program; yolo_v3_amd/extra_augment.py samples them), every
// step on the whole output of the step before.  tests/extra_aug_ref.py is the definition the kernel is held to, bit for bit.
//
// One launch per program slot, grid (workgroups per image, B): a workgroup reads its image's opcode for the slot, branches
// uniformly and walks the image in tiles of EX_TH x EX_TW pixels.  Step i of an image with n steps reads what step i - 1 wrote
// (step 0: the source, where it lies) and writes `out` when n - 1 - i is even, the workspace otherwise, so the last step of
// every image lands in `out` whatever n is; slots >= n do nothing, and an image without steps (or with a program that fails
// the checks) is copied through by slot 0.
//   stencils   the tile and its halo (up to 12 pixels for the Gaussian, 5 for the median) are staged in LDS through the border
//              rule, as interleaved bytes: a byte's horizontal neighbour of the same channel is 3 bytes away, adjacent lanes
//              read adjacent bytes (four lanes per bank word, no conflict)
//   GAUSS      both passes in the workgroup: rows into a second LDS tile, truncated to uint8, then columns; float64, scipy's order
//   MEDIAN     the k x k window in registers (one instantiation per k), then a binary search on the value: 8 counting rounds
//   pointwise  NOISE / ADD / MUL / CONTRAST / copy: a thread per pixel, no LDS
// (compiled with -ffp-contract=off: every float op rounds as the restatement's separate float32 / float64 operations do)
#include "yv3_common.h"

namespace {

constexpr int EX_TH = 32, EX_TW = 64, EX_NT = 256;
constexpr int EX_HALO = YV3_EXTRA_MAX_RADIUS;
constexpr int EX_ROWS = EX_TH + 2 * EX_HALO;             // 56
constexpr int EX_STRIDE = (EX_TW + 2 * EX_HALO) * 3;     // 264 bytes
constexpr int EX_MAX_SIDE = 1 << 28;                     // 2 * side must stay an int (the borders' period)

enum { EX_REFLECT, EX_REFLECT101, EX_REPLICATE };

__device__ inline int ex_border(int i, int n, int mode) {
    if (mode == EX_REPLICATE) return min(max(i, 0), n - 1);
    if (mode == EX_REFLECT) {                             // d c b a | a b c d | d c b a, period 2n
        const int p = 2 * n;
        i %= p;
        if (i < 0) i += p;
        return i >= n ? p - 1 - i : i;
    }
    if (n == 1) return 0;                                 // d c b | a b c d | c b a, period 2n - 2
    const int p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

__device__ inline bool ex_whole(double v, double bound) { return v == rint(v) && fabs(v) <= bound; }

// The checks yolo_v3_amd/extra_augment.py:check_programs restates on the host, in the same order.
__device__ inline int ex_check(const yv3_extra_program* __restrict__ P, int H, int W, long long so, long long src_bytes,
                               long long oo, long long out_bytes, bool& in_bounds) {
    in_bounds = false;
    if (H <= 0 || W <= 0 || H > EX_MAX_SIDE || W > EX_MAX_SIDE) return YV3_EINVAL;
    const long long n3 = (long long)H * W * 3;
    if (so < 0 || so > src_bytes || n3 > src_bytes - so || oo < 0 || oo > out_bytes || n3 > out_bytes - oo) return YV3_EINVAL;
    in_bounds = true;
    if (P->n_steps < 0 || P->n_steps > YV3_EXTRA_MAX_STEPS) return YV3_EINVAL;
    for (int i = 0; i < P->n_steps; ++i) {
        const yv3_extra_step& s = P->steps[i];
        const double v0 = s.v[0], v1 = s.v[1], v2 = s.v[2];
        switch (s.op) {
        case YV3_EXTRA_GAUSS: {
            if (!isfinite(v0) || v0 < 0.0 || v0 > 1e6) return YV3_EINVAL;
            const int r = (int)(4.0 * v0 + 0.5);
            if (r > YV3_EXTRA_MAX_RADIUS) return YV3_EINVAL;
            if (r > 0) {
                if (P->gauss_radius != r) return YV3_EINVAL;
                for (int j = 0; j <= r; ++j)
                    if (!isfinite(P->gauss_w[j]) || P->gauss_w[j] != P->gauss_w[2 * r - j]) return YV3_EINVAL;
            }
            break;
        }
        case YV3_EXTRA_AVERAGE:
            if (s.k < 2 || s.k > 7) return YV3_EINVAL;
            break;
        case YV3_EXTRA_MEDIAN:
            if (s.k < 3 || s.k > 11 || !(s.k & 1)) return YV3_EINVAL;
            break;
        case YV3_EXTRA_SHARPEN:
            if (!isfinite(v0) || !isfinite(v1)) return YV3_EINVAL;
            break;
        case YV3_EXTRA_NOISE:
            if (!isfinite(v0) || v0 < 0.0 || (s.per_channel != 0 && s.per_channel != 1)) return YV3_EINVAL;
            break;
        case YV3_EXTRA_ADD:
            if (!ex_whole(v0, 255.0) || !ex_whole(v1, 255.0) || !ex_whole(v2, 255.0)) return YV3_EINVAL;
            break;
        case YV3_EXTRA_MUL:
        case YV3_EXTRA_CONTRAST:
            if (!isfinite(v0) || !isfinite(v1) || !isfinite(v2)) return YV3_EINVAL;
            break;
        default:
            return YV3_EINVAL;
        }
    }
    return 0;
}

// The tile's th x tw pixels and a halo of (top, bottom, left, right) pixels, through the border rule: LDS row stride cols * 3.
__device__ inline void ex_stage(unsigned char* __restrict__ lds, const unsigned char* __restrict__ img, int H, int W, int y0, int x0,
                                int rows, int cols, int top, int left, int mode) {
    for (int i = threadIdx.x; i < rows * cols; i += EX_NT) {
        const int r = i / cols, c = i - r * cols;
        const int sy = ex_border(y0 - top + r, H, mode), sx = ex_border(x0 - left + c, W, mode);
        const unsigned char* p = img + ((long long)sy * W + sx) * 3;
        unsigned char* d = lds + (r * cols + c) * 3;
        d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
    }
}

template <int K>
__device__ inline void ex_median_tile(const unsigned char* __restrict__ s_in, int S, unsigned char* __restrict__ dst, int W, int y0,
                                      int x0, int th, int tw) {
    const int nb = tw * 3;
    for (int o = threadIdx.x; o < th * nb; o += EX_NT) {
        const int y = o / nb, xb = o - y * nb;
        int win[K * K];
#pragma unroll
        for (int dy = 0; dy < K; ++dy)
#pragma unroll
            for (int dx = 0; dx < K; ++dx) win[dy * K + dx] = s_in[(y + dy) * S + xb + 3 * dx];
        int lo = 0, hi = 255;
#pragma unroll 1
        for (int it = 0; it < 8; ++it) {                  // the smallest value with more than K K / 2 elements at or below it
            const int mid = (lo + hi) >> 1;
            int cnt = 0;
#pragma unroll
            for (int e = 0; e < K * K; ++e) cnt += win[e] <= mid ? 1 : 0;
            if (cnt > K * K / 2) hi = mid; else lo = mid + 1;
        }
        dst[((long long)(y0 + y) * W + x0) * 3 + xb] = (unsigned char)lo;
    }
}

// Philox4x32-10 (Salmon et al. 2011), the first two words of the block for counter (c0, c1, 0, 0)
__device__ inline void ex_philox(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t& x0, uint32_t& x1) {
    uint32_t c2 = 0, c3 = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    x0 = c0; x1 = c1;
}

__device__ inline double ex_normal(unsigned long long e, unsigned long long key) {
    uint32_t x0, x1;
    ex_philox((uint32_t)e, (uint32_t)(e >> 32), (uint32_t)key, (uint32_t)(key >> 32), x0, x1);
    const double u1 = ((double)x0 + 1.0) * 2.3283064365386963e-10, u2 = (double)x1 * 2.3283064365386963e-10;   // 2^-32
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

__device__ inline unsigned char ex_trunc_f32(float v) { return (unsigned char)(int)fminf(fmaxf(v, 0.f), 255.f); }

__global__ __launch_bounds__(EX_NT) void extra_slot_kernel(int slot, const unsigned char* src, long long src_bytes,
                                                           const long long* __restrict__ src_offsets, const int* __restrict__ hw,
                                                           const yv3_extra_program* __restrict__ programs,
                                                           unsigned char* out, long long out_bytes,
                                                           const long long* __restrict__ out_offsets, unsigned char* ws,
                                                           int* __restrict__ status) {
    __shared__ unsigned char s_in[EX_ROWS * EX_STRIDE];
    __shared__ unsigned char s_tmp[EX_TH * EX_STRIDE];
    __shared__ double s_w[2 * YV3_EXTRA_MAX_RADIUS + 1];
    const int b = blockIdx.y, t = threadIdx.x;
    const yv3_extra_program* P = programs + b;
    const int H = hw[2 * b], W = hw[2 * b + 1];
    const long long so = src_offsets[b], oo = out_offsets[b];
    bool in_bounds;
    const int code = ex_check(P, H, W, so, src_bytes, oo, out_bytes, in_bounds);
    if (slot == 0 && blockIdx.x == 0 && t == 0) status[b] = code;
    if (!in_bounds) return;
    const int n = code ? 0 : P->n_steps;
    if (slot >= max(n, 1)) return;
    // step i writes `out` when n - 1 - i is even
    const unsigned char* in = slot == 0 ? src + so : (((n - slot) & 1) ? ws : out) + oo;
    unsigned char* dst = (n == 0 || ((n - 1 - slot) & 1) == 0 ? out : ws) + oo;

    int op = 0, k = 0, per_channel = 0;
    double v0 = 0, v1 = 0, v2 = 0;
    unsigned long long key = 0;
    if (n) {
        const yv3_extra_step& s = P->steps[slot];
        op = s.op; k = s.k; per_channel = s.per_channel; v0 = s.v[0]; v1 = s.v[1]; v2 = s.v[2]; key = s.key;
    }
    int top = 0, bottom = 0, left = 0, right = 0, mode = EX_REFLECT;
    float kc = 0.f, ko = 0.f;
    if (op == YV3_EXTRA_GAUSS) {
        const int r = (int)(4.0 * v0 + 0.5);
        if (r == 0) op = 0;                               // skipped: a copy
        top = bottom = left = right = r;
        if (t <= 2 * r) s_w[t] = P->gauss_w[t];
    } else if (op == YV3_EXTRA_AVERAGE) {
        top = left = k / 2; bottom = right = k - 1 - k / 2; mode = EX_REFLECT101;
    } else if (op == YV3_EXTRA_MEDIAN) {
        top = bottom = left = right = k / 2; mode = EX_REPLICATE;
    } else if (op == YV3_EXTRA_SHARPEN) {
        top = bottom = left = right = 1; mode = EX_REFLECT101;
        const float a = (float)v0;
        kc = (float)(1.0 - v0) + a * (float)(8.0 + v1);
        ko = a * -1.f;
    }
    const bool stencil = op >= YV3_EXTRA_GAUSS && op <= YV3_EXTRA_SHARPEN;
    const float m0 = (float)v0, m1 = (float)v1, m2 = (float)v2;

    const int tiles_x = (W + EX_TW - 1) / EX_TW, tiles_y = (H + EX_TH - 1) / EX_TH;
    const long long n_tiles = (long long)tiles_x * tiles_y;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int ty = (int)(tile / tiles_x), tx = (int)(tile - (long long)ty * tiles_x);
        const int y0 = ty * EX_TH, x0 = tx * EX_TW;
        const int th = min(EX_TH, H - y0), tw = min(EX_TW, W - x0);
        if (!stencil) {
            for (int i = t; i < th * tw; i += EX_NT) {
                const int y = i / tw, x = i - y * tw;
                const long long pix = (long long)(y0 + y) * W + (x0 + x);
                const unsigned char* p = in + pix * 3;
                unsigned char* d = dst + pix * 3;
                const int p0 = p[0], p1 = p[1], p2 = p[2];
                if (op == YV3_EXTRA_NOISE) {
                    double z0, z1, z2;
                    if (per_channel) {
                        z0 = ex_normal((unsigned long long)pix * 3, key);
                        z1 = ex_normal((unsigned long long)pix * 3 + 1, key);
                        z2 = ex_normal((unsigned long long)pix * 3 + 2, key);
                    } else {
                        z0 = z1 = z2 = ex_normal((unsigned long long)pix, key);
                    }
                    d[0] = (unsigned char)(int)fmin(fmax((double)p0 + v0 * z0, 0.0), 255.0);
                    d[1] = (unsigned char)(int)fmin(fmax((double)p1 + v0 * z1, 0.0), 255.0);
                    d[2] = (unsigned char)(int)fmin(fmax((double)p2 + v0 * z2, 0.0), 255.0);
                } else if (op == YV3_EXTRA_ADD) {
                    d[0] = (unsigned char)min(max(p0 + (int)v0, 0), 255);
                    d[1] = (unsigned char)min(max(p1 + (int)v1, 0), 255);
                    d[2] = (unsigned char)min(max(p2 + (int)v2, 0), 255);
                } else if (op == YV3_EXTRA_MUL) {
                    d[0] = ex_trunc_f32((float)p0 * m0);
                    d[1] = ex_trunc_f32((float)p1 * m1);
                    d[2] = ex_trunc_f32((float)p2 * m2);
                } else if (op == YV3_EXTRA_CONTRAST) {
                    d[0] = ex_trunc_f32(m0 * ((float)p0 - 128.f) + 128.f);
                    d[1] = ex_trunc_f32(m1 * ((float)p1 - 128.f) + 128.f);
                    d[2] = ex_trunc_f32(m2 * ((float)p2 - 128.f) + 128.f);
                } else {
                    d[0] = (unsigned char)p0; d[1] = (unsigned char)p1; d[2] = (unsigned char)p2;
                }
            }
            continue;
        }
        const int rows = th + top + bottom, cols = tw + left + right, S = cols * 3, nb = tw * 3;
        ex_stage(s_in, in, H, W, y0, x0, rows, cols, top, left, mode);
        __syncthreads();
        unsigned char* drow = dst + ((long long)y0 * W + x0) * 3;          // + y * W * 3 + xb
        if (op == YV3_EXTRA_GAUSS) {
            const int r = top;
            for (int o = t; o < th * S; o += EX_NT) {                       // axis 0, every staged column
                const int y = o / S, j = o - y * S;
                const unsigned char* c = s_in + (y + r) * S + j;
                double acc = (double)c[0] * s_w[r];
                for (int jj = -r; jj < 0; ++jj) acc = acc + (double)((int)c[jj * S] + (int)c[-jj * S]) * s_w[r + jj];
                s_tmp[y * S + j] = (unsigned char)(int)acc;
            }
            __syncthreads();
            for (int o = t; o < th * nb; o += EX_NT) {                      // axis 1
                const int y = o / nb, xb = o - y * nb;
                const unsigned char* c = s_tmp + y * S + xb + 3 * r;
                double acc = (double)c[0] * s_w[r];
                for (int jj = -r; jj < 0; ++jj) acc = acc + (double)((int)c[3 * jj] + (int)c[-3 * jj]) * s_w[r + jj];
                drow[(long long)y * W * 3 + xb] = (unsigned char)(int)acc;
            }
        } else if (op == YV3_EXTRA_AVERAGE) {
            const double inv = 1.0 / (double)(k * k);
            for (int o = t; o < th * nb; o += EX_NT) {
                const int y = o / nb, xb = o - y * nb;
                int sum = 0;
                for (int dy = 0; dy < k; ++dy)
                    for (int dx = 0; dx < k; ++dx) sum += s_in[(y + dy) * S + xb + 3 * dx];
                drow[(long long)y * W * 3 + xb] = (unsigned char)(int)rint((double)sum * inv);
            }
        } else if (op == YV3_EXTRA_MEDIAN) {
            switch (k) {
            case 3: ex_median_tile<3>(s_in, S, dst, W, y0, x0, th, tw); break;
            case 5: ex_median_tile<5>(s_in, S, dst, W, y0, x0, th, tw); break;
            case 7: ex_median_tile<7>(s_in, S, dst, W, y0, x0, th, tw); break;
            case 9: ex_median_tile<9>(s_in, S, dst, W, y0, x0, th, tw); break;
            default: ex_median_tile<11>(s_in, S, dst, W, y0, x0, th, tw); break;
            }
        } else {                                                            // SHARPEN
            for (int o = t; o < th * nb; o += EX_NT) {
                const int y = o / nb, xb = o - y * nb;
                float acc = 0.f;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx)
                        acc = acc + (dy == 1 && dx == 1 ? kc : ko) * (float)s_in[(y + dy) * S + xb + 3 * dx];
                drow[(long long)y * W * 3 + xb] = (unsigned char)(int)fminf(fmaxf(rintf(acc), 0.f), 255.f);
            }
        }
        __syncthreads();                                                    // the next tile restages s_in / s_tmp
    }
}

}  // namespace

extern "C" size_t yv3_extra_augment_workspace_bytes(long long out_bytes) {
    return out_bytes > 0 ? (size_t)out_bytes : 0;
}

extern "C" int yv3_extra_augment(const unsigned char* src, long long src_bytes, const long long* src_offsets, const int* hw,
                                 const void* programs, int B, unsigned char* out, long long out_bytes, const long long* out_offsets,
                                 void* workspace, size_t workspace_bytes, int* status, void* stream) {
    if (!src || !src_offsets || !hw || !programs || !out || !out_offsets || !workspace || !status) return YV3_EINVAL;
    if (src_bytes <= 0 || out_bytes <= 0 || B <= 0 || B > 65535) return YV3_EINVAL;
    if (workspace_bytes < (size_t)out_bytes) return YV3_EWORKSPACE;
    // a workgroup per 32 x 64 tile of a 640 x 480 source up to batch 16, a few tiles per workgroup beyond
    const int per_image = max(1, min(4096, yv3_num_cu() * 32 / B));
    for (int slot = 0; slot < YV3_EXTRA_MAX_STEPS; ++slot) {
        hipLaunchKernelGGL(extra_slot_kernel, dim3(per_image, B), dim3(EX_NT), 0, (hipStream_t)stream, slot, src, src_bytes,
                           src_offsets, hw, (const yv3_extra_program*)programs, out, out_bytes, out_offsets,
                           (unsigned char*)workspace, status);
        YV3_CHECK_LAUNCH();
    }
    return 0;
}
