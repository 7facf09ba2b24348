// The update step of training (yolo_v3_amd/optim.py): the gradients' 2-norm, the clip coefficient, SGD with momentum / weight
// decay / Nesterov, and Adam / AdamW -- the arithmetic of torch's clip_grad_norm_, torch.optim.SGD and torch.optim.Adam, one fp32
// rounding per operation (this file is compiled with -ffp-contract=off), with the norm summed in fp64 in a fixed order.
// tests/optim_ref.py and tests/adam_ref.py restate it in numpy.
//
// Every kernel is multi-tensor.  The host cuts the tensor list into blocks of at most BLOCK_TENSORS entries and launches once per
// block; the block -- pointers, sizes, first chunk of each tensor -- travels by value in the kernel arguments, so the launch owns
// a snapshot of it: new .grad tensors and a new lr every step need no staging buffer that a later step could overwrite.  Each
// workgroup owns chunk c of one tensor, elements [c * CHUNK, min(n, (c + 1) * CHUNK)): thread t takes the 4-element groups
// t, t + THREADS, ... of the chunk, as float4 where all of the entry's pointers are 16-byte aligned and the group is whole, element
// by element otherwise.  The element -> thread map does not depend on the path, so neither do the bits.
#include "yv3_common.h"

namespace {

constexpr int CHUNK = YV3_OPTIM_CHUNK;
constexpr int THREADS = 256;
constexpr int GROUPS = CHUNK / (THREADS * 4);     // float4 groups per thread and chunk
constexpr int UNROLL = 4;                         // groups in flight per thread on the whole-chunk path
constexpr int BLOCK_TENSORS = 64;
constexpr long long MAX_LAUNCH_CHUNKS = 1ll << 30;
constexpr int COEF_TILE = 2048;
static_assert(CHUNK % (THREADS * 4 * UNROLL) == 0, "a chunk is a whole number of unrolled float4 rounds");

struct tensor_block {                             // 2312 bytes of kernel arguments
    float* p[BLOCK_TENSORS];
    float* g[BLOCK_TENSORS];
    float* buf[BLOCK_TENSORS];
    long long n[BLOCK_TENSORS];
    int chunk0[BLOCK_TENSORS + 1];                // chunk0[e] = first workgroup of entry e; chunk0[count] = the grid
    int count;
};

struct adam_block {                               // 3336 bytes of kernel arguments: five pointers per entry
    float* p[BLOCK_TENSORS];
    float* g[BLOCK_TENSORS];
    float* m[BLOCK_TENSORS];
    float* v[BLOCK_TENSORS];
    float* vmax[BLOCK_TENSORS];
    long long n[BLOCK_TENSORS];
    int chunk0[BLOCK_TENSORS + 1];
    int count;
};
static_assert(sizeof(adam_block) + 64 <= 4096, "the block and the scalars stay under 4 KB of kernel arguments");

struct sgd_params {
    float lr, momentum, one_minus_dampening, wd;
    int first, nesterov, maximize;
    const float* coef;                            // device: the clip coefficient, or NULL
};

struct adam_params {                              // the step's scalars, reduced in double on the host and rounded to fp32
    float w, beta2, one_minus_beta2, sqrt_bc2, eps, neg_step_size, decay;
    int first, maximize, decoupled;
    const float* coef;
};

// the entry whose chunks contain workgroup `wg` (uniform over the workgroup: scalar loads of the kernel arguments)
template <class Block>
__device__ __forceinline__ int find_entry(const Block& tb, int wg) {
    int lo = 0, hi = tb.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tb.chunk0[mid] <= wg) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool aligned16(const void* a) { return ((uintptr_t)a & 15) == 0; }

__device__ __forceinline__ double sumsq4(double acc, const float4& v) {
    acc += (double)v.x * (double)v.x;             // (an fp32 square is exact in fp64)
    acc += (double)v.y * (double)v.y;
    acc += (double)v.z * (double)v.z;
    acc += (double)v.w * (double)v.w;
    return acc;
}

// partials[part0 + workgroup] = sum of g^2 over the workgroup's chunk: per thread in element order, then a pairwise tree over
// the threads (s[t] += s[t + stride], stride = THREADS / 2 ... 1).  No atomics.
__global__ __launch_bounds__(THREADS) void grad_sumsq_kernel(const tensor_block tb, double* __restrict__ partials, long long part0) {
    __shared__ double s[THREADS];
    const int wg = blockIdx.x, t = threadIdx.x;
    const int e = find_entry(tb, wg);
    const long long base = (long long)(wg - tb.chunk0[e]) * CHUNK;
    const long long left = tb.n[e] - base;
    const int m = left < CHUNK ? (int)left : CHUNK;
    const float* g = tb.g[e] + base;
    const bool vec = aligned16(tb.g[e]);
    double acc = 0.0;
    if (vec && m == CHUNK) {
#pragma unroll
        for (int j = 0; j < GROUPS; ++j) acc = sumsq4(acc, *reinterpret_cast<const float4*>(g + (j * THREADS + t) * 4));
    } else {
        for (int j = 0; j < GROUPS; ++j) {
            const int i = (j * THREADS + t) * 4;
            if (i >= m) break;
            float4 v;
            if (vec && i + 4 <= m) {
                v = *reinterpret_cast<const float4*>(g + i);
            } else {
                v.x = g[i];
                v.y = i + 1 < m ? g[i + 1] : 0.f;
                v.z = i + 2 < m ? g[i + 2] : 0.f;
                v.w = i + 3 < m ? g[i + 3] : 0.f;
            }
            acc = sumsq4(acc, v);
        }
    }
    s[t] = acc;
    __syncthreads();
    for (int stride = THREADS / 2; stride > 0; stride >>= 1) {
        if (t < stride) s[t] += s[t + stride];
        __syncthreads();
    }
    if (t == 0) partials[part0 + wg] = s[0];
}

// out[0] = total_norm = fp32(sqrt(sum of the partials, in index order, fp64)); out[1] = min(max_norm / (total_norm + 1e-6), 1) in
// fp32, a NaN kept (torch.clamp keeps it).  One workgroup: all threads stage a tile of partials, thread 0 adds it up.
__global__ __launch_bounds__(THREADS) void clip_coef_kernel(const double* __restrict__ partials, long long count, float max_norm,
                                                            float* __restrict__ out) {
    __shared__ double tile[COEF_TILE];
    double sum = 0.0;
    for (long long t0 = 0; t0 < count; t0 += COEF_TILE) {
        const int m = count - t0 < COEF_TILE ? (int)(count - t0) : COEF_TILE;
        for (int i = threadIdx.x; i < m; i += THREADS) tile[i] = partials[t0 + i];
        __syncthreads();
        if (threadIdx.x == 0) {
            int i = 0;
            for (; i + 8 <= m; i += 8) {              // eight LDS reads in flight, added in index order
                double v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = tile[i + k];
#pragma unroll
                for (int k = 0; k < 8; ++k) sum += v[k];
            }
            for (; i < m; ++i) sum += tile[i];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float total_norm = (float)sqrt(sum);
        const float q = max_norm / (total_norm + 1e-6f);
        out[0] = total_norm;
        out[1] = q > 1.0f ? 1.0f : q;
    }
}

__global__ __launch_bounds__(THREADS) void grad_scale_kernel(const tensor_block tb, const float* __restrict__ coef_ptr) {
    const int wg = blockIdx.x, t = threadIdx.x;
    const int e = find_entry(tb, wg);
    const long long base = (long long)(wg - tb.chunk0[e]) * CHUNK;
    const long long left = tb.n[e] - base;
    const int m = left < CHUNK ? (int)left : CHUNK;
    float* g = tb.g[e] + base;
    const bool vec = aligned16(tb.g[e]);
    const float c = *coef_ptr;
    for (int j = 0; j < GROUPS; ++j) {
        const int i = (j * THREADS + t) * 4;
        if (i >= m) break;
        if (vec && i + 4 <= m) {
            float4 v = *reinterpret_cast<const float4*>(g + i);
            v.x = v.x * c; v.y = v.y * c; v.z = v.z * c; v.w = v.w * c;
            *reinterpret_cast<float4*>(g + i) = v;
        } else {
            for (int k = i; k < i + 4 && k < m; ++k) g[k] = g[k] * c;
        }
    }
}

// one element of torch.optim.SGD's update (torch/optim/sgd.py, _single_tensor_sgd), every operation one fp32 rounding
template <bool MOM>
__device__ __forceinline__ void sgd_element(float& p, float g, float& b, float c, bool clip, const sgd_params& a) {
#pragma clang fp contract(off)
    float gs = clip ? g * c : g;
    if (a.maximize) gs = -gs;
    float d = gs;
    if (a.wd != 0.f) { const float wp = a.wd * p; d = gs + wp; }
    if (MOM) {
        if (a.first) {
            b = d;
        } else {
            const float mb = a.momentum * b, dd = a.one_minus_dampening * d;
            b = mb + dd;
        }
        if (a.nesterov) { const float mb = a.momentum * b; d = d + mb; } else d = b;
    }
    const float step = -a.lr * d;
    p = p + step;
}

template <bool MOM>
__device__ __forceinline__ void sgd_vec4(float4& p, const float4& g, float4& b, float c, bool clip, const sgd_params& a) {
    sgd_element<MOM>(p.x, g.x, b.x, c, clip, a);
    sgd_element<MOM>(p.y, g.y, b.y, c, clip, a);
    sgd_element<MOM>(p.z, g.z, b.z, c, clip, a);
    sgd_element<MOM>(p.w, g.w, b.w, c, clip, a);
}

template <bool MOM>
__global__ __launch_bounds__(THREADS) void sgd_step_kernel(const tensor_block tb, const sgd_params a) {
    const int wg = blockIdx.x, t = threadIdx.x;
    const int e = find_entry(tb, wg);
    const long long base = (long long)(wg - tb.chunk0[e]) * CHUNK;
    const long long left = tb.n[e] - base;
    const int m = left < CHUNK ? (int)left : CHUNK;
    float* p = tb.p[e] + base;
    const float* g = tb.g[e] + base;
    float* buf = MOM ? tb.buf[e] + base : nullptr;
    const bool vec = aligned16(tb.p[e]) && aligned16(tb.g[e]) && (!MOM || aligned16(tb.buf[e]));
    const bool clip = a.coef != nullptr, read_buf = MOM && !a.first;
    const float c = clip ? *a.coef : 1.0f;
    if (vec && m == CHUNK) {
        // a whole aligned chunk: UNROLL groups' loads in flight before the first store (p, g and buf may not be told apart by the compiler)
        for (int j0 = 0; j0 < GROUPS; j0 += UNROLL) {
            float4 pv[UNROLL], gv[UNROLL], bv[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int i = ((j0 + u) * THREADS + t) * 4;
                gv[u] = *reinterpret_cast<const float4*>(g + i);
                pv[u] = *reinterpret_cast<const float4*>(p + i);
                bv[u] = read_buf ? *reinterpret_cast<const float4*>(buf + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int i = ((j0 + u) * THREADS + t) * 4;
                sgd_vec4<MOM>(pv[u], gv[u], bv[u], c, clip, a);
                *reinterpret_cast<float4*>(p + i) = pv[u];
                if (MOM) *reinterpret_cast<float4*>(buf + i) = bv[u];
            }
        }
        return;
    }
    for (int j = 0; j < GROUPS; ++j) {
        const int i = (j * THREADS + t) * 4;
        if (i >= m) break;
        if (vec && i + 4 <= m) {
            const float4 gv = *reinterpret_cast<const float4*>(g + i);
            float4 pv = *reinterpret_cast<const float4*>(p + i);
            float4 bv = read_buf ? *reinterpret_cast<const float4*>(buf + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            sgd_vec4<MOM>(pv, gv, bv, c, clip, a);
            *reinterpret_cast<float4*>(p + i) = pv;
            if (MOM) *reinterpret_cast<float4*>(buf + i) = bv;
        } else {
            for (int k = i; k < i + 4 && k < m; ++k) {
                float pk = p[k], bk = read_buf ? buf[k] : 0.f;
                sgd_element<MOM>(pk, g[k], bk, c, clip, a);
                p[k] = pk;
                if (MOM) buf[k] = bk;
            }
        }
    }
}

// one element of torch.optim.Adam's update (torch/optim/adam.py, _single_tensor_adam, not capturable), every operation one fp32
// rounding; sqrtf and / are correctly rounded and keep denormals (no fast-math flag on this file)
template <bool AMS>
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float& vmax, float c, bool clip,
                                             const adam_params& a) {
#pragma clang fp contract(off)
    float gs = clip ? g * c : g;
    if (a.maximize) gs = -gs;
    if (a.decoupled) {
        p = p * a.decay;
    } else if (a.decay != 0.f) {
        const float wp = a.decay * p;
        gs = gs + wp;
    }
    const float d = gs - m;
    if (fabsf(a.w) < 0.5f) {                      // torch's lerp
        const float wd = a.w * d;
        m = m + wd;
    } else {
        const float omw = 1.0f - a.w, dw = d * omw;
        m = gs - dw;
    }
    v = v * a.beta2;
    const float bg = a.one_minus_beta2 * gs, bgg = bg * gs;
    v = v + bgg;
    float s = v;
    if (AMS) {                                    // torch.maximum: a NaN on either side is kept
        vmax = vmax != vmax ? vmax : (v != v ? v : (vmax > v ? vmax : v));
        s = vmax;
    }
    const float r = sqrtf(s), rb = r / a.sqrt_bc2, den = rb + a.eps;
    const float q = m / den, step = a.neg_step_size * q;
    p = p + step;
}

template <bool AMS>
__device__ __forceinline__ void adam_vec4(float4& p, const float4& g, float4& m, float4& v, float4& vmax, float c, bool clip,
                                          const adam_params& a) {
    adam_element<AMS>(p.x, g.x, m.x, v.x, vmax.x, c, clip, a);
    adam_element<AMS>(p.y, g.y, m.y, v.y, vmax.y, c, clip, a);
    adam_element<AMS>(p.z, g.z, m.z, v.z, vmax.z, c, clip, a);
    adam_element<AMS>(p.w, g.w, m.w, v.w, vmax.w, c, clip, a);
}

// the geometry of sgd_step_kernel; on a first step exp_avg, exp_avg_sq and max_exp_avg_sq are taken as +0 and not read
template <bool AMS>
__global__ __launch_bounds__(THREADS) void adam_step_kernel(const adam_block tb, const adam_params a) {
    const int wg = blockIdx.x, t = threadIdx.x;
    const int e = find_entry(tb, wg);
    const long long base = (long long)(wg - tb.chunk0[e]) * CHUNK;
    const long long left = tb.n[e] - base;
    const int n = left < CHUNK ? (int)left : CHUNK;
    float* p = tb.p[e] + base;
    const float* g = tb.g[e] + base;
    float* m = tb.m[e] + base;
    float* v = tb.v[e] + base;
    float* vmax = AMS ? tb.vmax[e] + base : nullptr;
    const bool vec = aligned16(tb.p[e]) && aligned16(tb.g[e]) && aligned16(tb.m[e]) && aligned16(tb.v[e]) &&
                     (!AMS || aligned16(tb.vmax[e]));
    const bool clip = a.coef != nullptr, read = !a.first;
    const float c = clip ? *a.coef : 1.0f;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec && n == CHUNK) {
        for (int j0 = 0; j0 < GROUPS; j0 += UNROLL) {
            float4 pv[UNROLL], gv[UNROLL], mv[UNROLL], vv[UNROLL], xv[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int i = ((j0 + u) * THREADS + t) * 4;
                gv[u] = *reinterpret_cast<const float4*>(g + i);
                pv[u] = *reinterpret_cast<const float4*>(p + i);
                mv[u] = read ? *reinterpret_cast<const float4*>(m + i) : zero;
                vv[u] = read ? *reinterpret_cast<const float4*>(v + i) : zero;
                xv[u] = AMS && read ? *reinterpret_cast<const float4*>(vmax + i) : zero;
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int i = ((j0 + u) * THREADS + t) * 4;
                adam_vec4<AMS>(pv[u], gv[u], mv[u], vv[u], xv[u], c, clip, a);
                *reinterpret_cast<float4*>(p + i) = pv[u];
                *reinterpret_cast<float4*>(m + i) = mv[u];
                *reinterpret_cast<float4*>(v + i) = vv[u];
                if (AMS) *reinterpret_cast<float4*>(vmax + i) = xv[u];
            }
        }
        return;
    }
    for (int j = 0; j < GROUPS; ++j) {
        const int i = (j * THREADS + t) * 4;
        if (i >= n) break;
        if (vec && i + 4 <= n) {
            const float4 gv = *reinterpret_cast<const float4*>(g + i);
            float4 pv = *reinterpret_cast<const float4*>(p + i);
            float4 mv = read ? *reinterpret_cast<const float4*>(m + i) : zero;
            float4 vv = read ? *reinterpret_cast<const float4*>(v + i) : zero;
            float4 xv = AMS && read ? *reinterpret_cast<const float4*>(vmax + i) : zero;
            adam_vec4<AMS>(pv, gv, mv, vv, xv, c, clip, a);
            *reinterpret_cast<float4*>(p + i) = pv;
            *reinterpret_cast<float4*>(m + i) = mv;
            *reinterpret_cast<float4*>(v + i) = vv;
            if (AMS) *reinterpret_cast<float4*>(vmax + i) = xv;
        } else {
            for (int k = i; k < i + 4 && k < n; ++k) {
                float pk = p[k], mk = read ? m[k] : 0.f, vk = read ? v[k] : 0.f, xk = AMS && read ? vmax[k] : 0.f;
                adam_element<AMS>(pk, g[k], mk, vk, xk, c, clip, a);
                p[k] = pk;
                m[k] = mk;
                v[k] = vk;
                if (AMS) vmax[k] = xk;
            }
        }
    }
}

// Cuts entries [0, count) into blocks of type Block (at most BLOCK_TENSORS entries and MAX_LAUNCH_CHUNKS chunks each): fill(block,
// e, i) sets entry e's pointers from list entry i, launch(block, chunks before this block) launches it.  The sizes are checked
// for the whole list before the first launch.
template <class Block, class Fill, class Launch>
int cut_blocks(const long long* n, int count, Fill fill, Launch launch) {
    for (int i = 0; i < count; ++i) {
        if (n[i] <= 0) return YV3_EINVAL;
        if ((n[i] + CHUNK - 1) / CHUNK > MAX_LAUNCH_CHUNKS) return YV3_ELIMIT;
    }
    long long done = 0;
    int i = 0;
    while (i < count) {
        Block tb = {};
        long long chunks = 0;
        while (i < count && tb.count < BLOCK_TENSORS) {
            const long long c = (n[i] + CHUNK - 1) / CHUNK;
            if (tb.count && chunks + c > MAX_LAUNCH_CHUNKS) break;
            const int e = tb.count++;
            fill(tb, e, i);
            tb.n[e] = n[i];
            tb.chunk0[e] = (int)chunks;
            chunks += c;
            ++i;
        }
        tb.chunk0[tb.count] = (int)chunks;
        const int rc = launch(tb, done);
        if (rc) return rc;
        done += chunks;
    }
    return 0;
}

// cut_blocks for the (p, g, buf) lists of the norm and SGD; p and buf may be NULL
template <class Launch>
int for_each_block(float* const* p, const float* const* g, float* const* buf, const long long* n, int count, Launch launch) {
    if (count < 0 || (count > 0 && (!g || !n))) return YV3_EINVAL;
    for (int i = 0; i < count; ++i)
        if (!g[i] || (p && !p[i]) || (buf && !buf[i])) return YV3_EINVAL;
    return cut_blocks<tensor_block>(n, count, [&](tensor_block& tb, int e, int i) {
        tb.p[e] = p ? p[i] : nullptr;
        tb.g[e] = const_cast<float*>(g[i]);
        tb.buf[e] = buf ? buf[i] : nullptr;
    }, launch);
}

}  // namespace

extern "C" int yv3_optim_chunk(void) { return CHUNK; }

extern "C" int yv3_grad_sumsq(const float* const* g, const long long* n, int count, double* partials, long long partials_cap, void* stream) {
    if (count < 0 || (count > 0 && (!g || !n || !partials))) return YV3_EINVAL;
    long long total = 0;
    for (int i = 0; i < count; ++i) {
        if (n[i] <= 0) return YV3_EINVAL;
        total += (n[i] + CHUNK - 1) / CHUNK;
    }
    if (total > partials_cap) return YV3_EWORKSPACE;
    return for_each_block(nullptr, g, nullptr, n, count, [&](const tensor_block& tb, long long part0) {
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3(tb.chunk0[tb.count]), dim3(THREADS), 0, (hipStream_t)stream, tb, partials, part0);
        YV3_CHECK_LAUNCH();
        return 0;
    });
}

extern "C" int yv3_clip_coef(const double* partials, long long count, float max_norm, float* out, void* stream) {
    if (count < 0 || (count > 0 && !partials) || !out) return YV3_EINVAL;
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, partials, count, max_norm, out);
    YV3_CHECK_LAUNCH();
    return 0;
}

extern "C" int yv3_grad_scale(float* const* g, const long long* n, int count, const float* coef, void* stream) {
    if (!coef) return YV3_EINVAL;
    return for_each_block(nullptr, g, nullptr, n, count, [&](const tensor_block& tb, long long) {
        hipLaunchKernelGGL(grad_scale_kernel, dim3(tb.chunk0[tb.count]), dim3(THREADS), 0, (hipStream_t)stream, tb, coef);
        YV3_CHECK_LAUNCH();
        return 0;
    });
}

extern "C" int yv3_sgd_step(float* const* p, const float* const* g, float* const* buf, const long long* n, int count, const float* coef,
                            float lr, float momentum, float one_minus_dampening, float weight_decay, int flags, void* stream) {
    if (count < 0 || (count > 0 && !p) || (flags & ~(YV3_SGD_FIRST | YV3_SGD_NESTEROV | YV3_SGD_MAXIMIZE))) return YV3_EINVAL;
    const bool mom = momentum != 0.f;
    if (mom && count > 0 && !buf) return YV3_EINVAL;
    const sgd_params a = {lr, momentum, one_minus_dampening, weight_decay, (flags & YV3_SGD_FIRST) != 0,
                          (flags & YV3_SGD_NESTEROV) != 0, (flags & YV3_SGD_MAXIMIZE) != 0, coef};
    return for_each_block(p, g, mom ? buf : nullptr, n, count, [&](const tensor_block& tb, long long) {
        if (mom) hipLaunchKernelGGL(sgd_step_kernel<true>, dim3(tb.chunk0[tb.count]), dim3(THREADS), 0, (hipStream_t)stream, tb, a);
        else hipLaunchKernelGGL(sgd_step_kernel<false>, dim3(tb.chunk0[tb.count]), dim3(THREADS), 0, (hipStream_t)stream, tb, a);
        YV3_CHECK_LAUNCH();
        return 0;
    });
}

extern "C" int yv3_adam_step(float* const* p, const float* const* g, float* const* exp_avg, float* const* exp_avg_sq,
                             float* const* max_exp_avg_sq, const long long* n, int count, const float* coef, float w, float beta2,
                             float one_minus_beta2, float sqrt_bc2, float eps, float neg_step_size, float decay, int flags,
                             void* stream) {
    if (count < 0 || (flags & ~(YV3_ADAM_FIRST | YV3_ADAM_AMSGRAD | YV3_ADAM_MAXIMIZE | YV3_ADAM_DECOUPLED))) return YV3_EINVAL;
    const bool ams = (flags & YV3_ADAM_AMSGRAD) != 0;
    if (count > 0 && (!p || !g || !exp_avg || !exp_avg_sq || !n || (ams && !max_exp_avg_sq))) return YV3_EINVAL;
    for (int i = 0; i < count; ++i)
        if (!p[i] || !g[i] || !exp_avg[i] || !exp_avg_sq[i] || (ams && !max_exp_avg_sq[i])) return YV3_EINVAL;
    const adam_params a = {w, beta2, one_minus_beta2, sqrt_bc2, eps, neg_step_size, decay, (flags & YV3_ADAM_FIRST) != 0,
                           (flags & YV3_ADAM_MAXIMIZE) != 0, (flags & YV3_ADAM_DECOUPLED) != 0, coef};
    return cut_blocks<adam_block>(n, count, [&](adam_block& tb, int e, int i) {
        tb.p[e] = p[i];
        tb.g[e] = const_cast<float*>(g[i]);
        tb.m[e] = exp_avg[i];
        tb.v[e] = exp_avg_sq[i];
        tb.vmax[e] = ams ? max_exp_avg_sq[i] : nullptr;
    }, [&](const adam_block& tb, long long) {
        if (ams) hipLaunchKernelGGL(adam_step_kernel<true>, dim3(tb.chunk0[tb.count]), dim3(THREADS), 0, (hipStream_t)stream, tb, a);
        else hipLaunchKernelGGL(adam_step_kernel<false>, dim3(tb.chunk0[tb.count]), dim3(THREADS), 0, (hipStream_t)stream, tb, a);
        YV3_CHECK_LAUNCH();
        return 0;
    });
}
