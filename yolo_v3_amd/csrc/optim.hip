// The update step of training (yolo_v3_amd/optim.py): the gradients' 2-norm, the clip coefficient, and SGD with momentum / weight
// decay / Nesterov -- the arithmetic of torch's clip_grad_norm_ and torch.optim.SGD, one fp32 rounding per operation (this file is
// compiled with -ffp-contract=off), with the norm summed in fp64 in a fixed order.  tests/optim_ref.py restates it in numpy.
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

struct sgd_params {
    float lr, momentum, one_minus_dampening, wd;
    int first, nesterov, maximize;
    const float* coef;                            // device: the clip coefficient, or NULL
};

// the entry whose chunks contain workgroup `wg` (uniform over the workgroup: scalar loads of the kernel arguments)
__device__ __forceinline__ int find_entry(const tensor_block& tb, int wg) {
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

// Cuts entries [0, count) into tensor_blocks and calls launch(block, chunks before this block) for each.  Arguments are
// checked for the whole list before the first launch.
template <class Launch>
int for_each_block(float* const* p, const float* const* g, float* const* buf, const long long* n, int count, Launch launch) {
    if (count < 0 || (count > 0 && (!g || !n))) return YV3_EINVAL;
    for (int i = 0; i < count; ++i)
        if (!g[i] || n[i] <= 0 || (p && !p[i]) || (buf && !buf[i])) return YV3_EINVAL;
    long long done = 0;
    int i = 0;
    while (i < count) {
        tensor_block tb = {};
        long long chunks = 0;
        while (i < count && tb.count < BLOCK_TENSORS) {
            const long long c = (n[i] + CHUNK - 1) / CHUNK;
            if (c > MAX_LAUNCH_CHUNKS) return YV3_ELIMIT;
            if (tb.count && chunks + c > MAX_LAUNCH_CHUNKS) break;
            const int e = tb.count++;
            tb.p[e] = p ? p[i] : nullptr;
            tb.g[e] = const_cast<float*>(g[i]);
            tb.buf[e] = buf ? buf[i] : nullptr;
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
