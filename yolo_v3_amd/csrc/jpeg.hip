// Baseline JPEG decode of a batch of files (yv3_jpeg_decode_batch, include/yv3.h), bit for bit what libjpeg(-turbo)'s defaults
// give: file bytes + the host parser's records (jpeg_parse.cpp) -> uint8 RGB [H][W][3].  Four launches, integer arithmetic only:
//   layout_kernel    one workgroup: re-derives every image's geometry from its DEVICE record, checks its scan and destination
//                    ranges in 64 bits, hands out the workspace shares (coefficients, component planes, restart offsets) in batch
//                    order and writes status[b]; the kernels below touch nothing this one has not checked
//   entropy_kernel   one workgroup per image: the Huffman tables are built once in LDS from the specs (12.6 KB, no register or LDS
//                    footprint that would keep other images' workgroups off the CU), all lanes zero the image's coefficients and
//                    find its restart markers, then one lane decodes each restart segment (jpeg_entropy.h; a file without DRI
//                    is one segment, one lane): the parallelism is the many images in flight
//   idct_kernel      one lane per 8x8 block: dequantise, jidctint's two passes, +128, clamp -> the component's uint8 plane; a block
//                    outside the range in which every libjpeg build computes the same bytes (jpeg_pixel.h) raises the image's
//                    status to YV3_JPEG_S_RANGE
//   colour_kernel    one lane per 4 output pixels: fancy upsampling of the chroma planes (h2v1 / h2v2), YCbCr -> RGB, 12 bytes
//                    as three dword stores where the destination allows it
// An image whose status is not 0 after any stage is skipped by the later ones: its destination bytes are not written.
// (compiled with -ffp-contract=off like the other non-MFMA files; there is no floating point here)
#include "yv3_common.h"
#include "jpeg_parse.h"
#include "jpeg_pixel.h"

namespace {

__global__ __launch_bounds__(256) void layout_kernel(const yv3_jpeg_info* __restrict__ infos, const long long* __restrict__ src_offsets,
                                                     long long src_bytes, const long long* __restrict__ dst_offsets, long long dst_bytes,
                                                     int B, yv3_jpeg_slot* __restrict__ slots, long long ws_bytes, int* __restrict__ status) {
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        yv3_jpeg_geom g;
        const yv3_jpeg_info* f = infos + b;
        int code = yv3_jpeg_geometry(f, &g);
        if (!code) {
            const long long so = src_offsets[b], dof = dst_offsets[b], n3 = (long long)f->width * f->height * 3;
            const bool src_ok = so >= 0 && so <= src_bytes && f->scan_offset <= src_bytes - so &&
                                f->scan_length <= src_bytes - so - f->scan_offset && f->scan_length <= 0x7fffffffLL;
            const bool dst_ok = dof >= 0 && dof <= dst_bytes && n3 <= dst_bytes - dof;
            if (!src_ok || !dst_ok) code = YV3_JPEG_S_BOUNDS;
        }
        yv3_jpeg_slot s;
        s.coef_off = code ? 0 : g.coef_bytes;              // sizes for now; thread 0 turns them into offsets below
        s.plane_off = code ? 0 : g.plane_bytes;
        s.unit_off = code ? 0 : g.unit_bytes;
        s.status = code; s.pad = 0;
        slots[b] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long pos = yv3_jpeg_round256((long long)B * (long long)sizeof(yv3_jpeg_slot));
        for (int b = 0; b < B; ++b) {
            yv3_jpeg_slot s = slots[b];
            if (!s.status) {
                const long long total = s.coef_off + s.plane_off + s.unit_off;
                if (pos > ws_bytes || total > ws_bytes - pos) {
                    s.status = YV3_JPEG_S_BOUNDS;
                } else {
                    const long long c = pos, p = pos + s.coef_off, u = p + s.plane_off;
                    s.coef_off = c; s.plane_off = p; s.unit_off = u;
                    pos += total;
                }
                slots[b] = s;
            }
            status[b] = s.status;
        }
    }
}

__global__ __launch_bounds__(256) void entropy_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_offsets,
                                                      const yv3_jpeg_info* __restrict__ infos, yv3_jpeg_slot* __restrict__ slots,
                                                      unsigned char* __restrict__ ws, int* __restrict__ status) {
    __shared__ yv3_jpeg_hufftab tabs[8];
    __shared__ yv3_jpeg_geom g;
    __shared__ int counts[256];
    __shared__ int s_geom, s_status, s_total;
    __shared__ unsigned char sel[8];                       // td[0..3], ta[0..3]
    __shared__ unsigned char natural[64];
    const int b = blockIdx.x, t = threadIdx.x;
    const yv3_jpeg_slot slot = slots[b];
    if (slot.status) return;                               // the whole workgroup: layout_kernel refused the image
    const yv3_jpeg_info* f = infos + b;
    if (t == 0) { s_geom = yv3_jpeg_geometry(f, &g); s_status = 0; s_total = 0; }
    if (t < 8) sel[t] = t < 4 ? f->td[t] : f->ta[t - 4];
    if (t < 64) natural[t] = (unsigned char)yv3_jpeg_natural(t);
    __syncthreads();
    if (s_geom) {                                          // (not reachable after layout_kernel's check of the same record)
        if (t == 0) { slots[b].status = s_geom; status[b] = s_geom; }
        return;
    }
    if (t < 8 && f->huff_defined[t]) {
        const int code = yv3_jpeg_build_hufftab(f->huff_counts[t], f->huff_values[t], t < 4 ? 15 : 255, &tabs[t]);
        if (code) atomicMax(&s_status, code);
    }
    int4* cz = (int4*)(ws + slot.coef_off);
    const long long n16 = (long long)g.nblocks * 8;        // 128 bytes per block
    for (long long i = t; i < n16; i += 256) cz[i] = make_int4(0, 0, 0, 0);
    const unsigned char* scan = src + src_offsets[b] + f->scan_offset;
    const int len = (int)f->scan_length;                   // <= 2^31 - 1: layout_kernel
    int* marks = (int*)(ws + slot.unit_off);               // [nunits - 1] used, [nunits] reserved
    const int nunits = g.nunits;
    if (nunits > 1) {
        const int chunk = (len + 255) / 256;
        const long long lo = (long long)t * chunk;
        const long long hi = lo + chunk < len ? lo + chunk : len;
        int cnt = 0;
        for (long long i = lo; i < hi && i + 1 < len; ++i)
            if (scan[i] == 0xFF && (scan[i + 1] & 0xF8) == 0xD0) ++cnt;
        counts[t] = cnt;
        __syncthreads();
        if (t == 0) {
            int run = 0;
            for (int k = 0; k < 256; ++k) { const int c = counts[k]; counts[k] = run; run += c; }
            s_total = run;
        }
        __syncthreads();
        if (s_total != nunits - 1) {
            if (t == 0) atomicMax(&s_status, YV3_JPEG_S_MARKER);
        } else {
            int k = counts[t];
            for (long long i = lo; i < hi && i + 1 < len; ++i)
                if (scan[i] == 0xFF && (scan[i + 1] & 0xF8) == 0xD0) { if (k < nunits - 1) marks[k] = (int)i; ++k; }
        }
    }
    __syncthreads();
    const int before = s_status;                           // tables and markers; every lane reads it before any lane's decode can
    __syncthreads();                                       // raise it below, so the branch is the same for the whole workgroup
    if (before == 0) {
        short* coef = (short*)(ws + slot.coef_off);
        for (int u = t; u < nunits; u += 256) {
            int code = 0;
            long long begin = 0, end = len;
            if (u > 0) begin = (long long)marks[u - 1] + 2;
            if (u < nunits - 1) {
                end = marks[u];
                if (end < 0 || end + 1 >= len || scan[end + 1] != 0xD0 + (u & 7)) code = YV3_JPEG_S_MARKER;
            }
            if (begin < 0 || begin > len || end < begin) code = YV3_JPEG_S_MARKER;
            if (!code) {
                const int m0 = u * g.mcus_per_unit;
                const int m1 = g.nmcu - m0 < g.mcus_per_unit ? g.nmcu : m0 + g.mcus_per_unit;
                code = yv3_jpeg_decode_unit(scan, begin, end, &g, tabs, sel, sel + 4, natural, m0, m1, coef, g.nblocks);
            }
            if (code) atomicMax(&s_status, code);
        }
    }
    __syncthreads();
    if (t == 0) { slots[b].status = s_status; status[b] = s_status; }
}

__global__ __launch_bounds__(256) void idct_kernel(const yv3_jpeg_info* __restrict__ infos, yv3_jpeg_slot* slots,
                                                   unsigned char* __restrict__ ws, int* __restrict__ status) {
    __shared__ yv3_jpeg_geom g;
    __shared__ unsigned char quant[3][64];
    const int b = blockIdx.y, t = threadIdx.x;
    const yv3_jpeg_info* f = infos + b;
    __shared__ int s_geom;
    // Other workgroups of this image may raise its status while this one starts, so ONE lane reads it for the whole workgroup:
    // lanes that read it themselves could disagree, and some would leave before the barrier that publishes g.
    if (t == 0) {
        const int st = __hip_atomic_load(&slots[b].status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_geom = st ? st : yv3_jpeg_geometry(f, &g);       // status 0: layout_kernel accepted this record
    }
    if (t < 192) quant[t >> 6][t & 63] = yv3_jpeg_quant_of(f, t >> 6)[t & 63];      // (inside the record whatever its bytes are)
    const long long coef_off = slots[b].coef_off, plane_off = slots[b].plane_off;   // layout_kernel's, never written after it
    __syncthreads();
    if (s_geom) return;
    const short* coef = (const short*)(ws + coef_off);
    unsigned char* planes = ws + plane_off;
    for (int blk = blockIdx.x * 256 + t; blk < g.nblocks; blk += gridDim.x * 256) {
        const int c = (g.ncomp == 3 && blk >= g.base[2]) ? 2 : (g.ncomp == 3 && blk >= g.base[1]) ? 1 : 0;
        const int local = blk - g.base[c];
        const int by = local / g.bw[c], bx = local - by * g.bw[c];
        union { int4 v[8]; short s[64]; } in;
        const int4* p = (const int4*)(coef + (long long)blk * 64);
#pragma unroll
        for (int i = 0; i < 8; ++i) in.v[i] = p[i];
        union { uint2 v[8]; unsigned char s[64]; } out;
        if (yv3_jpeg_idct_block(in.s, quant[c], out.s, 8)) {
            // the image is dropped: colour_kernel skips it, and workgroups of this kernel that see the status early may return
            atomicMax(&slots[b].status, YV3_JPEG_S_RANGE);
            atomicMax(&status[b], YV3_JPEG_S_RANGE);
        }
        const long long pitch = (long long)g.bw[c] * 8;
        unsigned char* o = planes + (long long)g.base[c] * 64 + (long long)by * 8 * pitch + (long long)bx * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) *(uint2*)(o + i * pitch) = out.v[i];
    }
}

__global__ __launch_bounds__(256) void colour_kernel(const yv3_jpeg_info* __restrict__ infos, const yv3_jpeg_slot* __restrict__ slots,
                                                     const unsigned char* __restrict__ ws, unsigned char* __restrict__ dst,
                                                     const long long* __restrict__ dst_offsets) {
    __shared__ yv3_jpeg_geom g;
    const int b = blockIdx.y, t = threadIdx.x;
    const yv3_jpeg_slot slot = slots[b];
    if (slot.status) return;
    const yv3_jpeg_info* f = infos + b;
    __shared__ int s_geom;
    if (t == 0) s_geom = yv3_jpeg_geometry(f, &g);
    __syncthreads();
    if (s_geom) return;
    const int W = f->width, H = f->height;
    const long long n = (long long)W * H, ngroups = (n + 3) / 4;
    const unsigned char* planes = ws + slot.plane_off;
    unsigned char* d = dst + dst_offsets[b];               // [d, d + 3n) inside dst: layout_kernel
    const bool aligned = ((uintptr_t)d & 3) == 0;
    for (long long q = (long long)blockIdx.x * 256 + t; q < ngroups; q += (long long)gridDim.x * 256) {
        const long long i0 = q * 4;
        unsigned char px[12];
        const int valid = n - i0 < 4 ? (int)(n - i0) : 4;
        int y = (int)(i0 / W), x = (int)(i0 - (long long)y * W);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int rgb[3] = {0, 0, 0};
            if (k < valid) yv3_jpeg_pixel(planes, &g, x, y, rgb);
            px[3 * k] = (unsigned char)rgb[0]; px[3 * k + 1] = (unsigned char)rgb[1]; px[3 * k + 2] = (unsigned char)rgb[2];
            if (++x == W) { x = 0; ++y; }
        }
        if (valid == 4 && aligned) {
            unsigned* o = (unsigned*)(d + i0 * 3);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                o[k] = (unsigned)px[4 * k] | (unsigned)px[4 * k + 1] << 8 | (unsigned)px[4 * k + 2] << 16 | (unsigned)px[4 * k + 3] << 24;
        } else {
            for (int k = 0; k < 3 * valid; ++k) d[i0 * 3 + k] = px[k];
        }
    }
}

}  // namespace

extern "C" int yv3_jpeg_decode_batch(const yv3_jpeg_batch_desc* desc, void* ws, size_t ws_bytes, void* stream) {
    if (!desc || !ws || ((uintptr_t)ws & 255) != 0) return YV3_EINVAL;
    if (!desc->src || !desc->src_offsets || !desc->infos || !desc->infos_host || !desc->dst || !desc->dst_offsets || !desc->status)
        return YV3_EINVAL;
    const int B = desc->B;
    if (B <= 0 || B > 65535 || desc->src_bytes <= 0 || desc->dst_bytes <= 0) return YV3_EINVAL;
    long long max_blocks = 1, max_groups = 1;
    for (int b = 0; b < B; ++b) {
        yv3_jpeg_geom g;
        if (yv3_jpeg_geometry(desc->infos_host + b, &g)) return YV3_ESHAPE;
        const long long groups = ((long long)desc->infos_host[b].width * desc->infos_host[b].height + 3) / 4;
        if (g.nblocks > max_blocks) max_blocks = g.nblocks;
        if (groups > max_groups) max_groups = groups;
    }
    const size_t need = yv3_jpeg_batch_workspace(desc->infos_host, B, true);
    if (need == 0) return YV3_ESHAPE;
    if (ws_bytes < need) return YV3_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    yv3_jpeg_slot* slots = (yv3_jpeg_slot*)ws;
    unsigned char* wsb = (unsigned char*)ws;
    hipLaunchKernelGGL(layout_kernel, dim3(1), dim3(256), 0, s, desc->infos, desc->src_offsets, desc->src_bytes, desc->dst_offsets,
                       desc->dst_bytes, B, slots, (long long)ws_bytes, desc->status);
    YV3_CHECK_LAUNCH();
    hipLaunchKernelGGL(entropy_kernel, dim3(B), dim3(256), 0, s, desc->src, desc->src_offsets, desc->infos, slots, wsb, desc->status);
    YV3_CHECK_LAUNCH();
    const int gx_idct = (int)(max_blocks / 256 + 1 < 4096 ? max_blocks / 256 + 1 : 4096);
    hipLaunchKernelGGL(idct_kernel, dim3(gx_idct, B), dim3(256), 0, s, desc->infos, slots, wsb, desc->status);
    YV3_CHECK_LAUNCH();
    const int gx_col = (int)(max_groups / 256 + 1 < 4096 ? max_groups / 256 + 1 : 4096);
    hipLaunchKernelGGL(colour_kernel, dim3(gx_col, B), dim3(256), 0, s, desc->infos, slots, (const unsigned char*)wsb, desc->dst,
                       desc->dst_offsets);
    YV3_CHECK_LAUNCH();
    return 0;
}
