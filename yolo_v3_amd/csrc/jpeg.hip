// Baseline JPEG decode of a batch of files (yv3_jpeg_decode_batch, include/yv3.h), bit for bit what libjpeg(-turbo)'s defaults
// give: file bytes + the host parser's records (jpeg_parse.cpp) -> uint8 RGB [H][W][3].  Four launches, integer arithmetic only:
//   layout_kernel    one workgroup: re-derives every image's geometry from its DEVICE record, checks its scan and destination
//                    ranges in 64 bits, hands out the workspace shares (coefficients, component planes, restart offsets) in batch
//                    order and writes status[b]; the kernels below touch nothing this one has not checked
//   entropy_kernel   one workgroup per image: the Huffman tables are built once in LDS from the specs (12.6 KB, no register or LDS
//                    footprint that would keep other images' workgroups off the CU), all lanes zero the image's coefficients and
//                    find its restart markers, then one lane decodes each restart segment (jpeg_entropy.h; a file without DRI
//                    is one segment, one lane): the parallelism is the many images in flight
//   entropy_kernel<1> the same kernel with the self-synchronising stage (jpeg_sync.h; yv3_jpeg_decode_batch_ex, entropy =
//                    YV3_JPEG_ENTROPY_PARALLEL): a unit of YV3_JPEG_SYNC_MIN_BYTES or more is cut into subsequences of
//                    YV3_JPEG_SYNC_S bytes and decoded by the whole workgroup, a window of 256 subsequences at a time (sync_unit
//                    below); shorter units still take one lane each.  A unit the parallel path cannot establish as error-free is
//                    re-zeroed and handed to yv3_jpeg_decode_unit on one lane in the same launch, whose status stands
//   idct_kernel      one lane per 8x8 block: dequantise, jidctint's two passes, +128, clamp -> the component's uint8 plane; a block
//                    outside the range in which every libjpeg build computes the same bytes (jpeg_pixel.h) raises the image's
//                    status to YV3_JPEG_S_RANGE
//   colour_kernel    one lane per 4 output pixels: fancy upsampling of the chroma planes (h2v1 / h2v2), YCbCr -> RGB, 12 bytes
//                    as three dword stores where the destination allows it
//   layout_prog_kernel, entropy_prog_kernel   yv3_jpeg_decode_batch_prog with progressive images in the batch (jpeg_prog.h, DESIGN.md
//                    section 8f.2): the layout kernel's sibling re-checks the progressive device records and hands the later
//                    kernels frame records of its own making; one workgroup per progressive image decodes its scans level by
//                    level, independent scans side by side.  Baseline images of such a batch take entropy_kernel as always
// What more than one kernel needs is written once: the two layout kernels differ in the frame copy and the source check and share
// the range checks, the slot record and the hand-out of the workspace (baseline_src_ok, dst_ok, sized_slot, hand_out_shares); both entropy kernels
// cut a unit's bytes with yv3_jpeg_unit_bytes (jpeg_entropy.h, which the stand-alone host programs of tests/ run too);
// find_restart_markers is the workgroup's marker search, which entropy_kernel keeps written out (see there); and the three
// entry points are forwards to one decode_batch, which holds every argument check and the launch sequence.
// An image whose status is not 0 after any stage is skipped by the later ones: its destination bytes are not written.
// (compiled with -ffp-contract=off like the other non-MFMA files; there is no floating point here)
#include "yv3_common.h"
#include "jpeg_parse.h"
#include "jpeg_pixel.h"
#include "jpeg_sync.h"
#include "jpeg_prog.h"
#include <atomic>

namespace {

// every kernel launch of this file is counted (yv3_jpeg_launch_count: what tests and measurements read)
std::atomic<long long> g_launches{0};
#define YV3_JPEG_LAUNCH(...)                                   \
    do {                                                       \
        hipLaunchKernelGGL(__VA_ARGS__);                       \
        g_launches.fetch_add(1, std::memory_order_relaxed);    \
    } while (0)

static_assert(sizeof(yv3_jpeg_info) % 8 == 0, "layout_prog_kernel copies the records in 8-byte words");

// ---- what layout_kernel and layout_prog_kernel share ---------------------------------------------------------------------------
// These take values, not the record: the caller loads what it passes in one go, ahead of the compares (read through the record
// behind the && chain, each field is a global round trip of its own).
// The single scan (scan_offset, scan_length) of a baseline record yv3_jpeg_geometry accepted, inside a source buffer of
// src_bytes at offset so
__device__ bool baseline_src_ok(long long so, long long scan_offset, long long scan_length, long long src_bytes) {
    return so >= 0 && so <= src_bytes && scan_offset <= src_bytes - so && scan_length <= src_bytes - so - scan_offset &&
           scan_length <= 0x7fffffffLL;
}

// The n3 = 3 * width * height bytes of an image at offset dof of a destination buffer of dst_bytes, in 64 bits
__device__ bool dst_ok(long long dof, long long n3, long long dst_bytes) { return dof >= 0 && dof <= dst_bytes && n3 <= dst_bytes - dof; }

// An image's slot record from its status so far (0: geometry g); the three offsets are sizes for now (hand_out_shares)
__device__ yv3_jpeg_slot sized_slot(int code, const yv3_jpeg_geom& g, int prog) {
    yv3_jpeg_slot s;
    s.coef_off = code ? 0 : g.coef_bytes;
    s.plane_off = code ? 0 : g.plane_bytes;
    s.unit_off = code ? 0 : g.unit_bytes;
    s.status = code; s.prog = prog;
    return s;
}

// One lane, after a barrier behind the sized slots: the sizes of every accepted image become offsets from `pos` on, in batch order
// (an image whose share does not fit ws_bytes is refused), and status[b] is written for every image.
__device__ void hand_out_shares(yv3_jpeg_slot* slots, int B, long long pos, long long ws_bytes, int* status) {
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

__global__ __launch_bounds__(256) void layout_kernel(const yv3_jpeg_info* __restrict__ infos, const long long* __restrict__ src_offsets,
                                                     long long src_bytes, const long long* __restrict__ dst_offsets, long long dst_bytes,
                                                     int B, yv3_jpeg_slot* __restrict__ slots, long long ws_bytes, int* __restrict__ status) {
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        yv3_jpeg_geom g;
        const yv3_jpeg_info* f = infos + b;
        int code = yv3_jpeg_geometry(f, &g);
        if (!code) {
            const long long so = src_offsets[b], dof = dst_offsets[b], n3 = (long long)f->width * f->height * 3;
            const bool src_ok = baseline_src_ok(so, f->scan_offset, f->scan_length, src_bytes), fits = dst_ok(dof, n3, dst_bytes);
            if (!src_ok || !fits) code = YV3_JPEG_S_BOUNDS;
        }
        slots[b] = sized_slot(code, g, 0);
    }
    __syncthreads();
    if (threadIdx.x == 0)
        hand_out_shares(slots, B, yv3_jpeg_round256((long long)B * (long long)sizeof(yv3_jpeg_slot)), ws_bytes, status);
}

// One unit of YV3_JPEG_SYNC_MIN_BYTES or more, by the whole workgroup (every lane calls it with the same arguments).  0: coef
// holds exactly what yv3_jpeg_decode_unit would have written and that routine would return 0.  1: the caller hands the unit to
// it (an FF that is no stuffing pair, an error from a proven state, a wrong block count, a failed end check, a DC value out of
// range).  Windows of 256 subsequences, the first one's entry state proven: a speculative pass, at most YV3_JPEG_SYNC_P proving
// passes (each hands every lane its predecessor's exit state, or its own first bit again while that state is invalid; a lane whose
// entry state changed decodes again), then the proven
// prefix -- lane 0 and every lane whose entry state is its predecessor's exit state, up to the first break of that chain -- is
// committed by the write pass and the next window opens behind it.  Pass p proves lane p at the latest, so a window commits
// min(P + 1, its lanes) subsequences or more and the loop ends after at most nsub windows.  No lane waits on another's flag:
// every dependency goes through a barrier.
__device__ int sync_unit(const unsigned char* scan, long long begin, long long end, const yv3_jpeg_geom* g, const yv3_jpeg_hufftab* tabs,
                         const unsigned char* sel, const unsigned char* natural, short* coef, int m0, int m1) {
    constexpr int L = YV3_JPEG_SYNC_LANES, S = YV3_JPEG_SYNC_S;
    __shared__ yv3_jpeg_sync_state s_en[L], s_ex[L], s_entry;
    __shared__ int s_cnt[L], s_off[L];
    __shared__ long long s_dc[L][3];
    __shared__ int s_flag, s_np, s_base, s_err, s_fin;
    const int t = threadIdx.x;
    const int bpm = yv3_jpeg_sync_bpm(g), unit_blocks = (m1 - m0) * bpm, nblocks = g->nblocks;    // <= 6 * 2048 * 2048
    const long long nsub = (end - begin + S - 1) / S;
    __syncthreads();                                       // the previous unit's last reads of the flags
    if (t == 0) { s_flag = 0; s_err = 0; s_fin = 0; s_base = 0; s_entry.bit = begin * 8; s_entry.blk = 0; s_entry.zz = 0; }
    __syncthreads();
    for (long long i = begin + t; i < end; i += L)
        if (yv3_jpeg_sync_marker(scan, i, end)) s_flag = 1;
    __syncthreads();
    if (s_flag) return 1;
    long long w0 = 0;
    while (w0 < nsub) {                                    // every window commits at least its lane 0
        const int nl = nsub - w0 < L ? (int)(nsub - w0) : L;
        yv3_jpeg_sync_state en, ex;
        en.bit = -1; en.blk = 0; en.zz = 0; ex = en;
        int cnt = 0;
        long long cut = end;
        if (t < nl) {                                      // the speculative pass
            cut = yv3_jpeg_sync_cut(scan, begin, end, w0 + t + 1, S);
            if (t == 0) en = s_entry;
            else en.bit = yv3_jpeg_sync_cut(scan, begin, end, w0 + t, S) * 8;
            yv3_jpeg_sync_lane(scan, end, cut, &en, g, tabs, sel, sel + 4, natural, 0, nblocks, m0, 0, 0, &ex, &cnt);
            s_en[t] = en; s_ex[t] = ex; s_cnt[t] = cnt;
        }
        for (int p = 0; p < YV3_JPEG_SYNC_P; ++p) {        // the proving passes
            if (t == 0) s_flag = 0;
            __syncthreads();
            bool changed = false;
            yv3_jpeg_sync_state ne = en;
            if (t > 0 && t < nl) {
                ne = s_ex[t - 1];
                if (ne.bit < 0) { ne.bit = yv3_jpeg_sync_cut(scan, begin, end, w0 + t, S) * 8; ne.blk = 0; ne.zz = 0; }     // stay speculative
                changed = !yv3_jpeg_sync_same(ne, en);
                if (changed) s_flag = 1;
            }
            __syncthreads();
            const int any = s_flag;
            __syncthreads();                               // every lane has read the flag before lane 0 clears it for the next pass
            if (!any) break;                               // every chain link holds: the whole window is proven
            if (changed) {
                en = ne;
                yv3_jpeg_sync_lane(scan, end, cut, &en, g, tabs, sel, sel + 4, natural, 0, nblocks, m0, 0, 0, &ex, &cnt);
                s_en[t] = en; s_ex[t] = ex; s_cnt[t] = cnt;     // (s_ex[t] is read by lane t + 1 alone, before the barrier above)
            }
        }
        __syncthreads();
        if (t == 0) s_np = nl;
        __syncthreads();
        if (t > 0 && t < nl) {
            const yv3_jpeg_sync_state prev = s_ex[t - 1];
            if (prev.bit < 0 || !yv3_jpeg_sync_same(prev, en)) atomicMin(&s_np, t);
        }
        __syncthreads();
        const int np = s_np;                               // 1 <= np <= nl
        if (t == 0) {                                      // exclusive prefix sum of the proven block counts
            int run = s_base;
            for (int j = 0; j < np; ++j) {
                s_off[j] = run;
                run = s_cnt[j] < unit_blocks - run ? run + s_cnt[j] : unit_blocks;
            }
            s_base = run;
        }
        __syncthreads();
        if (t < np && s_off[t] < unit_blocks) {            // the write pass (a lane behind the unit's last block has nothing to write:
                                                           // the lane that completed that block makes the end checks)
            const int r = yv3_jpeg_sync_lane(scan, end, cut, &en, g, tabs, sel, sel + 4, natural, coef, nblocks, m0, s_off[t], unit_blocks,
                                             &ex, &cnt);
            if (r == YV3_JPEG_SYNC_ERROR) s_err = 1;
            if (r == YV3_JPEG_SYNC_FINISHED) s_fin = 1;
        }
        __syncthreads();
        if (s_err) return 1;
        if (s_fin) break;
        if (t == 0) s_entry = s_ex[np - 1];
        w0 += np;
        __syncthreads();
    }
    if (!s_fin) return 1;                                  // the bytes ran out before the unit's last block
    // the DC pass: each lane sums the differences of its run of MCUs, lane 0 scans the 256 sums, each lane applies its prefix
    const int M = m1 - m0, chunk = (M + L - 1) / L;
    const int lo = m0 + (t * chunk < M ? t * chunk : M), hi = m0 + ((t + 1) * chunk < M ? (t + 1) * chunk : M);
    long long sums[3] = {0, 0, 0};
    yv3_jpeg_sync_dc_sum(coef, g, nblocks, lo, hi, sums);
    for (int c = 0; c < 3; ++c) s_dc[t][c] = sums[c];
    __syncthreads();
    if (t == 0) {
        long long run[3] = {0, 0, 0};
        for (int j = 0; j < L; ++j)
            for (int c = 0; c < 3; ++c) { const long long v = s_dc[j][c]; s_dc[j][c] = run[c]; run[c] += v; }
    }
    __syncthreads();
    for (int c = 0; c < 3; ++c) sums[c] = s_dc[t][c];
    if (!yv3_jpeg_sync_dc_apply(coef, g, nblocks, lo, hi, sums)) s_err = 1;
    __syncthreads();
    return s_err;
}

// The restart markers of a scan of len bytes and nunits >= 2 units, by the whole workgroup (every lane calls it with the same
// arguments): each lane counts those of its 256th of the scan, lane 0 turns counts[256] into an exclusive prefix and their sum
// into *s_total, and where that is the nunits - 1 the scan must hold each lane writes its positions to marks[] in file order.
// Returns whether it is.  Both barriers are reached by all 256 lanes, and the result is read from LDS after a barrier, the same
// for every lane.  counts[] and *s_total (LDS) are the caller's again after its next barrier.
// entropy_prog_kernel calls it once per scan.  entropy_kernel carries the same search written out (see there): called from that
// kernel the routine compiles to other branches, which moves and re-registers the decode loop behind it.
__device__ __forceinline__ bool find_restart_markers(const unsigned char* scan, int len, int nunits, int* marks, int* counts, int* s_total) {
    const int t = threadIdx.x;
    const int chunk = (len + 255) / 256;
    const long long lo = (long long)t * chunk;
    const long long hi = lo + chunk < len ? lo + chunk : len;
    int cnt = 0;
    for (long long i = lo; i < hi; ++i)
        if (yv3_jpeg_restart_at(scan, i, len)) ++cnt;
    counts[t] = cnt;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int k = 0; k < 256; ++k) { const int c = counts[k]; counts[k] = run; run += c; }
        *s_total = run;
    }
    __syncthreads();
    if (*s_total != nunits - 1) return false;
    int k = counts[t];
    for (long long i = lo; i < hi; ++i)
        if (yv3_jpeg_restart_at(scan, i, len)) { if (k < nunits - 1) marks[k] = (int)i; ++k; }
    return true;
}

// The byte range [*begin, *end) of unit u between the restart markers found at marks[], and its MCUs [*m0, *m1).  0, or
// YV3_JPEG_S_MARKER for markers out of order or out of range.
__device__ int unit_range(const unsigned char* scan, int len, const int* marks, const yv3_jpeg_geom& g, int u, long long* begin,
                          long long* end, int* m0, int* m1) {
    const int code = yv3_jpeg_unit_bytes(scan, len, marks, g.nunits, u, begin, end);      // (first: the other order costs
    *m0 = u * g.mcus_per_unit;                                                            // entropy_kernel<1> a register)
    *m1 = g.nmcu - *m0 < g.mcus_per_unit ? g.nmcu : *m0 + g.mcus_per_unit;
    return code;
}

// SYNC 0: one lane per unit.  SYNC 1: long units go to sync_unit; `handed` [B] counts the units handed back to one lane.
template <int SYNC>
__global__ __launch_bounds__(256) void entropy_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_offsets,
                                                      const yv3_jpeg_info* __restrict__ infos, yv3_jpeg_slot* __restrict__ slots,
                                                      unsigned char* __restrict__ ws, int* __restrict__ status, int* __restrict__ handed) {
    __shared__ yv3_jpeg_hufftab tabs[8];
    __shared__ yv3_jpeg_geom g;
    __shared__ int counts[256];
    __shared__ int s_geom, s_status, s_total;
    __shared__ unsigned char sel[8];                       // td[0..3], ta[0..3]
    __shared__ unsigned char natural[64];
    const int b = blockIdx.x, t = threadIdx.x;
    const yv3_jpeg_slot slot = slots[b];
    if (SYNC && handed && t == 0) handed[b] = 0;           // whichever way the image leaves this kernel
    if (slot.status || slot.prog) return;                  // the whole workgroup: layout_kernel refused the image, or it is
                                                           // entropy_prog_kernel's
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
    if (nunits > 1) {                                      // find_restart_markers, written out: with the call this kernel's decode loop
                                                           // is laid out differently (same instructions, other registers and
                                                           // addresses), and the serial stage measured 2 % slower on one file set
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
        if constexpr (SYNC == 0) {
            for (int u = t; u < nunits; u += 256) {
                long long begin, end;
                int m0, m1;
                int code = unit_range(scan, len, marks, g, u, &begin, &end, &m0, &m1);
                if (!code) code = yv3_jpeg_decode_unit(scan, begin, end, &g, tabs, sel, sel + 4, natural, m0, m1, coef, g.nblocks);
                if (code) atomicMax(&s_status, code);
            }
        } else {
            __shared__ int s_long[256], s_nlong, s_handed;
            if (t == 0) s_handed = 0;
            for (int u0 = 0; u0 < nunits; u0 += 256) {     // 256 units a round: the short ones decoded, the long ones listed
                if (t == 0) s_nlong = 0;
                __syncthreads();
                const int u = u0 + t;
                if (u < nunits) {
                    long long begin, end;
                    int m0, m1;
                    int code = unit_range(scan, len, marks, g, u, &begin, &end, &m0, &m1);
                    if (!code) {
                        if (end - begin >= YV3_JPEG_SYNC_MIN_BYTES) s_long[atomicAdd(&s_nlong, 1)] = u;      // at most 256 a round
                        else code = yv3_jpeg_decode_unit(scan, begin, end, &g, tabs, sel, sel + 4, natural, m0, m1, coef, g.nblocks);
                    }
                    if (code) atomicMax(&s_status, code);
                }
                __syncthreads();
                const int nlong = s_nlong;
                for (int q = 0; q < nlong; ++q) {          // the whole workgroup, one long unit after the other
                    long long begin, end;
                    int m0, m1;
                    if (unit_range(scan, len, marks, g, s_long[q], &begin, &end, &m0, &m1)) continue;       // (it passed above)
                    if (sync_unit(scan, begin, end, &g, tabs, sel, natural, coef, m0, m1)) {
                        const int bpm = yv3_jpeg_sync_bpm(&g);
                        const long long n16u = (long long)(m1 - m0) * bpm * 8;
                        for (long long i = t; i < n16u; i += 256) {             // the unit's blocks, zero again
                            const long long blk = yv3_jpeg_sync_block(&g, m0 + (int)(i / 8 / bpm), (int)(i / 8 % bpm), g.nblocks);
                            if (blk >= 0) ((int4*)(coef + blk * 64))[i & 7] = make_int4(0, 0, 0, 0);
                        }
                        __syncthreads();
                        if (t == 0) {
                            const int code = yv3_jpeg_decode_unit(scan, begin, end, &g, tabs, sel, sel + 4, natural, m0, m1, coef, g.nblocks);
                            if (code) atomicMax(&s_status, code);
                            ++s_handed;
                        }
                    }
                }
                __syncthreads();
            }
            if (t == 0 && handed && s_handed) handed[b] = s_handed;
        }
    }
    __syncthreads();
    if (t == 0) { slots[b].status = s_status; status[b] = s_status; }
}

// layout_kernel for yv3_jpeg_decode_batch_prog with progressive images in the batch.  The info records are copied into the
// workspace (`frames`), where a progressive image's becomes a frame record (yv3_jpegp_as_frame): the later kernels read the
// copy.  A progressive image's DEVICE record is re-checked here -- its index, every scan's Ss / Se / Ah / Al, components and
// table indices (yv3_jpegp_check), every scan's byte range against the source buffer in 64 bits -- and its share of restart
// offsets is sized from the unit counts this kernel derives itself.
__global__ __launch_bounds__(256) void layout_prog_kernel(const yv3_jpeg_info* __restrict__ infos, const yv3_jpeg_prog* __restrict__ progs,
                                                          const int* __restrict__ prog_of, int P, const long long* __restrict__ src_offsets,
                                                          long long src_bytes, const long long* __restrict__ dst_offsets, long long dst_bytes,
                                                          int B, yv3_jpeg_slot* __restrict__ slots, yv3_jpeg_info* __restrict__ frames,
                                                          long long ws_bytes, int* __restrict__ status) {
    const long long nwords = (long long)B * (long long)(sizeof(yv3_jpeg_info) / 8);       // the record is a multiple of 8 bytes
    for (long long i = threadIdx.x; i < nwords; i += blockDim.x) ((long long*)frames)[i] = ((const long long*)infos)[i];
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        yv3_jpeg_geom g;
        yv3_jpeg_info* f = frames + b;
        const int pi = prog_of[b];
        int code;
        if (pi < 0) {
            code = pi == -1 ? yv3_jpeg_geometry(f, &g) : YV3_JPEG_S_INFO;
        } else if (pi >= P || f->reason != YV3_JPEG_PROGRESSIVE) {
            code = YV3_JPEG_S_INFO;
        } else {
            yv3_jpegp_as_frame(f);
            code = yv3_jpegp_geometry(f, progs + pi, &g);
        }
        if (!code) {
            const long long so = src_offsets[b], dof = dst_offsets[b], n3 = (long long)f->width * f->height * 3;
            bool src_ok = so >= 0 && so <= src_bytes;
            if (src_ok && pi < 0) {
                src_ok = baseline_src_ok(so, f->scan_offset, f->scan_length, src_bytes);
            } else if (src_ok) {
                const yv3_jpeg_prog* p = progs + pi;
                for (int i = 0; i < p->nscans; ++i) {        // offset, length >= 0 and length < 2^31: yv3_jpegp_check
                    const long long o = p->scans[i].offset, l = p->scans[i].length;
                    src_ok = src_ok && o <= src_bytes - so && l <= src_bytes - so - o;
                }
            }
            const bool fits = dst_ok(dof, n3, dst_bytes);
            if (!src_ok || !fits) code = YV3_JPEG_S_BOUNDS;
        }
        slots[b] = sized_slot(code, g, pi >= 0);
    }
    __syncthreads();
    if (threadIdx.x == 0)                                  // slots | frames | shares
        hand_out_shares(slots, B, yv3_jpeg_round256((long long)B * (long long)sizeof(yv3_jpeg_slot)) +
                                      yv3_jpeg_round256((long long)B * (long long)sizeof(yv3_jpeg_info)), ws_bytes, status);
}

// The entropy stage of a progressive image: one workgroup per image.  Lane 0 derives the geometry, every scan's unit count and
// the level of every scan (yv3_jpegp_levels) from the device record layout_prog_kernel checked; all lanes zero the coefficients
// and find every scan's restart markers.  Then level by level: lane 0 lists the level's scans and table slots, up to eight
// lanes build the level's Huffman tables in LDS, and the level's units -- all independent: they code different coefficients
// or different blocks -- are dealt to lanes across the four waves first (longest first, in a snake: unit i of a round of 256
// goes to wave i mod 4, or 3 - i mod 4 on odd rows of four, lane i / 4), so that a few long scans do not share one wave; a
// level with more units than lanes takes several rounds.  Levels
// are separated by barriers; every loop bound around a barrier is read from LDS after a barrier, the same for all lanes.
// `frames`: layout_prog_kernel's copies.
__global__ __launch_bounds__(256) void entropy_prog_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ src_offsets,
                                                           const yv3_jpeg_info* __restrict__ frames, const yv3_jpeg_prog* __restrict__ progs,
                                                           const int* __restrict__ prog_of, yv3_jpeg_slot* __restrict__ slots,
                                                           unsigned char* __restrict__ ws, int* __restrict__ status) {
    __shared__ yv3_jpeg_hufftab tabs[YV3_JPEGP_LEVEL_TABLES];
    __shared__ yv3_jpeg_geom g;
    __shared__ int counts[256];
    __shared__ int s_units[YV3_JPEGP_MAX_SCANS], s_first[YV3_JPEGP_MAX_SCANS], s_cum[YV3_JPEGP_MAX_SCANS + 1];
    __shared__ unsigned char s_level[YV3_JPEGP_MAX_SCANS], s_list[YV3_JPEGP_MAX_SCANS], s_slot[YV3_JPEGP_MAX_SCANS];
    __shared__ unsigned char s_tabsrc[YV3_JPEGP_LEVEL_TABLES], s_tabdc[YV3_JPEGP_LEVEL_TABLES];
    __shared__ int s_geom, s_status, s_total, s_nscans, s_nlevels, s_nlist, s_ntabs;
    __shared__ unsigned char natural[64];
    const int b = blockIdx.x, t = threadIdx.x;
    const yv3_jpeg_slot slot = slots[b];
    if (!slot.prog || slot.status) return;                 // the whole workgroup: a baseline image, or one layout_prog_kernel refused
    const yv3_jpeg_info* f = frames + b;
    const yv3_jpeg_prog* p = progs + prog_of[b];           // 0 <= prog_of[b] < P: layout_prog_kernel
    if (t == 0) {
        s_geom = yv3_jpegp_geometry(f, p, &g);
        s_status = 0; s_total = 0; s_nscans = 0; s_nlevels = 0;
        if (!s_geom) {
            s_nscans = p->nscans;
            int first = 0;
            for (int i = 0; i < p->nscans; ++i) {
                const yv3_jpegp_scan* sc = p->scans + i;
                s_units[i] = yv3_jpegp_scan_units(yv3_jpegp_scan_items(&g, sc->ns, sc->comp[0]), sc->restart_interval);
                s_first[i] = first;
                first += s_units[i];                           // <= the units the share was sized for: the same sum
            }
            s_nlevels = yv3_jpegp_levels(p, s_level);
            for (int i = 0; i < p->nscans; ++i)
                if (s_level[i] != p->scans[i].level) s_geom = YV3_JPEG_S_INFO;      // the parser's schedule is this one
        }
    }
    if (t < 64) natural[t] = (unsigned char)yv3_jpeg_natural(t);
    __syncthreads();
    if (s_geom) {
        if (t == 0) { slots[b].status = s_geom; status[b] = s_geom; }
        return;
    }
    int4* cz = (int4*)(ws + slot.coef_off);
    const long long n16 = (long long)g.nblocks * 8;
    for (long long i = t; i < n16; i += 256) cz[i] = make_int4(0, 0, 0, 0);
    const unsigned char* file = src + src_offsets[b];
    int* marks = (int*)(ws + slot.unit_off);               // scan i: [s_first[i], s_first[i] + s_units[i] - 1) used
    const int nscans = s_nscans, nlevels = s_nlevels;
    for (int i = 0; i < nscans; ++i) {                     // the restart markers of every scan that has some
        const int nunits = s_units[i];
        if (nunits < 2) continue;                          // (the same for every lane: read from LDS after a barrier)
        const bool found = find_restart_markers(file + p->scans[i].offset, (int)p->scans[i].length, nunits, marks + s_first[i], counts,
                                                &s_total);
        if (!found && t == 0) atomicMax(&s_status, YV3_JPEG_S_MARKER);
        __syncthreads();                                   // counts[] and s_total are free for the next scan
    }
    short* coef = (short*)(ws + slot.coef_off);
    for (int lev = 1; lev <= nlevels; ++lev) {
        __syncthreads();                                   // the level before: its coefficients, and its reads of the lists
        if (t == 0) {
            int n = 0, nt = 0, cum = 0;
            for (int i = 0; i < nscans; ++i) {             // the level's scans, the most bytes per unit first
                if (s_level[i] != lev) continue;
                const yv3_jpegp_scan* sc = p->scans + i;
                const long long key = sc->length / s_units[i];
                int j = n++;
                while (j > 0 && p->scans[s_list[j - 1]].length / s_units[s_list[j - 1]] < key) { s_list[j] = s_list[j - 1]; --j; }
                s_list[j] = (unsigned char)i;
                s_slot[i] = (unsigned char)nt;
                const int need = yv3_jpegp_scan_tables(sc);
                for (int q = 0; q < need && nt < YV3_JPEGP_LEVEL_TABLES; ++q) {          // (never more: yv3_jpegp_levels)
                    s_tabsrc[nt] = sc->tab[q]; s_tabdc[nt] = sc->ss == 0; ++nt;
                }
            }
            for (int j = 0; j < n; ++j) { s_cum[j] = cum; cum += s_units[s_list[j]]; }
            s_cum[n] = cum; s_nlist = n; s_ntabs = nt;
        }
        __syncthreads();
        if (t < s_ntabs) {
            const yv3_jpegp_table* spec = p->tables + (s_tabsrc[t] < YV3_JPEGP_MAX_TABLES ? s_tabsrc[t] : 0);
            const int code = yv3_jpeg_build_hufftab(spec->counts, spec->values, s_tabdc[t] ? 15 : 255, &tabs[t]);
            if (code) atomicMax(&s_status, code);
        }
        __syncthreads();
        const int before = s_status;                       // every lane reads it before any lane's decode can raise it
        const int nlist = s_nlist, total = s_cum[nlist];
        __syncthreads();
        if (before) continue;                              // the image is lost; the remaining levels do nothing
        // lane q of wave w takes unit 4q + w of a round, on odd q unit 4q + 3 - w: a snake, so that the fifth longest unit shares
        // a wave with the fourth and not with the longest
        for (int u = (t & 63) << 2 | ((t & 1) ? 3 - (t >> 6) : t >> 6); u < total; u += 256) {
            int j = 0;
            while (j + 1 < nlist && u >= s_cum[j + 1]) ++j;
            const int i = s_list[j], k = u - s_cum[j], nunits = s_units[i];
            const yv3_jpegp_scan sc = p->scans[i];
            const int len = (int)sc.length;
            const unsigned char* scan = file + sc.offset;
            long long begin, end;
            int code = yv3_jpeg_unit_bytes(scan, len, marks + s_first[i], nunits, k, &begin, &end);
            const int items = yv3_jpegp_scan_items(&g, sc.ns, sc.comp[0]);
            const int per = sc.restart_interval ? sc.restart_interval : items;
            const int i0 = k * per, i1 = items - i0 < per ? items : i0 + per;
            const yv3_jpeg_hufftab* tp[3];
            for (int q = 0; q < 3; ++q) tp[q] = tabs + ((s_slot[i] + q) & (YV3_JPEGP_LEVEL_TABLES - 1));
            if (!code) code = yv3_jpegp_decode_unit(scan, begin, end, &g, &sc, tp, natural, i0, i1, coef, g.nblocks);
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

// The three entry points: every argument check (before any launch), then four launches, five with progressive images (P > 0:
// layout_prog_kernel instead of layout_kernel, the later kernels read its frame records, and entropy_prog_kernel runs behind
// entropy_kernel).  With P == 0 the four record pointers are not looked at.
int decode_batch(const yv3_jpeg_batch_desc* d, const yv3_jpeg_prog* progs, const yv3_jpeg_prog* progs_host, const int* prog_of,
                 const int* prog_of_host, int P, int entropy, int* handed_over, void* ws, size_t ws_bytes, void* stream) {
    if (entropy != YV3_JPEG_ENTROPY_SERIAL && entropy != YV3_JPEG_ENTROPY_PARALLEL) return YV3_EINVAL;
    if (!d || !ws || ((uintptr_t)ws & 255) != 0) return YV3_EINVAL;
    if (!d->src || !d->src_offsets || !d->infos || !d->infos_host || !d->dst || !d->dst_offsets || !d->status) return YV3_EINVAL;
    if (P != 0 && (!progs || !progs_host || !prog_of || !prog_of_host)) return YV3_EINVAL;
    const int B = d->B;
    if (B <= 0 || B > 65535 || P < 0 || P > 65535 || d->src_bytes <= 0 || d->dst_bytes <= 0) return YV3_EINVAL;
    long long max_blocks = 1, max_groups = 1;
    const size_t need = yv3_jpeg_batch_workspace(d->infos_host, B, prog_of_host, progs_host, P, true, &max_blocks, &max_groups);
    if (need == 0) return YV3_ESHAPE;
    if (ws_bytes < need) return YV3_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    yv3_jpeg_slot* slots = (yv3_jpeg_slot*)ws;
    unsigned char* wsb = (unsigned char*)ws;
    const yv3_jpeg_info* infos = d->infos;                 // what the kernels behind the layout read: the records, or its frames
    if (P) {
        yv3_jpeg_info* frames = (yv3_jpeg_info*)(wsb + yv3_jpeg_round256((long long)B * (long long)sizeof(yv3_jpeg_slot)));
        YV3_JPEG_LAUNCH(layout_prog_kernel, dim3(1), dim3(256), 0, s, d->infos, progs, prog_of, P, d->src_offsets, d->src_bytes,
                           d->dst_offsets, d->dst_bytes, B, slots, frames, (long long)ws_bytes, d->status);
        infos = frames;
    } else {
        YV3_JPEG_LAUNCH(layout_kernel, dim3(1), dim3(256), 0, s, d->infos, d->src_offsets, d->src_bytes, d->dst_offsets, d->dst_bytes, B,
                           slots, (long long)ws_bytes, d->status);
    }
    YV3_CHECK_LAUNCH();
    // (a batch of progressive images alone still takes this launch: its workgroups leave at once, after zeroing handed_over)
    if (entropy == YV3_JPEG_ENTROPY_PARALLEL)
        YV3_JPEG_LAUNCH(entropy_kernel<1>, dim3(B), dim3(256), 0, s, d->src, d->src_offsets, infos, slots, wsb, d->status, handed_over);
    else
        YV3_JPEG_LAUNCH(entropy_kernel<0>, dim3(B), dim3(256), 0, s, d->src, d->src_offsets, infos, slots, wsb, d->status, (int*)0);
    YV3_CHECK_LAUNCH();
    if (P) {
        YV3_JPEG_LAUNCH(entropy_prog_kernel, dim3(B), dim3(256), 0, s, d->src, d->src_offsets, infos, progs, prog_of, slots, wsb, d->status);
        YV3_CHECK_LAUNCH();
    }
    const int gx_idct = (int)(max_blocks / 256 + 1 < 4096 ? max_blocks / 256 + 1 : 4096);
    YV3_JPEG_LAUNCH(idct_kernel, dim3(gx_idct, B), dim3(256), 0, s, infos, slots, wsb, d->status);
    YV3_CHECK_LAUNCH();
    const int gx_col = (int)(max_groups / 256 + 1 < 4096 ? max_groups / 256 + 1 : 4096);
    YV3_JPEG_LAUNCH(colour_kernel, dim3(gx_col, B), dim3(256), 0, s, infos, slots, (const unsigned char*)wsb, d->dst, d->dst_offsets);
    YV3_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int yv3_jpeg_decode_batch(const yv3_jpeg_batch_desc* desc, void* ws, size_t ws_bytes, void* stream) {
    return decode_batch(desc, 0, 0, 0, 0, 0, YV3_JPEG_ENTROPY_SERIAL, 0, ws, ws_bytes, stream);
}

extern "C" int yv3_jpeg_decode_batch_ex(const yv3_jpeg_batch_desc* desc, int entropy, int* handed_over, void* ws, size_t ws_bytes,
                                        void* stream) {
    return decode_batch(desc, 0, 0, 0, 0, 0, entropy, handed_over, ws, ws_bytes, stream);
}

extern "C" int yv3_jpeg_decode_batch_prog(const yv3_jpeg_batch_desc_prog* desc, int entropy, int* handed_over, void* ws, size_t ws_bytes,
                                          void* stream) {
    if (!desc) return YV3_EINVAL;
    return decode_batch(&desc->base, desc->progs, desc->progs_host, desc->prog_of, desc->prog_of_host, desc->P, entropy, handed_over, ws,
                        ws_bytes, stream);
}

extern "C" long long yv3_jpeg_launch_count(void) { return g_launches.load(std::memory_order_relaxed); }
