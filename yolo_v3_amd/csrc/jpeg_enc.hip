// Baseline JPEG encode of a batch of uint8 images (RGB or grey, any sizes) on the GPU: the file libjpeg writes for the same pixels,
// quality and subsampling with its standard Huffman tables (the arithmetic is in jpeg_enc.h, shared with the
// host entry points).  Nine launches for the whole batch, none of them waits for the host:
//   layout   one thread checks every record and lays the images out in the workspace
//   coef     one thread per 8x8 block of the scan: colour conversion, downsampling, edge replication, forward DCT, quantisation;
//            int16 coefficients in zigzag order, blocks in scan order, dummy blocks included
//   size     one thread per block: the bit length of its tokens (its DC predictor is the quantised DC `coef` wrote for the block
//            before it in its component: no chain), summed per chunk of 256 blocks
//   scan     one workgroup per image: exclusive prefix sum of the chunk sums (wave64 scans)
//   zero     clears the words of the bit buffer the image will use
//   emit     one thread per block: the chunk's offset plus a scan inside the workgroup gives its bit offset; whole words are
//            stored, the first and last word of a block, which it shares with its neighbours, are OR-combined (atomicOr of
//            disjoint bits: the result does not depend on the order)
//   count    FF bytes per 4096 bytes of the padded scan
//   finish   one workgroup per image: prefix sum of those counts, the file's length against the capacity, header, EOI, status
//   scatter  bytes to their place behind the header, 00 after every FF
// Results are written with ordinary vector stores; there is no inline assembly here.
#include "yv3_common.h"
#include "jpeg_enc.h"

namespace {

__constant__ yv3_enc_tables D_TAB = yv3_enc_make_tables();
__constant__ yv3_enc_spec D_SPEC = YV3_ENC_SPEC;

constexpr int T = 256;                                          // threads per workgroup, everywhere

struct enc_layout {
    yv3_enc_geom g;
    long long blk0, chunk0, word0, bchunk0;                     // the image's first block / block chunk / bit-buffer word / byte chunk
    unsigned nchunks, words_cap, nbchunks_cap;
    unsigned total_bits, nbytes;
    int hdr_len, fits;
};

// what an image of nblk blocks takes of each workspace region
YV3_HD inline unsigned enc_chunks(unsigned nblk) { return (nblk + YV3_ENC_CHUNK - 1) / YV3_ENC_CHUNK; }
YV3_HD inline unsigned enc_words(unsigned nblk) {                // a multiple of 4: 16-byte accesses; + 1: the word after the last bit
    return (unsigned)((((unsigned long long)nblk * YV3_ENC_BLOCK_BITS + 31) / 32 + 1 + 3) / 4 * 4);
}
YV3_HD inline unsigned enc_bchunks(unsigned nblk) { return (unsigned)(((unsigned long long)enc_words(nblk) * 4 + YV3_ENC_BYTE_CHUNK - 1) / YV3_ENC_BYTE_CHUNK); }

struct enc_totals {
    long long blocks, chunks, words, bchunks;
    unsigned max_blocks, max_words, max_bchunks;
};

struct enc_regions {
    size_t layout, coef, bits, chunk, word, bchunk, total;
};

inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }

enc_regions enc_make_regions(const enc_totals& t, int B) {
    enc_regions r;
    r.layout = 0;
    r.coef = up256(r.layout + (size_t)B * sizeof(enc_layout));
    r.bits = up256(r.coef + (size_t)t.blocks * 128);
    r.chunk = up256(r.bits + (size_t)t.blocks * 4);
    r.word = up256(r.chunk + (size_t)t.chunks * 4);
    r.bchunk = up256(r.word + (size_t)t.words * 4);
    r.total = up256(r.bchunk + (size_t)t.bchunks * 4);
    return r;
}

// 0, or the YV3_E* code of the first record that is no image this encoder takes
int enc_host_totals(const yv3_jpeg_enc_image* im, int B, enc_totals* t) {
    *t = enc_totals{};
    for (int b = 0; b < B; ++b) {
        const yv3_jpeg_enc_image& i = im[b];
        if (i.width < 1 || i.height < 1 || (i.ncomp != 1 && i.ncomp != 3) || i.subsampling < 0 || i.subsampling > 2 || i.quality < 1 ||
            i.quality > 100 || i.pitch < (long long)i.width * i.ncomp)
            return YV3_EINVAL;
        const yv3_enc_geom g = yv3_enc_geometry(i.width, i.height, i.ncomp, i.subsampling, i.quality, i.pitch);
        if (!g.ok) return YV3_ELIMIT;
        t->blocks += g.nblk;
        t->chunks += enc_chunks(g.nblk);
        t->words += enc_words(g.nblk);
        t->bchunks += enc_bchunks(g.nblk);
        if (g.nblk > t->max_blocks) t->max_blocks = g.nblk;
        if (enc_words(g.nblk) > t->max_words) t->max_words = enc_words(g.nblk);
        if (enc_bchunks(g.nblk) > t->max_bchunks) t->max_bchunks = enc_bchunks(g.nblk);
    }
    return 0;
}

// ---- layout: the device's own reading of the records, held to the capacities the host sized the workspace and the grids by ----
__global__ void enc_layout_kernel(const yv3_jpeg_enc_image* __restrict__ images, int B, enc_totals cap, enc_layout* __restrict__ layout,
                                  int* __restrict__ out_len, int* __restrict__ status) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long blocks = 0, chunks = 0, words = 0, bchunks = 0;
    for (int b = 0; b < B; ++b) {
        const yv3_jpeg_enc_image im = images[b];
        enc_layout l = {};
        int st = 0;
        l.g = yv3_enc_geometry(im.width, im.height, im.ncomp, im.subsampling, im.quality, im.pitch);
        if (!l.g.ok || !im.pixels || !im.out || im.out_cap < 0) {
            st = YV3_JPEGE_S_INFO;
        } else {
            l.nchunks = enc_chunks(l.g.nblk);
            l.words_cap = enc_words(l.g.nblk);
            l.nbchunks_cap = enc_bchunks(l.g.nblk);
            if (blocks + l.g.nblk > cap.blocks || chunks + l.nchunks > cap.chunks || words + l.words_cap > cap.words ||
                bchunks + l.nbchunks_cap > cap.bchunks || l.g.nblk > cap.max_blocks || l.words_cap > cap.max_words ||
                l.nbchunks_cap > cap.max_bchunks)
                st = YV3_JPEGE_S_BOUNDS;
        }
        if (st) {
            l = enc_layout{};
        } else {
            l.blk0 = blocks;
            l.chunk0 = chunks;
            l.word0 = words;
            l.bchunk0 = bchunks;
            l.hdr_len = yv3_enc_header_length(im.ncomp);             // (writing it is enc_finish_kernel's, one workgroup per image)
            blocks += l.g.nblk;
            chunks += l.nchunks;
            words += l.words_cap;
            bchunks += l.nbchunks_cap;
        }
        layout[b] = l;
        status[b] = st;
        out_len[b] = 0;
    }
}

// ---- coefficients --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(T) enc_coef_kernel(const yv3_jpeg_enc_image* __restrict__ images, const enc_layout* __restrict__ layout,
                                                     int16_t* __restrict__ coef) {
    const int b = blockIdx.y;
    const enc_layout& l = layout[b];
    if (!l.g.ok || (unsigned)blockIdx.x * T >= l.g.nblk) return;                    // (uniform over the workgroup)
    __shared__ uint16_t q[2][64];
    const yv3_jpeg_enc_image im = images[b];
    if (threadIdx.x < 128) {
        const int t = threadIdx.x >> 6, i = threadIdx.x & 63;
        const int scale = im.quality < 50 ? 5000 / im.quality : 200 - 2 * im.quality;
        const int v = (D_TAB.quant[t][i] * scale + 50) / 100;
        q[t][i] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
    __syncthreads();
    const unsigned idx = blockIdx.x * T + threadIdx.x;
    if (idx >= l.g.nblk) return;
    const yv3_enc_block blk = yv3_enc_locate(l.g, idx);
    yv3_enc_block src = blk;                                                        // a dummy block: the last real block before it in the MCU
    for (unsigned back = 1; src.dummy; ++back) src = yv3_enc_locate(l.g, idx - back);
    int d[64];
    yv3_enc_load_block(im.pixels, im.pitch, im.width, im.height, im.ncomp, l.g, src.comp, src.bx, src.by, d);
    yv3_enc_fdct_quantise(d, q[src.comp ? 1 : 0]);
    uint4* out = reinterpret_cast<uint4*>(coef + (l.blk0 + idx) * 64);
    for (int k8 = 0; k8 < 8; ++k8) {
        unsigned w[4];
        for (int j = 0; j < 4; ++j) {
            const int k = k8 * 8 + 2 * j;
            const int lo = blk.dummy && k ? 0 : d[D_TAB.natural_of_zigzag[k]], hi = blk.dummy ? 0 : d[D_TAB.natural_of_zigzag[k + 1]];
            w[j] = ((unsigned)lo & 0xFFFFu) | ((unsigned)hi << 16);
        }
        out[k8] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ---- scans over a workgroup of 256 threads (four wave64 scans and their four sums) ---------------------------------------------------
__device__ inline unsigned group_exclusive_scan(unsigned v, unsigned* total, unsigned* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    unsigned base = 0, tot = 0;
    for (int i = 0; i < T / 64; ++i) {
        if (i < wave) base += lds[i];
        tot += lds[i];
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

__device__ inline int pred_dc(const int16_t* coef, const enc_layout& l, const yv3_enc_block& blk) {
    return blk.pred < 0 ? 0 : coef[(l.blk0 + blk.pred) * 64];
}

__global__ void __launch_bounds__(T) enc_size_kernel(const enc_layout* __restrict__ layout, const int16_t* __restrict__ coef,
                                                     unsigned* __restrict__ block_bits, unsigned* __restrict__ chunk_bits,
                                                     int* __restrict__ status) {
    __shared__ unsigned lds[T / 64];
    const int b = blockIdx.y;
    const enc_layout& l = layout[b];
    if (!l.g.ok || blockIdx.x >= l.nchunks) return;
    const unsigned idx = blockIdx.x * T + threadIdx.x;
    unsigned bits = 0;
    if (idx < l.g.nblk) {
        const yv3_enc_block blk = yv3_enc_locate(l.g, idx);
        const int t = blk.comp ? 1 : 0;
        yv3_enc_count_sink sink;
        if (!yv3_enc_block_tokens(coef + (l.blk0 + idx) * 64, pred_dc(coef, l, blk), D_TAB.dc[t], D_TAB.ac[t], sink))
            status[b] = YV3_JPEGE_S_RANGE;
        bits = sink.bits;
        block_bits[l.blk0 + idx] = bits;
    }
    unsigned total;
    group_exclusive_scan(bits, &total, lds);
    if (threadIdx.x == 0) chunk_bits[l.chunk0 + blockIdx.x] = total;
}

// in place: counts[i] becomes the sum of the counts before it; returns the sum of all
__device__ inline unsigned scan_in_place(unsigned* counts, unsigned n, unsigned* lds) {
    unsigned carry = 0;
    for (unsigned i0 = 0; i0 < n; i0 += T) {
        const unsigned i = i0 + threadIdx.x;
        const unsigned v = i < n ? counts[i] : 0;
        unsigned total;
        const unsigned ex = group_exclusive_scan(v, &total, lds);
        if (i < n) counts[i] = carry + ex;
        carry += total;
    }
    return carry;
}

__global__ void __launch_bounds__(T) enc_scan_kernel(enc_layout* __restrict__ layout, unsigned* __restrict__ chunk_bits) {
    __shared__ unsigned lds[T / 64];
    enc_layout& l = layout[blockIdx.x];
    if (!l.g.ok) return;
    const unsigned total = scan_in_place(chunk_bits + l.chunk0, l.nchunks, lds);
    if (threadIdx.x == 0) {
        l.total_bits = total;
        l.nbytes = (unsigned)(((unsigned long long)total + 7) / 8);
    }
}

__global__ void __launch_bounds__(T) enc_zero_kernel(const enc_layout* __restrict__ layout, unsigned* __restrict__ words) {
    const enc_layout& l = layout[blockIdx.y];
    if (!l.g.ok) return;
    const unsigned used = l.total_bits / 32 + 2;                                    // <= words_cap: total_bits <= nblk * YV3_ENC_BLOCK_BITS
    const unsigned w = (blockIdx.x * T + threadIdx.x) * 4;
    if (w < used && w + 4 <= l.words_cap) *reinterpret_cast<uint4*>(words + l.word0 + w) = make_uint4(0, 0, 0, 0);
}

// bits most significant first: bit p of the scan is bit 31 - p % 32 of word p / 32
struct enc_bit_sink {
    unsigned* words;
    unsigned long long acc;
    int n;
    bool first;
    __device__ void put(uint32_t code, int len) {
        acc |= (unsigned long long)code << (64 - n - len);
        n += len;
        if (n >= 32) {
            const unsigned w = (unsigned)(acc >> 32);
            if (first) atomicOr(words, w); else *words = w;                         // the first word holds the end of the block before
            first = false;
            ++words;
            acc <<= 32;
            n -= 32;
        }
    }
    __device__ void finish() {
        if (n) atomicOr(words, (unsigned)(acc >> 32));                              // the last word holds the start of the next block
    }
};

__global__ void __launch_bounds__(T) enc_emit_kernel(const enc_layout* __restrict__ layout, const int16_t* __restrict__ coef,
                                                     const unsigned* __restrict__ block_bits, const unsigned* __restrict__ chunk_bits,
                                                     unsigned* __restrict__ words) {
    __shared__ unsigned lds[T / 64];
    const int b = blockIdx.y;
    const enc_layout& l = layout[b];
    if (!l.g.ok || blockIdx.x >= l.nchunks) return;
    const unsigned idx = blockIdx.x * T + threadIdx.x;
    const bool live = idx < l.g.nblk;
    unsigned total;
    const unsigned offset = chunk_bits[l.chunk0 + blockIdx.x] + group_exclusive_scan(live ? block_bits[l.blk0 + idx] : 0, &total, lds);
    if (!live) return;
    const yv3_enc_block blk = yv3_enc_locate(l.g, idx);
    const int t = blk.comp ? 1 : 0;
    enc_bit_sink sink = {words + l.word0 + offset / 32, 0, (int)(offset % 32), true};
    yv3_enc_block_tokens(coef + (l.blk0 + idx) * 64, pred_dc(coef, l, blk), D_TAB.dc[t], D_TAB.ac[t], sink);
    sink.finish();
}

// ---- stuffing ------------------------------------------------------------------------------------------------------------------
// the 16 scan bytes of this thread (first byte index i0; bytes from nbytes on read as 0), the last byte of the scan padded with ones
__device__ inline void load_bytes(const enc_layout& l, const unsigned* words, unsigned i0, unsigned char* byte) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (i0 < l.nbytes) v = *reinterpret_cast<const uint4*>(words + l.word0 + i0 / 4);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    for (int j = 0; j < 16; ++j) {
        unsigned c = (w[j >> 2] >> (24 - 8 * (j & 3))) & 255u;
        const unsigned i = i0 + j;
        if (i + 1 == l.nbytes && (l.total_bits & 7)) c |= (1u << (8 - (l.total_bits & 7))) - 1;
        byte[j] = (unsigned char)(i < l.nbytes ? c : 0);
    }
}

__global__ void __launch_bounds__(T) enc_count_kernel(const enc_layout* __restrict__ layout, const unsigned* __restrict__ words,
                                                      unsigned* __restrict__ chunk_ff) {
    __shared__ unsigned lds[T / 64];
    const enc_layout& l = layout[blockIdx.y];
    if (!l.g.ok || (unsigned long long)blockIdx.x * YV3_ENC_BYTE_CHUNK >= l.nbytes) return;
    unsigned char byte[16];
    load_bytes(l, words, (blockIdx.x * T + threadIdx.x) * 16, byte);
    unsigned n = 0, total;
    for (int j = 0; j < 16; ++j) n += byte[j] == 0xFF;
    group_exclusive_scan(n, &total, lds);
    if (threadIdx.x == 0) chunk_ff[l.bchunk0 + blockIdx.x] = total;
}

__global__ void __launch_bounds__(T) enc_finish_kernel(const yv3_jpeg_enc_image* __restrict__ images, enc_layout* __restrict__ layout,
                                                       unsigned* __restrict__ chunk_ff, int* __restrict__ out_len, int* __restrict__ status) {
    __shared__ unsigned lds[T / 64];
    const int b = blockIdx.x;
    enc_layout& l = layout[b];
    if (!l.g.ok) return;
    const unsigned nff = scan_in_place(chunk_ff + l.bchunk0, (l.nbytes + YV3_ENC_BYTE_CHUNK - 1) / YV3_ENC_BYTE_CHUNK, lds);
    if (threadIdx.x != 0) return;
    const yv3_jpeg_enc_image im = images[b];
    const long long total = (long long)l.hdr_len + l.nbytes + nff + 2;
    out_len[b] = (int)total;                                                        // the length the file has, or would have had
    if (status[b] != 0) return;                                                     // (YV3_JPEGE_S_RANGE from enc_size_kernel)
    if (total > im.out_cap) {
        status[b] = YV3_JPEGE_S_SPACE;
        return;
    }
    l.fits = 1;
    yv3_enc_write_header(D_SPEC, im.width, im.height, im.ncomp, l.g.hs, l.g.vs, im.quality, im.out, im.out_cap);
    im.out[total - 2] = 0xFF;
    im.out[total - 1] = 0xD9;
}

__global__ void __launch_bounds__(T) enc_scatter_kernel(const yv3_jpeg_enc_image* __restrict__ images, const enc_layout* __restrict__ layout,
                                                        const unsigned* __restrict__ words, const unsigned* __restrict__ chunk_ff) {
    __shared__ unsigned lds[T / 64];
    const int b = blockIdx.y;
    const enc_layout& l = layout[b];
    if (!l.fits || (unsigned long long)blockIdx.x * YV3_ENC_BYTE_CHUNK >= l.nbytes) return;
    unsigned char byte[16];
    const unsigned i0 = (blockIdx.x * T + threadIdx.x) * 16;
    load_bytes(l, words, i0, byte);
    unsigned n = 0, total;
    for (int j = 0; j < 16; ++j) n += byte[j] == 0xFF;
    const unsigned before = chunk_ff[l.bchunk0 + blockIdx.x] + group_exclusive_scan(n, &total, lds);
    unsigned char* out = images[b].out + l.hdr_len + (long long)i0 + before;       // finish checked the whole file against the capacity
    for (int j = 0; j < 16 && i0 + j < l.nbytes; ++j) {
        *out++ = byte[j];
        if (byte[j] == 0xFF) *out++ = 0;
    }
}

int enc_subsampling_ok(int ncomp, int subsampling) { return (ncomp == 1 || ncomp == 3) && subsampling >= 0 && subsampling <= 2; }

}  // namespace

extern "C" long long yv3_jpeg_encode_header(int width, int height, int ncomp, int subsampling, int quality, unsigned char* out, long long cap) {
    if (width < 1 || height < 1 || !enc_subsampling_ok(ncomp, subsampling) || quality < 1 || quality > 100 || cap < 0 || (cap && !out))
        return YV3_EINVAL;
    if (width > YV3_ENC_MAX_SIDE || height > YV3_ENC_MAX_SIDE) return YV3_ELIMIT;
    const yv3_enc_geom g = yv3_enc_geometry(width, height, ncomp, subsampling, quality, (long long)width * ncomp);
    if (!g.ok) return YV3_ELIMIT;
    const int n = yv3_enc_write_header(YV3_ENC_SPEC, width, height, ncomp, g.hs, g.vs, quality, out, cap);
    return n == yv3_enc_header_length(ncomp) ? n : YV3_EINVAL;        // (the kernels lay the file out by the closed form)
}

extern "C" long long yv3_jpeg_encode_bound(int width, int height, int ncomp, int subsampling) {
    if (width < 1 || height < 1 || !enc_subsampling_ok(ncomp, subsampling)) return YV3_EINVAL;
    const yv3_enc_geom g = yv3_enc_geometry(width, height, ncomp, subsampling, 75, (long long)width * ncomp);
    if (!g.ok) return YV3_ELIMIT;
    const long long scan = ((long long)g.nblk * YV3_ENC_BLOCK_BITS + 7) / 8;
    return yv3_enc_header_length(ncomp) + 2 * scan + 2;
}

extern "C" size_t yv3_jpeg_encode_workspace_bytes(const yv3_jpeg_enc_image* images_host, int B) {
    enc_totals t;
    if (!images_host || B < 1 || B > 65535 || enc_host_totals(images_host, B, &t)) return 0;
    return enc_make_regions(t, B).total;
}

extern "C" int yv3_jpeg_encode_batch(const yv3_jpeg_enc_desc* desc, void* ws, size_t ws_bytes, void* stream) {
    if (!desc || !desc->images || !desc->images_host || !desc->out_len || !desc->status || !ws || ((uintptr_t)ws & 255)) return YV3_EINVAL;
    const int B = desc->B;
    if (B < 1 || B > 65535) return YV3_EINVAL;
    enc_totals t;
    if (const int rc = enc_host_totals(desc->images_host, B, &t)) return rc;
    for (int b = 0; b < B; ++b)
        if (!desc->images_host[b].pixels || !desc->images_host[b].out || desc->images_host[b].out_cap < 0) return YV3_EINVAL;
    const enc_regions r = enc_make_regions(t, B);
    if (ws_bytes < r.total) return YV3_EWORKSPACE;
    char* base = static_cast<char*>(ws);
    enc_layout* layout = reinterpret_cast<enc_layout*>(base + r.layout);
    int16_t* coef = reinterpret_cast<int16_t*>(base + r.coef);
    unsigned* block_bits = reinterpret_cast<unsigned*>(base + r.bits);
    unsigned* chunk_bits = reinterpret_cast<unsigned*>(base + r.chunk);
    unsigned* words = reinterpret_cast<unsigned*>(base + r.word);
    unsigned* chunk_ff = reinterpret_cast<unsigned*>(base + r.bchunk);
    hipStream_t s = (hipStream_t)stream;
    const dim3 per_block(enc_chunks(t.max_blocks), B), per_bytes(t.max_bchunks, B);

    hipLaunchKernelGGL(enc_layout_kernel, dim3(1), dim3(64), 0, s, desc->images, B, t, layout, desc->out_len, desc->status);
    YV3_CHECK_LAUNCH();
    hipLaunchKernelGGL(enc_coef_kernel, per_block, dim3(T), 0, s, desc->images, layout, coef);
    YV3_CHECK_LAUNCH();
    hipLaunchKernelGGL(enc_size_kernel, per_block, dim3(T), 0, s, layout, coef, block_bits, chunk_bits, desc->status);
    YV3_CHECK_LAUNCH();
    hipLaunchKernelGGL(enc_scan_kernel, dim3(B), dim3(T), 0, s, layout, chunk_bits);
    YV3_CHECK_LAUNCH();
    hipLaunchKernelGGL(enc_zero_kernel, dim3((t.max_words + 4 * T - 1) / (4 * T), B), dim3(T), 0, s, layout, words);
    YV3_CHECK_LAUNCH();
    hipLaunchKernelGGL(enc_emit_kernel, per_block, dim3(T), 0, s, layout, coef, block_bits, chunk_bits, words);
    YV3_CHECK_LAUNCH();
    hipLaunchKernelGGL(enc_count_kernel, per_bytes, dim3(T), 0, s, layout, words, chunk_ff);
    YV3_CHECK_LAUNCH();
    hipLaunchKernelGGL(enc_finish_kernel, dim3(B), dim3(T), 0, s, desc->images, layout, chunk_ff, desc->out_len, desc->status);
    YV3_CHECK_LAUNCH();
    hipLaunchKernelGGL(enc_scatter_kernel, per_bytes, dim3(T), 0, s, desc->images, layout, words, chunk_ff);
    YV3_CHECK_LAUNCH();
    return 0;
}
