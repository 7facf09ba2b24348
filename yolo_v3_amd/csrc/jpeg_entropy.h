// Baseline JPEG: the frame geometry, the Huffman decode tables and the entropy decode of one unit (a whole scan, or one restart
// segment when DRI is set), as inline functions that compile for the GPU (jpeg.hip) and, without HIP, for the host
// (jpeg_parse.cpp, the stand-alone sanitizer program of tests/test_jpeg_host.py).  Every access is bounded: the bit reader by the
// unit's byte range (bits past its end read as 0 and are counted), block indices by the image's block count, coefficient indices
// by 63.  Damaged data gives a YV3_JPEG_S_* status, never a wild access.
#pragma once
#include <stdint.h>
#include "yv3.h"

#ifdef __HIPCC__
#define YV3_HD __host__ __device__ static inline
#define YV3_UNROLL _Pragma("unroll")
#else
#define YV3_HD static inline
#define YV3_UNROLL
#endif

#define YV3_JPEG_MAX_SIDE 16384
#define YV3_JPEG_LOOK_BITS 9

// What the kernels need of a frame, derived from a yv3_jpeg_info.  Component c is stored as a plane of bw[c] x bh[c] blocks
// (whole MCUs); block (by, bx) of component c is block base[c] + by * bw[c] + bx of the image.
struct yv3_jpeg_geom {
    int ncomp, hmax, vmax;
    int mcu_w, mcu_h, nmcu, nunits, mcus_per_unit, nblocks;
    int h[3], v[3], bw[3], bh[3], base[3];
    int cw[3], ch[3];                    // true size of each component: ceil(W * h / hmax) x ceil(H * v / vmax)
    long long coef_bytes, plane_bytes, unit_bytes, total_bytes;     // the image's share of the workspace (256-aligned parts)
};

YV3_HD long long yv3_jpeg_round256(long long n) { return (n + 255) / 256 * 256; }

// 0, or YV3_JPEG_S_INFO for a record yv3_jpeg_parse cannot have accepted (whatever its bytes are)
YV3_HD int yv3_jpeg_geometry(const yv3_jpeg_info* f, yv3_jpeg_geom* g) {
    if (f->reason != 0) return YV3_JPEG_S_INFO;
    if (f->width < 1 || f->height < 1 || f->width > YV3_JPEG_MAX_SIDE || f->height > YV3_JPEG_MAX_SIDE) return YV3_JPEG_S_INFO;
    if (f->ncomp != 1 && f->ncomp != 3) return YV3_JPEG_S_INFO;
    if (f->restart_interval < 0 || f->restart_interval > 65535) return YV3_JPEG_S_INFO;
    if (f->scan_offset < 0 || f->scan_length < 0) return YV3_JPEG_S_INFO;
    g->ncomp = f->ncomp;
    for (int c = 0; c < f->ncomp; ++c) {
        if (f->tq[c] > 3 || f->td[c] > 3 || f->ta[c] > 3) return YV3_JPEG_S_INFO;
        if (!f->quant_defined[f->tq[c]] || !f->huff_defined[f->td[c]] || !f->huff_defined[4 + f->ta[c]]) return YV3_JPEG_S_INFO;
        const int h = f->h[c], v = f->v[c];
        if (c == 0) { if (!((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2))) return YV3_JPEG_S_INFO; }
        else if (h != 1 || v != 1) return YV3_JPEG_S_INFO;
        g->h[c] = h; g->v[c] = v;
    }
    if (f->ncomp == 1) { g->h[0] = 1; g->v[0] = 1; }          // a one-component scan is not interleaved: one block per MCU
    g->hmax = g->h[0]; g->vmax = g->v[0];
    g->mcu_w = (f->width + 8 * g->hmax - 1) / (8 * g->hmax);
    g->mcu_h = (f->height + 8 * g->vmax - 1) / (8 * g->vmax);
    g->nmcu = g->mcu_w * g->mcu_h;                            // <= 2048 * 2048
    g->mcus_per_unit = f->restart_interval ? f->restart_interval : g->nmcu;
    g->nunits = (g->nmcu + g->mcus_per_unit - 1) / g->mcus_per_unit;
    int base = 0;
    for (int c = 0; c < g->ncomp; ++c) {
        g->bw[c] = g->mcu_w * g->h[c]; g->bh[c] = g->mcu_h * g->v[c]; g->base[c] = base;
        base += g->bw[c] * g->bh[c];
        g->cw[c] = (f->width * g->h[c] + g->hmax - 1) / g->hmax;
        g->ch[c] = (f->height * g->v[c] + g->vmax - 1) / g->vmax;
    }
    g->nblocks = base;                                         // <= 3 * 2048 * 2048
    g->coef_bytes = yv3_jpeg_round256((long long)base * 128);
    g->plane_bytes = yv3_jpeg_round256((long long)base * 64);
    g->unit_bytes = yv3_jpeg_round256((long long)g->nunits * 4);
    g->total_bytes = g->coef_bytes + g->plane_bytes + g->unit_bytes;
    return 0;
}

// One Huffman table: a 9-bit lookahead (length << 8 | symbol, 0 = longer code) and, for the longer codes, libjpeg's
// maxcode / valoffset walk.  1420 bytes; eight of them fit a workgroup's LDS many times over.
struct yv3_jpeg_hufftab {
    uint16_t look[1 << YV3_JPEG_LOOK_BITS];
    int32_t maxcode[18];               // [l]: largest code of length l (-1: none), [17]: a sentinel above every 16-bit code
    int32_t valoff[17];                // [l]: index of the first value of length l minus its code
    uint8_t vals[256];
};

// 0 or YV3_JPEG_S_HUFFTABLE (more than 256 codes, or a length whose codes do not fit it).  max_value: 15 for a DC table.
YV3_HD int yv3_jpeg_build_hufftab(const unsigned char* counts, const unsigned char* values, int max_value, yv3_jpeg_hufftab* t) {
    int total = 0;
    for (int l = 0; l < 16; ++l) total += counts[l];
    if (total > 256) return YV3_JPEG_S_HUFFTABLE;
    for (int i = 0; i < (1 << YV3_JPEG_LOOK_BITS); ++i) t->look[i] = 0;
    for (int i = 0; i < 256; ++i) t->vals[i] = i < total ? values[i] : 0;
    for (int i = 0; i < total; ++i) if (values[i] > max_value) return YV3_JPEG_S_HUFFTABLE;
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = counts[l - 1];
        if (code + n > (1 << l)) return YV3_JPEG_S_HUFFTABLE;
        t->valoff[l] = k - code;
        t->maxcode[l] = n ? code + n - 1 : -1;
        if (l <= YV3_JPEG_LOOK_BITS) {
            for (int i = 0; i < n; ++i) {
                const int first = (code + i) << (YV3_JPEG_LOOK_BITS - l), span = 1 << (YV3_JPEG_LOOK_BITS - l);
                for (int j = 0; j < span; ++j) t->look[first + j] = (uint16_t)((l << 8) | t->vals[k + i]);
            }
        }
        code = (code + n) << 1;
        k += n;
    }
    t->maxcode[17] = 0x7fffffff;
    t->valoff[0] = 0; t->maxcode[0] = -1;
    return 0;
}

// The bit reader of one unit: bytes [pos, end) of the scan, FF 00 unstuffed.  Past `end` it supplies zero bits and counts
// them in `pad`; an FF followed by anything but 00 inside a unit (units are cut at the markers) sets `bad`.
struct yv3_jpeg_bits {
    const unsigned char* scan;
    long long pos, end;
    unsigned long long acc;             // the next bits, left-aligned
    int n, pad, bad;                    // valid bits in acc; how many of the last ones are padding
};

YV3_HD void yv3_jpeg_fill(yv3_jpeg_bits& b) {
    while (b.n <= 56) {
        unsigned long long c = 0;
        if (b.pos < b.end) {
            c = b.scan[b.pos++];
            if (c == 0xFF) {                                   // FF 00 is a data byte FF; FF before anything else is a marker
                if (b.pos < b.end && b.scan[b.pos] == 0) ++b.pos;
                else { b.bad = 1; b.pos = b.end; c = 0; b.pad += 8; }
            }
        } else {
            b.pad += 8;
        }
        b.acc |= c << (56 - b.n);
        b.n += 8;
    }
}

YV3_HD int yv3_jpeg_peek(const yv3_jpeg_bits& b, int k) { return (int)(b.acc >> (64 - k)); }      // 1 <= k <= 16, after a fill
YV3_HD void yv3_jpeg_skip(yv3_jpeg_bits& b, int k) { b.acc <<= k; b.n -= k; }

// One symbol, or -1 for a pattern that is no code.  Needs 16 valid bits (a fill gives 57).
YV3_HD int yv3_jpeg_symbol(yv3_jpeg_bits& b, const yv3_jpeg_hufftab* t) {
    const int e = t->look[yv3_jpeg_peek(b, YV3_JPEG_LOOK_BITS)];
    if (e) { yv3_jpeg_skip(b, e >> 8); return e & 255; }
    const int code16 = yv3_jpeg_peek(b, 16);
    int l = YV3_JPEG_LOOK_BITS + 1;
    while (l <= 16 && (code16 >> (16 - l)) > t->maxcode[l]) ++l;
    if (l > 16) return -1;
    const int idx = t->valoff[l] + (code16 >> (16 - l));
    if ((unsigned)idx > 255u) return -1;
    yv3_jpeg_skip(b, l);
    return t->vals[idx];
}

// s bits as a signed value (ITU T.81 F.2.2.1 EXTEND), 1 <= s <= 16
YV3_HD int yv3_jpeg_receive_extend(yv3_jpeg_bits& b, int s) {
    const int v = yv3_jpeg_peek(b, s);
    yv3_jpeg_skip(b, s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// zigzag position -> natural (row-major) index
#define YV3_JPEG_NATURAL_ORDER {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, \
                                28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, \
                                54, 47, 55, 62, 63}
YV3_HD int yv3_jpeg_natural(int k) {
    const unsigned char zz[64] = YV3_JPEG_NATURAL_ORDER;
    return zz[k & 63];
}

// Whether a restart marker (FF D0 .. FF D7) stands at byte i of a scan of len bytes
YV3_HD bool yv3_jpeg_restart_at(const unsigned char* scan, long long i, long long len) {
    return i + 1 < len && scan[i] == 0xFF && (scan[i + 1] & 0xF8) == 0xD0;
}

// The byte range [*begin, *end) of unit u of a scan of len bytes and nunits units, between the restart markers found at
// marks[0 .. nunits - 2] (int in the kernels, long long in the host programs).  0, or YV3_JPEG_S_MARKER for markers out of
// order or out of range.  Which MCUs or items the unit holds is the caller's: baseline and progressive scans differ there.
template <typename M>
YV3_HD int yv3_jpeg_unit_bytes(const unsigned char* scan, long long len, const M* marks, int nunits, int u, long long* begin,
                               long long* end) {
    int code = 0;
    *begin = 0; *end = len;
    if (u > 0) *begin = (long long)marks[u - 1] + 2;
    if (u < nunits - 1) {
        *end = marks[u];
        if (*end < 0 || *end + 1 >= len || scan[*end + 1] != 0xD0 + (u & 7)) code = YV3_JPEG_S_MARKER;
    }
    if (*begin < 0 || *begin > len || *end < *begin) code = YV3_JPEG_S_MARKER;
    return code;
}

// Decodes MCUs [mcu0, mcu1) of the frame from bytes [begin, end) of `scan` into coef ([nblocks][64] int16, natural order,
// zeroed by the caller: EOB and runs leave zeros).  tabs: the eight tables (DC 0..3, AC 0..3); td / ta: the selectors per
// component; natural: yv3_jpeg_natural as a table of 64 (the kernel keeps it in LDS).  DC prediction starts at 0 (a unit
// begins the scan or follows a restart marker).  Returns 0 or YV3_JPEG_S_*.
YV3_HD int yv3_jpeg_decode_unit(const unsigned char* scan, long long begin, long long end, const yv3_jpeg_geom* g,
                                const yv3_jpeg_hufftab* tabs, const unsigned char* td, const unsigned char* ta,
                                const unsigned char* natural, int mcu0, int mcu1, short* coef, int nblocks) {
    yv3_jpeg_bits b;
    b.scan = scan; b.pos = begin; b.end = end; b.acc = 0; b.n = 0; b.pad = 0; b.bad = 0;
    int pred[3] = {0, 0, 0};
    for (int mcu = mcu0; mcu < mcu1; ++mcu) {
        const int my = mcu / g->mcu_w, mx = mcu - my * g->mcu_w;
        for (int c = 0; c < g->ncomp; ++c) {
            const yv3_jpeg_hufftab* dc = tabs + (td[c] & 3);
            const yv3_jpeg_hufftab* ac = tabs + 4 + (ta[c] & 3);
            for (int vy = 0; vy < g->v[c]; ++vy)
                for (int hx = 0; hx < g->h[c]; ++hx) {
                    const long long blk = (long long)g->base[c] + (long long)(my * g->v[c] + vy) * g->bw[c] + mx * g->h[c] + hx;
                    if (blk < 0 || blk >= nblocks) return YV3_JPEG_S_COEF;
                    short* out = coef + blk * 64;
                    yv3_jpeg_fill(b);
                    int s = yv3_jpeg_symbol(b, dc);
                    if (s < 0 || s > 15) return YV3_JPEG_S_CODE;
                    if (s) { yv3_jpeg_fill(b); pred[c] += yv3_jpeg_receive_extend(b, s); }
                    if (pred[c] < -32768 || pred[c] > 32767) return YV3_JPEG_S_DC;
                    out[0] = (short)pred[c];
                    for (int k = 1; k < 64; ++k) {
                        yv3_jpeg_fill(b);
                        const int rs = yv3_jpeg_symbol(b, ac);
                        if (rs < 0) return YV3_JPEG_S_CODE;
                        const int r = rs >> 4;
                        s = rs & 15;
                        if (s) {
                            k += r;
                            if (k > 63) return YV3_JPEG_S_COEF;
                            out[natural[k]] = (short)yv3_jpeg_receive_extend(b, s);
                        } else if (r == 15) {
                            k += 15;
                            if (k > 63) return YV3_JPEG_S_COEF;
                        } else {
                            break;                                                  // EOB
                        }
                    }
                    if (b.bad) return YV3_JPEG_S_MARKER;
                    if (b.pad > b.n) return YV3_JPEG_S_OVERRUN;                     // this block used bits that are not there
                }
        }
    }
    if (b.bad) return YV3_JPEG_S_MARKER;
    if (b.pos < b.end || b.n - b.pad >= 8) return YV3_JPEG_S_EXTRA;                 // an encoder pads to the next byte only
    return 0;
}
