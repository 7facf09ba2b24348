// Progressive JPEG (SOF2, ITU T.81 annex G): the checks of a yv3_jpeg_prog record, the level schedule of its scans and the entropy
// decode of one unit of one scan (a whole scan or one of its restart segments), as inline functions for the GPU (jpeg.hip) and,
// without HIP, for the host (jpeg_parse.cpp, the stand-alone sanitizer program of tests/test_jpeg_prog_host.py).  The bit reader,
// the table builder and the natural-order table are jpeg_entropy.h's.  Every access is bounded as there; everything libjpeg
// would warn about is a status.
#pragma once
#include <string.h>
#include "jpeg_entropy.h"

#define YV3_JPEGP_LEVEL_TABLES 8          // Huffman tables one level may use: what the kernel keeps in LDS

// The frame of an accepted progressive file as the baseline geometry, IDCT and colour code read it: *f becomes a record
// yv3_jpeg_geometry accepts (no scan, selectors 0).  Only the new entry points do this, on copies of their own.
YV3_HD void yv3_jpegp_as_frame(yv3_jpeg_info* f) {
    f->reason = 0; f->restart_interval = 0; f->scan_offset = 0; f->scan_length = 0;
    for (int c = 0; c < 4; ++c) { f->td[c] = 0; f->ta[c] = 0; }
    f->huff_defined[0] = 1; f->huff_defined[4] = 1;
}

// The blocks a scan walks and its units: an interleaved scan walks the frame's MCUs, a one-component scan the component's own
// block grid, ceil(cw / 8) x ceil(ch / 8), which the restart interval counts.  (g of a one-component frame has h = v = 1.)
YV3_HD int yv3_jpegp_scan_items(const yv3_jpeg_geom* g, int ns, int c0) {
    if (ns > 1) return g->nmcu;
    return ((g->cw[c0] + 7) / 8) * ((g->ch[c0] + 7) / 8);
}
YV3_HD int yv3_jpegp_scan_units(int items, int restart_interval) {
    return restart_interval ? (items + restart_interval - 1) / restart_interval : 1;
}

// 0, or YV3_JPEG_S_INFO for a record yv3_jpeg_parse_ex cannot have produced (whatever its bytes are).  *total_units: the sum
// of the scans' unit counts (<= 64 * 3 * 2048 * 2048), which sizes the image's share of restart offsets.
YV3_HD int yv3_jpegp_check(const yv3_jpeg_prog* p, const yv3_jpeg_geom* g, long long* total_units) {
    *total_units = 0;
    if (p->accepted != 1 || p->nscans < 1 || p->nscans > YV3_JPEGP_MAX_SCANS || p->ntables < 0 || p->ntables > YV3_JPEGP_MAX_TABLES)
        return YV3_JPEG_S_INFO;
    for (int i = 0; i < p->nscans; ++i) {
        const yv3_jpegp_scan* s = p->scans + i;
        if (s->ns < 1 || s->ns > 3 || s->ns > g->ncomp) return YV3_JPEG_S_INFO;
        for (int j = 0; j < s->ns; ++j) {
            if (s->comp[j] >= g->ncomp || (j && s->comp[j] <= s->comp[j - 1])) return YV3_JPEG_S_INFO;
        }
        if (s->ss == 0 ? s->se != 0 : (s->ns != 1 || s->se < s->ss || s->se > 63)) return YV3_JPEG_S_INFO;
        if (s->al > 13 || (s->ah != 0 && s->ah != s->al + 1)) return YV3_JPEG_S_INFO;
        if (s->ss == 0 && s->ah == 0) { for (int j = 0; j < s->ns; ++j) if (s->tab[j] >= p->ntables) return YV3_JPEG_S_INFO; }
        if (s->ss > 0 && s->tab[0] >= p->ntables) return YV3_JPEG_S_INFO;
        if (s->restart_interval < 0 || s->restart_interval > 65535) return YV3_JPEG_S_INFO;
        if (s->offset < 0 || s->length < 0 || s->length > 0x7fffffffLL) return YV3_JPEG_S_INFO;
        *total_units += yv3_jpegp_scan_units(yv3_jpegp_scan_items(g, s->ns, s->comp[0]), s->restart_interval);
    }
    return 0;
}

// The geometry of an accepted progressive image from its frame record (after yv3_jpegp_as_frame) and its progressive record:
// yv3_jpeg_geometry's, with the restart-offset share sized for all scans' units.  0 or YV3_JPEG_S_INFO.
YV3_HD int yv3_jpegp_geometry(const yv3_jpeg_info* frame, const yv3_jpeg_prog* p, yv3_jpeg_geom* g) {
    long long units;
    if (yv3_jpeg_geometry(frame, g) != 0 || yv3_jpegp_check(p, g, &units) != 0) return YV3_JPEG_S_INFO;
    g->unit_bytes = yv3_jpeg_round256(units * 4);
    g->total_bytes = g->coef_bytes + g->plane_bytes + g->unit_bytes;
    return 0;
}

// The Huffman tables a scan needs in LDS
YV3_HD int yv3_jpegp_scan_tables(const yv3_jpegp_scan* s) { return s->ss > 0 ? 1 : s->ah == 0 ? s->ns : 0; }

// The level of every scan (level[i], 1-based; returns the number of levels).  Two scans depend on each other only if they code
// the same component and their bands overlap: level = 1 + the highest level of an earlier scan the scan depends on -- raised
// further while that level's scans already use YV3_JPEGP_LEVEL_TABLES tables.  A pure function of the record, so the parser's
// levels and the kernel's are the same numbers.  (A record yv3_jpegp_check accepted.)
YV3_HD int yv3_jpegp_levels(const yv3_jpeg_prog* p, unsigned char* level) {
    unsigned char used[YV3_JPEGP_MAX_SCANS + 1];
    for (int i = 0; i <= YV3_JPEGP_MAX_SCANS; ++i) used[i] = 0;
    int nlevels = 0;
    for (int i = 0; i < p->nscans; ++i) {
        const yv3_jpegp_scan* s = p->scans + i;
        int lev = 1;
        for (int k = 0; k < i; ++k) {
            const yv3_jpegp_scan* e = p->scans + k;
            if (e->se < s->ss || s->se < e->ss) continue;
            bool shared = false;
            for (int a = 0; a < s->ns; ++a)
                for (int b = 0; b < e->ns; ++b) shared = shared || s->comp[a] == e->comp[b];
            if (shared && level[k] + 1 > lev) lev = level[k] + 1;
        }
#if defined(YV3_MEASURE) && defined(YV3_JPEGP_BARRIER_PER_SCAN)
        lev = i + 1;                                                      // the measurement build's comparison: plain file order
#endif
        const int need = yv3_jpegp_scan_tables(s);
        while (used[lev] + need > YV3_JPEGP_LEVEL_TABLES) ++lev;         // lev <= i + 1: a level no earlier scan has is empty
        used[lev] = (unsigned char)(used[lev] + need);
        level[i] = (unsigned char)lev;
        if (lev > nlevels) nlevels = lev;
    }
    return nlevels;
}

YV3_HD int yv3_jpegp_bit(yv3_jpeg_bits& b) {
    yv3_jpeg_fill(b);
    const int v = yv3_jpeg_peek(b, 1);
    yv3_jpeg_skip(b, 1);
    return v;
}

// Decodes items [i0, i1) of scan `s` from bytes [begin, end) of `data` into coef ([nblocks][64] int16, natural order; zeroed
// before the image's first scan).  Items are MCUs of the frame for an interleaved scan and blocks of the component's own grid,
// row by row, for a one-component scan (the padding blocks of the MCU-padded plane are never touched).  tabs[j]: the table of
// the scan's component j (first DC scans) or tabs[0] (AC scans); natural: yv3_jpeg_natural as a table of 64.  A unit begins
// the scan or follows a restart marker: DC predictions and the EOB run start at 0.  Returns 0 or a status.
YV3_HD int yv3_jpegp_decode_unit(const unsigned char* data, long long begin, long long end, const yv3_jpeg_geom* g,
                                 const yv3_jpegp_scan* s, const yv3_jpeg_hufftab* const* tabs, const unsigned char* natural,
                                 int i0, int i1, short* coef, int nblocks) {
    yv3_jpeg_bits b;
    b.scan = data; b.pos = begin; b.end = end; b.acc = 0; b.n = 0; b.pad = 0; b.bad = 0;
    const int ns = s->ns, ss = s->ss, se = s->se, ah = s->ah, al = s->al;
    const int p1 = 1 << al;
    if (ss == 0) {                                                          // DC: first or refinement, interleaved or not
        int pred[3] = {0, 0, 0};
        const int c0 = s->comp[0];
        const int wc = ns > 1 ? g->mcu_w : (g->cw[c0] + 7) / 8;
        for (int i = i0; i < i1; ++i) {
            const int iy = i / wc, ix = i - iy * wc;
            for (int j = 0; j < ns; ++j) {
                const int c = s->comp[j] < 3 ? s->comp[j] : 0;
                const int hc = ns > 1 ? g->h[c] : 1, vc = ns > 1 ? g->v[c] : 1;
                for (int vy = 0; vy < vc; ++vy)
                    for (int hx = 0; hx < hc; ++hx) {
                        const long long blk = (long long)g->base[c] + (long long)(iy * vc + vy) * g->bw[c] + ix * hc + hx;
                        if (blk < 0 || blk >= nblocks) return YV3_JPEG_S_COEF;
                        short* out = coef + blk * 64;
                        if (ah == 0) {
                            yv3_jpeg_fill(b);
                            const int sz = yv3_jpeg_symbol(b, tabs[j]);
                            if (sz < 0 || sz > 15) return YV3_JPEG_S_CODE;
                            if (sz) pred[j] += yv3_jpeg_receive_extend(b, sz);      // (16 + 15 bits of the 57 a fill gives)
                            if (pred[j] < -32768 || pred[j] > 32767) return YV3_JPEG_S_DC;
                            const int v = pred[j] * p1;
                            if (v < -32768 || v > 32767) return YV3_JPEG_S_DC;
                            out[0] = (short)v;
                        } else if (yv3_jpegp_bit(b)) {
                            out[0] = (short)(out[0] | p1);
                        }
                        if (b.bad) return YV3_JPEG_S_MARKER;
                        if (b.pad > b.n) return YV3_JPEG_S_OVERRUN;
                    }
            }
        }
    } else {                                                                // AC: one component, its own grid
        const int c = s->comp[0] < 3 ? s->comp[0] : 0;
        const int wc = (g->cw[c] + 7) / 8;
        const yv3_jpeg_hufftab* ac = tabs[0];
        int eobrun = 0;
        for (int i = i0; i < i1; ++i) {
            const int iy = i / wc, ix = i - iy * wc;
            const long long blk = (long long)g->base[c] + (long long)iy * g->bw[c] + ix;
            if (blk < 0 || blk >= nblocks) return YV3_JPEG_S_COEF;
            short* out = coef + blk * 64;
            if (ah == 0) {
                if (eobrun > 0) { --eobrun; continue; }
                for (int k = ss; k <= se; ++k) {
                    yv3_jpeg_fill(b);
                    const int rs = yv3_jpeg_symbol(b, ac);
                    if (rs < 0) return YV3_JPEG_S_CODE;
                    const int r = rs >> 4, sz = rs & 15;
                    if (sz) {
                        k += r;
                        if (k > se) return YV3_JPEG_S_COEF;
                        const int v = yv3_jpeg_receive_extend(b, sz) * p1;
                        if (v < -32768 || v > 32767) return YV3_JPEGP_S_VALUE;
                        out[natural[k]] = (short)v;
                    } else if (r == 15) {
                        k += 15;
                        if (k > se) return YV3_JPEG_S_COEF;
                    } else {                                                // EOBr: this block and 2^r - 1 + bits more
                        eobrun = 1 << r;
                        if (r) { eobrun += yv3_jpeg_peek(b, r); yv3_jpeg_skip(b, r); }
                        --eobrun;
                        break;
                    }
                }
            } else {
                // The block as it stands, read once (a coefficient read per decision would cost a memory latency each): which of
                // its coefficients have history (nz) and which of those hold bit p1 already (hp), as masks over zigzag positions.
                // The corrections are collected in corr and applied from the same copy behind the block's last symbol.  (Other
                // scans of the level write other coefficients of the block meanwhile: nothing outside the band is used or stored.)
                short c[64];
                memcpy(c, __builtin_assume_aligned(out, 16), 128);
                unsigned long long nz = 0, hp = 0, corr = 0;
                const unsigned char zz[64] = YV3_JPEG_NATURAL_ORDER;
                YV3_UNROLL
                for (int k = 1; k < 64; ++k) {
                    nz |= (unsigned long long)(c[zz[k]] != 0) << k;
                    hp |= (unsigned long long)((c[zz[k]] & p1) != 0) << k;
                }
                int k = ss;
                if (eobrun == 0) {
                    for (; k <= se; ++k) {
                        yv3_jpeg_fill(b);
                        const int rs = yv3_jpeg_symbol(b, ac);
                        if (rs < 0) return YV3_JPEG_S_CODE;
                        int r = rs >> 4, val = 0;
                        const int sz = rs & 15;
                        if (sz) {
                            if (sz != 1) return YV3_JPEGP_S_REFINE;
                            val = yv3_jpeg_peek(b, 1) ? p1 : -p1;           // a newly non-zero coefficient
                            yv3_jpeg_skip(b, 1);
                        } else if (r != 15) {
                            eobrun = 1 << r;
                            if (r) { eobrun += yv3_jpeg_peek(b, r); yv3_jpeg_skip(b, r); }
                            break;                                          // the rest of this block is the run's first
                        }
                        // over the coefficients with history (a correction bit each) and r without (ZRL: r = 15, then one more)
                        for (; k <= se; ++k) {
                            if ((nz >> k) & 1) { if (yv3_jpegp_bit(b)) corr |= 1ull << k; }
                            else if (--r < 0) break;
                        }
                        if (k > se) return YV3_JPEG_S_COEF;                 // the run did not end inside the band
                        if (val) out[natural[k]] = (short)val;
                        if (b.pad > b.n) return YV3_JPEG_S_OVERRUN;         // (bounds the work on a unit that has run dry)
                    }
                }
                if (eobrun > 0) {
                    for (; k <= se; ++k)
                        if (((nz >> k) & 1) && yv3_jpegp_bit(b)) corr |= 1ull << k;
                    --eobrun;
                }
                corr &= ~hp;                                                // (jdphuff.c: a set bit p1 is left alone)
                if (corr) {
                    bool fits = true;
                    YV3_UNROLL
                    for (int q = 1; q < 64; ++q)
                        if ((corr >> q) & 1) {                              // the magnitude grows by p1
                            const int v = c[zz[q]] >= 0 ? c[zz[q]] + p1 : c[zz[q]] - p1;
                            if (v < -32768 || v > 32767) fits = false;
                            else out[zz[q]] = (short)v;
                        }
                    if (!fits) return YV3_JPEGP_S_VALUE;
                }
            }
            if (b.bad) return YV3_JPEG_S_MARKER;
            if (b.pad > b.n) return YV3_JPEG_S_OVERRUN;
        }
        if (eobrun > 0) return YV3_JPEG_S_COEF;                             // an EOB run past the unit's last block
    }
    if (b.bad) return YV3_JPEG_S_MARKER;
    if (b.pos < b.end || b.n - b.pad >= 8) return YV3_JPEG_S_EXTRA;
    return 0;
}
