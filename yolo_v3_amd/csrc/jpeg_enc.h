// Baseline JPEG encode, the code shared by the host entry points and the kernels of jpeg_enc.hip:
// libjpeg's rules restated -- quality scaling, the 16-bit fixed-point RGB -> YCbCr, h2v1 / h2v2 downsampling with its alternating
// bias, edge replication, the "islow" forward DCT with its rounding division, the Huffman tokens of a block -- and the header in
// the order libjpeg writes it.  Everything is integer arithmetic, so host and device give the same bytes.
#pragma once
#include <stdint.h>
#include "yv3.h"

#ifdef __HIPCC__
#define YV3_HD __host__ __device__
#else
#define YV3_HD
#endif

// ---- standard data (ITU T.81 annex K) --------------------------------------------------------------------------------------
struct yv3_enc_spec {
    uint8_t quant[2][64];          // base tables, natural order: luma, chroma
    uint8_t dc_counts[2][16], dc_values[2][12];
    uint8_t ac_counts[2][16], ac_values[2][162];
    uint8_t natural_of_zigzag[64];
};

constexpr yv3_enc_spec YV3_ENC_SPEC = {
    {{16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
     {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}},
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}},
    {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}},
    {{1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51,
      98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84,
      85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136,
      137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184,
      185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231,
      232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
     {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98,
      114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74,
      83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133,
      134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180,
      181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227,
      228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}},
    {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
     49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}};

// The encoder's view of the tables: per symbol (code << 8 | length), length 0 = no code.  Built at compile time (annex C).
struct yv3_enc_tables {
    uint32_t dc[2][12];
    uint32_t ac[2][256];
    uint8_t quant[2][64];
    uint8_t natural_of_zigzag[64];
};

constexpr yv3_enc_tables yv3_enc_make_tables() {
    yv3_enc_tables t = {};
    for (int id = 0; id < 2; ++id) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < YV3_ENC_SPEC.dc_counts[id][len - 1]; ++i) t.dc[id][YV3_ENC_SPEC.dc_values[id][k++]] = (code++ << 8) | (uint32_t)len;
            code <<= 1;
        }
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < YV3_ENC_SPEC.ac_counts[id][len - 1]; ++i) t.ac[id][YV3_ENC_SPEC.ac_values[id][k++]] = (code++ << 8) | (uint32_t)len;
            code <<= 1;
        }
        for (int i = 0; i < 64; ++i) t.quant[id][i] = YV3_ENC_SPEC.quant[id][i];
    }
    for (int i = 0; i < 64; ++i) t.natural_of_zigzag[i] = YV3_ENC_SPEC.natural_of_zigzag[i];
    return t;
}

// ---- geometry --------------------------------------------------------------------------------------------------------------
#define YV3_ENC_MAX_SIDE      16384
#define YV3_ENC_MAX_BLOCKS    2000000      // x YV3_ENC_BLOCK_BITS < 2^32: every bit offset of an image fits 32 bits
#define YV3_ENC_BLOCK_BITS    1660         // 11 + 11 for DC (chroma's longest code), 63 x (16 + 10) for AC: no block is longer
#define YV3_ENC_CHUNK         256          // blocks per workgroup of the size and emit kernels
#define YV3_ENC_BYTE_CHUNK    4096         // scan bytes per workgroup of the count and scatter kernels (256 threads x 16)
#define YV3_ENC_HEADER_MAX    640          // (a colour header is 623 bytes, a grey one 328)

struct yv3_enc_geom {
    int ok;                 // 0: the fields describe no image this encoder takes
    int hs, vs;             // luma sampling factors (1 x 1 for a grey image)
    int mcu_w, mcu_h, bpm;  // MCUs per row / column, blocks per MCU (grey: one block)
    int blocks_w, blocks_h; // real luma blocks: ceil(W / 8), ceil(H / 8)
    unsigned nblk;          // blocks in scan order, dummy blocks included
};

YV3_HD static inline yv3_enc_geom yv3_enc_geometry(long long width, long long height, int ncomp, int subsampling, int quality, long long pitch) {
    yv3_enc_geom g = {};
    if (width < 1 || height < 1 || width > YV3_ENC_MAX_SIDE || height > YV3_ENC_MAX_SIDE) return g;
    if ((ncomp != 1 && ncomp != 3) || subsampling < 0 || subsampling > 2 || quality < 1 || quality > 100) return g;
    if (pitch < width * ncomp) return g;
    g.hs = ncomp == 3 && subsampling >= 1 ? 2 : 1;
    g.vs = ncomp == 3 && subsampling == 2 ? 2 : 1;
    g.blocks_w = (int)((width + 7) / 8);
    g.blocks_h = (int)((height + 7) / 8);
    g.mcu_w = (g.blocks_w + g.hs - 1) / g.hs;
    g.mcu_h = (g.blocks_h + g.vs - 1) / g.vs;
    g.bpm = ncomp == 3 ? g.hs * g.vs + 2 : 1;
    const long long n = (long long)g.mcu_w * g.mcu_h * g.bpm;
    if (n > YV3_ENC_MAX_BLOCKS) return g;
    g.nblk = (unsigned)n;
    g.ok = 1;
    return g;
}

// A block of the scan: its component (0 luma, 1 Cb, 2 Cr), its block coordinates inside the component, whether it is a dummy
// block, and the scan index of the block that holds its DC predictor (-1: the predictor is 0).
struct yv3_enc_block {
    int comp, bx, by, dummy;
    long long pred;
};

YV3_HD static inline yv3_enc_block yv3_enc_locate(const yv3_enc_geom& g, unsigned idx) {
    yv3_enc_block b = {};
    const unsigned mcu = idx / (unsigned)g.bpm;
    const int k = (int)(idx - mcu * (unsigned)g.bpm), nl = g.bpm == 1 ? 1 : g.hs * g.vs;
    const int mx = (int)(mcu % (unsigned)g.mcu_w), my = (int)(mcu / (unsigned)g.mcu_w);
    if (k < nl) {
        b.comp = 0;
        b.bx = mx * g.hs + k % g.hs;
        b.by = my * g.vs + k / g.hs;
        b.dummy = b.bx >= g.blocks_w || b.by >= g.blocks_h;
        b.pred = k > 0 ? (long long)idx - 1 : (mcu > 0 ? (long long)idx - g.bpm + nl - 1 : -1);
    } else {
        b.comp = k - nl + 1;
        b.bx = mx;
        b.by = my;
        b.pred = mcu > 0 ? (long long)idx - g.bpm : -1;
    }
    return b;
}

// ---- pixels to coefficients ------------------------------------------------------------------------------------------------
YV3_HD static inline void yv3_enc_quant_table(const uint8_t* base, int quality, uint16_t* q) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        int v = (base[i] * scale + 50) / 100;
        q[i] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
}

// one component sample at full resolution; x and y already clamped into the image
YV3_HD static inline int yv3_enc_sample(const unsigned char* px, long long pitch, int ncomp, int comp, int x, int y) {
    const unsigned char* p = px + (long long)y * pitch + (long long)x * ncomp;
    if (ncomp == 1) return p[0];
    const int r = p[0], g = p[1], b = p[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// The 64 samples of block (bx, by) of a component, minus 128.  Edges: a column past the image repeats the last one; a chroma row
// past the last downsampled row repeats THAT row, whose own missing full-resolution row repeats the image's last row.
YV3_HD static inline void yv3_enc_load_block(const unsigned char* px, long long pitch, int W, int H, int ncomp, const yv3_enc_geom& g,
                                             int comp, int bx, int by, int* d) {
    const int h = comp ? g.hs : 1, v = comp ? g.vs : 1;
    const int rows_down = (H + v - 1) / v;
    for (int yy = 0; yy < 8; ++yy) {
        int r = by * 8 + yy;
        if (r > rows_down - 1) r = rows_down - 1;
        for (int xx = 0; xx < 8; ++xx) {
            const int c = bx * 8 + xx;
            int s;
            if (h == 1) {
                s = yv3_enc_sample(px, pitch, ncomp, comp, c < W ? c : W - 1, r);
            } else {
                const int x0 = 2 * c < W ? 2 * c : W - 1, x1 = 2 * c + 1 < W ? 2 * c + 1 : W - 1;
                if (v == 1) {
                    s = (yv3_enc_sample(px, pitch, ncomp, comp, x0, r) + yv3_enc_sample(px, pitch, ncomp, comp, x1, r) + (c & 1)) >> 1;
                } else {
                    const int y0 = 2 * r, y1 = 2 * r + 1 < H ? 2 * r + 1 : H - 1;
                    s = (yv3_enc_sample(px, pitch, ncomp, comp, x0, y0) + yv3_enc_sample(px, pitch, ncomp, comp, x1, y0) +
                         yv3_enc_sample(px, pitch, ncomp, comp, x0, y1) + yv3_enc_sample(px, pitch, ncomp, comp, x1, y1) + 1 + (c & 1)) >> 2;
                }
            }
            d[yy * 8 + xx] = s - 128;
        }
    }
}

// jfdctint ("islow": CONST_BITS 13, PASS1_BITS 2) along 8 values `stride` apart; first = the row pass
YV3_HD static inline void yv3_enc_fdct_pass(int* d, int stride, bool first) {
    const int d0 = d[0], d1 = d[stride], d2 = d[2 * stride], d3 = d[3 * stride], d4 = d[4 * stride], d5 = d[5 * stride],
              d6 = d[6 * stride], d7 = d[7 * stride];
    int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int n = first ? 11 : 15, half = 1 << (n - 1);
    if (first) {
        d[0] = (t10 + t11) * 4;
        d[4 * stride] = (t10 - t11) * 4;
    } else {
        d[0] = (t10 + t11 + 2) >> 2;
        d[4 * stride] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    d[2 * stride] = (z1 + t13 * 6270 + half) >> n;
    d[6 * stride] = (z1 - t12 * 15137 + half) >> n;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446;
    t5 *= 16819;
    t6 *= 25172;
    t7 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7 * stride] = (t4 + z1 + z3 + half) >> n;
    d[5 * stride] = (t5 + z2 + z4 + half) >> n;
    d[3 * stride] = (t6 + z2 + z3 + half) >> n;
    d[stride] = (t7 + z1 + z4 + half) >> n;
}

// forward DCT of d[64] (samples - 128, natural order) in place, then libjpeg's rounding division by 8 q
YV3_HD static inline void yv3_enc_fdct_quantise(int* d, const uint16_t* q) {
    for (int r = 0; r < 8; ++r) yv3_enc_fdct_pass(d + 8 * r, 1, true);
    for (int c = 0; c < 8; ++c) yv3_enc_fdct_pass(d + c, 8, false);
    for (int i = 0; i < 64; ++i) {
        const int dv = 8 * q[i], c = d[i], a = ((c < 0 ? -c : c) + (dv >> 1)) / dv;
        d[i] = c < 0 ? -a : a;
    }
}

// ---- coefficients to tokens ------------------------------------------------------------------------------------------------
YV3_HD static inline int yv3_enc_category(int v) {
    unsigned a = (unsigned)(v < 0 ? -v : v);
    int n = 0;
    while (a) {
        ++n;
        a >>= 1;
    }
    return n;
}

// The tokens of one block, zz[64] in zigzag order, after predictor `pred`: sink.put(code, length) per token, code and the value's
// bits already joined (at most 26 bits).  Returns false for a DC difference above category 11 or an AC value above category 10,
// which no table here codes: such a value is coded as 0, and the caller reports the image.
template <typename Sink>
YV3_HD static inline bool yv3_enc_block_tokens(const int16_t* zz, int pred, const uint32_t* dc, const uint32_t* ac, Sink& sink) {
    bool ok = true;
    int diff = (int)zz[0] - pred, s = yv3_enc_category(diff);
    if (s > 11) {
        ok = false;
        diff = 0;
        s = 0;
    }
    {
        const uint32_t e = dc[s];
        const uint32_t bits = (uint32_t)(diff < 0 ? diff + (1 << s) - 1 : diff);
        sink.put(((e >> 8) << s) | bits, (int)(e & 255) + s);
    }
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        int v = zz[k];
        s = yv3_enc_category(v);
        if (s > 10) {
            ok = false;
            v = 0;
        }
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            sink.put(ac[0xF0] >> 8, (int)(ac[0xF0] & 255));
            run -= 16;
        }
        const uint32_t e = ac[run << 4 | s];
        const uint32_t bits = (uint32_t)(v < 0 ? v + (1 << s) - 1 : v);
        sink.put(((e >> 8) << s) | bits, (int)(e & 255) + s);
        run = 0;
    }
    if (run) sink.put(ac[0] >> 8, (int)(ac[0] & 255));
    return ok;
}

struct yv3_enc_count_sink {
    unsigned bits = 0;
    YV3_HD void put(uint32_t, int len) { bits += (unsigned)len; }
};

// ---- header ----------------------------------------------------------------------------------------------------------------
// the header's length: SOI + APP0, a DQT per table, SOF0, a DC and an AC DHT per table, SOS (623 bytes in colour, 328 in grey)
YV3_HD static inline int yv3_enc_header_length(int ncomp) {
    const int ntab = ncomp == 3 ? 2 : 1;
    return 20 + ntab * 69 + (10 + 3 * ncomp) + ntab * ((21 + (int)sizeof(yv3_enc_spec::dc_values[0])) + (21 + (int)sizeof(yv3_enc_spec::ac_values[0]))) +
           (8 + 2 * ncomp);
}

// SOI, APP0, one DQT per table, SOF0, DHT DC0 AC0 (DC1 AC1), SOS: libjpeg's order.  Writes at most cap bytes to out and returns the
// header's length whether or not it fitted (out may be null with cap 0).
YV3_HD static inline int yv3_enc_write_header(const yv3_enc_spec& spec, int W, int H, int ncomp, int hs, int vs, int quality, unsigned char* out,
                                              long long cap) {
    int n = 0;
#define YV3_ENC_PUT(b) do { if (n < cap) out[n] = (unsigned char)(b); ++n; } while (0)
    const unsigned char app0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int i = 0; i < 20; ++i) YV3_ENC_PUT(app0[i]);
    const int ntab = ncomp == 3 ? 2 : 1;
    for (int t = 0; t < ntab; ++t) {
        uint16_t q[64];
        yv3_enc_quant_table(spec.quant[t], quality, q);
        YV3_ENC_PUT(0xFF); YV3_ENC_PUT(0xDB); YV3_ENC_PUT(0); YV3_ENC_PUT(67); YV3_ENC_PUT(t);
        for (int k = 0; k < 64; ++k) YV3_ENC_PUT(q[spec.natural_of_zigzag[k]]);
    }
    YV3_ENC_PUT(0xFF); YV3_ENC_PUT(0xC0); YV3_ENC_PUT(0); YV3_ENC_PUT(8 + 3 * ncomp); YV3_ENC_PUT(8);
    YV3_ENC_PUT(H >> 8); YV3_ENC_PUT(H & 255); YV3_ENC_PUT(W >> 8); YV3_ENC_PUT(W & 255); YV3_ENC_PUT(ncomp);
    for (int c = 0; c < ncomp; ++c) {
        YV3_ENC_PUT(c + 1); YV3_ENC_PUT(c == 0 ? (hs << 4 | vs) : 0x11); YV3_ENC_PUT(c ? 1 : 0);
    }
    for (int t = 0; t < ntab; ++t) {
        for (int cls = 0; cls < 2; ++cls) {
            const uint8_t* counts = cls ? spec.ac_counts[t] : spec.dc_counts[t];
            const uint8_t* values = cls ? spec.ac_values[t] : spec.dc_values[t];
            int nv = 0;
            for (int i = 0; i < 16; ++i) nv += counts[i];
            YV3_ENC_PUT(0xFF); YV3_ENC_PUT(0xC4); YV3_ENC_PUT((19 + nv) >> 8); YV3_ENC_PUT((19 + nv) & 255); YV3_ENC_PUT(cls << 4 | t);
            for (int i = 0; i < 16; ++i) YV3_ENC_PUT(counts[i]);
            for (int i = 0; i < nv; ++i) YV3_ENC_PUT(values[i]);
        }
    }
    YV3_ENC_PUT(0xFF); YV3_ENC_PUT(0xDA); YV3_ENC_PUT(0); YV3_ENC_PUT(6 + 2 * ncomp); YV3_ENC_PUT(ncomp);
    for (int c = 0; c < ncomp; ++c) {
        YV3_ENC_PUT(c + 1); YV3_ENC_PUT(c ? 0x11 : 0);
    }
    YV3_ENC_PUT(0); YV3_ENC_PUT(63); YV3_ENC_PUT(0);
#undef YV3_ENC_PUT
    return n;
}
