// Baseline JPEG after the entropy decode, as libjpeg's defaults compute it, in integer arithmetic: the "islow" inverse DCT of
// one block and one output pixel of "fancy" chroma upsampling + YCbCr -> RGB.  Host/device inline functions: jpeg.hip's
// kernels call them per block and per pixel, and the stand-alone host program of tests/test_jpeg_host.py runs the same code.
#pragma once
#include "jpeg_entropy.h"

// jidctint.c: CONST_BITS = 13, PASS1_BITS = 2, FIX(x) = round(x * 8192)
#define YV3_FIX_0_298631336 2446
#define YV3_FIX_0_390180644 3196
#define YV3_FIX_0_541196100 4433
#define YV3_FIX_0_765366865 6270
#define YV3_FIX_0_899976223 7373
#define YV3_FIX_1_175875602 9633
#define YV3_FIX_1_501321110 12299
#define YV3_FIX_1_847759065 15137
#define YV3_FIX_1_961570560 16069
#define YV3_FIX_2_053119869 16819
#define YV3_FIX_2_562915447 20995
#define YV3_FIX_3_072711026 25172

// One 1-D pass over d[0..7] (already dequantised ints).  shift = 11 for the column pass, 18 for the row pass.
YV3_HD void yv3_jpeg_idct_1d(const int* d, int shift, int* o) {
    // unsigned: the same bits as libjpeg's signed arithmetic wherever that does not overflow, and defined where damaged data would
    unsigned z1, z2, z3, z4, z5, tmp0, tmp1, tmp2, tmp3, tmp10, tmp11, tmp12, tmp13;
    z2 = (unsigned)d[2]; z3 = (unsigned)d[6];
    z1 = (z2 + z3) * YV3_FIX_0_541196100;
    tmp2 = z1 - z3 * YV3_FIX_1_847759065;
    tmp3 = z1 + z2 * YV3_FIX_0_765366865;
    z2 = (unsigned)d[0]; z3 = (unsigned)d[4];
    tmp0 = (z2 + z3) << 13;
    tmp1 = (z2 - z3) << 13;
    tmp10 = tmp0 + tmp3; tmp13 = tmp0 - tmp3; tmp11 = tmp1 + tmp2; tmp12 = tmp1 - tmp2;
    tmp0 = (unsigned)d[7]; tmp1 = (unsigned)d[5]; tmp2 = (unsigned)d[3]; tmp3 = (unsigned)d[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2; z4 = tmp1 + tmp3;
    z5 = (z3 + z4) * YV3_FIX_1_175875602;
    tmp0 *= YV3_FIX_0_298631336; tmp1 *= YV3_FIX_2_053119869; tmp2 *= YV3_FIX_3_072711026; tmp3 *= YV3_FIX_1_501321110;
    z1 *= 0u - YV3_FIX_0_899976223; z2 *= 0u - YV3_FIX_2_562915447; z3 *= 0u - YV3_FIX_1_961570560; z4 *= 0u - YV3_FIX_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const unsigned rnd = 1u << (shift - 1);
    o[0] = (int)(tmp10 + tmp3 + rnd) >> shift; o[7] = (int)(tmp10 - tmp3 + rnd) >> shift;
    o[1] = (int)(tmp11 + tmp2 + rnd) >> shift; o[6] = (int)(tmp11 - tmp2 + rnd) >> shift;
    o[2] = (int)(tmp12 + tmp1 + rnd) >> shift; o[5] = (int)(tmp12 - tmp1 + rnd) >> shift;
    o[3] = (int)(tmp13 + tmp0 + rnd) >> shift; o[4] = (int)(tmp13 - tmp0 + rnd) >> shift;
}

// The range in which every libjpeg IDCT gives the same bytes.  libjpeg-turbo's SIMD jidctint keeps the dequantised
// coefficients and the column pass's outputs in 16-bit words and adds pairs of them as words; the C jidctint masks its
// range-limit index to 10 bits.  Outside these bounds each build wraps its own way; inside them all agree with 32-bit
// arithmetic and a clamp.  Blocks of real 8-bit samples stay far inside (coefficients within 1024, column pass within
// 6000, samples within 400 of the level shift), so only damaged or hand-made data is refused.
#define YV3_JPEG_WORD_LIMIT 16383          // |dequantised coefficient|, |column-pass output|: the sum of two fits a word
#define YV3_JPEG_SAMPLE_MIN (-512)         // row-pass output before the +128
#define YV3_JPEG_SAMPLE_MAX 511

// 1 when v lies outside [-YV3_JPEG_WORD_LIMIT, YV3_JPEG_WORD_LIMIT]
YV3_HD unsigned yv3_jpeg_off_word(int v) { return (unsigned)v + YV3_JPEG_WORD_LIMIT > 2u * YV3_JPEG_WORD_LIMIT; }

// The quantiser table of component c (the same selection for the kernel and the host program)
YV3_HD const unsigned char* yv3_jpeg_quant_of(const yv3_jpeg_info* f, int c) { return f->quant[f->tq[c] & 3]; }

// coef[64] int16 (natural order) * quant[64] -> out: 8 rows of 8 samples, `stride` bytes apart.  Returns 0, or
// YV3_JPEG_S_RANGE for a block outside the range above: its samples are then not libjpeg's and the image is not to be used.
// (Unsigned arithmetic where a shift could overflow: such a block gives other samples, never an access outside the block.)
YV3_HD int yv3_jpeg_idct_block(const short* coef, const unsigned char* quant, unsigned char* out, long long stride) {
    int ws[64];
    unsigned off = 0;
    YV3_UNROLL
    for (int x = 0; x < 8; ++x) {
        int d[8], o[8];
        YV3_UNROLL
        for (int y = 0; y < 8; ++y) { d[y] = (int)coef[8 * y + x] * (int)quant[8 * y + x]; off |= yv3_jpeg_off_word(d[y]); }
        yv3_jpeg_idct_1d(d, 11, o);
        YV3_UNROLL
        for (int y = 0; y < 8; ++y) { ws[8 * y + x] = o[y]; off |= yv3_jpeg_off_word(o[y]); }
    }
    YV3_UNROLL
    for (int y = 0; y < 8; ++y) {
        int o[8];
        yv3_jpeg_idct_1d(ws + 8 * y, 18, o);
        YV3_UNROLL
        for (int x = 0; x < 8; ++x) {
            off |= (unsigned)(o[x] - YV3_JPEG_SAMPLE_MIN) > (unsigned)(YV3_JPEG_SAMPLE_MAX - YV3_JPEG_SAMPLE_MIN);
            const int s = o[x] + 128;                 // |o| < 2^14 after the shift by 18
            out[y * stride + x] = (unsigned char)(s < 0 ? 0 : s > 255 ? 255 : s);
        }
    }
    return off ? YV3_JPEG_S_RANGE : 0;
}

// Chroma sample of output pixel (x, y) from plane p (row pitch `pitch`, true size cw x ch) under sampling hmax x vmax relative
// to a 1x1 chroma component: 1x1 copies, 2x1 is h2v1_fancy_upsample, 2x2 is h2v2_fancy_upsample (jdsample.c); a chroma plane of
// one or two columns is replicated instead, as jinit_upsampler chooses.
YV3_HD int yv3_jpeg_chroma(const unsigned char* p, long long pitch, int cw, int ch, int hmax, int vmax, int x, int y) {
    if (hmax == 1) return p[(long long)y * pitch + x];
    const int cx = x >> 1;
    if (cw <= 2) return p[(long long)(vmax == 2 ? y >> 1 : y) * pitch + cx];      // jinit_upsampler: fancy only above 2 columns
    if (vmax == 1) {
        const unsigned char* r = p + (long long)y * pitch;
        const int s = r[cx];
        if (x & 1) return cx == cw - 1 ? s : (3 * s + r[cx + 1] + 2) >> 2;
        return cx == 0 ? s : (3 * s + r[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;
    int fy = (y & 1) ? cy + 1 : cy - 1;
    fy = fy < 0 ? 0 : fy > ch - 1 ? ch - 1 : fy;
    const unsigned char* near = p + (long long)cy * pitch;
    const unsigned char* far = p + (long long)fy * pitch;
    const int t = 3 * near[cx] + far[cx];
    if (x & 1) return cx == cw - 1 ? (4 * t + 7) >> 4 : (3 * t + 3 * near[cx + 1] + far[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * t + 8) >> 4 : (3 * t + 3 * near[cx - 1] + far[cx - 1] + 8) >> 4;
}

YV3_HD int yv3_jpeg_clamp(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// jdcolor.c's tables, evaluated: SCALEBITS = 16, arithmetic shifts
YV3_HD void yv3_jpeg_ycc_to_rgb(int Y, int cb, int cr, int* rgb) {
    cb -= 128; cr -= 128;
    rgb[0] = yv3_jpeg_clamp(Y + ((91881 * cr + 32768) >> 16));
    rgb[1] = yv3_jpeg_clamp(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    rgb[2] = yv3_jpeg_clamp(Y + ((116130 * cb + 32768) >> 16));
}

// RGB of output pixel (x, y), x < width, y < height, from the image's component planes (plane c at planes + base[c] * 64, pitch bw[c] * 8)
YV3_HD void yv3_jpeg_pixel(const unsigned char* planes, const yv3_jpeg_geom* g, int x, int y, int* rgb) {
    const int Y = planes[(long long)g->base[0] * 64 + (long long)y * (g->bw[0] * 8) + x];
    if (g->ncomp == 1) { rgb[0] = rgb[1] = rgb[2] = Y; return; }
    const int cb = yv3_jpeg_chroma(planes + (long long)g->base[1] * 64, g->bw[1] * 8, g->cw[1], g->ch[1], g->hmax, g->vmax, x, y);
    const int cr = yv3_jpeg_chroma(planes + (long long)g->base[2] * 64, g->bw[2] * 8, g->cw[2], g->ch[2], g->hmax, g->vmax, x, y);
    yv3_jpeg_ycc_to_rgb(Y, cb, cr, rgb);
}
