// Self-synchronising parallel entropy decode of one unit (a whole scan or one restart segment) of a baseline JPEG: the per-lane
// pieces, as inline functions that compile for the GPU (jpeg.hip's entropy_kernel<1>) and for the host (the stand-alone sanitizer
// program of tests/test_jpeg_sync_host.py, which emulates lanes and passes with loops).  DESIGN.md section 8f has the algorithm.
//
// The unit's bytes [begin, end) are cut into subsequences of YV3_JPEG_SYNC_S bytes, one lane each.  A decoder's state at a symbol
// boundary is (bit, blk, zz): `bit` is the RAW position of the symbol's first bit, 8 * (byte index in the scan) + (bit in the byte,
// MSB first), and never lies in the 00 of an FF 00 pair, so two lanes that read the same bit give it the same number; `blk` is the
// block inside the MCU; `zz` the zigzag index, 0 = the next symbol is a DC code.  A "symbol" is a Huffman code with its extra bits.
// A lane decodes the symbols that BEGIN inside its subsequence.  Every access is bounded as in jpeg_entropy.h: the bit reader by
// the unit's end, block indices by the unit's and the image's block counts, coefficient indices by 63, loops by the byte count.
#pragma once
#include "jpeg_entropy.h"

#define YV3_JPEG_SYNC_S 64             // bytes per subsequence (the host program also runs S / 2)
#define YV3_JPEG_SYNC_LANES 256        // subsequences per window = lanes of the workgroup
#define YV3_JPEG_SYNC_P 16             // proving passes per window at the most; a window commits >= min(P + 1, its lanes) subsequences
#define YV3_JPEG_SYNC_MIN_BYTES (4 * YV3_JPEG_SYNC_S)     // a shorter unit goes to one lane and yv3_jpeg_decode_unit, as before

// yv3_jpeg_sync_lane's answers
#define YV3_JPEG_SYNC_RAN 0            // decoded up to the subsequence's end; *out is the exit state
#define YV3_JPEG_SYNC_ERROR 1          // no code, a run past 63, a block past the unit's, data left over, ...; *out is invalid
#define YV3_JPEG_SYNC_FINISHED 2       // (write mode) the unit's last block is complete and the serial routine's end checks hold

struct yv3_jpeg_sync_state {
    long long bit;                     // < 0: invalid (an error on the way here; not a file error unless the entry state was proven)
    int blk, zz;
};

YV3_HD bool yv3_jpeg_sync_same(const yv3_jpeg_sync_state& a, const yv3_jpeg_sync_state& b) {
    return a.bit == b.bit && a.blk == b.blk && a.zz == b.zz;
}

// blocks per MCU: 1 / 3 / 4 / 6 for grey / 4:4:4 / 4:2:2 / 4:2:0
YV3_HD int yv3_jpeg_sync_bpm(const yv3_jpeg_geom* g) { return g->h[0] * g->v[0] + g->ncomp - 1; }

// the component of block j of an MCU (0 <= j < bpm)
YV3_HD int yv3_jpeg_sync_comp(const yv3_jpeg_geom* g, int j) {
    const int nb0 = g->h[0] * g->v[0];
    return j < nb0 ? 0 : j - nb0 + 1;
}

// the image's block index of block j of MCU `mcu`, in yv3_jpeg_decode_unit's order; -1 outside [0, nblocks)
YV3_HD long long yv3_jpeg_sync_block(const yv3_jpeg_geom* g, int mcu, int j, int nblocks) {
    const int c = yv3_jpeg_sync_comp(g, j);
    if (j < 0 || c >= g->ncomp || mcu < 0) return -1;
    const int vy = c ? 0 : j / g->h[0], hx = c ? 0 : j - vy * g->h[0];
    const int my = mcu / g->mcu_w, mx = mcu - my * g->mcu_w;
    const long long blk = (long long)g->base[c] + (long long)(my * g->v[c] + vy) * g->bw[c] + mx * g->h[c] + hx;
    return blk < 0 || blk >= nblocks ? -1 : blk;
}

// An FF at byte i of the unit that is not followed by 00 inside the unit: the serial reader calls it a marker.  A unit that has
// one is handed to the serial routine before any lane decodes, so the lanes below never meet one.
YV3_HD bool yv3_jpeg_sync_marker(const unsigned char* scan, long long i, long long end) {
    return scan[i] == 0xFF && (i + 1 >= end || scan[i + 1] != 0);
}

// The first byte of subsequence i (0 <= i <= nsub; nsub gives `end`): begin + i * S, moved one byte on when that is the 00 of an
// FF 00 pair (only the bytes of such a pair are stuffing; an FF cannot itself be stuffing).
YV3_HD long long yv3_jpeg_sync_cut(const unsigned char* scan, long long begin, long long end, long long i, int S) {
    long long e = begin + i * S;
    if (e >= end) return end;
    if (e > begin && scan[e] == 0 && scan[e - 1] == 0xFF) ++e;
    return e;
}

// yv3_jpeg_fill that also counts in `own` the bits it loads from bytes before `cut`
YV3_HD void yv3_jpeg_sync_fill(yv3_jpeg_bits& b, long long cut, int& own) {
    while (b.n <= 56) {
        unsigned long long c = 0;
        if (b.pos < b.end) {
            if (b.pos < cut) own += 8;
            c = b.scan[b.pos++];
            if (c == 0xFF) {
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

// One lane: from the state *in, decodes every symbol that begins before byte `cut` (its subsequence's end, from
// yv3_jpeg_sync_cut) of the unit that ends at `end`; *out = the state after the last of them, *completed = blocks completed.
// coef == 0: nothing is written and the unit's block count is not known (the speculative and proving passes).
// coef != 0 (the write pass; *in is proven): `first` blocks of the unit are complete before *in; coefficients of the symbols go
// to coef (zeroed by the caller; a DC position receives the DIFFERENCE), blocks are bounded by unit_blocks and nblocks, and the
// lane that completes block unit_blocks - 1 stops there, applies the serial routine's end checks and answers FINISHED.
YV3_HD int yv3_jpeg_sync_lane(const unsigned char* scan, long long end, long long cut, const yv3_jpeg_sync_state* in,
                              const yv3_jpeg_geom* g, const yv3_jpeg_hufftab* tabs, const unsigned char* td, const unsigned char* ta,
                              const unsigned char* natural, short* coef, int nblocks, int mcu0, int first, int unit_blocks,
                              yv3_jpeg_sync_state* out, int* completed) {
    const int bpm = yv3_jpeg_sync_bpm(g);
    *completed = 0;
    *out = *in;
    if (in->bit < 0 || in->blk < 0 || in->blk >= bpm || in->zz < 0 || in->zz > 63 || (in->bit >> 3) > end) { out->bit = -1; return YV3_JPEG_SYNC_ERROR; }
    yv3_jpeg_bits b;
    b.scan = scan; b.pos = in->bit >> 3; b.end = end; b.acc = 0; b.n = 0; b.pad = 0; b.bad = 0;
    int own = 0, blk = in->blk, k = in->zz, done = 0;
    bool finished = false;
    short* o = 0;
    if (coef && k) {                                              // the entry state lies inside block `first` of the unit
        const long long at = first < unit_blocks ? yv3_jpeg_sync_block(g, mcu0 + first / bpm, blk, nblocks) : -1;
        if (at < 0) { out->bit = -1; return YV3_JPEG_SYNC_ERROR; }
        o = coef + at * 64;
    }
    yv3_jpeg_sync_fill(b, cut, own);
    yv3_jpeg_skip(b, (int)(in->bit & 7));
    own -= (int)(in->bit & 7);
    const bool past = in->bit >= cut * 8;                         // nothing of this subsequence is left: the state passes through
    const long long most = (past ? 0 : (cut - (in->bit >> 3)) * 8) + 8;     // every symbol takes a bit of the subsequence
    for (long long it = 0; it < most; ++it) {
        yv3_jpeg_sync_fill(b, cut, own);
        if (coef && k == 0 && first + done >= unit_blocks) { finished = true; break; }
        if (own <= 0) break;                                      // the next symbol begins at or past `cut`
        const int n0 = b.n;
        if (k == 0) {
            if (coef) {
                const long long at = yv3_jpeg_sync_block(g, mcu0 + (first + done) / bpm, blk, nblocks);
                if (at < 0) { out->bit = -1; return YV3_JPEG_SYNC_ERROR; }
                o = coef + at * 64;
            }
            const int s = yv3_jpeg_symbol(b, tabs + (td[yv3_jpeg_sync_comp(g, blk)] & 3));
            if (s < 0 || s > 15) { out->bit = -1; return YV3_JPEG_SYNC_ERROR; }
            const int v = s ? yv3_jpeg_receive_extend(b, s) : 0;  // (57 bits after a fill: a code and its extra bits fit)
            if (o) o[0] = (short)v;                               // |v| <= 32767
            k = 1;
        } else {
            const int rs = yv3_jpeg_symbol(b, tabs + 4 + (ta[yv3_jpeg_sync_comp(g, blk)] & 3));
            if (rs < 0) { out->bit = -1; return YV3_JPEG_SYNC_ERROR; }
            const int r = rs >> 4, s = rs & 15;
            if (s) {
                k += r;
                if (k > 63) { out->bit = -1; return YV3_JPEG_SYNC_ERROR; }
                const int v = yv3_jpeg_receive_extend(b, s);
                if (o) o[natural[k]] = (short)v;
                ++k;
            } else if (r == 15) {
                k += 15;
                if (k > 63) { out->bit = -1; return YV3_JPEG_SYNC_ERROR; }
                ++k;
            } else {
                k = 64;                                           // EOB
            }
        }
        own -= n0 - b.n;
        if (k == 64) {
            k = 0; ++done;
            if (++blk == bpm) blk = 0;
            if (coef && (b.bad || b.pad > b.n)) { out->bit = -1; return YV3_JPEG_SYNC_ERROR; }     // as the serial routine, per block
        }
    }
    *completed = done;
    if (finished) {
        if (b.bad || b.pos < b.end || b.n - b.pad >= 8) { out->bit = -1; return YV3_JPEG_SYNC_ERROR; }
        out->bit = end * 8; out->blk = 0; out->zz = 0;
        return YV3_JPEG_SYNC_FINISHED;
    }
    if (own > 0 || b.bad) { out->bit = -1; return YV3_JPEG_SYNC_ERROR; }     // (own > 0: the loop bound, not reachable)
    if (coef && cut >= end) { out->bit = -1; return YV3_JPEG_SYNC_ERROR; }   // the data ended before the unit's last block
    if (past) return YV3_JPEG_SYNC_RAN;                           // *out == *in
    // the exit position: -own bits past `cut`, over whole data bytes first
    long long pos = cut;
    int e = -own;
    while (e >= 8 && pos < end) { pos += (scan[pos] == 0xFF) ? 2 : 1; e -= 8; }
    if (pos >= end) { pos = end; e = 0; }
    out->bit = pos * 8 + e; out->blk = blk; out->zz = k;
    return YV3_JPEG_SYNC_RAN;
}

// The DC pass.  The write pass leaves DC DIFFERENCES; the DC value of a block is the sum of its component's differences up to
// it in scan order within the unit (prediction starts at 0).  sums[c] += the differences of MCUs [lo, hi); 64-bit, so 12 M blocks
// of +-32767 cannot overflow.
YV3_HD void yv3_jpeg_sync_dc_sum(const short* coef, const yv3_jpeg_geom* g, int nblocks, int lo, int hi, long long* sums) {
    const int bpm = yv3_jpeg_sync_bpm(g);
    for (int mcu = lo; mcu < hi; ++mcu)
        for (int j = 0; j < bpm; ++j) {
            const long long at = yv3_jpeg_sync_block(g, mcu, j, nblocks);
            if (at >= 0) sums[yv3_jpeg_sync_comp(g, j)] += coef[at * 64];
        }
}

// Replaces the differences of MCUs [lo, hi) by the DC values, pred[c] being the sums before `lo`.  false: a prefix lies outside
// 16 bits (the serial routine's YV3_JPEG_S_DC).
YV3_HD bool yv3_jpeg_sync_dc_apply(short* coef, const yv3_jpeg_geom* g, int nblocks, int lo, int hi, long long* pred) {
    const int bpm = yv3_jpeg_sync_bpm(g);
    bool ok = true;
    for (int mcu = lo; mcu < hi; ++mcu)
        for (int j = 0; j < bpm; ++j) {
            const long long at = yv3_jpeg_sync_block(g, mcu, j, nblocks);
            if (at < 0) { ok = false; continue; }
            long long& p = pred[yv3_jpeg_sync_comp(g, j)];
            p += coef[at * 64];
            if (p < -32768 || p > 32767) ok = false;
            else coef[at * 64] = (short)p;
        }
    return ok;
}
