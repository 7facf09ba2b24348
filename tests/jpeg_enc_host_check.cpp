// Stand-alone host program: the encoder's shared code (csrc/jpeg_enc.h) walked on the CPU in the kernels' order -- coefficients
// per block of the scan, each block's bit length, a prefix sum, every block written at its own bit offset into a zeroed buffer,
// then padding, stuffing, header and EOI.  Usage: jpeg_enc_host_check IN OUT.  IN holds records of five little-endian int32
// (width, height, ncomp, subsampling, quality) followed by the pixels; OUT receives, per record, an int32 length and the file.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpeg_enc.h"

namespace {

constexpr yv3_enc_tables TAB = yv3_enc_make_tables();

struct bit_sink {                                                 // enc_bit_sink of jpeg_enc.hip, with plain ORs
    uint32_t* words;
    unsigned long long acc;
    int n;
    void put(uint32_t code, int len) {
        acc |= (unsigned long long)code << (64 - n - len);
        n += len;
        if (n >= 32) {
            *words++ |= (uint32_t)(acc >> 32);
            acc <<= 32;
            n -= 32;
        }
    }
    void finish() {
        if (n) *words |= (uint32_t)(acc >> 32);
    }
};

std::vector<unsigned char> encode(const unsigned char* px, int W, int H, int ncomp, int subsampling, int quality) {
    const yv3_enc_geom g = yv3_enc_geometry(W, H, ncomp, subsampling, quality, (long long)W * ncomp);
    if (!g.ok) return {};
    uint16_t q[2][64];
    for (int t = 0; t < 2; ++t) yv3_enc_quant_table(YV3_ENC_SPEC.quant[t], quality, q[t]);
    std::vector<int16_t> coef((size_t)g.nblk * 64);
    for (unsigned idx = 0; idx < g.nblk; ++idx) {
        const yv3_enc_block blk = yv3_enc_locate(g, idx);
        yv3_enc_block src = blk;
        for (unsigned back = 1; src.dummy; ++back) src = yv3_enc_locate(g, idx - back);
        int d[64];
        yv3_enc_load_block(px, (long long)W * ncomp, W, H, ncomp, g, src.comp, src.bx, src.by, d);
        yv3_enc_fdct_quantise(d, q[src.comp ? 1 : 0]);
        for (int k = 0; k < 64; ++k) coef[(size_t)idx * 64 + k] = (int16_t)(blk.dummy && k ? 0 : d[TAB.natural_of_zigzag[k]]);
    }
    std::vector<unsigned> offset(g.nblk + 1, 0);
    bool ok = true;
    for (unsigned idx = 0; idx < g.nblk; ++idx) {
        const yv3_enc_block blk = yv3_enc_locate(g, idx);
        const int t = blk.comp ? 1 : 0, pred = blk.pred < 0 ? 0 : coef[(size_t)blk.pred * 64];
        yv3_enc_count_sink sink;
        ok &= yv3_enc_block_tokens(&coef[(size_t)idx * 64], pred, TAB.dc[t], TAB.ac[t], sink);
        if (sink.bits > YV3_ENC_BLOCK_BITS) ok = false;
        offset[idx + 1] = offset[idx] + sink.bits;
    }
    if (!ok) return {};
    const unsigned total = offset[g.nblk];
    std::vector<uint32_t> words(total / 32 + 2, 0);
    for (unsigned k = 0; k < g.nblk; ++k) {
        const unsigned idx = g.nblk - 1 - k;                      // any order gives the same words
        const yv3_enc_block blk = yv3_enc_locate(g, idx);
        const int t = blk.comp ? 1 : 0, pred = blk.pred < 0 ? 0 : coef[(size_t)blk.pred * 64];
        bit_sink sink = {&words[offset[idx] / 32], 0, (int)(offset[idx] % 32)};
        yv3_enc_block_tokens(&coef[(size_t)idx * 64], pred, TAB.dc[t], TAB.ac[t], sink);
        sink.finish();
    }
    std::vector<unsigned char> out(YV3_ENC_HEADER_MAX);
    const int hdr = yv3_enc_write_header(YV3_ENC_SPEC, W, H, ncomp, g.hs, g.vs, quality, out.data(), (long long)out.size());
    if (hdr > YV3_ENC_HEADER_MAX) return {};
    out.resize(hdr);
    const unsigned nbytes = (total + 7) / 8;
    for (unsigned i = 0; i < nbytes; ++i) {
        unsigned c = (words[i / 4] >> (24 - 8 * (i & 3))) & 255u;
        if (i + 1 == nbytes && (total & 7)) c |= (1u << (8 - (total & 7))) - 1;
        out.push_back((unsigned char)c);
        if (c == 0xFF) out.push_back(0);
    }
    out.push_back(0xFF);
    out.push_back(0xD9);
    return out;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t rec[5];
    int count = 0;
    while (fread(rec, 4, 5, in) == 5) {
        if (rec[0] < 1 || rec[1] < 1 || rec[0] > 4096 || rec[1] > 4096 || (rec[2] != 1 && rec[2] != 3)) return 3;
        std::vector<unsigned char> px((size_t)rec[0] * rec[1] * rec[2]);
        if (fread(px.data(), 1, px.size(), in) != px.size()) return 3;
        const std::vector<unsigned char> file = encode(px.data(), rec[0], rec[1], rec[2], rec[3], rec[4]);
        const int32_t n = (int32_t)file.size();
        fwrite(&n, 4, 1, out);
        fwrite(file.data(), 1, file.size(), out);
        ++count;
    }
    fclose(in);
    fclose(out);
    printf("encoded %d\n", count);
    return 0;
}
