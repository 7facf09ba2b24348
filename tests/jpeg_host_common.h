// What the stand-alone host programs of tests/ share (jpeg_host_check.cpp, jpeg_sync_host_check.cpp, jpeg_prog_host_check.cpp):
// file and random-number helpers, the exact-size heap copy that lets ASan guard both ends of an input, the restart-marker
// search and the way from coefficients to pixels, and the serial baseline decode.  Markers and unit byte ranges go through the
// helpers of csrc/jpeg_entropy.h, so the sanitizers run the range arithmetic the kernels run.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../yolo_v3_amd/csrc/jpeg_parse.cpp"
#include "../yolo_v3_amd/csrc/jpeg_pixel.h"

static inline std::vector<unsigned char> read_file(const char* path) {
    std::vector<unsigned char> v;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    unsigned char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

// "W H\n" + W*H*3 bytes; false when the file cannot be written
static inline bool write_rgb(const char* path, int width, int height, const std::vector<unsigned char>& rgb) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    fprintf(f, "%d %d\n", width, height);
    fwrite(rgb.data(), 1, rgb.size(), f);
    fclose(f);
    return true;
}

static unsigned long long rng_state;
static inline unsigned rnd() {                                       // splitmix64: the same inputs for the same seed everywhere
    unsigned long long z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (unsigned)((z ^ (z >> 31)) >> 16);
}

// A heap copy of exactly the input's size: ASan guards both ends, so a read one byte outside the input is a report
struct ExactCopy {
    unsigned char* data;
    size_t size;
    explicit ExactCopy(const std::vector<unsigned char>& v) : data((unsigned char*)malloc(v.size() ? v.size() : 1)), size(v.size()) {
        if (size) memcpy(data, v.data(), size);
    }
    ~ExactCopy() { free(data); }
    ExactCopy(const ExactCopy&) = delete;
    ExactCopy& operator=(const ExactCopy&) = delete;
};

// The positions of the restart markers of a scan, in file order (what find_restart_markers of jpeg.hip writes to marks[])
static inline std::vector<long long> restart_marks(const unsigned char* scan, long long len) {
    std::vector<long long> marks;
    for (long long i = 0; i < len; ++i)
        if (yv3_jpeg_restart_at(scan, i, len)) marks.push_back(i);
    return marks;
}

// idct_kernel and colour_kernel, serially: coefficients -> component planes -> rgb [H][W][3].  f: the frame's record (its
// quantisation tables and size).  0, or YV3_JPEG_S_RANGE for a block outside the range every libjpeg agrees on.
static inline int coef_to_rgb(const yv3_jpeg_info* f, const yv3_jpeg_geom& g, const std::vector<short>& coef, std::vector<unsigned char>* rgb) {
    std::vector<unsigned char> planes((size_t)g.nblocks * 64);
    for (int c = 0; c < g.ncomp; ++c)
        for (int by = 0; by < g.bh[c]; ++by)
            for (int bx = 0; bx < g.bw[c]; ++bx)
                if (yv3_jpeg_idct_block(coef.data() + ((size_t)g.base[c] + (size_t)by * g.bw[c] + bx) * 64, yv3_jpeg_quant_of(f, c),
                                        planes.data() + (size_t)g.base[c] * 64 + ((size_t)by * 8 * g.bw[c] + bx) * 8, g.bw[c] * 8))
                    return YV3_JPEG_S_RANGE;
    rgb->resize((size_t)f->width * f->height * 3);
    for (int y = 0; y < f->height; ++y)
        for (int x = 0; x < f->width; ++x) {
            int px[3];
            yv3_jpeg_pixel(planes.data(), &g, x, y, px);
            for (int k = 0; k < 3; ++k) (*rgb)[((size_t)y * f->width + x) * 3 + k] = (unsigned char)px[k];
        }
    return 0;
}

// What jpeg.hip's kernels do for a baseline file, serially.  rgb may be null (entropy decode only).
static inline int host_decode(const unsigned char* data, size_t n, yv3_jpeg_info* info, std::vector<unsigned char>* rgb) {
    if (yv3_jpeg_parse(data, n, info) != 0) return -1;
    if (info->reason) return 0;
    yv3_jpeg_geom g;
    if (yv3_jpeg_geometry(info, &g)) return YV3_JPEG_S_INFO;
    if ((unsigned long long)info->scan_offset + (unsigned long long)info->scan_length > n) return YV3_JPEG_S_BOUNDS;
    // exact-size copy of the scan: the entropy routine sees nothing but its own bytes
    std::vector<unsigned char> scan_copy(data + info->scan_offset, data + info->scan_offset + info->scan_length);
    const unsigned char* scan = scan_copy.data();
    const long long len = info->scan_length;
    std::vector<yv3_jpeg_hufftab> tabs(8);
    for (int t = 0; t < 8; ++t)
        if (info->huff_defined[t] && yv3_jpeg_build_hufftab(info->huff_counts[t], info->huff_values[t], t < 4 ? 15 : 255, &tabs[t]))
            return YV3_JPEG_S_HUFFTABLE;
    std::vector<long long> marks;
    if (info->restart_interval) marks = restart_marks(scan, len);
    if ((long long)marks.size() != g.nunits - 1) return YV3_JPEG_S_MARKER;
    std::vector<short> coef((size_t)g.nblocks * 64, 0);
    const unsigned char natural[64] = YV3_JPEG_NATURAL_ORDER;
    for (int u = 0; u < g.nunits; ++u) {
        long long begin, end;
        int st = yv3_jpeg_unit_bytes(scan, len, marks.data(), g.nunits, u, &begin, &end);
        const int m0 = u * g.mcus_per_unit, m1 = m0 + g.mcus_per_unit < g.nmcu ? m0 + g.mcus_per_unit : g.nmcu;
        if (!st) st = yv3_jpeg_decode_unit(scan, begin, end, &g, tabs.data(), info->td, info->ta, natural, m0, m1, coef.data(), g.nblocks);
        if (st) return st;
    }
    return rgb ? coef_to_rgb(info, g, coef, rgb) : 0;
}
