// Stand-alone host program for tests/test_jpeg_host.py: the JPEG parser, the entropy routine and the pixel arithmetic of the
// GPU decoder, compiled for the CPU with -fsanitize=address,undefined and never loaded into Python.
//   jpeg_host_check decode IN.jpg OUT.rgb    full decode; OUT = "W H\n" + W*H*3 bytes; prints "reason R status S"
//   jpeg_host_check fuzz IN.jpg SEED         every prefix truncation, seeded single-byte corruptions and random bytes after the
//                                            valid header: parser + entropy decode on exact-size heap copies (a read past the
//                                            end is an ASan report); prints how many inputs ended in each (reason, status)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <utility>
#include <vector>
#include "../yolo_v3_amd/csrc/jpeg_parse.cpp"
#include "../yolo_v3_amd/csrc/jpeg_pixel.h"

// What jpeg.hip's kernels do, serially.  rgb may be null (entropy decode only).
static int host_decode(const unsigned char* data, size_t n, yv3_jpeg_info* info, std::vector<unsigned char>* rgb) {
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
    if (info->restart_interval)
        for (long long i = 0; i + 1 < len; ++i)
            if (scan[i] == 0xFF && scan[i + 1] >= 0xD0 && scan[i + 1] <= 0xD7) marks.push_back(i);
    if ((long long)marks.size() != g.nunits - 1) return YV3_JPEG_S_MARKER;
    std::vector<short> coef((size_t)g.nblocks * 64, 0);
    const unsigned char natural[64] = YV3_JPEG_NATURAL_ORDER;
    for (int u = 0; u < g.nunits; ++u) {
        if (u < g.nunits - 1 && scan[marks[u] + 1] != 0xD0 + (u & 7)) return YV3_JPEG_S_MARKER;
        const long long begin = u ? marks[u - 1] + 2 : 0, end = u < g.nunits - 1 ? marks[u] : len;
        const int m0 = u * g.mcus_per_unit, m1 = m0 + g.mcus_per_unit < g.nmcu ? m0 + g.mcus_per_unit : g.nmcu;
        const int st = yv3_jpeg_decode_unit(scan, begin, end, &g, tabs.data(), info->td, info->ta, natural, m0, m1, coef.data(), g.nblocks);
        if (st) return st;
    }
    if (!rgb) return 0;
    std::vector<unsigned char> planes((size_t)g.nblocks * 64);
    for (int c = 0; c < g.ncomp; ++c)
        for (int by = 0; by < g.bh[c]; ++by)
            for (int bx = 0; bx < g.bw[c]; ++bx)
                if (yv3_jpeg_idct_block(coef.data() + ((size_t)g.base[c] + (size_t)by * g.bw[c] + bx) * 64, yv3_jpeg_quant_of(info, c),
                                        planes.data() + (size_t)g.base[c] * 64 + ((size_t)by * 8 * g.bw[c] + bx) * 8, g.bw[c] * 8))
                    return YV3_JPEG_S_RANGE;
    rgb->resize((size_t)info->width * info->height * 3);
    for (int y = 0; y < info->height; ++y)
        for (int x = 0; x < info->width; ++x) {
            int px[3];
            yv3_jpeg_pixel(planes.data(), &g, x, y, px);
            for (int k = 0; k < 3; ++k) (*rgb)[((size_t)y * info->width + x) * 3 + k] = (unsigned char)px[k];
        }
    return 0;
}

static std::vector<unsigned char> read_file(const char* path) {
    std::vector<unsigned char> v;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    unsigned char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

static unsigned long long rng_state;
static unsigned rnd() {                                       // splitmix64: the same inputs for the same seed everywhere
    unsigned long long z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (unsigned)((z ^ (z >> 31)) >> 16);
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "decode")) {
        const std::vector<unsigned char> file = read_file(argv[2]);
        yv3_jpeg_info info;
        std::vector<unsigned char> rgb;
        const int st = host_decode(file.data(), file.size(), &info, &rgb);
        printf("reason %d status %d\n", info.reason, st);
        if (info.reason == 0 && st == 0) {
            FILE* f = fopen(argv[3], "wb");
            if (!f) return 2;
            fprintf(f, "%d %d\n", info.width, info.height);
            fwrite(rgb.data(), 1, rgb.size(), f);
            fclose(f);
        }
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "fuzz")) {
        const std::vector<unsigned char> file = read_file(argv[2]);
        rng_state = strtoull(argv[3], 0, 10);
        yv3_jpeg_info info;
        if (host_decode(file.data(), file.size(), &info, 0) != 0 || info.reason != 0) { printf("the input itself does not decode\n"); return 3; }
        const size_t header = (size_t)info.scan_offset;
        std::map<std::pair<int, int>, int> seen;
        int inputs = 0;
        auto run = [&](const std::vector<unsigned char>& v) {
            unsigned char* exact = (unsigned char*)malloc(v.size() ? v.size() : 1);     // exact size: ASan guards both ends
            if (!v.empty()) memcpy(exact, v.data(), v.size());
            yv3_jpeg_info fi;
            const int st = host_decode(exact, v.size(), &fi, 0);
            free(exact);
            ++seen[std::make_pair(fi.reason, st)];
            ++inputs;
        };
        for (size_t cut = 0; cut < file.size(); ++cut) run(std::vector<unsigned char>(file.begin(), file.begin() + cut));
        for (int i = 0; i < 2000; ++i) {                                                // single-byte corruptions, anywhere
            std::vector<unsigned char> v = file;
            v[rnd() % v.size()] ^= (unsigned char)(1 + rnd() % 255);
            run(v);
        }
        for (int i = 0; i < 500; ++i) {                                                 // random bytes after the valid header
            std::vector<unsigned char> v(file.begin(), file.begin() + header);
            const size_t extra = rnd() % 600;
            for (size_t k = 0; k < extra; ++k) v.push_back((unsigned char)rnd());
            run(v);
        }
        for (int i = 0; i < 300; ++i) {                                                 // a damaged Huffman or quantisation table
            std::vector<unsigned char> v = file;
            v[rnd() % header] = (unsigned char)rnd();
            run(v);
        }
        printf("inputs %d\n", inputs);
        for (const auto& kv : seen) printf("reason %d status %d count %d\n", kv.first.first, kv.first.second, kv.second);
        return 0;
    }
    fprintf(stderr, "usage: jpeg_host_check decode IN OUT | fuzz IN SEED\n");
    return 2;
}
