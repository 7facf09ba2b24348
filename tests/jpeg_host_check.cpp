// Stand-alone host program for tests/test_jpeg_host.py: the JPEG parser, the entropy routine and the pixel arithmetic of the
// GPU decoder, compiled for the CPU with -fsanitize=address,undefined and never loaded into Python.
//   jpeg_host_check decode IN.jpg OUT.rgb    full decode; OUT = "W H\n" + W*H*3 bytes; prints "reason R status S"
//   jpeg_host_check fuzz IN.jpg SEED         every prefix truncation, seeded single-byte corruptions and random bytes after the
//                                            valid header: parser + entropy decode on exact-size heap copies (a read past the
//                                            end is an ASan report); prints how many inputs ended in each (reason, status)
#include <map>
#include <utility>
#include "jpeg_host_common.h"

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "decode")) {
        const std::vector<unsigned char> file = read_file(argv[2]);
        yv3_jpeg_info info;
        std::vector<unsigned char> rgb;
        const int st = host_decode(file.data(), file.size(), &info, &rgb);
        printf("reason %d status %d\n", info.reason, st);
        if (info.reason == 0 && st == 0 && !write_rgb(argv[3], info.width, info.height, rgb)) return 2;
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
            const ExactCopy exact(v);
            yv3_jpeg_info fi;
            const int st = host_decode(exact.data, exact.size, &fi, 0);
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
