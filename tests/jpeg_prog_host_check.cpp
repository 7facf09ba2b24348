// Stand-alone host program for tests/test_jpeg_prog_host.py: yv3_jpeg_parse_ex, the progressive entropy routine (level by level,
// each level in file order) and the IDCT and pixel arithmetic of the GPU decoder, compiled for the CPU with
// -fsanitize=address,undefined and never loaded into Python.  A baseline file takes the baseline decode of jpeg_host_common.h.
//   jpeg_prog_host_check decode IN OUT [IN OUT ...]   full decode of each IN; OUT = "W H\n" + W*H*3 bytes when it decodes; prints
//                                                     "reason R accepted A status S levels L" per file
//   jpeg_prog_host_check fuzz IN SEED                 every prefix truncation, 2000 seeded single-byte corruptions of the scan
//                                                     data and 300 of the headers, on exact-size heap copies, each decoded to
//                                                     its pixels; prints how many inputs ended in each (reason, accepted, status)
#include <map>
#include <tuple>
#include "jpeg_host_common.h"
#include "../yolo_v3_amd/csrc/jpeg_prog.h"

// What layout_prog_kernel, entropy_prog_kernel, idct_kernel and colour_kernel do, serially.
static int host_decode_prog(const unsigned char* data, size_t n, yv3_jpeg_info* info, yv3_jpeg_prog* prog, std::vector<unsigned char>* rgb) {
    if (yv3_jpeg_parse_ex(data, n, YV3_JPEGP_ACCEPT, info, prog) != 0) return -1;
    if (!prog->accepted) return info->reason ? 0 : host_decode(data, n, info, rgb);
    yv3_jpeg_info frame = *info;
    yv3_jpegp_as_frame(&frame);
    yv3_jpeg_geom g;
    if (yv3_jpegp_geometry(&frame, prog, &g)) return YV3_JPEG_S_INFO;
    unsigned char level[YV3_JPEGP_MAX_SCANS];
    if (yv3_jpegp_levels(prog, level) != prog->nlevels) return YV3_JPEG_S_INFO;
    std::vector<short> coef((size_t)g.nblocks * 64, 0);
    const unsigned char natural[64] = YV3_JPEG_NATURAL_ORDER;
    std::vector<yv3_jpeg_hufftab> tabs(3);
    // the restart markers of every scan first, then level by level as the kernel: the units of a level are independent, the
    // status of a level is the largest of its units', and the first level with a status ends the decode
    std::vector<std::vector<long long>> marks(prog->nscans);
    for (int i = 0; i < prog->nscans; ++i) {
        const yv3_jpegp_scan* sc = prog->scans + i;
        if (level[i] != sc->level) return YV3_JPEG_S_INFO;
        if ((unsigned long long)sc->offset + (unsigned long long)sc->length > n) return YV3_JPEG_S_BOUNDS;
        const unsigned char* scan = data + sc->offset;
        const int nunits = yv3_jpegp_scan_units(yv3_jpegp_scan_items(&g, sc->ns, sc->comp[0]), sc->restart_interval);
        if (nunits > 1) marks[i] = restart_marks(scan, sc->length);
        if (nunits > 1 && (long long)marks[i].size() != nunits - 1) return YV3_JPEG_S_MARKER;
    }
    for (int lev = 1; lev <= prog->nlevels; ++lev) {
        int status = 0;
        for (int i = 0; i < prog->nscans; ++i) {
            const yv3_jpegp_scan* sc = prog->scans + i;
            if (level[i] != lev) continue;
            std::vector<unsigned char> scan_copy(data + sc->offset, data + sc->offset + sc->length);     // exact size: nothing but its own bytes
            const unsigned char* scan = scan_copy.data();
            const long long len = sc->length;
            const yv3_jpeg_hufftab* tp[3] = {&tabs[0], &tabs[1], &tabs[2]};
            bool tables_ok = true;
            for (int j = 0; j < yv3_jpegp_scan_tables(sc); ++j)
                if (yv3_jpeg_build_hufftab(prog->tables[sc->tab[j]].counts, prog->tables[sc->tab[j]].values, sc->ss ? 255 : 15, &tabs[j]))
                    tables_ok = false;
            if (!tables_ok) { if (status < YV3_JPEG_S_HUFFTABLE) status = YV3_JPEG_S_HUFFTABLE; continue; }
            const int items = yv3_jpegp_scan_items(&g, sc->ns, sc->comp[0]);
            const int nunits = yv3_jpegp_scan_units(items, sc->restart_interval), per = sc->restart_interval ? sc->restart_interval : items;
            for (int u = 0; u < nunits; ++u) {
                long long begin, end;
                int st = yv3_jpeg_unit_bytes(scan, len, marks[i].data(), nunits, u, &begin, &end);
                const int i0 = u * per, i1 = items - i0 < per ? items : i0 + per;
                if (!st) st = yv3_jpegp_decode_unit(scan, begin, end, &g, sc, tp, natural, i0, i1, coef.data(), g.nblocks);
                if (st > status) status = st;
            }
        }
        if (status) return status;
    }
    return rgb ? coef_to_rgb(&frame, g, coef, rgb) : 0;
}

int main(int argc, char** argv) {
    static yv3_jpeg_prog prog;
    if (argc >= 4 && argc % 2 == 0 && !strcmp(argv[1], "decode")) {
        for (int a = 2; a + 1 < argc; a += 2) {
            const std::vector<unsigned char> file = read_file(argv[a]);
            const ExactCopy exact(file);
            yv3_jpeg_info info;
            std::vector<unsigned char> rgb;
            const int st = host_decode_prog(exact.data, exact.size, &info, &prog, &rgb);
            printf("reason %d accepted %d status %d levels %d\n", info.reason, prog.accepted, st, prog.nlevels);
            if ((info.reason == 0 || prog.accepted) && st == 0 && !write_rgb(argv[a + 1], info.width, info.height, rgb)) return 2;
        }
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "fuzz")) {
        const std::vector<unsigned char> file = read_file(argv[2]);
        rng_state = strtoull(argv[3], 0, 10);
        yv3_jpeg_info info;
        if (host_decode_prog(file.data(), file.size(), &info, &prog, 0) != 0 || !prog.accepted) { printf("the input itself does not decode\n"); return 3; }
        const size_t header = (size_t)prog.scans[0].offset;
        std::map<std::tuple<int, int, int>, int> seen;
        int inputs = 0;
        auto run = [&](const std::vector<unsigned char>& v) {
            const ExactCopy exact(v);
            yv3_jpeg_info fi;
            std::vector<unsigned char> rgb;                                             // the IDCT and the pixels too: RANGE is a status
            const int st = host_decode_prog(exact.data, exact.size, &fi, &prog, &rgb);
            ++seen[std::make_tuple(fi.reason, prog.accepted, st)];
            ++inputs;
        };
        for (size_t cut = 0; cut < file.size(); ++cut) run(std::vector<unsigned char>(file.begin(), file.begin() + cut));
        for (int i = 0; i < 2000; ++i) {                                                // the scan data (and the headers between the scans)
            std::vector<unsigned char> v = file;
            v[header + rnd() % (v.size() - header)] ^= (unsigned char)(1 + rnd() % 255);
            run(v);
        }
        for (int i = 0; i < 300; ++i) {                                                 // the headers before the first scan
            std::vector<unsigned char> v = file;
            v[rnd() % header] = (unsigned char)rnd();
            run(v);
        }
        printf("inputs %d\n", inputs);
        for (const auto& kv : seen)
            printf("reason %d accepted %d status %d count %d\n", std::get<0>(kv.first), std::get<1>(kv.first), std::get<2>(kv.first), kv.second);
        return 0;
    }
    fprintf(stderr, "usage: jpeg_prog_host_check decode IN OUT [IN OUT ...] | fuzz IN SEED\n");
    return 2;
}
