// Stand-alone host program for tests/test_jpeg_sync_host.py: the self-synchronising entropy decoder of csrc/jpeg_sync.h -- the
// very inline functions entropy_kernel<1> runs -- with the lanes, the passes and the barriers of jpeg.hip's sync_unit emulated by
// loops, compiled for the CPU with -fsanitize=address,undefined and never loaded into Python.  S is a template parameter: every
// check runs at YV3_JPEG_SYNC_S and at half of it, so that the subsequence boundaries fall differently.
//   jpeg_sync_host_check decode IN.jpg OUT.rgb S   parallel decode against yv3_jpeg_decode_unit (status, every coefficient) and an
//                                                  independent bit-by-bit walk (the state at every subsequence's first symbol);
//                                                  OUT = "W H\n" + pixels; prints a summary line and one line per subsequence
//   jpeg_sync_host_check fuzz IN.jpg SEED          every prefix truncation, 2000 seeded single-byte corruptions, 500 random
//                                                  tails, at S and S / 2: parallel status == serial status, equal coefficients
//                                                  at status 0; prints the counts
#include "jpeg_host_common.h"
#include "../yolo_v3_amd/csrc/jpeg_sync.h"

struct UnitStats {
    long long nsub = 0, windows = 0, passes = 0;          // passes: proving passes in which some lane decoded again
    std::vector<yv3_jpeg_sync_state> proven;               // [nsub]; bit == -2: never used (the unit's last block was complete before it)
};

// sync_unit of jpeg.hip: each `for (t ...)` is what the lanes do between two barriers
template <int S>
static int sync_unit_host(const unsigned char* scan, long long begin, long long end, const yv3_jpeg_geom* g, const yv3_jpeg_hufftab* tabs,
                          const unsigned char* sel, const unsigned char* natural, short* coef, int m0, int m1, UnitStats* st) {
    const int L = YV3_JPEG_SYNC_LANES;
    std::vector<yv3_jpeg_sync_state> s_en(L), s_ex(L), en(L), ex(L), ne(L);
    std::vector<int> s_cnt(L), s_off(L), cnt(L);
    std::vector<long long> cut(L);
    std::vector<char> changed(L);
    yv3_jpeg_sync_state s_entry;
    const int bpm = yv3_jpeg_sync_bpm(g), unit_blocks = (m1 - m0) * bpm, nblocks = g->nblocks;
    const long long nsub = (end - begin + S - 1) / S;
    st->nsub = nsub;
    st->proven.assign((size_t)nsub, yv3_jpeg_sync_state{-2, 0, 0});
    int s_flag = 0, s_err = 0, s_fin = 0, s_base = 0;
    s_entry.bit = begin * 8; s_entry.blk = 0; s_entry.zz = 0;
    for (long long i = begin; i < end; ++i)
        if (yv3_jpeg_sync_marker(scan, i, end)) s_flag = 1;
    if (s_flag) return 1;
    long long w0 = 0;
    while (w0 < nsub) {
        const int nl = nsub - w0 < L ? (int)(nsub - w0) : L;
        ++st->windows;
        for (int t = 0; t < nl; ++t) {
            cut[t] = yv3_jpeg_sync_cut(scan, begin, end, w0 + t + 1, S);
            en[t].bit = -1; en[t].blk = 0; en[t].zz = 0;
            if (t == 0) en[t] = s_entry;
            else en[t].bit = yv3_jpeg_sync_cut(scan, begin, end, w0 + t, S) * 8;
            yv3_jpeg_sync_lane(scan, end, cut[t], &en[t], g, tabs, sel, sel + 4, natural, 0, nblocks, m0, 0, 0, &ex[t], &cnt[t]);
            s_en[t] = en[t]; s_ex[t] = ex[t]; s_cnt[t] = cnt[t];
        }
        for (int p = 0; p < YV3_JPEG_SYNC_P; ++p) {
            s_flag = 0;
            for (int t = 0; t < nl; ++t) {
                changed[t] = 0;
                if (t > 0) {
                    ne[t] = s_ex[t - 1];
                    if (ne[t].bit < 0) { ne[t].bit = yv3_jpeg_sync_cut(scan, begin, end, w0 + t, S) * 8; ne[t].blk = 0; ne[t].zz = 0; }
                    changed[t] = !yv3_jpeg_sync_same(ne[t], en[t]);
                    if (changed[t]) s_flag = 1;
                }
            }
            if (!s_flag) break;
            ++st->passes;
            for (int t = 0; t < nl; ++t)
                if (changed[t]) {
                    en[t] = ne[t];
                    yv3_jpeg_sync_lane(scan, end, cut[t], &en[t], g, tabs, sel, sel + 4, natural, 0, nblocks, m0, 0, 0, &ex[t], &cnt[t]);
                }
            for (int t = 0; t < nl; ++t)
                if (changed[t]) { s_en[t] = en[t]; s_ex[t] = ex[t]; s_cnt[t] = cnt[t]; }
        }
        int s_np = nl;
        for (int t = nl - 1; t > 0; --t)
            if (s_ex[t - 1].bit < 0 || !yv3_jpeg_sync_same(s_ex[t - 1], en[t])) s_np = t;
        const int np = s_np;
        int run = s_base;
        for (int j = 0; j < np; ++j) {
            s_off[j] = run;
            run = s_cnt[j] < unit_blocks - run ? run + s_cnt[j] : unit_blocks;
        }
        s_base = run;
        for (int t = 0; t < np; ++t) {
            if (s_off[t] >= unit_blocks) continue;        // behind the unit's last block: its entry state is not used
            st->proven[(size_t)(w0 + t)] = en[t];
            const int r = yv3_jpeg_sync_lane(scan, end, cut[t], &en[t], g, tabs, sel, sel + 4, natural, coef, nblocks, m0, s_off[t], unit_blocks,
                                             &ex[t], &cnt[t]);
            if (r == YV3_JPEG_SYNC_ERROR) s_err = 1;
            if (r == YV3_JPEG_SYNC_FINISHED) s_fin = 1;
        }
        if (s_err) return 1;
        if (s_fin) break;
        s_entry = s_ex[np - 1];
        w0 += np;
    }
    if (!s_fin) return 1;
    const int M = m1 - m0, chunk = (M + L - 1) / L;
    std::vector<long long> s_dc((size_t)L * 3, 0);
    for (int t = 0; t < L; ++t) {
        const int lo = m0 + (t * chunk < M ? t * chunk : M), hi = m0 + ((t + 1) * chunk < M ? (t + 1) * chunk : M);
        yv3_jpeg_sync_dc_sum(coef, g, nblocks, lo, hi, &s_dc[(size_t)t * 3]);
    }
    long long runs[3] = {0, 0, 0};
    for (int j = 0; j < L; ++j)
        for (int c = 0; c < 3; ++c) { const long long v = s_dc[(size_t)j * 3 + c]; s_dc[(size_t)j * 3 + c] = runs[c]; runs[c] += v; }
    for (int t = 0; t < L; ++t) {
        const int lo = m0 + (t * chunk < M ? t * chunk : M), hi = m0 + ((t + 1) * chunk < M ? (t + 1) * chunk : M);
        if (!yv3_jpeg_sync_dc_apply(coef, g, nblocks, lo, hi, &s_dc[(size_t)t * 3])) s_err = 1;
    }
    return s_err;
}

struct Decode {
    yv3_jpeg_info info;
    yv3_jpeg_geom g;
    int status = 0, handed = 0, long_units = 0;
    std::vector<short> coef;
    std::vector<unsigned char> scan;
    std::vector<long long> marks;
    std::vector<yv3_jpeg_hufftab> tabs;
    std::vector<UnitStats> units;                          // of the long units, with their number
    std::vector<int> unit_no;
};

// The entropy stage of a file as entropy_kernel<SYNC> runs it: parallel = 0 is the serial kernel (the reference of every
// comparison), S the subsequence size of the parallel one.  -1: the parser refused the file (d->info.reason), nothing to decode.
template <int S>
static int entropy_host(const unsigned char* data, size_t n, bool parallel, Decode* d) {
    if (yv3_jpeg_parse(data, n, &d->info) != 0 || d->info.reason) return -1;
    const yv3_jpeg_info* info = &d->info;
    if (yv3_jpeg_geometry(info, &d->g)) { d->status = YV3_JPEG_S_INFO; return 0; }
    const yv3_jpeg_geom& g = d->g;
    if ((unsigned long long)info->scan_offset + (unsigned long long)info->scan_length > n) { d->status = YV3_JPEG_S_BOUNDS; return 0; }
    d->scan.assign(data + info->scan_offset, data + info->scan_offset + info->scan_length);     // exact size: ASan guards its ends
    const unsigned char* scan = d->scan.data();
    const long long len = info->scan_length;
    d->tabs.resize(8);
    int status = 0;
    for (int t = 0; t < 8; ++t)
        if (info->huff_defined[t] && yv3_jpeg_build_hufftab(info->huff_counts[t], info->huff_values[t], t < 4 ? 15 : 255, &d->tabs[t]))
            status = YV3_JPEG_S_HUFFTABLE;
    if (g.nunits > 1) d->marks = restart_marks(scan, len);
    if (g.nunits > 1 && (long long)d->marks.size() != g.nunits - 1 && status < YV3_JPEG_S_MARKER) status = YV3_JPEG_S_MARKER;
    d->coef.assign((size_t)g.nblocks * 64, 0);
    if (status) { d->status = status; return 0; }
    const unsigned char natural[64] = YV3_JPEG_NATURAL_ORDER;
    unsigned char sel[8];
    for (int t = 0; t < 8; ++t) sel[t] = t < 4 ? info->td[t] : info->ta[t - 4];
    for (int u = 0; u < g.nunits; ++u) {
        long long begin, end;
        int code = yv3_jpeg_unit_bytes(scan, len, d->marks.data(), g.nunits, u, &begin, &end);
        if (!code) {
            const int m0 = u * g.mcus_per_unit;
            const int m1 = g.nmcu - m0 < g.mcus_per_unit ? g.nmcu : m0 + g.mcus_per_unit;
            bool serial = true;
            if (parallel && end - begin >= 4 * S) {
                ++d->long_units;
                d->units.emplace_back();
                d->unit_no.push_back(u);
                serial = sync_unit_host<S>(scan, begin, end, &g, d->tabs.data(), sel, natural, d->coef.data(), m0, m1, &d->units.back()) != 0;
                if (serial) {
                    ++d->handed;
                    const int bpm = yv3_jpeg_sync_bpm(&g);
                    for (long long q = 0; q < (long long)(m1 - m0) * bpm; ++q) {
                        const long long blk = yv3_jpeg_sync_block(&g, m0 + (int)(q / bpm), (int)(q % bpm), g.nblocks);
                        if (blk >= 0) memset(&d->coef[(size_t)blk * 64], 0, 128);
                    }
                }
            }
            if (serial) code = yv3_jpeg_decode_unit(scan, begin, end, &g, d->tabs.data(), sel, sel + 4, natural, m0, m1, d->coef.data(), g.nblocks);
        }
        if (code > status) status = code;
    }
    d->status = status;
    return 0;
}

// An independent walk of one unit, one bit at a time over the raw bytes: the state at every symbol's first bit, and the state
// after the unit's last symbol.  Only for units the serial routine decodes with status 0.
struct Walk {
    const unsigned char* scan;
    long long pos, end;
    int o;
    long long bit() const { return pos * 8 + o; }
    int next() {
        if (pos >= end) return 0;
        const int v = (scan[pos] >> (7 - o)) & 1;
        if (++o == 8) { o = 0; pos += scan[pos] == 0xFF ? 2 : 1; if (pos > end) pos = end; }
        return v;
    }
    int symbol(const yv3_jpeg_hufftab* t) {
        int code = 0;
        for (int l = 1; l <= 16; ++l) {
            code = code << 1 | next();
            if (code <= t->maxcode[l]) return t->vals[t->valoff[l] + code];
        }
        return -1;
    }
};

static void serial_states(const unsigned char* scan, long long begin, long long end, const yv3_jpeg_geom* g, const yv3_jpeg_hufftab* tabs,
                          const unsigned char* sel, int unit_blocks, std::vector<yv3_jpeg_sync_state>* out) {
    Walk w = {scan, begin, end, 0};
    const int bpm = yv3_jpeg_sync_bpm(g);
    for (int q = 0; q < unit_blocks; ++q) {
        const int j = q % bpm, c = yv3_jpeg_sync_comp(g, j);
        out->push_back(yv3_jpeg_sync_state{w.bit(), j, 0});
        int s = w.symbol(tabs + (sel[c] & 3));
        for (int i = 0; i < s; ++i) w.next();
        for (int k = 1; k < 64;) {
            out->push_back(yv3_jpeg_sync_state{w.bit(), j, k});
            const int rs = w.symbol(tabs + 4 + (sel[4 + c] & 3));
            if (rs < 0) return;
            s = rs & 15;
            if (s) { k += (rs >> 4) + 1; for (int i = 0; i < s; ++i) w.next(); }
            else if ((rs >> 4) == 15) k += 16;
            else break;
        }
    }
    out->push_back(yv3_jpeg_sync_state{w.bit(), 0, 0});   // after the last symbol
}

template <int S>
static int decode_main(const std::vector<unsigned char>& file, const char* out_path) {
    Decode ser, par;
    if (entropy_host<S>(file.data(), file.size(), false, &ser) != 0) { printf("reason %d\n", ser.info.reason); return 0; }
    entropy_host<S>(file.data(), file.size(), true, &par);
    long long nsub = 0, windows = 0, passes = 0;
    for (const UnitStats& u : par.units) { nsub += u.nsub; windows += u.windows; passes += u.passes; }
    printf("reason 0 status %d serial %d coef_equal %d handed %d long_units %d units %d scan_bytes %lld nsub %lld windows %lld passes %lld\n",
           par.status, ser.status, (int)(par.coef == ser.coef), par.handed, par.long_units, par.g.nunits, (long long)par.info.scan_length,
           nsub, windows, passes);
    if (ser.status == 0) {
        unsigned char sel[8];
        for (int t = 0; t < 8; ++t) sel[t] = t < 4 ? par.info.td[t] : par.info.ta[t - 4];
        const long long len = par.info.scan_length;
        for (size_t q = 0; q < par.units.size(); ++q) {
            const int u = par.unit_no[q];
            long long begin, end;
            yv3_jpeg_unit_bytes(par.scan.data(), len, par.marks.data(), par.g.nunits, u, &begin, &end);      // (it passed in entropy_host)
            const int m0 = u * par.g.mcus_per_unit, m1 = par.g.nmcu - m0 < par.g.mcus_per_unit ? par.g.nmcu : m0 + par.g.mcus_per_unit;
            std::vector<yv3_jpeg_sync_state> truth;
            serial_states(par.scan.data(), begin, end, &par.g, par.tabs.data(), sel, (m1 - m0) * yv3_jpeg_sync_bpm(&par.g), &truth);
            size_t at = 0;
            for (long long i = 0; i < par.units[q].nsub; ++i) {
                // the serial decoder's state at the first symbol that begins at or past the subsequence's first byte
                const long long first = i ? begin + i * S : begin;
                while (at + 1 < truth.size() && truth[at].bit < first * 8) ++at;
                const yv3_jpeg_sync_state& p = par.units[q].proven[(size_t)i];
                printf("sub %d %lld symbols %d parallel %lld %d %d serial %lld %d %d\n", u, i, (int)(at + 1 < truth.size()), p.bit, p.blk, p.zz,
                       truth[at].bit, truth[at].blk, truth[at].zz);
            }
        }
    }
    if (par.status == 0) {
        std::vector<unsigned char> rgb;
        if (coef_to_rgb(&par.info, par.g, par.coef, &rgb)) return 3;
        if (!write_rgb(out_path, par.info.width, par.info.height, rgb)) return 2;
    }
    return 0;
}

struct FuzzCount { int inputs = 0, decoded = 0, ok = 0, errors = 0, mismatches = 0, handed = 0, long_units = 0; };

template <int S>
static void fuzz_one(const std::vector<unsigned char>& v, FuzzCount* c) {
    const ExactCopy exact(v);
    Decode ser, par;
    ++c->inputs;
    if (entropy_host<S>(exact.data, exact.size, false, &ser) == 0) {
        entropy_host<S>(exact.data, exact.size, true, &par);
        ++c->decoded;
        c->handed += par.handed;
        c->long_units += par.long_units;
        if (ser.status == 0) ++c->ok; else ++c->errors;
        if (par.status != ser.status || (ser.status == 0 && par.coef != ser.coef)) {
            ++c->mismatches;
            fprintf(stderr, "mismatch: S %d size %zu serial %d parallel %d\n", S, v.size(), ser.status, par.status);
        }
    }
}

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "decode")) {
        const std::vector<unsigned char> file = read_file(argv[2]);
        const int S = atoi(argv[4]);
        if (S == YV3_JPEG_SYNC_S) return decode_main<YV3_JPEG_SYNC_S>(file, argv[3]);
        if (S == YV3_JPEG_SYNC_S / 2) return decode_main<YV3_JPEG_SYNC_S / 2>(file, argv[3]);
        fprintf(stderr, "S must be %d or %d\n", YV3_JPEG_SYNC_S, YV3_JPEG_SYNC_S / 2);
        return 2;
    }
    if (argc == 4 && !strcmp(argv[1], "fuzz")) {
        const std::vector<unsigned char> file = read_file(argv[2]);
        rng_state = strtoull(argv[3], 0, 10);
        yv3_jpeg_info info;
        if (yv3_jpeg_parse(file.data(), file.size(), &info) != 0 || info.reason) { printf("the input itself is refused\n"); return 3; }
        const size_t header = (size_t)info.scan_offset;
        FuzzCount c;
        auto run = [&](const std::vector<unsigned char>& v) { fuzz_one<YV3_JPEG_SYNC_S>(v, &c); fuzz_one<YV3_JPEG_SYNC_S / 2>(v, &c); };
        for (size_t cut = 0; cut < file.size(); ++cut) run(std::vector<unsigned char>(file.begin(), file.begin() + cut));
        for (int i = 0; i < 2000; ++i) {
            std::vector<unsigned char> v = file;
            v[rnd() % v.size()] ^= (unsigned char)(1 + rnd() % 255);
            run(v);
        }
        for (int i = 0; i < 500; ++i) {
            std::vector<unsigned char> v(file.begin(), file.begin() + header);
            const size_t extra = rnd() % 600;
            for (size_t k = 0; k < extra; ++k) v.push_back((unsigned char)rnd());
            run(v);
        }
        printf("inputs %d decoded %d ok %d errors %d mismatches %d handed %d long_units %d\n", c.inputs, c.decoded, c.ok, c.errors, c.mismatches,
               c.handed, c.long_units);
        return 0;
    }
    fprintf(stderr, "usage: jpeg_sync_host_check decode IN OUT S | fuzz IN SEED\n");
    return 2;
}
