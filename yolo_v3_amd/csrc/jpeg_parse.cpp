// yv3_jpeg_parse: the marker walk of a JPEG file into a yv3_jpeg_info (plain host C++, no HIP; see yv3.h for what is accepted).
// yv3_jpeg_parse_ex: the same walk, which with YV3_JPEGP_ACCEPT goes on through a progressive file's scans into a yv3_jpeg_prog.
// Every read goes through at() / need(), which know the buffer's size: no byte outside data[0, n) is touched, whatever the
// bytes are.  A file is accepted only when every field the kernels use has been seen and checked; anything else gets a reason.
#include <string.h>
#include "jpeg_parse.h"
#include "jpeg_prog.h"

namespace {

struct Reader {
    const unsigned char* d;
    size_t n;
    bool need(size_t pos, size_t len) const { return pos <= n && len <= n - pos; }
    unsigned at(size_t pos) const { return d[pos]; }                          // callers check need() first
    unsigned be16(size_t pos) const { return (unsigned)d[pos] << 8 | d[pos + 1]; }
};

int refuse(yv3_jpeg_info* out, int reason) { out->reason = reason; return 0; }

// A DHT payload into out's tables; false for a malformed one.  redefined (or null): [8], set to -1 for every table read.
bool read_dht(const Reader& r, size_t seg, size_t seg_end, yv3_jpeg_info* out, int* redefined) {
    size_t p = seg;
    while (p < seg_end) {
        const unsigned tc = r.at(p) >> 4, th = r.at(p) & 15;
        if (tc > 1 || th > 3 || seg_end - p < 17) return false;
        const unsigned t = 4 * tc + th;
        size_t total = 0;
        for (int l = 0; l < 16; ++l) { out->huff_counts[t][l] = (unsigned char)r.at(p + 1 + l); total += out->huff_counts[t][l]; }
        if (total > 256 || seg_end - (p + 17) < total) return false;
        memset(out->huff_values[t], 0, 256);
        for (size_t i = 0; i < total; ++i) out->huff_values[t][i] = (unsigned char)r.at(p + 17 + i);
        yv3_jpeg_hufftab tab;
        out->huff_defined[t] = yv3_jpeg_build_hufftab(out->huff_counts[t], out->huff_values[t], tc ? 255 : 15, &tab) == 0;
        if (redefined) redefined[t] = -1;
        p += 17 + total;
    }
    return true;
}

// The frame rules both walks apply at the first SOS, when every APPn in front of it has been seen: 0, or the reason.  Three
// components must be known to be YCbCr, with luma 1x1 / 2x1 / 2x2 and chroma 1x1.
int frame_rules(yv3_jpeg_info* out, const unsigned char* ids, bool jfif, bool adobe) {
    if (out->ncomp == 3) {
        if (adobe) return YV3_JPEG_COLORSPACE;
        if (!jfif && !(ids[0] == 1 && ids[1] == 2 && ids[2] == 3)) return YV3_JPEG_COLORSPACE;
        if (!((out->h[0] == 1 && out->v[0] == 1) || (out->h[0] == 2 && out->v[0] == 1) || (out->h[0] == 2 && out->v[0] == 2)))
            return YV3_JPEG_SAMPLING;
        for (int c = 1; c < 3; ++c)
            if (out->h[c] != 1 || out->v[c] != 1) return YV3_JPEG_SAMPLING;
    } else {
        out->h[0] = out->v[0] = 1;          // a single component is never interleaved: its factors change nothing
    }
    return 0;
}

int parse_progressive(const Reader& r, size_t pos, const unsigned char* ids, bool jfif, bool adobe, yv3_jpeg_info* out, yv3_jpeg_prog* prog);

// yv3_jpeg_parse (prog null) and yv3_jpeg_parse_ex: one walk.  With prog, SOF2 is read like SOF0 and the walk goes on in
// parse_progressive at the first SOS.
int parse_file(const unsigned char* data, size_t n, yv3_jpeg_info* out, yv3_jpeg_prog* prog) {
    memset(out, 0, sizeof(*out));
    out->reason = YV3_JPEG_NOT_JPEG;
    if (!data) return YV3_EINVAL;
    const Reader r = {data, n};
    if (!r.need(0, 2) || r.at(0) != 0xFF || r.at(1) != 0xD8) return 0;
    bool have_sof = false, jfif = false, adobe = false, progressive = false;
    unsigned char ids[4] = {0, 0, 0, 0};
    size_t pos = 2;
    for (;;) {
        // the next marker: FF, any number of fill FFs, a code
        if (!r.need(pos, 2) || r.at(pos) != 0xFF) return refuse(out, YV3_JPEG_MALFORMED);
        while (r.need(pos, 2) && r.at(pos + 1) == 0xFF) ++pos;
        if (!r.need(pos, 2)) return refuse(out, YV3_JPEG_MALFORMED);
        const unsigned m = r.at(pos + 1);
        pos += 2;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;                    // stand-alone markers
        if (m == 0xD9 || m == 0x00) return refuse(out, YV3_JPEG_MALFORMED);                  // EOI before any scan
        if (!r.need(pos, 2)) return refuse(out, YV3_JPEG_MALFORMED);
        const size_t len = r.be16(pos);
        if (len < 2 || !r.need(pos, len)) return refuse(out, YV3_JPEG_MALFORMED);
        const size_t seg = pos + 2, seg_end = pos + len;                                     // payload [seg, seg_end)
        if (m == 0xC2 && !prog) return refuse(out, YV3_JPEG_PROGRESSIVE);
        if (m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) || (m >= 0xCD && m <= 0xCF) || m == 0xCC)
            return refuse(out, YV3_JPEG_SOF);                                                // (CC: arithmetic conditioning)
        if (m == 0xC0 || m == 0xC1 || m == 0xC2) {
            progressive = m == 0xC2;
            if (have_sof || seg_end - seg < 6) return refuse(out, YV3_JPEG_MALFORMED);
            if (r.at(seg) != 8) return refuse(out, YV3_JPEG_PRECISION);
            out->height = (int)r.be16(seg + 1);
            out->width = (int)r.be16(seg + 3);
            const unsigned nc = r.at(seg + 5);
            if (seg_end - seg != 6 + 3 * (size_t)nc) return refuse(out, YV3_JPEG_MALFORMED);
            if (nc != 1 && nc != 3) return refuse(out, YV3_JPEG_COMPONENTS);
            if (out->width < 1 || out->height < 1 || out->width > YV3_JPEG_MAX_SIDE || out->height > YV3_JPEG_MAX_SIDE)
                return refuse(out, YV3_JPEG_SIZE);
            out->ncomp = (int)nc;
            for (unsigned c = 0; c < nc; ++c) {
                ids[c] = (unsigned char)r.at(seg + 6 + 3 * c);
                out->h[c] = (unsigned char)(r.at(seg + 7 + 3 * c) >> 4);
                out->v[c] = (unsigned char)(r.at(seg + 7 + 3 * c) & 15);
                out->tq[c] = (unsigned char)r.at(seg + 8 + 3 * c);
                if (out->tq[c] > 3 || out->h[c] < 1 || out->h[c] > 4 || out->v[c] < 1 || out->v[c] > 4) return refuse(out, YV3_JPEG_MALFORMED);
            }
            have_sof = true;
        } else if (m == 0xDB) {
            size_t p = seg;
            while (p < seg_end) {
                const unsigned pq = r.at(p) >> 4, tq = r.at(p) & 15;
                if (pq != 0) return refuse(out, YV3_JPEG_PRECISION);
                if (tq > 3 || seg_end - p < 65) return refuse(out, YV3_JPEG_MALFORMED);
                for (int k = 0; k < 64; ++k) out->quant[tq][yv3_jpeg_natural(k)] = (unsigned char)r.at(p + 1 + k);
                out->quant_defined[tq] = 1;
                p += 65;
            }
        } else if (m == 0xC4) {
            if (!read_dht(r, seg, seg_end, out, 0)) return refuse(out, YV3_JPEG_MALFORMED);
        } else if (m == 0xDD) {
            if (seg_end - seg != 2) return refuse(out, YV3_JPEG_MALFORMED);
            out->restart_interval = (int)r.be16(seg);
        } else if (m == 0xE0) {
            if (seg_end - seg >= 14 && memcmp(data + seg, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xE1) {
            if (seg_end - seg >= 6 && memcmp(data + seg, "Exif\0\0", 6) == 0) out->has_exif = 1;
        } else if (m == 0xEE) {
            if (seg_end - seg >= 12 && memcmp(data + seg, "Adobe", 5) == 0) adobe = true;
        } else if (m == 0xDA) {
            if (!have_sof) return refuse(out, YV3_JPEG_MALFORMED);
            if (progressive) return parse_progressive(r, pos - 2, ids, jfif, adobe, out, prog);
            if (seg_end - seg < 1) return refuse(out, YV3_JPEG_MALFORMED);
            const unsigned ns = r.at(seg);
            if (ns < 1 || ns > 4 || seg_end - seg != 4 + 2 * (size_t)ns) return refuse(out, YV3_JPEG_MALFORMED);
            if ((int)ns != out->ncomp) return refuse(out, YV3_JPEG_MULTISCAN);
            for (unsigned c = 0; c < ns; ++c) {
                if (r.at(seg + 1 + 2 * c) != ids[c]) return refuse(out, YV3_JPEG_MULTISCAN);       // another order is another scan layout
                out->td[c] = (unsigned char)(r.at(seg + 2 + 2 * c) >> 4);
                out->ta[c] = (unsigned char)(r.at(seg + 2 + 2 * c) & 15);
                if (out->td[c] > 3 || out->ta[c] > 3) return refuse(out, YV3_JPEG_MALFORMED);
            }
            const size_t tail = seg + 1 + 2 * ns;
            if (r.at(tail) != 0 || r.at(tail + 1) != 63 || r.at(tail + 2) != 0) return refuse(out, YV3_JPEG_MULTISCAN);   // Ss, Se, Ah/Al
            if (const int why = frame_rules(out, ids, jfif, adobe)) return refuse(out, why);
            for (int c = 0; c < out->ncomp; ++c)
                if (!out->quant_defined[out->tq[c]] || !out->huff_defined[out->td[c]] || !out->huff_defined[4 + out->ta[c]])
                    return refuse(out, YV3_JPEG_TABLES);
            // the entropy-coded data: up to the first FF that is followed by neither 00 nor FF nor (with DRI) RSTn
            size_t p = seg_end;
            out->scan_offset = (long long)p;
            bool ended = false;
            while (p < n) {
                const unsigned char* f = (const unsigned char*)memchr(data + p, 0xFF, n - p);
                if (!f) { p = n; break; }
                p = (size_t)(f - data);
                if (p + 1 >= n) { p = n; break; }                        // a lone FF at the end: truncated
                const unsigned c = r.at(p + 1);
                if (c == 0x00 || c == 0xFF || (out->restart_interval && c >= 0xD0 && c <= 0xD7)) { p += (c == 0xFF) ? 1 : 2; continue; }
                ended = true;
                break;
            }
            out->scan_length = (long long)(p - seg_end);
            if (ended && r.at(p + 1) != 0xD9) return refuse(out, YV3_JPEG_MULTISCAN);     // DNL, more scans, tables: not ours
            yv3_jpeg_geom g;
            out->reason = 0;
            if (yv3_jpeg_geometry(out, &g) != 0) return refuse(out, YV3_JPEG_MALFORMED);
            return 0;
        }
        pos = seg_end;
    }
}

// The walk of a progressive file from its first SOS (at `pos`) to EOI: every scan into prog, the script checked as it goes.
int parse_progressive(const Reader& r, size_t pos, const unsigned char* ids, bool jfif, bool adobe, yv3_jpeg_info* out, yv3_jpeg_prog* prog) {
    const size_t n = r.n;
    if (const int why = frame_rules(out, ids, jfif, adobe)) return refuse(out, why);
    if (out->ncomp == 3 && (ids[0] == ids[1] || ids[0] == ids[2] || ids[1] == ids[2])) return refuse(out, YV3_JPEG_MALFORMED);
    for (int c = 0; c < out->ncomp; ++c)
        if (!out->quant_defined[out->tq[c]]) return refuse(out, YV3_JPEG_TABLES);
    yv3_jpeg_geom g;
    {
        yv3_jpeg_info frame = *out;
        yv3_jpegp_as_frame(&frame);
        if (yv3_jpeg_geometry(&frame, &g) != 0) return refuse(out, YV3_JPEG_MALFORMED);
    }
    int pool_of[8];                                          // tables[] entry of each table in force, -1: not taken by a scan yet
    for (int t = 0; t < 8; ++t) pool_of[t] = -1;
    signed char state[3][64];                                // the Al each coefficient has been coded down to, -1: not coded yet
    memset(state, -1, sizeof state);
    int ri = out->restart_interval;
    for (;;) {
        if (!r.need(pos, 2) || r.at(pos) != 0xFF) return refuse(out, YV3_JPEG_MALFORMED);
        while (r.need(pos, 2) && r.at(pos + 1) == 0xFF) ++pos;
        if (!r.need(pos, 2)) return refuse(out, YV3_JPEG_MALFORMED);
        const unsigned m = r.at(pos + 1);
        pos += 2;
        if (m == 0xD9) break;
        if (m == 0x00) return refuse(out, YV3_JPEG_MALFORMED);
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) return refuse(out, YV3_JPEGP_SCRIPT);
        if (!r.need(pos, 2)) return refuse(out, YV3_JPEG_MALFORMED);
        const size_t len = r.be16(pos);
        if (len < 2 || !r.need(pos, len)) return refuse(out, YV3_JPEG_MALFORMED);
        const size_t seg = pos + 2, seg_end = pos + len;
        if (m == 0xC4) {
            if (!read_dht(r, seg, seg_end, out, pool_of)) return refuse(out, YV3_JPEG_MALFORMED);
        } else if (m == 0xDD) {
            if (seg_end - seg != 2) return refuse(out, YV3_JPEG_MALFORMED);
            ri = (int)r.be16(seg);
        } else if (m == 0xDB) {
            return refuse(out, YV3_JPEGP_DQT);
        } else if (m == 0xFE || (m >= 0xE0 && m <= 0xEF)) {
            // comments and application segments carry no decoding state
        } else if (m == 0xDA) {
            if (seg_end - seg < 1) return refuse(out, YV3_JPEG_MALFORMED);
            const unsigned ns = r.at(seg);
            if (ns < 1 || ns > 4 || seg_end - seg != 4 + 2 * (size_t)ns) return refuse(out, YV3_JPEG_MALFORMED);
            if ((int)ns > out->ncomp) return refuse(out, YV3_JPEG_MALFORMED);
            if (prog->nscans >= YV3_JPEGP_MAX_SCANS) return refuse(out, YV3_JPEGP_CAPACITY);
            yv3_jpegp_scan* sc = prog->scans + prog->nscans;
            memset(sc, 0, sizeof *sc);
            sc->ns = (unsigned char)ns;
            sc->tab[0] = sc->tab[1] = sc->tab[2] = 255;
            unsigned td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
            for (unsigned j = 0; j < ns; ++j) {
                const unsigned id = r.at(seg + 1 + 2 * j);
                int c = -1;
                for (int k = out->ncomp - 1; k >= 0; --k) if (ids[k] == id) c = k;
                if (c < 0) return refuse(out, YV3_JPEG_MALFORMED);
                if (j && c <= sc->comp[j - 1]) return refuse(out, YV3_JPEGP_SCAN);
                sc->comp[j] = (unsigned char)c;
                td[j] = r.at(seg + 2 + 2 * j) >> 4; ta[j] = r.at(seg + 2 + 2 * j) & 15;
                if (td[j] > 3 || ta[j] > 3) return refuse(out, YV3_JPEG_MALFORMED);
            }
            const size_t tail = seg + 1 + 2 * ns;
            const unsigned ss = r.at(tail), se = r.at(tail + 1), ah = r.at(tail + 2) >> 4, al = r.at(tail + 2) & 15;
            if (ss == 0 ? se != 0 : (ns != 1 || se < ss || se > 63)) return refuse(out, YV3_JPEGP_SCAN);
            if (al > 13 || (ah != 0 && ah != al + 1)) return refuse(out, YV3_JPEGP_SCAN);
            sc->ss = (unsigned char)ss; sc->se = (unsigned char)se; sc->ah = (unsigned char)ah; sc->al = (unsigned char)al;
            sc->restart_interval = ri;
            const int ntab = yv3_jpegp_scan_tables(sc);
            for (int j = 0; j < ntab; ++j) {
                const unsigned t = ss ? 4 + ta[j] : td[j];
                if (!out->huff_defined[t]) return refuse(out, YV3_JPEG_TABLES);
                if (pool_of[t] < 0) {
                    if (prog->ntables >= YV3_JPEGP_MAX_TABLES) return refuse(out, YV3_JPEGP_CAPACITY);
                    memcpy(prog->tables[prog->ntables].counts, out->huff_counts[t], 16);
                    memcpy(prog->tables[prog->ntables].values, out->huff_values[t], 256);
                    pool_of[t] = prog->ntables++;
                }
                sc->tab[j] = (unsigned char)pool_of[t];
            }
            for (unsigned j = 0; j < ns; ++j) {
                signed char* st = state[sc->comp[j]];
                if (ss > 0 && st[0] < 0) return refuse(out, YV3_JPEGP_SCRIPT);               // AC before DC
                for (unsigned k = ss; k <= se; ++k) {
                    if (ah == 0 ? st[k] >= 0 : st[k] != (int)ah) return refuse(out, YV3_JPEGP_SCRIPT);
                    st[k] = (signed char)al;
                }
            }
            // the entropy-coded data: up to the first FF that is followed by neither 00 nor FF nor (with DRI) RSTn
            size_t p = seg_end;
            bool ended = false;
            while (p < n) {
                const unsigned char* f = (const unsigned char*)memchr(r.d + p, 0xFF, n - p);
                if (!f) { p = n; break; }
                p = (size_t)(f - r.d);
                if (p + 1 >= n) { p = n; break; }
                const unsigned c = r.at(p + 1);
                if (c == 0x00 || c == 0xFF || (ri && c >= 0xD0 && c <= 0xD7)) { p += (c == 0xFF) ? 1 : 2; continue; }
                ended = true;
                break;
            }
            sc->offset = (long long)seg_end;
            sc->length = (long long)(p - seg_end);
            ++prog->nscans;
            if (!ended) break;                               // a truncated file: the device finds what is missing
            pos = p;
            continue;
        } else {
            return refuse(out, YV3_JPEGP_SCRIPT);            // DNL, another frame, ...
        }
        pos = seg_end;
    }
    for (int c = 0; c < out->ncomp; ++c)
        for (int k = 0; k < 64; ++k)
            if (state[c][k] != 0) return refuse(out, YV3_JPEGP_SCRIPT);
    prog->accepted = 1;
    long long units;
    if (yv3_jpegp_check(prog, &g, &units) != 0) { prog->accepted = 0; return refuse(out, YV3_JPEG_MALFORMED); }
    unsigned char level[YV3_JPEGP_MAX_SCANS];
    prog->nlevels = yv3_jpegp_levels(prog, level);
    for (int i = 0; i < prog->nscans; ++i) prog->scans[i].level = level[i];
    out->reason = YV3_JPEG_PROGRESSIVE;
    return 0;
}

}  // namespace

extern "C" int yv3_jpeg_parse(const unsigned char* data, size_t n, yv3_jpeg_info* out) { return parse_file(data, n, out, 0); }

extern "C" int yv3_jpeg_parse_ex(const unsigned char* data, size_t n, int accept, yv3_jpeg_info* out, yv3_jpeg_prog* prog) {
    if (accept & ~YV3_JPEGP_ACCEPT) return YV3_EINVAL;
    if (accept && !prog) return YV3_EINVAL;
    if (prog) memset(prog, 0, sizeof *prog);
    const int rc = parse_file(data, n, out, accept ? prog : 0);
    if (prog && !prog->accepted) memset(prog, 0, sizeof *prog);
    return rc;
}

size_t yv3_jpeg_batch_workspace(const yv3_jpeg_info* infos, int B, const int* prog_of, const yv3_jpeg_prog* progs, int P, bool strict,
                                long long* max_blocks, long long* max_groups) {
    if (!infos || B <= 0 || B > 65535 || P < 0 || P > 65535 || (P && (!prog_of || !progs))) return 0;
    long long total = yv3_jpeg_round256((long long)B * (long long)sizeof(yv3_jpeg_slot));
    if (P) total += yv3_jpeg_round256((long long)B * (long long)sizeof(yv3_jpeg_info));       // layout_prog_kernel's frame records
    for (int b = 0; b < B; ++b) {
        yv3_jpeg_geom g;
        const int pi = P ? prog_of[b] : -1;
        bool ok;
        if (pi < 0) {
            ok = pi == -1 && yv3_jpeg_geometry(infos + b, &g) == 0;
        } else {
            yv3_jpeg_info frame = infos[b];
            yv3_jpegp_as_frame(&frame);
            ok = pi < P && infos[b].reason == YV3_JPEG_PROGRESSIVE && yv3_jpegp_geometry(&frame, progs + pi, &g) == 0;
        }
        if (!ok) {
            if (strict || P) return 0;
            continue;
        }
        total += g.total_bytes;
        const long long groups = ((long long)infos[b].width * infos[b].height + 3) / 4;
        if (max_blocks && g.nblocks > *max_blocks) *max_blocks = g.nblocks;
        if (max_groups && groups > *max_groups) *max_groups = groups;
    }
    return (size_t)total;
}

extern "C" size_t yv3_jpeg_workspace_bytes_prog(const yv3_jpeg_info* infos_host, const int* prog_of_host, const yv3_jpeg_prog* progs_host,
                                                int P, int B, int entropy) {
    if (entropy != YV3_JPEG_ENTROPY_SERIAL && entropy != YV3_JPEG_ENTROPY_PARALLEL) return 0;
    return yv3_jpeg_batch_workspace(infos_host, B, prog_of_host, progs_host, P, false, 0, 0);
}

extern "C" size_t yv3_jpeg_workspace_bytes_ex(const yv3_jpeg_info* infos_host, int B, int entropy) {
    return yv3_jpeg_workspace_bytes_prog(infos_host, 0, 0, 0, B, entropy);      // (the parallel stage's records live in LDS)
}

extern "C" size_t yv3_jpeg_workspace_bytes(const yv3_jpeg_info* infos_host, int B) {
    return yv3_jpeg_workspace_bytes_prog(infos_host, 0, 0, 0, B, YV3_JPEG_ENTROPY_SERIAL);
}
