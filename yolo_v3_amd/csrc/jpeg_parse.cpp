// yv3_jpeg_parse: the marker walk of a JPEG file into a yv3_jpeg_info (plain host C++, no HIP; see yv3.h for what is accepted).
// Every read goes through at() / need(), which know the buffer's size: no byte outside data[0, n) is touched, whatever the
// bytes are.  A file is accepted only when every field the kernels use has been seen and checked; anything else gets a reason.
#include <string.h>
#include "jpeg_parse.h"

namespace {

struct Reader {
    const unsigned char* d;
    size_t n;
    bool need(size_t pos, size_t len) const { return pos <= n && len <= n - pos; }
    unsigned at(size_t pos) const { return d[pos]; }                          // callers check need() first
    unsigned be16(size_t pos) const { return (unsigned)d[pos] << 8 | d[pos + 1]; }
};

int refuse(yv3_jpeg_info* out, int reason) { out->reason = reason; return 0; }

}  // namespace

extern "C" int yv3_jpeg_parse(const unsigned char* data, size_t n, yv3_jpeg_info* out) {
    if (!out) return YV3_EINVAL;
    memset(out, 0, sizeof(*out));
    out->reason = YV3_JPEG_NOT_JPEG;
    if (!data) return YV3_EINVAL;
    const Reader r = {data, n};
    if (!r.need(0, 2) || r.at(0) != 0xFF || r.at(1) != 0xD8) return 0;
    bool have_sof = false, jfif = false, adobe = false;
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
        if (m == 0xC2) return refuse(out, YV3_JPEG_PROGRESSIVE);
        if (m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) || (m >= 0xCD && m <= 0xCF) || m == 0xCC)
            return refuse(out, YV3_JPEG_SOF);                                                // (CC: arithmetic conditioning)
        if (m == 0xC0 || m == 0xC1) {
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
            size_t p = seg;
            while (p < seg_end) {
                const unsigned tc = r.at(p) >> 4, th = r.at(p) & 15;
                if (tc > 1 || th > 3 || seg_end - p < 17) return refuse(out, YV3_JPEG_MALFORMED);
                const unsigned t = 4 * tc + th;
                size_t total = 0;
                for (int l = 0; l < 16; ++l) { out->huff_counts[t][l] = (unsigned char)r.at(p + 1 + l); total += out->huff_counts[t][l]; }
                if (total > 256 || seg_end - (p + 17) < total) return refuse(out, YV3_JPEG_MALFORMED);
                memset(out->huff_values[t], 0, 256);
                for (size_t i = 0; i < total; ++i) out->huff_values[t][i] = (unsigned char)r.at(p + 17 + i);
                yv3_jpeg_hufftab tab;
                out->huff_defined[t] = yv3_jpeg_build_hufftab(out->huff_counts[t], out->huff_values[t], tc ? 255 : 15, &tab) == 0;
                p += 17 + total;
            }
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
            if (out->ncomp == 3) {
                if (adobe) return refuse(out, YV3_JPEG_COLORSPACE);
                if (!jfif && !(ids[0] == 1 && ids[1] == 2 && ids[2] == 3)) return refuse(out, YV3_JPEG_COLORSPACE);
                if (!((out->h[0] == 1 && out->v[0] == 1) || (out->h[0] == 2 && out->v[0] == 1) || (out->h[0] == 2 && out->v[0] == 2)))
                    return refuse(out, YV3_JPEG_SAMPLING);
                for (int c = 1; c < 3; ++c)
                    if (out->h[c] != 1 || out->v[c] != 1) return refuse(out, YV3_JPEG_SAMPLING);
            } else {
                out->h[0] = out->v[0] = 1;          // a single component is never interleaved: its factors change nothing
            }
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

size_t yv3_jpeg_batch_workspace(const yv3_jpeg_info* infos, int B, bool strict) {
    if (!infos || B <= 0 || B > 65535) return 0;
    long long total = yv3_jpeg_round256((long long)B * (long long)sizeof(yv3_jpeg_slot));
    for (int b = 0; b < B; ++b) {
        yv3_jpeg_geom g;
        if (yv3_jpeg_geometry(infos + b, &g) == 0) total += g.total_bytes;
        else if (strict) return 0;
    }
    return (size_t)total;
}

extern "C" size_t yv3_jpeg_workspace_bytes(const yv3_jpeg_info* infos_host, int B) {
    return yv3_jpeg_batch_workspace(infos_host, B, false);
}

extern "C" size_t yv3_jpeg_workspace_bytes_ex(const yv3_jpeg_info* infos_host, int B, int entropy) {
    if (entropy != YV3_JPEG_ENTROPY_SERIAL && entropy != YV3_JPEG_ENTROPY_PARALLEL) return 0;
    return yv3_jpeg_batch_workspace(infos_host, B, false);      // the parallel stage's records live in LDS
}
