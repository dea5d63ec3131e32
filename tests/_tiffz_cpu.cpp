// Test-side harness: the host parse of the decoder for deflate TIFF files and the arithmetic its kernels run
// (kobato-eyes_amd/csrc/ke_tiffz_parse.h, ke_tiffz_core.h, ke_png_core.h's ke_inflate_zlib and, through them, ke_tiffc_parse.h and
// ke_tiff_parse.h) built with the host C++ compiler into a shared library that tests/test_tiffz_cpu.py loads with ctypes.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ke_tiffz_parse.h"

extern "C" {

// status, width, height, channels, compression, predictor, strips, rows per strip of one file
int tiffz_cpu_probe(const uint8_t *file, uint64_t size, int32_t *info) {
    KeTiffcInfo h;
    ke_parse_tiffz(file, (size_t)size, nullptr, h);
    info[0] = h.t.status; info[1] = h.t.width; info[2] = h.t.height; info[3] = h.t.channels;
    info[4] = h.compression; info[5] = h.predictor; info[6] = h.t.nstrips; info[7] = h.t.rows_per_strip;
    return 0;
}

// out: height * width * channels bytes (from tiffz_cpu_probe)
int tiffz_cpu_decode(const uint8_t *file, uint64_t size, uint8_t *out) {
    KeTiffcInfo h;
    std::vector<KeTiffcStrip> strips;
    ke_parse_tiffz(file, (size_t)size, &strips, h);
    if (h.t.status != KE_TIFF_OK) return h.t.status;
    return ke_tiffz_decode_cpu(file, h, strips, out);
}

// the parsers next to it: status of ke_parse_tiff (which 0) and ke_parse_tiffc (which 1); their answers must not depend on the new one
int tiffz_cpu_probe_other(const uint8_t *file, uint64_t size, int32_t which) {
    if (which == 0) {
        KeTiffInfo t;
        ke_parse_tiff(file, (size_t)size, nullptr, t);
        return t.status;
    }
    KeTiffcInfo h;
    ke_parse_tiffc(file, (size_t)size, nullptr, h);
    return h.t.status;
}

// The kernels' way for one strip (ke_tiffz_inflate): literals to their place, every match written down as {destination,
// distance << 9 | (length - 3)} and its bytes left open.  plane: the strip's bytes; rec: want / 3 + 2 records of two uint32.
// Hands back the record count, the bytes the strip yields and the stream's trailer.
int tiffz_cpu_strip_records(const uint8_t *file, uint64_t size, int32_t strip, uint8_t *plane, uint32_t *rec, uint32_t *nrec, uint32_t *want_out,
                            uint32_t *trailer) {
    KeTiffcInfo h;
    std::vector<KeTiffcStrip> strips;
    ke_parse_tiffz(file, (size_t)size, &strips, h);
    *nrec = *want_out = *trailer = 0;
    if (h.t.status != KE_TIFF_OK) return h.t.status;
    if (strip < 0 || strip >= h.t.nstrips) return -1;
    const int y0 = strip * h.t.rows_per_strip, rows = std::min(h.t.rows_per_strip, h.t.height - y0);
    const uint32_t want = (uint32_t)((size_t)rows * h.t.width * h.t.spp);
    struct RecordingSink {
        uint8_t *plane;
        uint32_t *rec;
        uint32_t n, nrec;
        void put(uint8_t b) { plane[n++] = b; }
        void copy(uint32_t dist, uint32_t len) {
            rec[2 * nrec] = n;
            rec[2 * nrec + 1] = (dist << 9) | (len - 3);
            ++nrec;
            n += len;
        }
        uint32_t size() const { return n; }
        bool matches_now(bool) const { return true; }
        void finish() {}
    } sink{plane, rec, 0, 0};
    const int st = ke_tiffz_strip_cpu(file + strips[(size_t)strip].off, strips[(size_t)strip].bytes, want, sink, trailer);
    *nrec = sink.nrec;
    *want_out = want;
    return st;
}

// The Adler-32 as ke_tiffz_copies sums it: the 64 lanes' shares (here a loop), added up, joined.  p must be readable up to the
// next multiple of 16 behind n.
uint32_t tiffz_cpu_adler_by_lanes(const uint8_t *p, uint32_t n) {
    uint32_t s1 = 0, s2 = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const KeTiffzAdlerLane mine = ke_tiffz_adler_lane(p, n, lane);
        s1 += mine.s1;
        s2 += mine.s2;
    }
    return ke_tiffz_adler_join(n, s1, s2);
}
}

#ifdef KE_TIFFZ_MAIN
// A program of its own for the sanitised build: decodes every file named on the command line, prints "status width height
// channels adler" per file -- adler: 1 where the lanes' sum of the pixels equals the sequential one -- and leaves the pixels in
// <file>.out.
int main(int argc, char **argv) {
    for (int k = 1; k < argc; ++k) {
        std::vector<uint8_t> data;
        if (FILE *f = fopen(argv[k], "rb")) {
            uint8_t buf[65536];
            size_t got;
            while ((got = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + got);
            fclose(f);
        }
        std::vector<uint8_t> exact(data.begin(), data.end());          // no slack behind the file's last byte
        int32_t info[8];
        tiffz_cpu_probe(exact.data(), exact.size(), info);
        int st = info[0], same = 1;
        if (st == 0) {
            const size_t n = (size_t)info[1] * info[2] * info[3];
            std::vector<uint8_t> out((n + 15) / 16 * 16);
            st = tiffz_cpu_decode(exact.data(), exact.size(), out.data());
            if (st == 0) {
                if (n <= (size_t)KE_TIFFC_MAX_STRIP) same = tiffz_cpu_adler_by_lanes(out.data(), (uint32_t)n) == ke_adler32(out.data(), n);
                if (FILE *f = fopen((std::string(argv[k]) + ".out").c_str(), "wb")) { fwrite(out.data(), 1, n, f); fclose(f); }
            }
        }
        printf("%d %d %d %d %d\n", st, info[1], info[2], info[3], same);
    }
    return 0;
}
#endif
