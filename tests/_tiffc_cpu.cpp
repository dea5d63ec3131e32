// Test-side harness: the host parse and the stream arithmetic of the decoder for LZW and PackBits TIFF files
// (kobato-eyes_amd/csrc/ke_tiffc_parse.h, ke_tiffc_core.h and, through them, ke_tiff_parse.h) built with the host C++ compiler
// into a shared library that tests/test_tiffc_cpu.py loads with ctypes.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ke_lz_records.h"
#include "ke_tiffc_parse.h"

extern "C" {

// status, width, height, channels, compression, predictor, strips, rows per strip of one file
int tiffc_cpu_probe(const uint8_t *file, uint64_t size, int32_t *info) {
    KeTiffcInfo h;
    ke_parse_tiffc(file, (size_t)size, nullptr, h);
    info[0] = h.t.status; info[1] = h.t.width; info[2] = h.t.height; info[3] = h.t.channels;
    info[4] = h.compression; info[5] = h.predictor; info[6] = h.t.nstrips; info[7] = h.t.rows_per_strip;
    return 0;
}

// out: height * width * channels bytes (from tiffc_cpu_probe)
int tiffc_cpu_decode(const uint8_t *file, uint64_t size, uint8_t *out) {
    KeTiffcInfo h;
    std::vector<KeTiffcStrip> strips;
    ke_parse_tiffc(file, (size_t)size, &strips, h);
    if (h.t.status != KE_TIFF_OK) return h.t.status;
    return ke_tiffc_decode_cpu(file, h, strips, out);
}

// The kernels' way for one strip (ke_tiffc_codes): its stream walked through the sink the kernels use (ke_lz_records.h).  plane:
// the strip's bytes + 2, the literals land in it; rec: bytes / 2 + 2 records of two uint32; want: the bytes the strip yields.
int tiffc_cpu_strip_records(const uint8_t *file, uint64_t size, int32_t strip, uint8_t *plane, uint32_t *rec, uint32_t *nrec, uint32_t *want_out) {
    KeTiffcInfo h;
    std::vector<KeTiffcStrip> strips;
    ke_parse_tiffc(file, (size_t)size, &strips, h);
    *nrec = *want_out = 0;
    if (h.t.status != KE_TIFF_OK) return h.t.status;
    if (strip < 0 || strip >= h.t.nstrips) return -1;
    const int y0 = strip * h.t.rows_per_strip, rows = std::min(h.t.rows_per_strip, h.t.height - y0);
    const uint32_t want = (uint32_t)((size_t)rows * h.t.width * h.t.spp);
    KeTiffcHostSrc src{file + strips[(size_t)strip].off};
    static thread_local KeTiffcHostDict dict;
    KeLzRecSink sink{plane, reinterpret_cast<KeLzRec *>(rec), 0, 0};
    const int st = h.compression == KE_TIFFC_LZW ? ke_tiffc_lzw(src, 0u, strips[(size_t)strip].bytes, want, dict, sink)
                                                 : ke_tiffc_packbits(src, 0u, strips[(size_t)strip].bytes, want, sink);
    *nrec = sink.nrec;
    *want_out = want;
    return st;
}

// the uncompressed parser next to it: its answers must not depend on the new one
int tiffc_cpu_probe_plain(const uint8_t *file, uint64_t size, int32_t *info) {
    KeTiffInfo t;
    ke_parse_tiff(file, (size_t)size, nullptr, t);
    info[0] = t.status; info[1] = t.width; info[2] = t.height; info[3] = t.channels;
    return 0;
}
}

#ifdef KE_TIFFC_MAIN
// A program of its own for the sanitised build: decodes every file named on the command line, prints "status width height
// channels" per file and leaves the pixels in <file>.out.
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
        tiffc_cpu_probe(exact.data(), exact.size(), info);
        int st = info[0];
        if (st == 0) {
            std::vector<uint8_t> out((size_t)info[1] * info[2] * info[3]);
            st = tiffc_cpu_decode(exact.data(), exact.size(), out.data());
            if (st == 0)
                if (FILE *f = fopen((std::string(argv[k]) + ".out").c_str(), "wb")) { fwrite(out.data(), 1, out.size(), f); fclose(f); }
        }
        printf("%d %d %d %d\n", st, info[1], info[2], info[3]);
    }
    return 0;
}
#endif
