// Test-side harness: the host parse and the arithmetic of the decoder for lossy WebP files with an alpha plane
// (kobato-eyes_amd/csrc/ke_webpa_parse.h, ke_webpa_core.h and, through them, the lossy and lossless decoders' headers) built with
// the host C++ compiler into a shared library that tests/test_webpa_cpu.py loads with ctypes.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ke_webpa_parse.h"

extern "C" {

// status, width, height, channels, EXIF / XMP present, method (-1: the flag alone), filter, pre-processing of one file
int webpa_cpu_probe(const uint8_t *file, uint64_t size, int32_t *info) {
    KeWebpaHeader h;
    ke_parse_webpa(file, (size_t)size, h);
    info[0] = h.f.status; info[1] = h.f.width; info[2] = h.f.height; info[3] = 4; info[4] = h.f.meta;
    info[5] = h.method; info[6] = h.filter; info[7] = h.pre;
    return 0;
}

// out: width * height * 4 bytes (from webpa_cpu_probe)
int webpa_cpu_decode(const uint8_t *file, uint64_t size, uint8_t *out) {
    KeWebpaHeader h;
    ke_parse_webpa(file, (size_t)size, h);
    if (h.f.status != KE_WEBPA_OK) return h.f.status;
    std::vector<uint64_t> scratch(ke_webp_scratch_bytes(h.f) / 8 + 2);
    std::vector<uint32_t> mem((size_t)ke_webpa_plane_words(h) + 1);
    return ke_webpa_decode_cpu(file, h, (uint8_t *)scratch.data(), mem.data(), out);
}

// One plane's inverse filter on its own: stored -> out, both width * height bytes.
int webpa_cpu_unfilter(int filter, const uint8_t *stored, uint8_t *out, int width, int height) {
    ke_alph_unfilter(filter, [stored](size_t j) { return (uint32_t)stored[j]; }, out, 1, width, height);
    return 0;
}
}

#ifdef KE_WEBPA_MAIN
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
        webpa_cpu_probe(exact.data(), exact.size(), info);
        int st = info[0];
        if (st == 0) {
            std::vector<uint8_t> out((size_t)info[1] * info[2] * 4);
            st = webpa_cpu_decode(exact.data(), exact.size(), out.data());
            if (st == 0)
                if (FILE *f = fopen((std::string(argv[k]) + ".out").c_str(), "wb")) { fwrite(out.data(), 1, out.size(), f); fclose(f); }
        }
        printf("%d %d %d %d\n", st, info[1], info[2], 4);
    }
    return 0;
}
#endif
