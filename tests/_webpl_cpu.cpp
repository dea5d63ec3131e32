// Test-side harness: the lossless WebP decoder's host parse and its arithmetic (kobato-eyes_amd/csrc/ke_webpl_parse.h,
// ke_webpl_core.h) built with the host C++ compiler into a shared library that tests/test_webpl_cpu.py loads with ctypes.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ke_webpl_parse.h"

extern "C" {

// status, width, height, channels, EXIF / XMP present of one file
int webpl_cpu_probe(const uint8_t *file, uint64_t size, int32_t *info) {
    KeWebplHeader h;
    ke_parse_webpl(file, (size_t)size, h);
    info[0] = h.status; info[1] = h.width; info[2] = h.height; info[3] = h.channels; info[4] = h.meta;
    return 0;
}

// out: width * height * channels bytes (from webpl_cpu_probe)
int webpl_cpu_decode(const uint8_t *file, uint64_t size, uint8_t *out) {
    KeWebplHeader h;
    ke_parse_webpl(file, (size_t)size, h);
    if (h.status != KE_WEBPL_OK) return h.status;
    std::vector<uint32_t> mem((size_t)ke_vp8l_scratch_words(h.width, h.height));
    return ke_webpl_decode_cpu(file, h, mem.data(), out);
}
}

#ifdef KE_WEBPL_MAIN
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
        int32_t info[5];
        webpl_cpu_probe(exact.data(), exact.size(), info);
        int st = info[0];
        if (st == 0) {
            std::vector<uint8_t> out((size_t)info[1] * info[2] * info[3]);
            st = webpl_cpu_decode(exact.data(), exact.size(), out.data());
            if (st == 0)
                if (FILE *f = fopen((std::string(argv[k]) + ".out").c_str(), "wb")) { fwrite(out.data(), 1, out.size(), f); fclose(f); }
        }
        printf("%d %d %d %d\n", st, info[1], info[2], info[3]);
    }
    return 0;
}
#endif
