// Test-side harness: the host parse and the arithmetic of the decoder for the first frame of animated WebP files
// (kobato-eyes_amd/csrc/ke_webpn_parse.h and, through it, the three still decoders' headers) built with the host C++ compiler
// into a program of its own (-DKE_WEBPN_MAIN), which tests/test_webpn_cpu.py runs under AddressSanitizer and UBSan.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ke_webpn_parse.h"

// status, canvas width, canvas height, channels, EXIF / XMP present, codec of frame 0, frames of one file
static void webpn_cpu_probe(const uint8_t *file, size_t size, int32_t *info) {
    KeWebpnHeader h;
    ke_parse_webpn(file, size, h);
    info[0] = h.status; info[1] = h.canvas_w; info[2] = h.canvas_h; info[3] = h.channels; info[4] = h.meta; info[5] = h.codec; info[6] = h.frames;
}

// out: canvas width * canvas height * channels bytes (from webpn_cpu_probe)
static int webpn_cpu_decode(const uint8_t *file, size_t size, uint8_t *out) {
    KeWebpnHeader h;
    ke_parse_webpn(file, size, h);
    if (h.status != KE_WEBPN_OK) return h.status;
    const bool lossless = h.codec == KE_WEBPN_LOSSLESS;
    std::vector<uint64_t> scratch(lossless ? 2 : ke_webp_scratch_bytes(h.a.f) / 8 + 2);
    std::vector<uint32_t> mem((size_t)(lossless ? ke_vp8l_scratch_words(h.width, h.height) : ke_webpa_plane_words(h.a)) + 1);
    std::vector<uint8_t> frame((size_t)h.width * h.height * 4);
    return ke_webpn_decode_cpu(file, h, (uint8_t *)scratch.data(), mem.data(), frame.data(), out);
}

#ifdef KE_WEBPN_MAIN
// webpn_cpu <directory> <count>: decodes <directory>/0.webp .. <count - 1>.webp, prints "status width height channels meta codec
// frames" per file and leaves the pixels of a taken one in <directory>/<k>.out.
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const std::string dir = argv[1];
    const long count = atol(argv[2]);
    for (long k = 0; k < count; ++k) {
        std::vector<uint8_t> data;
        const std::string path = dir + "/" + std::to_string(k);
        if (FILE *f = fopen((path + ".webp").c_str(), "rb")) {
            uint8_t buf[65536];
            size_t got;
            while ((got = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + got);
            fclose(f);
        }
        std::vector<uint8_t> exact(data.begin(), data.end());          // no slack behind the file's last byte
        int32_t info[7];
        webpn_cpu_probe(exact.data(), exact.size(), info);
        int st = info[0];
        if (st == 0) {
            std::vector<uint8_t> out((size_t)info[1] * info[2] * info[3]);
            st = webpn_cpu_decode(exact.data(), exact.size(), out.data());
            if (st == 0)
                if (FILE *f = fopen((path + ".out").c_str(), "wb")) { fwrite(out.data(), 1, out.size(), f); fclose(f); }
        }
        printf("%d %d %d %d %d %d %d\n", st, info[1], info[2], info[3], info[4], info[5], info[6]);
    }
    return 0;
}
#endif
