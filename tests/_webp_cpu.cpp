// Test-side harness: the WebP decoder's host parse and its arithmetic (kobato-eyes_amd/csrc/ke_webp_parse.h, ke_webp_core.h)
// built with the host C++ compiler into a shared library that tests/test_webp_cpu.py loads with ctypes.
#include <cstdlib>
#include <vector>

#include "ke_webp_parse.h"

extern "C" {

// status, width, height, EXIF / XMP present of one file
int webp_cpu_probe(const uint8_t *file, uint64_t size, int32_t *info) {
    KeWebpHeader h;
    ke_parse_webp(file, (size_t)size, h);
    info[0] = h.status; info[1] = h.width; info[2] = h.height; info[3] = h.meta;
    return 0;
}

// rgb: width * height * 3 bytes (from webp_cpu_probe); yuv (nullable): the filtered planes, mb_w * mb_h * 384 bytes
int webp_cpu_decode(const uint8_t *file, uint64_t size, uint8_t *rgb, uint8_t *yuv) {
    KeWebpHeader h;
    ke_parse_webp(file, (size_t)size, h);
    if (h.status != KE_WEBP_OK) return h.status;
    std::vector<uint8_t> scratch(ke_webp_scratch_bytes(h) + 16);
    uint8_t *s = scratch.data() + ((16 - ((uintptr_t)scratch.data() & 15)) & 15);
    return ke_webp_decode_cpu(file, h, s, rgb, yuv);
}
}
