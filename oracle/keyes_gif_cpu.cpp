// keyes_gif_cpu.cpp -- TEST INFRASTRUCTURE: the GIF container walk and LZW arithmetic of the product
// (kobato-eyes_amd/csrc/ke_gif_core.h, the header ke_gif.hip compiles) driven sequentially on the CPU, so that the CPU test suite
// can hold it against the installed Pillow without a GPU.  Only tests/ load this library; the product never does.
#include <vector>

#include "../kobato-eyes_amd/csrc/ke_gif_core.h"
#include "../kobato-eyes_amd/csrc/ke_lz_records.h"

namespace {
struct MemSrc {
    const uint8_t *p;
    uint8_t byte(uint32_t pos) const { return p[pos]; }
};
struct VecDict {
    uint32_t at[4096], n[4096];
    void set(uint32_t code, uint32_t pos, uint32_t len) { at[code] = pos; n[code] = len; }
    void get(uint32_t code, uint32_t &pos, uint32_t &len) const { pos = at[code]; len = n[code]; }
};
struct VecSink {
    std::vector<uint8_t> &v;
    void literal(uint8_t b) { v.push_back(b); }
    void copy(uint32_t from, uint32_t len) {
        for (uint32_t k = 0; k < len; ++k) v.push_back(v[from + k]);      // may run into its own output by one character
    }
};
}  // namespace

extern "C" {

int ko_gif_probe(const uint8_t *file, uint64_t size, int32_t *w, int32_t *h, int32_t *ch) {
    KeGifInfo info;
    ke_parse_gif(file, (size_t)size, info);
    *w = info.width; *h = info.height; *ch = info.channels;
    return info.status;
}

int ko_gif_decode(const uint8_t *file, uint64_t size, uint8_t *out) {
    KeGifInfo info;
    ke_parse_gif(file, (size_t)size, info);
    if (info.status != KE_GIF_OK) return info.status;
    const uint32_t want = (uint32_t)info.width * (uint32_t)info.height;
    std::vector<uint8_t> idx;
    idx.reserve(want);
    MemSrc src{file};
    static thread_local VecDict dict;
    VecSink sink{idx};
    const int rc = ke_gif_lzw(src, info.data_off, (uint32_t)size, info.bits, want, dict, sink);
    if (rc != KE_GIF_OK) return rc;
    for (int k = 0; k < info.height; ++k) {
        uint8_t *dst = out + (size_t)ke_gif_row(k, info.height, info.interlace) * info.width;
        for (int x = 0; x < info.width; ++x) dst[x] = info.lut[idx[(size_t)k * info.width + x]];
    }
    return KE_GIF_OK;
}

// The kernels' way, first half (ke_gif_codes): the code stream walked through the sink the kernels use (ke_lz_records.h).  idx:
// width * height + 2 bytes, the literals land in it; rec: width * height / 2 + 2 records of two uint32 (the bound the kernel's
// scratch rests on, ke_gif.hip) -- a stream that wrote more would be caught by the sanitised build, not here.
int ko_gif_records(const uint8_t *file, uint64_t size, uint8_t *idx, uint32_t *rec, uint32_t *nrec) {
    KeGifInfo info;
    ke_parse_gif(file, (size_t)size, info);
    *nrec = 0;
    if (info.status != KE_GIF_OK) return info.status;
    MemSrc src{file};
    static thread_local VecDict dict;
    KeLzRecSink sink{idx, reinterpret_cast<KeLzRec *>(rec), 0, 0};
    const int rc = ke_gif_lzw(src, info.data_off, (uint32_t)size, info.bits, (uint32_t)info.width * (uint32_t)info.height, dict, sink);
    *nrec = sink.nrec;
    return rc;
}

// Second half (ke_gif_copies, ke_gif_rows), as plainly as it can be said: the recorded copies made strictly in order, byte by
// byte, each {destination, distance << 9 | (length - 2)}; then index -> luma, rows to their places.  -1: a record that reaches
// outside the frame's indices and the one byte of slack behind them.
int ko_gif_replay(const uint8_t *file, uint64_t size, uint8_t *idx, const uint32_t *rec, uint32_t nrec, uint8_t *out) {
    KeGifInfo info;
    ke_parse_gif(file, (size_t)size, info);
    if (info.status != KE_GIF_OK) return info.status;
    const uint64_t want = (uint64_t)info.width * info.height;
    for (uint32_t k = 0; k < nrec; ++k) {
        const uint64_t dst = rec[2 * k], dist = rec[2 * k + 1] >> 9, len = (rec[2 * k + 1] & 511u) + 2;
        if (dist == 0 || dist > dst || dst + len > want + 1) return -1;
        for (uint64_t j = 0; j < len; ++j) idx[dst + j] = idx[dst + j - dist];
    }
    for (int k = 0; k < info.height; ++k) {
        uint8_t *dst = out + (size_t)ke_gif_row(k, info.height, info.interlace) * info.width;
        for (int x = 0; x < info.width; ++x) dst[x] = info.lut[idx[(size_t)k * info.width + x]];
    }
    return KE_GIF_OK;
}

}  // extern "C"
