// ke_tiffz_parse.h -- host-side parsing for the decoder of deflate-compressed TIFF files (ke_tiffz.hip) and the CPU build the
// tests hold against Pillow (tests/_tiffz_cpu.cpp).  Replaces `Image.open(path)` + pixel access of the reference's batch hasher
// (src/core/fastsig.py:31-34) for baseline 8-bit strip files whose Compression is 8 ("Adobe deflate") or its old alias 32946,
// Predictor absent, 1 or 2 (libtiff's ZIP codec honours the tag for both values), in the photometric layouts ke_tiff_parse.h
// takes, with the same pixels.  Pillow hands these files to libtiff as it does LZW and PackBits ones, so the directory
// whitelist is ke_tiffc_parse.h's, shared, not copied (ke_parse_tiff_compressed).
//
// A strip is one zlib stream (RFC 1950).  Nothing of it is looked at here: ke_inflate_zlib refuses a bad header.  The rule the
// decoders hold a strip to is stricter than libtiff's in two named places:
//   * the stream is complete -- header, deflate data, the four bytes of its Adler-32 -- and ke_inflate_zlib takes it;
//   * it yields exactly the bytes of the strip's rows, and their Adler-32 is the stream's; bytes behind the stream are ignored.
// libtiff stops inflating when the strip is full, so it also takes a stream that would yield more ("too long") and one whose
// trailer is cut or missing ("cut trailer"); both are KE_TIFF_CORRUPT here and go to Pillow, which opens them.  Every other
// refusal is Pillow's as well: a wrong trailer, a stream that yields too little, raw deflate, a gzip wrapper, a preset
// dictionary.
#pragma once

#include "ke_tiffc_parse.h"
#include "ke_tiffz_core.h"

enum { KE_TIFFZ_DEFLATE = 8, KE_TIFFZ_DEFLATE_OLD = 32946 };

// strips: the image's strips are appended (nothing is appended unless the status is KE_TIFF_OK)
static inline void ke_parse_tiffz(const uint8_t *p, size_t size, std::vector<KeTiffcStrip> *strips, KeTiffcInfo &info) {
    ke_parse_tiff_compressed(p, size, strips, info, {KE_TIFFZ_DEFLATE, KE_TIFFZ_DEFLATE_OLD});
}

#ifndef __HIPCC__
#include "ke_png_core.h"

// ---- the whole decoder on the host, for the tests: ke_inflate_zlib with the reference tables and a plain sink
struct KeTiffzHostSrc {
    const uint8_t *p;
    uint32_t len;
    uint32_t word(uint32_t k) const {                     // the k-th little-endian dword of the strip's bytes, zeros past its end
        uint32_t w = 0;
        for (uint32_t j = 0; j < 4; ++j)
            if ((uint64_t)k * 4 + j < len) w |= (uint32_t)p[(size_t)k * 4 + j] << (8 * j);
        return w;
    }
    void tick(uint32_t) {}
};
struct KeTiffzHostSink {
    uint8_t *plane;
    uint32_t n;
    void put(uint8_t b) { plane[n++] = b; }
    void copy(uint32_t dist, uint32_t len) {
        for (uint32_t k = 0; k < len; ++k, ++n) plane[n] = plane[n - dist];
    }
    uint32_t size() const { return n; }
    bool matches_now(bool) const { return true; }         // one stream: a match is finished where it starts
    void finish() {}
};

// One strip by the rule above into plane[0, want): KE_TIFF_OK or KE_TIFF_CORRUPT.
template <typename Sink>
static inline int ke_tiffz_strip_cpu(const uint8_t *z, uint32_t bytes, uint32_t want, Sink &sink, uint32_t *trailer) {
    KeTiffzHostSrc src{z, bytes};
    KeBitsLsb<KeTiffzHostSrc> bits{&src, 0, 0, 0};
    KeInflateTables tab;
    const int rc = ke_inflate_zlib(bits, sink, bytes, want, tab, trailer);
    return rc == KE_PNG_OK && sink.size() == want ? KE_TIFF_OK : KE_TIFF_CORRUPT;
}

// out: height * width * channels bytes
static inline int ke_tiffz_decode_cpu(const uint8_t *file, const KeTiffcInfo &info, const std::vector<KeTiffcStrip> &strips, uint8_t *out) {
    const KeTiffInfo &t = info.t;
    const size_t stride = (size_t)t.width * t.spp;
    std::vector<uint8_t> plane((size_t)t.rows_per_strip * stride);
    for (int s = 0; s < t.nstrips; ++s) {
        const int y0 = s * t.rows_per_strip, rows = std::min(t.rows_per_strip, t.height - y0);
        const uint32_t want = (uint32_t)(rows * stride);
        KeTiffzHostSink sink{plane.data(), 0};
        uint32_t trailer = 0;
        if (ke_tiffz_strip_cpu(file + strips[(size_t)s].off, strips[(size_t)s].bytes, want, sink, &trailer) != KE_TIFF_OK) return KE_TIFF_CORRUPT;
        if (ke_adler32(plane.data(), want) != trailer) return KE_TIFF_CORRUPT;
        ke_tiffc_strip_rows_cpu(info, plane.data(), y0, rows, out);
    }
    return KE_TIFF_OK;
}
#endif
