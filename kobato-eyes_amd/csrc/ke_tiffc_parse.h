// ke_tiffc_parse.h -- host-side parsing for the decoder of LZW and PackBits TIFF files (ke_tiffc.hip) and the CPU build the tests
// hold against Pillow (tests/_tiffc_cpu.cpp).  Replaces `Image.open(path)` + pixel access of the reference's batch hasher
// (src/core/fastsig.py:31-34) for baseline 8-bit strip files whose Compression is 5 or 32773, Predictor absent, 1 or 2, in the
// photometric layouts ke_tiff_parse.h takes (its directory reading is used: ke_parse_tiff_directory), with the same pixels.
//
// For these files Pillow's Python parser decides mode and size but libtiff's own directory reader decides what is decoded, so
// the whitelist is tighter than the uncompressed one -- where the two readers can disagree the file is refused:
//   * the directory's entries ascend strictly by tag (so no tag appears twice), each of a TIFF 6.0 type with a count above 0
//     and its data inside the file; only tags of a fixed list appear (layout, resolution, text, ICC profile);
//   * BitsPerSample has one value per sample; tile tags, ImageDepth and the like are absent;
//   * StripOffsets and StripByteCounts (required) have one value per strip, ceil(height / RowsPerStrip) of them (libtiff reads
//     strip 0: "only the last offset counts" is the raw decoder's rule); a byte count of 0 is refused, a strip that leaves
//     the file is KE_TIFF_CORRUPT (libtiff's read fails, Pillow raises);
//   * Predictor is absent or one SHORT of 1 or 2 (undone for LZW; libtiff's PackBits codec does not know the tag and shows the
//     samples as stored, so the same here);
//   * an LZW strip opens with the clear code, 9 bits MSB-first -- which also refuses libtiff's old-style LSB-first streams
//     (first byte 0, bit 0 of the second set).
// Any status but 0 sends the file to Pillow at every seam.
#pragma once

#include <algorithm>

#include "ke_tiff_parse.h"
#include "ke_tiffc_core.h"

struct KeTiffcInfo {
    KeTiffInfo t;                        // t.nstrips strips of t.rows_per_strip rows (the last one of what is left)
    int32_t compression, predictor;      // 5 / 32773 (ke_tiffz_parse.h: 8 / 32946); 1 / 2
};
struct KeTiffcStrip { uint32_t off, bytes; };      // inside the file

enum { KE_TIFFC_MAX_PIXELS = 1 << 26 };            // per file: the strips' planes are scratch memory next to the pixels

// The parse of a strip file whose Compression is one of `accepts`: what the decoder of deflate files (ke_tiffz_parse.h) shares
// with this one -- libtiff's directory reader decides for both, so the whitelist above is the same; the stream rules (the
// predictor a codec does not know, the opening of an LZW strip) go by the file's compression.
// strips: the image's strips are appended (nothing is appended unless the status is KE_TIFF_OK)
static inline void ke_parse_tiff_compressed(const uint8_t *p, size_t size, std::vector<KeTiffcStrip> *strips, KeTiffcInfo &info,
                                            std::initializer_list<uint32_t> accepts) {
    uint32_t comp = 0;
    std::vector<uint32_t> offs;
    info.compression = 0;
    info.predictor = 1;
    ke_parse_tiff_directory(p, size, &offs, info.t, &comp, accepts);
    if (info.t.status != KE_TIFF_OK) return;
    KeTiffInfo &t = info.t;
    t.status = KE_TIFF_UNSUPPORTED;
    // A second pass over the directory, with ke_tiff_parse.h's field reader: the first is tolerant the way Pillow's parser is
    // (skips, replaces, stops early) and keeps only the tags it knows; this one is about what it tolerates -- order, every
    // entry's type, count and place, tags outside the list.
    const KeTiffBytes bytes_of{p, p[0] == 'I'};
    auto rd16 = [&](size_t o) { return bytes_of.rd16(o); };
    auto rd32 = [&](size_t o) { return bytes_of.rd32(o); };
    const size_t ifd = rd32(4), n = rd16(ifd);                     // inside the file: the directory was read once already
    static const uint32_t allowed[] = {254, 255, 256, 257, 258, 259, 262, 266, 269, 270, 271, 272, 273, 274, 277, 278, 279, 280, 281, 282,
                                       283, 284, 285, 296, 297, 305, 306, 315, 316, 317, 320, 338, 339, 33432, 34675};
    const int *unit = ke_tiff_unit;                                // (types 1..12 only: the TIFF 6.0 ones)
    struct Field { uint32_t type, count; size_t at; bool have; } counts{0, 0, 0, false}, pred{0, 0, 0, false}, bits{0, 0, 0, false};
    int64_t before = -1;
    for (size_t k = 0; k < n; ++k) {
        const size_t e = ifd + 2 + 12 * k;
        const uint32_t id = rd16(e), type = rd16(e + 2), count = rd32(e + 4);
        if ((int64_t)id <= before) return;
        before = id;
        bool listed = false;
        for (uint32_t a : allowed) listed = listed || a == id;
        if (!listed || type == 0 || type > 12 || count == 0) return;
        const uint64_t bytes = (uint64_t)count * unit[type];
        size_t at = e + 8;
        if (bytes > 4) {
            const uint64_t off = rd32(e + 8);
            if (off + bytes > size) return;
            at = (size_t)off;
        }
        const bool integer = type == 3 || type == 4;
        // the layout tags in their plain form only: SHORT or LONG (ke_parse_tiff_directory checked counts and values of the
        // ones it reads; a type libtiff converts and Pillow does not, or the other way round, never gets here)
        for (uint32_t layout : {256u, 257u, 258u, 259u, 262u, 266u, 273u, 274u, 277u, 278u, 279u, 284u, 317u, 338u, 339u})
            if (id == layout && !integer) return;
        if (id == 279) counts = Field{type, count, at, true};
        if (id == 317) pred = Field{type, count, at, true};
        if (id == 258) bits = Field{type, count, at, true};
    }
    auto value = [&](const Field &f, uint32_t which) { return f.type == 3 ? rd16(f.at + 2 * (size_t)which) : rd32(f.at + 4 * (size_t)which); };
    if (!bits.have || bits.count != (uint32_t)t.spp) return;
    if (pred.have) {
        if (pred.type != 3 || pred.count != 1) return;
        const uint32_t v = value(pred, 0);
        if (v != 1 && v != 2) return;
        // the tag belongs to libtiff's LZW and ZIP codecs: in a PackBits file libtiff does not know it and the samples stay as stored
        info.predictor = comp == KE_TIFFC_PACKBITS ? 1 : (int32_t)v;
    }
    if ((uint64_t)t.width * t.height > KE_TIFFC_MAX_PIXELS) return;
    const uint64_t stride = (uint64_t)t.width * t.spp;
    if (stride * (uint64_t)t.rows_per_strip > KE_TIFFC_MAX_STRIP) return;
    if (!counts.have || counts.count != (uint32_t)t.nstrips || offs.size() != (size_t)t.nstrips) return;
    for (uint32_t s = 0; s < (uint32_t)t.nstrips; ++s) {
        const uint64_t off = offs[s], bytes = value(counts, s);
        if (bytes == 0) return;
        if (off > size || bytes > size - off) {
            t.status = KE_TIFF_CORRUPT;
            return;
        }
        if (comp == KE_TIFFC_LZW && (bytes < 2 || p[off] != 0x80 || (p[off + 1] & 0x80))) return;      // the clear code, 1 0000 0000
    }
    if (strips)
        for (uint32_t s = 0; s < (uint32_t)t.nstrips; ++s) strips->push_back(KeTiffcStrip{offs[s], value(counts, s)});
    info.compression = (int32_t)comp;
    t.status = KE_TIFF_OK;
}

static inline void ke_parse_tiffc(const uint8_t *p, size_t size, std::vector<KeTiffcStrip> *strips, KeTiffcInfo &info) {
    ke_parse_tiff_compressed(p, size, strips, info, {KE_TIFFC_LZW, KE_TIFFC_PACKBITS});
}

// One strip's rows on the host (what ke_tiffc_rows does on the GPU): predictor 2 undone in place, then ke_tiff_unpack's mapping
// into the pixels.  plane: the strip's bytes as its stream yields them; out: height * width * channels bytes.
static inline void ke_tiffc_strip_rows_cpu(const KeTiffcInfo &info, uint8_t *plane, int y0, int rows, uint8_t *out) {
    const KeTiffInfo &t = info.t;
    const size_t stride = (size_t)t.width * t.spp;
    for (int r = 0; r < rows; ++r) {
        uint8_t *row = plane + (size_t)r * stride;
        if (info.predictor == 2)
            for (size_t k = (size_t)t.spp; k < stride; ++k) row[k] = (uint8_t)(row[k] + row[k - (size_t)t.spp]);
        uint8_t *dst = out + (size_t)(y0 + r) * t.width * t.channels;
        if (t.spp == t.channels) {
            for (size_t k = 0; k < stride; ++k) dst[k] = t.mapped ? t.lut[row[k]] : row[k];
        } else {
            for (int x = 0; x < t.width; ++x)
                for (int c = 0; c < 3; ++c) dst[3 * (size_t)x + c] = row[4 * (size_t)x + c];
        }
    }
}

#ifndef __HIPCC__
// ---- the whole decoder on the host, for the tests: the walkers of ke_tiffc_core.h with the copies made as they come
struct KeTiffcHostSrc {
    const uint8_t *p;
    uint32_t byte(uint32_t pos) const { return p[pos]; }
};
struct KeTiffcHostDict {
    uint32_t pos[4096], len[4096];
    void set(uint32_t code, uint32_t at, uint32_t n) { pos[code] = at; len[code] = n; }
    void get(uint32_t code, uint32_t &at, uint32_t &n) const { at = pos[code]; n = len[code]; }
};
struct KeTiffcHostSink {
    uint8_t *plane;
    uint32_t out;
    void literal(uint8_t b) { plane[out++] = b; }
    void copy(uint32_t from, uint32_t len) {
        for (uint32_t k = 0; k < len; ++k, ++out) plane[out] = plane[from + k];
    }
};

// out: height * width * channels bytes
static inline int ke_tiffc_decode_cpu(const uint8_t *file, const KeTiffcInfo &info, const std::vector<KeTiffcStrip> &strips, uint8_t *out) {
    const KeTiffInfo &t = info.t;
    const size_t stride = (size_t)t.width * t.spp;
    std::vector<uint8_t> plane((size_t)t.rows_per_strip * stride);
    KeTiffcHostDict dict;
    for (int s = 0; s < t.nstrips; ++s) {
        const int y0 = s * t.rows_per_strip, rows = std::min(t.rows_per_strip, t.height - y0);
        const uint32_t want = (uint32_t)(rows * stride);
        KeTiffcHostSrc src{file + strips[(size_t)s].off};
        KeTiffcHostSink sink{plane.data(), 0};
        const int st = info.compression == KE_TIFFC_LZW ? ke_tiffc_lzw(src, 0u, strips[(size_t)s].bytes, want, dict, sink)
                                                       : ke_tiffc_packbits(src, 0u, strips[(size_t)s].bytes, want, sink);
        if (st != KE_TIFFC_OK) return st;
        ke_tiffc_strip_rows_cpu(info, plane.data(), y0, rows, out);
    }
    return KE_TIFFC_OK;
}
#endif
