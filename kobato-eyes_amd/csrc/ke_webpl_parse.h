// ke_webpl_parse.h -- host-side WebP container walk and VP8L header parse for the GPU's lossless decoder (ke_webpl.hip) and the
// CPU build the tests hold against Pillow (tests/_webpl_cpu.cpp).  Replaces `Image.open(path)` of the reference's batch hasher
// (src/core/fastsig.py:31-34) for the lossless still images Pillow's WebPImagePlugin decodes through libwebp.
//
// What is taken is a whitelist, and everything else is refused (KE_WEBPL_UNSUPPORTED: Pillow decides):
//   - the simple format: RIFF / WEBP / one "VP8L" chunk and nothing else inside the RIFF size;
//   - the extended format: a 10-byte VP8X chunk first, with no flags but ICC / EXIF / XMP / alpha, then one "VP8L" chunk among
//     ICCP / EXIF / "XMP " chunks (skipped), the image's size equal to the canvas;
//   - version 0, at most kWebplMaxPixels pixels.
// "VP8 " (ke_webp_parse.h's), ALPH, ANIM / ANMF and unknown chunks are refused.  A RIFF or chunk size that does not fit the
// file, a chunk too short for the header, a wrong signature: KE_WEBPL_CORRUPT.
// Pillow opens a file as RGBA where the VP8L header's alpha bit is set, whatever the alpha flag of a VP8X chunk says.
#pragma once

#include <stdint.h>

#include <cstring>

#include "ke_webpl_core.h"

struct KeWebplHeader {
    int32_t status;
    int32_t width, height;
    int32_t channels;        // 3, or 4 where Pillow opens the file as RGBA
    int32_t meta;            // an EXIF or XMP chunk is present
    uint32_t off, size;      // the VP8L chunk's payload inside the file
};

namespace ke_webpl_detail {
inline uint32_t le24(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }
inline uint32_t le32(const uint8_t *p) { return le24(p) | ((uint32_t)p[3] << 24); }
inline bool tag(const uint8_t *p, const char *t) { return std::memcmp(p, t, 4) == 0; }
}  // namespace ke_webpl_detail

// The 5-byte header of the VP8L payload h.off / h.size name, whichever container walk found it (this file's, or
// ke_webpn_parse.h's inside an ANMF chunk); cw x ch: the size the container wants of the image, 0 where it names none.
static inline void ke_webpl_stream_header(const uint8_t *p, KeWebplHeader &h, int cw, int ch) {
    using namespace ke_webpl_detail;
    h.status = KE_WEBPL_UNSUPPORTED;
    const uint8_t *f = p + h.off;
    if (h.size < 5 || f[0] != 0x2f) { h.status = KE_WEBPL_CORRUPT; return; }
    const uint32_t bits = le32(f + 1);
    h.width = (int)(bits & 0x3fff) + 1;
    h.height = (int)((bits >> 14) & 0x3fff) + 1;
    h.channels = ((bits >> 28) & 1) ? 4 : 3;
    if ((bits >> 29) != 0) return;                                     // version
    if (cw && (cw != h.width || ch != h.height)) return;
    if ((int64_t)h.width * h.height > kWebplMaxPixels) return;
    h.status = KE_WEBPL_OK;
}

static inline void ke_parse_webpl(const uint8_t *p, size_t size, KeWebplHeader &h) {
    using namespace ke_webpl_detail;
    std::memset(&h, 0, sizeof h);
    h.status = KE_WEBPL_UNSUPPORTED;
    if (size < 12 || !tag(p, "RIFF") || !tag(p + 8, "WEBP")) return;
    const uint64_t riff_end = (uint64_t)le32(p + 4) + 8;
    if (riff_end < 20 || riff_end > size) { h.status = KE_WEBPL_CORRUPT; return; }
    if (riff_end & 1) return;
    uint64_t pos = 12;
    bool first = true, extended = false, have = false;
    int canvas_w = 0, canvas_h = 0;
    while (pos < riff_end) {
        if (pos + 8 > riff_end) { h.status = KE_WEBPL_CORRUPT; return; }
        const uint8_t *c = p + pos;
        const uint64_t cs = le32(c + 4), body = pos + 8;
        if (body + cs > riff_end) { h.status = KE_WEBPL_CORRUPT; return; }
        const uint64_t next = body + cs + (cs & 1);
        if (next > riff_end) return;                                   // the padding byte is missing
        if (tag(c, "VP8L")) {
            if (have) return;
            have = true;
            h.off = (uint32_t)body;
            h.size = (uint32_t)cs;
            if (!extended && next != riff_end) return;                 // simple format: the chunk and nothing else
        } else if (first && tag(c, "VP8X")) {
            if (cs != 10) return;
            const uint8_t flags = c[8];
            if (flags & ~0x3C) return;                                 // animation, reserved bits
            extended = true;
            canvas_w = (int)le24(c + 12) + 1;
            canvas_h = (int)le24(c + 15) + 1;
        } else if (extended && tag(c, "ICCP")) {
        } else if (extended && (tag(c, "EXIF") || tag(c, "XMP "))) {
            h.meta = 1;
        } else {
            return;                                                    // "VP8 ", ALPH, ANIM, ANMF, unknown chunks
        }
        first = false;
        pos = next;
    }
    if (!have) return;
    ke_webpl_stream_header(p, h, extended ? canvas_w : 0, canvas_h);
}

// One pixel's bytes: R, G, B and, with four channels, A.
KE_HD void ke_vp8l_store(uint32_t argb, uint8_t *o, int channels) {
    o[0] = (uint8_t)(argb >> 16); o[1] = (uint8_t)(argb >> 8); o[2] = (uint8_t)argb;
    if (channels == 4) o[3] = (uint8_t)(argb >> 24);
}

// The inverse transforms of a decoded stream on the CPU, last to first: the same steps as ke_webpl_transform_k, one after the
// other.  Returns where the finished W x H image lies (the front of mem).
static inline uint32_t *ke_vp8l_undo_transforms_cpu(uint32_t *mem, const KeVp8lPlan &plan, int W, int H) {
    uint32_t *pix = mem + plan.pix;
    for (int k = plan.ntrans - 1; k >= 0; --k) {
        const KeVp8lXform &t = plan.t[k];
        const int w = t.xsize;
        const uint32_t *data = mem + t.data;
        if (t.type == KE_VP8L_PREDICTOR) {
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < w; ++x) pix[(size_t)y * w + x] = ke_vp8l_add(pix[(size_t)y * w + x], ke_vp8l_predict(pix, w, x, y, data, t.bits));
        } else if (t.type == KE_VP8L_CROSS_COLOUR) {
            const int sw = ke_vp8l_subsample(w, t.bits);
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < w; ++x) pix[(size_t)y * w + x] = ke_vp8l_cross_colour(pix[(size_t)y * w + x], data[(size_t)(y >> t.bits) * sw + (x >> t.bits)]);
        } else if (t.type == KE_VP8L_SUBTRACT_GREEN) {
            for (size_t i = 0; i < (size_t)w * H; ++i) pix[i] = ke_vp8l_add_green(pix[i]);
        } else {                                                       // the packed rows lie behind where their pixels go
            const int sw = ke_vp8l_subsample(w, t.bits);
            uint32_t *wide = mem + ((size_t)W * H - (size_t)w * H);
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < w; ++x) wide[(size_t)y * w + x] = ke_vp8l_colour_index(pix + (size_t)y * sw, x, t.bits, data);
            pix = wide;
        }
    }
    return pix;
}

// The CPU decode the tests hold against Pillow: the same steps as the kernels, one after the other.  mem:
// ke_vp8l_scratch_words(width, height) words; out: width * height * channels bytes.  Returns the status.
static inline int ke_webpl_decode_cpu(const uint8_t *file, const KeWebplHeader &h, uint32_t *mem, uint8_t *out) {
    if (h.status != KE_WEBPL_OK) return h.status;
    const int W = h.width, H = h.height;
    KeVp8lPlan plan;
    const int st = ke_vp8l_decode_stream(file + h.off, h.size, W, H, mem, ke_vp8l_scratch_words(W, H), plan);
    if (st != KE_WEBPL_OK) return st;
    const uint32_t *pix = ke_vp8l_undo_transforms_cpu(mem, plan, W, H);
    for (size_t i = 0; i < (size_t)W * H; ++i) ke_vp8l_store(pix[i], out + i * h.channels, h.channels);
    return KE_WEBPL_OK;
}
