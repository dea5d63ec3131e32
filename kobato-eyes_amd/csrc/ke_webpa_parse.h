// ke_webpa_parse.h -- host-side container walk for lossy WebP files with an alpha plane, for the GPU decoder (ke_webpa.hip) and
// the CPU build the tests hold against Pillow (tests/_webpa_cpu.cpp).  Replaces `Image.open(path)` of the reference's batch
// hasher (src/core/fastsig.py:31-34) for the RGBA files Pillow's WebPImagePlugin decodes through libwebp's WebPAnimDecoder:
// what `cwebp` and `Image.save("x.webp")` write for a picture with transparency.
//
// What is taken is a whitelist, and everything else is refused (KE_WEBPA_UNSUPPORTED: Pillow decides):
//   - the extended format only: a 10-byte VP8X chunk first with the alpha flag set and no flags beside it but ICC / EXIF / XMP;
//   - one "VP8 " chunk -- a key frame ke_webp_parse.h's frame parse takes, its size equal to the canvas -- among ICCP / EXIF /
//     "XMP " chunks (skipped);
//   - no ALPH chunk (Pillow opens the file as RGBA with alpha 255), or one directly in front of the frame, as the demuxer wants
//     it: method 0 (at least width * height bytes behind the header byte; more are ignored) or 1, any filter, pre-processing 0
//     or 1.
// Files without the alpha flag belong to ke_webp_parse.h (an ALPH chunk without the flag is dropped by the demuxer, and Pillow's
// alpha is then not the chunk's: refused); "VP8L" images to ke_webpl_parse.h.  KE_WEBPA_CORRUPT, as libwebp fails them: a RIFF
// or chunk size that does not fit the file, two ALPH chunks, an ALPH chunk behind the frame, a chunk of fewer than two bytes, a
// raw plane shorter than the image, method 2 / 3, pre-processing 2 / 3, a reserved bit; and whatever the frame parse
// calls corrupt.
#pragma once

#include <stdint.h>

#include <cstring>

#include "ke_webp_parse.h"
#include "ke_webpa_core.h"
#include "ke_webpl_parse.h"

struct KeWebpaHeader {
    KeWebpHeader f;          // the frame's record; f.status is the whole file's
    int32_t method;          // KE_ALPH_OPAQUE / KE_ALPH_RAW / KE_ALPH_VP8L
    int32_t filter, pre;
    uint32_t alph_off, alph_size;   // what follows the ALPH chunk's header byte, inside the file
};

// The container alone: the "VP8 " payload, the ALPH payload (alph_size 0: none), the canvas, whether an EXIF or XMP chunk is
// present.  The order and count of chunks are held to what the demuxer takes (StoreFrame: ALPH chunks, then the image; a
// second frame is an error).  Returns a status.
static inline int ke_webpa_container(const uint8_t *p, size_t size, uint32_t &vp8_off, uint32_t &vp8_size, uint32_t &alph_off,
                                     uint32_t &alph_size, int &have_alph, int &canvas_w, int &canvas_h, int &meta) {
    using namespace ke_webp_detail;
    vp8_off = vp8_size = alph_off = alph_size = 0;
    have_alph = canvas_w = canvas_h = meta = 0;
    if (size < 12 || !tag(p, "RIFF") || !tag(p + 8, "WEBP")) return KE_WEBPA_UNSUPPORTED;
    const uint64_t riff_end = (uint64_t)le32(p + 4) + 8;
    if (riff_end < 20) return KE_WEBPA_CORRUPT;
    if (riff_end > size) return KE_WEBPA_CORRUPT;                    // the demuxer wants the whole RIFF
    if (riff_end & 1) return KE_WEBPA_UNSUPPORTED;
    uint64_t pos = 12;
    bool first = true, have_vp8 = false, alph_open = false;          // alph_open: the last chunk was the ALPH chunk
    while (pos < riff_end) {
        if (pos + 8 > riff_end) return KE_WEBPA_CORRUPT;
        const uint8_t *c = p + pos;
        const uint64_t cs = le32(c + 4), body = pos + 8;
        if (body + cs > riff_end) return KE_WEBPA_CORRUPT;
        const uint64_t next = body + cs + (cs & 1);
        if (next > riff_end) return KE_WEBPA_UNSUPPORTED;            // the padding byte is missing
        if (first) {
            if (!tag(c, "VP8X") || cs != 10) return KE_WEBPA_UNSUPPORTED;   // the simple format has no alpha plane
            const uint8_t flags = c[8];
            if (flags & ~0x3C) return KE_WEBPA_UNSUPPORTED;          // animation, reserved bits
            if (!(flags & 0x10)) return KE_WEBPA_UNSUPPORTED;        // no alpha flag: ke_webp_decode's file
            canvas_w = (int)le24(c + 12) + 1;
            canvas_h = (int)le24(c + 15) + 1;
        } else if (tag(c, "ALPH")) {
            if (have_alph || have_vp8) return KE_WEBPA_CORRUPT;      // a second one, or one behind the frame: a second frame
            have_alph = 1;
            alph_off = (uint32_t)body;
            alph_size = (uint32_t)cs;
        } else if (alph_open && !tag(c, "VP8 ")) {
            return KE_WEBPA_UNSUPPORTED;                             // the frame has to follow its plane
        } else if (tag(c, "VP8 ")) {
            if (have_vp8) return KE_WEBPA_UNSUPPORTED;
            have_vp8 = true;
            vp8_off = (uint32_t)body;
            vp8_size = (uint32_t)cs;
        } else if (tag(c, "ICCP")) {
        } else if (tag(c, "EXIF") || tag(c, "XMP ")) {
            meta = 1;
        } else {
            return KE_WEBPA_UNSUPPORTED;                             // VP8L, VP8X again, ANIM, ANMF, unknown chunks
        }
        alph_open = tag(c, "ALPH");
        first = false;
        pos = next;
    }
    return have_vp8 ? KE_WEBPA_OK : KE_WEBPA_UNSUPPORTED;
}

// The ALPH chunk's header byte and what the plane needs of the payload h.alph_off / h.alph_size name, beside a frame whose tag
// passed -- whichever container walk found the two (this file's, or ke_webpn_parse.h's inside an ANMF chunk).
static inline void ke_webpa_alph_at(const uint8_t *p, KeWebpaHeader &h) {
    if (h.f.status != KE_WEBP_OK) return;
    if (h.alph_size < 2) { h.f.status = KE_WEBPA_CORRUPT; return; }
    KeAlphHeader a;
    h.f.status = ke_alph_header(p[h.alph_off], a);
    if (h.f.status != KE_WEBPA_OK) return;
    h.method = a.method; h.filter = a.filter; h.pre = a.pre;
    h.alph_off += 1;
    h.alph_size -= 1;
    if (h.method == KE_ALPH_RAW && (uint64_t)h.alph_size < (uint64_t)h.f.width * h.f.height) h.f.status = KE_WEBPA_CORRUPT;
}

// The container, the frame tag and the ALPH header: status, size, what ke_webpa_probe reports.  A file that passes here can
// still be refused by ke_parse_webpa (the frame's boolean-coded header) and by the decode (the token partitions, the plane's
// stream).
static inline void ke_webpa_tag(const uint8_t *p, size_t size, KeWebpaHeader &h) {
    std::memset(&h, 0, sizeof h);
    h.method = KE_ALPH_OPAQUE;
    int cw, ch, have_alph;
    h.f.status = ke_webpa_container(p, size, h.f.vp8_off, h.f.vp8_size, h.alph_off, h.alph_size, have_alph, cw, ch, h.f.meta);
    if (h.f.status != KE_WEBPA_OK) return;
    ke_webp_frame_tag_at(p, h.f, cw, ch);
    if (have_alph) ke_webpa_alph_at(p, h);
}

static inline void ke_parse_webpa(const uint8_t *p, size_t size, KeWebpaHeader &h) {
    ke_webpa_tag(p, size, h);
    ke_webp_frame_header(p, h.f);
}

// Words of scratch the plane needs beside the frame's: a method-1 stream's decoder memory, a raw plane's bytes.
static inline uint64_t ke_webpa_plane_words(const KeWebpaHeader &h) {
    if (h.method == KE_ALPH_VP8L) return ke_vp8l_scratch_words(h.f.width, h.f.height);
    if (h.method == KE_ALPH_RAW) return ((uint64_t)h.f.width * h.f.height + 3) / 4;
    return 0;
}

// The CPU decode the tests hold against Pillow: the same steps as the kernels, one after the other.  scratch:
// ke_webp_scratch_bytes(h.f) bytes, 16-aligned; mem: ke_webpa_plane_words(h) words; rgba: width * height * 4 bytes.
static inline int ke_webpa_decode_cpu(const uint8_t *file, const KeWebpaHeader &h, uint8_t *scratch, uint32_t *mem, uint8_t *rgba) {
    if (h.f.status != KE_WEBPA_OK) return h.f.status;
    const int W = h.f.width, H = h.f.height;
    int st = ke_webp_decode_cpu(file, h.f, scratch, rgba, nullptr, 4);
    if (st != KE_WEBP_OK) return st;
    uint8_t *alpha = rgba + 3;
    if (h.method == KE_ALPH_OPAQUE) {
        for (size_t j = 0; j < (size_t)W * H; ++j) alpha[j * 4] = 255;
    } else if (h.method == KE_ALPH_RAW) {
        const uint8_t *src = file + h.alph_off;
        ke_alph_unfilter(h.filter, [src](size_t j) { return (uint32_t)src[j]; }, alpha, 4, W, H);
    } else {
        KeVp8lBits b;
        ke_vp8l_bits_init(b, file + h.alph_off, h.alph_size);
        KeVp8lPlan plan;
        st = ke_vp8l_decode_body(b, W, H, mem, ke_vp8l_scratch_words(W, H), plan);
        if (st != KE_WEBPL_OK) return st;
        const uint32_t *pix = ke_vp8l_undo_transforms_cpu(mem, plan, W, H);
        ke_alph_unfilter(h.filter, [pix](size_t j) { return (pix[j] >> 8) & 255u; }, alpha, 4, W, H);
    }
    return KE_WEBPA_OK;
}
