// ke_webpn_parse.h -- host-side container walk for animated WebP files, for the GPU decoder of their first frame (ke_webpn.hip)
// and the CPU build the tests hold against Pillow (tests/_webpn_cpu.cpp).  Replaces `Image.open(path)` of the reference's batch
// hasher (src/core/fastsig.py:31-34), which for an animation yields frame 0: an all-zero canvas of the VP8X size -- RGBA where
// the VP8X alpha flag is set, RGB otherwise, whatever the frame carries -- with the frame's own pixels in its rectangle,
// unpremultiplied.  Frame 0 is a key frame, so its blend and dispose bits and the ANIM background colour change nothing.
//
// Pillow opens an animation only if the whole file demuxes, so the walk goes over every chunk with the demuxer's rules:
//   - RIFF / WEBP, the whole RIFF present; a 10-byte VP8X chunk first with the animation flag set (without it the file is one
//     of the still decoders': refused here);
//   - ANIM (at least 6 bytes) before the first ANMF; ALPH / "VP8 " / VP8L / VP8X chunks outside an ANMF chunk are errors;
//   - every ANMF: 16 bytes of header (offsets stored halved, width and height minus one), then the frame's sub-chunks as the
//     demuxer stores them -- an ALPH chunk, then one "VP8 " chunk, or one VP8L chunk alone --, up to the first other chunk,
//     which is read on as a chunk of the file's (so unknown chunks behind the image are skipped).  The image's own size has
//     to be the header's here, the rectangle lies inside the canvas, the sub-chunks end inside the ANMF payload, an ALPH chunk stands in
//     front of its frame and not beside a VP8L image;
//   - every image passes what the demuxer asks of its first bytes (a VP8 key frame to be shown, profile 0..3, partition 0
//     inside the chunk, a size; a VP8L signature and version 0), also in later frames, whose streams are not read further;
//   - ICCP / EXIF / "XMP " and unknown chunks are skipped.
// Frame 0's sub-chunks go through the still decoders' frame parsers with their policies: ke_webp_parse.h's frame tag and
// boolean-coded header, ke_webpa_parse.h's ALPH header byte, ke_webpl_parse.h's stream header.  KE_WEBPN_CORRUPT where the
// demuxer fails the file (Pillow fails then) and where those parsers say so; KE_WEBPN_UNSUPPORTED for everything else that is
// not taken: files without the flag, a canvas over kWebplMaxPixels, an odd RIFF size, a VP8X chunk of another size, a frame in
// whose ANMF header the size is not the bitstream's own, an ANMF chunk without an image in it, fewer than 8 bytes left over at
// the end.
#pragma once

#include <stdint.h>

#include <cstring>

#include "ke_webpa_parse.h"

enum { KE_WEBPN_OK = 0, KE_WEBPN_UNSUPPORTED = 1, KE_WEBPN_CORRUPT = 2 };
enum { KE_WEBPN_LOSSY = 0, KE_WEBPN_LOSSY_ALPHA = 1, KE_WEBPN_LOSSLESS = 2 };    // frame 0's codec

struct KeWebpnHeader {
    int32_t status;
    int32_t canvas_w, canvas_h;
    int32_t channels;        // 4 where the VP8X alpha flag is set, 3 otherwise
    int32_t x, y;            // frame 0's offset inside the canvas
    int32_t width, height;   // frame 0's size
    int32_t codec;           // KE_WEBPN_*
    int32_t meta;            // an EXIF or XMP chunk is present
    int32_t frames;
    KeWebpaHeader a;         // frame 0 where it is lossy: the frame's record and its plane's (KE_ALPH_OPAQUE without one)
    KeWebplHeader l;         // frame 0 where it is lossless
};

namespace ke_webpn_detail {
// What the demuxer asks of an image's first bytes (WebPGetFeatures): the size, or false.
inline bool vp8_info(const uint8_t *f, uint64_t n, int &w, int &h) {
    using namespace ke_webp_detail;
    if (n < 10) return false;
    const uint32_t bits = le24(f);
    if ((bits & 1) || ((bits >> 1) & 7) > 3 || !((bits >> 4) & 1) || (bits >> 5) >= n) return false;
    if (f[3] != 0x9d || f[4] != 0x01 || f[5] != 0x2a) return false;
    w = (int)(le16(f + 6) & 0x3fff);
    h = (int)(le16(f + 8) & 0x3fff);
    return w != 0 && h != 0;
}
inline bool vp8l_info(const uint8_t *f, uint64_t n, int &w, int &h) {
    using namespace ke_webp_detail;
    if (n < 5 || f[0] != 0x2f || (f[4] >> 5) != 0) return false;
    const uint32_t bits = le32(f + 1);
    w = (int)(bits & 0x3fff) + 1;
    h = (int)((bits >> 14) & 0x3fff) + 1;
    return true;
}
}  // namespace ke_webpn_detail

// The container alone: canvas, channels, frame 0's rectangle, codec and where its sub-chunks lie (h.a.f.vp8_off / vp8_size,
// h.a.alph_off / alph_size with the header byte, h.l.off / size).  Returns a status.
static inline int ke_webpn_container(const uint8_t *p, size_t size, KeWebpnHeader &h) {
    using namespace ke_webp_detail;
    if (size < 12 || !tag(p, "RIFF") || !tag(p + 8, "WEBP")) return KE_WEBPN_UNSUPPORTED;
    const uint64_t riff_end = (uint64_t)le32(p + 4) + 8;
    if (riff_end < 20) return KE_WEBPN_CORRUPT;
    if (riff_end > size) return KE_WEBPN_CORRUPT;                    // the demuxer wants the whole RIFF
    if (riff_end & 1) return KE_WEBPN_UNSUPPORTED;
    uint64_t pos = 12;
    if (pos + 8 > riff_end) return KE_WEBPN_CORRUPT;
    if (!tag(p + pos, "VP8X") || le32(p + pos + 4) != 10) return KE_WEBPN_UNSUPPORTED;
    if (pos + 18 > riff_end) return KE_WEBPN_CORRUPT;
    const uint8_t flags = p[pos + 8];
    if (!(flags & 0x02)) return KE_WEBPN_UNSUPPORTED;                // no animation flag: a still decoder's file
    if (flags & ~0x3E) return KE_WEBPN_CORRUPT;                      // reserved bits: the demuxer calls the file invalid
    h.canvas_w = (int)le24(p + pos + 12) + 1;
    h.canvas_h = (int)le24(p + pos + 15) + 1;
    h.channels = (flags & 0x10) ? 4 : 3;
    if ((int64_t)h.canvas_w * h.canvas_h > kWebplMaxPixels) return KE_WEBPN_UNSUPPORTED;
    pos += 18;
    bool anim = false;
    while (pos != riff_end) {
        if (riff_end - pos < 8) return KE_WEBPN_UNSUPPORTED;         // the demuxer waits for more
        const uint8_t *c = p + pos;
        const uint64_t cs = le32(c + 4), padded = cs + (cs & 1), body = pos + 8;
        if (padded > riff_end - body) return KE_WEBPN_CORRUPT;
        if (tag(c, "VP8X") || tag(c, "ALPH") || tag(c, "VP8 ") || tag(c, "VP8L")) return KE_WEBPN_CORRUPT;   // frames lie in ANMF chunks
        if (tag(c, "ANIM")) {
            if (padded < 6) return KE_WEBPN_CORRUPT;
            anim = true;                                             // (a second one is skipped)
        } else if (tag(c, "ANMF")) {
            if (!anim || padded < 16) return KE_WEBPN_CORRUPT;
            const int fx = 2 * (int)le24(c + 8), fy = 2 * (int)le24(c + 11), fw = 1 + (int)le24(c + 14), fh = 1 + (int)le24(c + 17);
            const uint64_t payload = padded - 16;
            uint64_t at = body + 16;
            if (riff_end - at < 8) return KE_WEBPN_UNSUPPORTED;
            // the frame's sub-chunks as the demuxer stores them: ALPH, then the image, up to the first chunk that is neither
            uint64_t alph = 0, alph_size = 0, image = 0, image_size = 0;
            bool have_alph = false, have_image = false, lossless = false;
            for (;;) {
                const uint8_t *s = p + at;
                const uint64_t ss = le32(s + 4), spadded = ss + (ss & 1);
                if (spadded > riff_end - (at + 8)) return KE_WEBPN_CORRUPT;
                if (tag(s, "ALPH")) {
                    if (have_alph) break;
                    if (have_image) return KE_WEBPN_CORRUPT;         // a plane behind its frame
                    have_alph = true;
                    alph = at + 8; alph_size = ss;
                } else if (tag(s, "VP8 ") || tag(s, "VP8L")) {
                    const bool l = tag(s, "VP8L");
                    if (l && have_alph) return KE_WEBPN_CORRUPT;     // VP8L has its own alpha
                    if (have_image) break;
                    int iw = 0, ih = 0;
                    // (the demuxer hands over the padding byte too; neither check reads it)
                    if (!(l ? ke_webpn_detail::vp8l_info(s + 8, ss, iw, ih) : ke_webpn_detail::vp8_info(s + 8, ss, iw, ih))) return KE_WEBPN_CORRUPT;
                    if (iw != fw || ih != fh) return KE_WEBPN_UNSUPPORTED;   // (the demuxer goes by the bitstream's size)
                    have_image = true;
                    lossless = l;
                    image = at + 8; image_size = ss;
                } else {
                    break;
                }
                at += 8 + spadded;
                if (at == riff_end) break;
                if (riff_end - at < 8) return KE_WEBPN_UNSUPPORTED;
            }
            if (at - (body + 16) > payload) return KE_WEBPN_CORRUPT;  // the sub-chunks run past the ANMF chunk
            if (!have_image) return have_alph ? KE_WEBPN_CORRUPT : KE_WEBPN_UNSUPPORTED;
            if (fx + fw > h.canvas_w || fy + fh > h.canvas_h) return KE_WEBPN_CORRUPT;
            if (h.frames == 0) {
                h.x = fx; h.y = fy; h.width = fw; h.height = fh;
                h.codec = lossless ? KE_WEBPN_LOSSLESS : have_alph ? KE_WEBPN_LOSSY_ALPHA : KE_WEBPN_LOSSY;
                if (lossless) {
                    h.l.off = (uint32_t)image; h.l.size = (uint32_t)image_size;
                } else {
                    h.a.f.vp8_off = (uint32_t)image; h.a.f.vp8_size = (uint32_t)image_size;
                    h.a.alph_off = (uint32_t)alph; h.a.alph_size = (uint32_t)alph_size;
                }
            }
            ++h.frames;
            pos = at;                                                // what is left of the ANMF payload is read as chunks of the file
            continue;
        } else if (tag(c, "EXIF") || tag(c, "XMP ")) {
            h.meta = 1;
        }
        pos = body + padded;
    }
    return h.frames ? KE_WEBPN_OK : KE_WEBPN_CORRUPT;
}

// The container and frame 0's tag, ALPH header byte or stream header: status, canvas, channels -- what ke_webpn_probe reports.
// A file that passes here can still be refused by ke_parse_webpn (a lossy frame's boolean-coded header) and by the decode.
static inline void ke_webpn_tag(const uint8_t *p, size_t size, KeWebpnHeader &h) {
    std::memset(&h, 0, sizeof h);
    h.a.method = KE_ALPH_OPAQUE;
    h.status = ke_webpn_container(p, size, h);
    if (h.status != KE_WEBPN_OK) return;
    if (h.codec == KE_WEBPN_LOSSLESS) {
        ke_webpl_stream_header(p, h.l, h.width, h.height);
        h.status = h.l.status;
    } else {
        ke_webp_frame_tag_at(p, h.a.f, h.width, h.height);
        if (h.codec == KE_WEBPN_LOSSY_ALPHA) ke_webpa_alph_at(p, h.a);
        h.status = h.a.f.status;
    }
}

static inline void ke_parse_webpn(const uint8_t *p, size_t size, KeWebpnHeader &h) {
    ke_webpn_tag(p, size, h);
    if (h.status != KE_WEBPN_OK || h.codec == KE_WEBPN_LOSSLESS) return;
    ke_webp_frame_header(p, h.a.f);
    h.status = h.a.f.status;
}

// One canvas pixel from the frame's: R, G, B and, with four channels, A.
KE_HD void ke_webpn_store(uint32_t rgba, uint8_t *o, int channels) {
    o[0] = (uint8_t)rgba; o[1] = (uint8_t)(rgba >> 8); o[2] = (uint8_t)(rgba >> 16);
    if (channels == 4) o[3] = (uint8_t)(rgba >> 24);
}

// The CPU decode the tests hold against Pillow: frame 0 by the still decoders' CPU steps, then placed on the zeroed canvas.
// scratch: ke_webp_scratch_bytes(h.a.f) bytes, 16-aligned, and mem: ke_webpa_plane_words(h.a) words for a lossy frame; mem:
// ke_vp8l_scratch_words(width, height) words for a lossless one; frame: width * height * 4 bytes; out: canvas_w * canvas_h *
// channels bytes.
static inline int ke_webpn_decode_cpu(const uint8_t *file, const KeWebpnHeader &h, uint8_t *scratch, uint32_t *mem, uint8_t *frame, uint8_t *out) {
    if (h.status != KE_WEBPN_OK) return h.status;
    const int W = h.width, H = h.height, ch = h.channels;
    if (h.codec == KE_WEBPN_LOSSLESS) {
        KeVp8lPlan plan;
        const int st = ke_vp8l_decode_stream(file + h.l.off, h.l.size, W, H, mem, ke_vp8l_scratch_words(W, H), plan);
        if (st != KE_WEBPL_OK) return st;
        const uint32_t *pix = ke_vp8l_undo_transforms_cpu(mem, plan, W, H);
        for (size_t j = 0; j < (size_t)W * H; ++j) ke_vp8l_store(pix[j], frame + j * 4, 4);
    } else {
        const int st = ke_webpa_decode_cpu(file, h.a, scratch, mem, frame);
        if (st != KE_WEBPA_OK) return st;
    }
    std::memset(out, 0, (size_t)h.canvas_w * h.canvas_h * ch);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const uint8_t *s = frame + ((size_t)y * W + x) * 4;
            uint8_t *o = out + ((size_t)(h.y + y) * h.canvas_w + h.x + x) * ch;
            o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
            if (ch == 4) o[3] = s[3];
        }
    return KE_WEBPN_OK;
}
