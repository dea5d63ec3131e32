// ke_webp_parse.h -- host-side WebP container walk and VP8 frame-header parse for the GPU decoder (ke_webp.hip) and the CPU
// build the tests hold against Pillow (tests/_webp_cpu.cpp).  Replaces `Image.open(path)` of the reference's batch hasher
// (src/core/fastsig.py:31-34) for the lossy still images Pillow's WebPImagePlugin decodes through libwebp's WebPAnimDecoder.
//
// What is taken is a whitelist, and everything else is refused (KE_WEBP_UNSUPPORTED: Pillow decides):
//   - the simple format: RIFF / WEBP / one "VP8 " chunk and nothing else inside the RIFF size (bytes behind it are ignored,
//     as the demuxer ignores them);
//   - the extended format: a 10-byte VP8X chunk first, with no flags but ICC / EXIF / XMP, then one "VP8 " chunk among
//     ICCP / EXIF / "XMP " chunks (skipped: Pillow applies none of them when it opens the file), the frame's size equal to
//     the canvas;
//   - a key frame with show_frame set, profile 0..3, at most kWebpMaxMbs macroblocks.
// Lossless (VP8L), ALPH, ANIM / ANMF and unknown chunks are refused.  A RIFF or chunk size that does not fit the file, a
// partition that cannot hold its sizes, a frame header that reads past partition 0: KE_WEBP_CORRUPT (libwebp fails those).
#pragma once

#include <stdint.h>

#include <cstring>

#include "ke_webp_core.h"

namespace ke_webp_detail {
inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le24(const uint8_t *p) { return le16(p) | ((uint32_t)p[2] << 16); }
inline uint32_t le32(const uint8_t *p) { return le24(p) | ((uint32_t)p[3] << 24); }
inline bool tag(const uint8_t *p, const char *t) { return std::memcmp(p, t, 4) == 0; }
}  // namespace ke_webp_detail

// The container alone: the "VP8 " payload [*vp8_off, + *vp8_size), the canvas of a VP8X file (0 for the simple format) and
// whether an EXIF or XMP chunk is present (Pillow's getexif() reads an orientation from either: exif_transpose turns by it).  Returns a status.
static inline int ke_webp_container(const uint8_t *p, size_t size, uint32_t &vp8_off, uint32_t &vp8_size, int &canvas_w,
                                    int &canvas_h, int &meta) {
    using namespace ke_webp_detail;
    vp8_off = vp8_size = 0;
    canvas_w = canvas_h = 0;
    meta = 0;
    if (size < 12 || !tag(p, "RIFF") || !tag(p + 8, "WEBP")) return KE_WEBP_UNSUPPORTED;
    const uint64_t riff_end = (uint64_t)le32(p + 4) + 8;
    if (riff_end < 20) return KE_WEBP_CORRUPT;
    if (riff_end > size) return KE_WEBP_CORRUPT;                     // the demuxer wants the whole RIFF
    if (riff_end & 1) return KE_WEBP_UNSUPPORTED;
    uint64_t pos = 12;
    bool first = true, extended = false, have_vp8 = false;
    while (pos < riff_end) {
        if (pos + 8 > riff_end) return KE_WEBP_CORRUPT;
        const uint8_t *c = p + pos;
        const uint64_t cs = le32(c + 4), body = pos + 8;
        if (body + cs > riff_end) return KE_WEBP_CORRUPT;
        const uint64_t next = body + cs + (cs & 1);
        if (next > riff_end) return KE_WEBP_UNSUPPORTED;              // the padding byte is missing
        if (tag(c, "VP8 ")) {
            if (have_vp8) return KE_WEBP_UNSUPPORTED;
            have_vp8 = true;
            vp8_off = (uint32_t)body;
            vp8_size = (uint32_t)cs;
            if (!extended && next != riff_end) return KE_WEBP_UNSUPPORTED;   // simple format: the chunk and nothing else
        } else if (first && tag(c, "VP8X")) {
            if (cs != 10) return KE_WEBP_UNSUPPORTED;
            const uint8_t flags = c[8];
            if (flags & ~0x2C) return KE_WEBP_UNSUPPORTED;            // alpha, animation, reserved bits
            extended = true;
            canvas_w = (int)le24(c + 12) + 1;
            canvas_h = (int)le24(c + 15) + 1;
        } else if (extended && tag(c, "ICCP")) {
        } else if (extended && (tag(c, "EXIF") || tag(c, "XMP "))) {
            meta = 1;
        } else {
            return KE_WEBP_UNSUPPORTED;                               // VP8L, ALPH, ANIM, ANMF, unknown chunks
        }
        first = false;
        pos = next;
    }
    return have_vp8 ? KE_WEBP_OK : KE_WEBP_UNSUPPORTED;
}

// The frame tag of the payload h.vp8_off / h.vp8_size name, whichever container walk found it (this file's, or
// ke_webpa_parse.h's for files with an alpha plane); cw x ch: the canvas of a VP8X file, 0 for the simple format.
static inline void ke_webp_frame_tag_at(const uint8_t *p, KeWebpHeader &h, int cw, int ch) {
    using namespace ke_webp_detail;
    h.status = KE_WEBP_CORRUPT;
    const uint8_t *f = p + h.vp8_off;
    const uint32_t n = h.vp8_size;
    if (n < 10) return;
    const uint32_t bits = le24(f);
    const uint32_t part0 = bits >> 5;
    if (bits & 1) { h.status = KE_WEBP_UNSUPPORTED; return; }          // an inter frame
    if (((bits >> 1) & 7) > 3) { h.status = KE_WEBP_UNSUPPORTED; return; }
    if (!((bits >> 4) & 1)) { h.status = KE_WEBP_UNSUPPORTED; return; }  // show_frame 0
    if (part0 >= n) return;
    if (f[3] != 0x9d || f[4] != 0x01 || f[5] != 0x2a) return;
    const int W = (int)(le16(f + 6) & 0x3fff), H = (int)(le16(f + 8) & 0x3fff);
    if (W == 0 || H == 0) { h.status = KE_WEBP_UNSUPPORTED; return; }
    if (cw && (cw != W || ch != H)) { h.status = KE_WEBP_UNSUPPORTED; return; }
    h.width = W; h.height = H;
    h.mb_w = (W + 15) >> 4; h.mb_h = (H + 15) >> 4;
    if (h.mb_w * h.mb_h > kWebpMaxMbs) { h.status = KE_WEBP_UNSUPPORTED; return; }
    if (part0 > n - 10) return;
    h.status = KE_WEBP_OK;
}

// The container and the frame tag (section 9.1, 9.2): status, size, macroblocks -- what ke_webp_probe reports, without the
// boolean-coded part of the header.  A file that passes here can still be refused by ke_parse_webp.
static inline void ke_webp_frame_tag(const uint8_t *p, size_t size, KeWebpHeader &h) {
    std::memset(&h, 0, sizeof h);
    int cw, ch;
    h.status = ke_webp_container(p, size, h.vp8_off, h.vp8_size, cw, ch, h.meta);
    if (h.status != KE_WEBP_OK) return;
    ke_webp_frame_tag_at(p, h, cw, ch);
}

// The boolean-coded frame header (section 9) and the token partitions of a frame whose tag passed.
static inline void ke_webp_frame_header(const uint8_t *p, KeWebpHeader &h) {
    using namespace ke_webp_detail;
    if (h.status != KE_WEBP_OK) return;
    h.status = KE_WEBP_CORRUPT;
    const uint32_t n = h.vp8_size, part0 = le24(p + h.vp8_off) >> 5;
    // partition 0: offsets relative to the file from here on
    const uint32_t base = h.vp8_off;
    KeVp8Bool br;
    ke_vp8_init(br, p, base + 10, base + 10 + part0);
    ke_vp8_value(br, p, 1);                                          // colour space
    ke_vp8_value(br, p, 1);                                          // clamping type (libwebp always clamps)
    // segments (9.3)
    int use_segment = ke_vp8_value(br, p, 1), absolute = 1;
    int quant[4] = {0, 0, 0, 0}, fstr[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; ++k) h.seg_probs[k] = 255;
    if (use_segment) {
        h.update_map = (int)ke_vp8_value(br, p, 1);
        if (ke_vp8_value(br, p, 1)) {
            absolute = (int)ke_vp8_value(br, p, 1);
            for (int s = 0; s < 4; ++s) quant[s] = ke_vp8_value(br, p, 1) ? ke_vp8_signed_value(br, p, 7) : 0;
            for (int s = 0; s < 4; ++s) fstr[s] = ke_vp8_value(br, p, 1) ? ke_vp8_signed_value(br, p, 6) : 0;
        }
        if (h.update_map)
            for (int s = 0; s < 3; ++s) h.seg_probs[s] = (uint8_t)(ke_vp8_value(br, p, 1) ? ke_vp8_value(br, p, 8) : 255u);
    }
    if (br.eof) return;
    // filter (9.4)
    const int simple = (int)ke_vp8_value(br, p, 1), level = (int)ke_vp8_value(br, p, 6), sharp = (int)ke_vp8_value(br, p, 3);
    const int use_lf_delta = (int)ke_vp8_value(br, p, 1);
    int ref_lf[4] = {0, 0, 0, 0}, mode_lf[4] = {0, 0, 0, 0};
    if (use_lf_delta && ke_vp8_value(br, p, 1)) {
        for (int i = 0; i < 4; ++i)
            if (ke_vp8_value(br, p, 1)) ref_lf[i] = ke_vp8_signed_value(br, p, 6);
        for (int i = 0; i < 4; ++i)
            if (ke_vp8_value(br, p, 1)) mode_lf[i] = ke_vp8_signed_value(br, p, 6);
    }
    h.filter_type = level == 0 ? 0 : simple ? 1 : 2;
    if (br.eof) return;
    // token partitions (9.5)
    const uint32_t last = (1u << ke_vp8_value(br, p, 2)) - 1;
    h.num_parts = (int)last + 1;
    {
        const uint32_t start = base + 10 + part0, end = base + n;
        uint32_t size_left = end - start;
        if (size_left < 3 * last) return;
        uint32_t part_start = start + 3 * last;
        size_left -= 3 * last;
        for (uint32_t k = 0; k < last; ++k) {
            uint32_t psize = le24(p + start + 3 * k);
            if (psize > size_left) psize = size_left;
            ke_vp8_init(h.parts[k], p, part_start, part_start + psize);
            part_start += psize;
            size_left -= psize;
        }
        ke_vp8_init(h.parts[last], p, part_start, end);
        if (part_start >= end) return;
    }
    // quantisers (9.6)
    const int base_q = (int)ke_vp8_value(br, p, 7);
    int dq[5];
    for (int k = 0; k < 5; ++k) dq[k] = ke_vp8_value(br, p, 1) ? ke_vp8_signed_value(br, p, 4) : 0;   // y1dc y2dc y2ac uvdc uvac
    auto clip = [](int v, int m) { return v < 0 ? 0 : v > m ? m : v; };
    for (int s = 0; s < 4; ++s) {
        int q = base_q;
        if (use_segment) {
            q = quant[s];
            if (!absolute) q += base_q;
        }
        int16_t *m = h.dq[s];
        m[0] = kVp8DcTable[clip(q + dq[0], 127)];
        m[1] = (int16_t)kVp8AcTable[clip(q, 127)];
        m[2] = (int16_t)(kVp8DcTable[clip(q + dq[1], 127)] * 2);
        int y2ac = (kVp8AcTable[clip(q + dq[2], 127)] * 101581) >> 16;
        m[3] = (int16_t)(y2ac < 8 ? 8 : y2ac);
        m[4] = kVp8DcTable[clip(q + dq[3], 117)];
        m[5] = (int16_t)kVp8AcTable[clip(q + dq[4], 127)];
    }
    // filter strengths per segment and B_PRED (libwebp's PrecomputeFilterStrengths)
    for (int s = 0; s < 4; ++s) {
        int base_level = level;
        if (use_segment) {
            base_level = fstr[s];
            if (!absolute) base_level += level;
        }
        for (int i4 = 0; i4 <= 1; ++i4) {
            int lv = base_level;
            if (use_lf_delta) {
                lv += ref_lf[0];
                if (i4) lv += mode_lf[0];
            }
            lv = lv < 0 ? 0 : lv > 63 ? 63 : lv;
            if (lv > 0) {
                int il = lv;
                if (sharp > 0) {
                    il >>= sharp > 4 ? 2 : 1;
                    if (il > 9 - sharp) il = 9 - sharp;
                }
                if (il < 1) il = 1;
                h.f_ilevel[s][i4] = (uint8_t)il;
                h.f_limit[s][i4] = (uint8_t)(2 * lv + il);
                h.f_hev[s][i4] = (uint8_t)(lv >= 40 ? 2 : lv >= 15 ? 1 : 0);
            }
        }
    }
    ke_vp8_value(br, p, 1);                                          // refresh_entropy_probs: one frame, no use
    // coefficient probabilities (13.4)
    for (int t = 0; t < 4; ++t)
        for (int b = 0; b < 8; ++b)
            for (int c = 0; c < 3; ++c)
                for (int k = 0; k < 11; ++k)
                    h.probas[t][b][c][k] = ke_vp8_bit(br, p, kVp8CoeffsUpdateProba[t][b][c][k]) ? (uint8_t)ke_vp8_value(br, p, 8)
                                                                                               : kVp8CoeffsProba0[t][b][c][k];
    h.use_skip = (int)ke_vp8_value(br, p, 1);
    if (h.use_skip) h.skip_p = (int)ke_vp8_value(br, p, 8);
    if (br.eof) return;
    h.p0 = br;
    h.status = KE_WEBP_OK;
}

// The whole record: container, frame header (section 9) and the token partitions.
static inline void ke_parse_webp(const uint8_t *p, size_t size, KeWebpHeader &h) {
    ke_webp_frame_tag(p, size, h);
    ke_webp_frame_header(p, h);
}

// The CPU decode the tests hold against Pillow: the same steps as the kernels, one after the other.  scratch: at least
// ke_webp_scratch_bytes(h) bytes, 16-aligned; rgb: width * height * 3 bytes -- or, with stride 4, the first three of every
// pixel's four bytes (ke_webpa_parse.h fills in the fourth).  Returns the status.
static inline size_t ke_webp_scratch_bytes(const KeWebpHeader &h) { return (size_t)h.mb_w * h.mb_h * (sizeof(KeWebpMb) + 768 + 384) + 64; }

static inline int ke_webp_decode_cpu(const uint8_t *file, const KeWebpHeader &h, uint8_t *scratch, uint8_t *rgb, uint8_t *yuv_out = nullptr,
                                     int stride = 3) {
    if (h.status != KE_WEBP_OK) return h.status;
    const size_t nmb = (size_t)h.mb_w * h.mb_h;
    int16_t *coeffs = (int16_t *)scratch;
    uint8_t *planes = scratch + nmb * 768;
    KeWebpMb *mbs = (KeWebpMb *)(planes + nmb * 384);
    const int st = ke_webp_tokens(h, file, mbs, coeffs, planes);     // (the planes serve as the columns' contexts first)
    if (st != KE_WEBP_OK) return st;
    uint8_t *Y = planes, *U = planes + nmb * 256, *V = U + nmb * 64;
    for (int y = 0; y < h.mb_h; ++y)
        for (int x = 0; x < h.mb_w; ++x) ke_webp_recon_mb(mbs[y * h.mb_w + x], coeffs + (size_t)(y * h.mb_w + x) * 384, Y, U, V, h.mb_w, x, y);
    for (int y = 0; y < h.mb_h; ++y)
        for (int x = 0; x < h.mb_w; ++x) ke_webp_filter_mb(h, mbs[y * h.mb_w + x], Y, U, V, x, y);
    if (yuv_out) std::memcpy(yuv_out, planes, nmb * 384);
    for (int y = 0; y < h.height; ++y)
        for (int x = 0; x < h.width; ++x) ke_webp_rgb_at(Y, U, V, h.mb_w, h.width, h.height, x, y, rgb + ((size_t)y * h.width + x) * stride);
    return KE_WEBP_OK;
}
