// ke_webpa_core.h -- the alpha plane of a lossy WebP file (the ALPH chunk beside one VP8 key frame): header byte and inverse
// filters, shared by the HIP kernels (ke_webpa.hip), the host parser (ke_webpa_parse.h) and the CPU build the tests hold against
// Pillow (tests/_webpa_cpu.cpp).  Plain C++ without allocation; KE_HD marks what the device compiles too.
//
// What is restated here is the published container specification's ALPH chunk as libwebp decodes it for Pillow's
// `Image.open(path)` -- the decode step of the reference's batch hasher (src/core/fastsig.py:31-34) and of safe_load_image
// (src/utils/image_io.py:60-138):
//   header byte   : bits 0-1 method (0: the plane's bytes as they are, 1: a VP8L stream without its 5-byte header whose green
//                   channel is the plane -- ke_vp8l_decode_body), bits 2-3 filter, bits 4-5 pre-processing (0, or 1: the
//                   encoder quantised the levels; nothing to undo, Pillow does not dither), bits 6-7 reserved;
//   filters       : value = (stored + predictor) & 255; the predictor is 0 at (0, 0), the left pixel in the rest of row 0, the
//                   pixel above in the rest of column 0, elsewhere none / left (horizontal) / above (vertical) /
//                   clip(left + above - above-left, 0, 255) (gradient).
// The frame beside the plane is ke_webp_core.h's, the stream of a method-1 plane ke_webpl_core.h's.
#pragma once

#include <stdint.h>

#include "ke_webp_core.h"
#include "ke_webpl_core.h"

enum { KE_WEBPA_OK = 0, KE_WEBPA_UNSUPPORTED = 1, KE_WEBPA_CORRUPT = 2 };
enum { KE_ALPH_OPAQUE = -1, KE_ALPH_RAW = 0, KE_ALPH_VP8L = 1 };       // OPAQUE: the VP8X alpha flag without an ALPH chunk
enum { KE_ALPH_FILTER_NONE = 0, KE_ALPH_FILTER_HORIZONTAL = 1, KE_ALPH_FILTER_VERTICAL = 2, KE_ALPH_FILTER_GRADIENT = 3 };

struct KeAlphHeader {
    int32_t method, filter, pre;
};

// The header byte: libwebp's ALPHInit, as Pillow drives it, fails a method above 1, a pre-processing above 1 and a set reserved bit.
KE_HD int ke_alph_header(uint8_t byte, KeAlphHeader &a) {
    a.method = byte & 3;
    a.filter = (byte >> 2) & 3;
    a.pre = (byte >> 4) & 3;
    if (a.method > KE_ALPH_VP8L || a.pre > 1 || (byte >> 6) != 0) return KE_WEBPA_CORRUPT;
    return KE_WEBPA_OK;
}

KE_HD uint32_t ke_alph_gradient(uint32_t left, uint32_t above, uint32_t above_left) {
    const int g = (int)left + (int)above - (int)above_left;
    return g < 0 ? 0u : g > 255 ? 255u : (uint32_t)g;
}

// The predictor of pixel (x, y) from its finished neighbours (those outside the plane are never looked at).
KE_HD uint32_t ke_alph_predict(int filter, int x, int y, uint32_t left, uint32_t above, uint32_t above_left) {
    if (y == 0) return x == 0 ? 0u : left;
    if (x == 0) return above;
    return filter == KE_ALPH_FILTER_HORIZONTAL ? left : filter == KE_ALPH_FILTER_VERTICAL ? above : ke_alph_gradient(left, above, above_left);
}

// The whole plane in raster order, one pixel after the other: what the kernels' scans and wavefront have to equal.
// in(j) yields the stored value of pixel j; out: the plane's bytes, `stride` apart.
template <typename In>
KE_HD void ke_alph_unfilter(int filter, In in, uint8_t *out, size_t stride, int W, int H) {
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t j = (size_t)y * W + x;
            uint32_t v = in(j);
            if (filter != KE_ALPH_FILTER_NONE) {
                const uint32_t l = x ? out[(j - 1) * stride] : 0u, t = y ? out[(j - W) * stride] : 0u, tl = x && y ? out[(j - W - 1) * stride] : 0u;
                v = (v + ke_alph_predict(filter, x, y, l, t, tl)) & 255u;
            }
            out[j * stride] = (uint8_t)v;
        }
}
