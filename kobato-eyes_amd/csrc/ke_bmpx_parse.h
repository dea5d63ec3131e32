// ke_bmpx_parse.h -- host-side header parsing for the decoder of the BMP files ke_bmp_parse.h leaves out (ke_bmpx.hip) and the CPU
// build the tests hold against Pillow (tests/_bmpx_cpu.cpp).  Replaces `Image.open(path)` + pixel access of the reference's
// batch hasher (src/core/fastsig.py:31-34) for
//   RLE8 (compression 1 with 8 bits) and RLE4 (compression 2 with 4 bits), which Pillow reads with BmpRleDecoder, a Python loop;
//   uncompressed 1-bit and 4-bit palette files (raw modes P;1 and P;4);
//   16-bit files: compression 0 (BGR;15) and BITFIELDS with the masks of 555 (BGR;15) or 565 (BGR;16)
// -- palette files as the luma `convert("L")` makes of them (ke_parse_bmp's table), 16-bit files as RGB.  The header is read by
// ke_read_bmp_header, the reader ke_parse_bmp uses: the same header sizes, limits and defaults.  Left to Pillow (UNSUPPORTED)
// although it opens them: RLE8 with 4 bits and RLE4 with 8 (the plugin looks at the compression only); an uncompressed 1- or
// 4-bit file whose palette passes Pillow's grayscale test in any way but "two colours, black then white, at 1 bit" -- Pillow
// then reads the packed bytes as 8-bit samples (mode L) or 4-bit data as 1-bit (mode 1); an RLE file with that two-colour
// palette (mode 1 meets a P raw mode); more than 256 colours; a palette that leaves the file; an RLE file of more than 2 GiB.
// Everything ke_parse_bmp takes is UNSUPPORTED here.  CORRUPT: no BMP signature; uncompressed rows that leave the file ("image file is truncated" -- the padding
// behind the last stored row may be missing, as for Pillow; ke_parse_bmp is stricter there and stays so); an RLE
// stream that starts beyond the file -- and, known only after the walk (ke_bmpx_core.h), one that yields too few pixels.
#pragma once

#include "ke_bmp_parse.h"
#include "ke_bmpx_core.h"

enum : uint64_t { KE_BMPX_MAX_RLE_FILE = 1ull << 31 };      // bytes of an RLE file: far from where 32-bit positions + a window wrap

struct KeBmpxInfo {
    int32_t status;
    int32_t width, height, channels;     // channels of the pixels that leave: 1 (luma of a palette file) or 3 (RGB of a 16-bit file)
    int32_t kind;                        // KE_BMPX_RLE8 ... KE_BMPX_RGB565
    int32_t topdown;
    uint32_t data_off, stride;           // pixel data from the start of the file; bytes per stored row (0 for RLE)
    uint8_t lut[256];                    // palette index -> luma
};

static inline void ke_parse_bmpx(const uint8_t *p, size_t size, KeBmpxInfo &info) {
    std::memset(&info, 0, sizeof info);
    KeBmpHeader h;
    info.status = ke_read_bmp_header(p, size, h);
    if (info.status != KE_BMP_OK) return;
    info.status = KE_BMPX_UNSUPPORTED;
    int kind = 0;
    if (h.comp == 1 && h.bits == 8) kind = KE_BMPX_RLE8;
    else if (h.comp == 2 && h.bits == 4) kind = KE_BMPX_RLE4;
    else if (h.comp == 0 && h.bits == 1) kind = KE_BMPX_P1;
    else if (h.comp == 0 && h.bits == 4) kind = KE_BMPX_P4;
    else if (h.comp == 0 && h.bits == 16) kind = KE_BMPX_RGB555;
    else if (h.comp == 3 && h.bits == 16) {
        if (h.mask[0] == 0x7C00u && h.mask[1] == 0x3E0u && h.mask[2] == 0x1Fu) kind = KE_BMPX_RGB555;
        else if (h.mask[0] == 0xF800u && h.mask[1] == 0x7E0u && h.mask[2] == 0x1Fu) kind = KE_BMPX_RGB565;
    }
    if (!kind) return;
    const bool rle = kind == KE_BMPX_RLE8 || kind == KE_BMPX_RLE4;
    size_t pos = h.pos;
    if (h.bits <= 8) {
        // ke_parse_bmp's palette reading, with the two-colour case: Pillow holds two colours against (0, 255), any other count
        // against 0, 1, 2, ...
        if (h.colors == 0 || h.colors > 256 || pos + 4 * (size_t)h.colors > size) return;
        bool gray = true;
        for (uint64_t k = 0; k < h.colors; ++k) {
            const uint8_t *e = p + pos + 4 * (size_t)k;
            info.lut[k] = (uint8_t)((e[2] * 19595u + e[1] * 38470u + e[0] * 7471u + 0x8000u) >> 16);
            const uint8_t want = h.colors == 2 ? (uint8_t)(255 * k) : (uint8_t)k;
            gray = gray && e[0] == want && e[1] == want && e[2] == want;
        }
        if (gray) {
            if (h.colors == 2) {
                if (kind != KE_BMPX_P1) return;                                 // mode "1": 0 / 255, which the table gives already
            } else {
                if (!rle) return;                                               // mode "L" over packed bytes
                for (int k = 0; k < 256; ++k) info.lut[k] = (uint8_t)k;         // mode "L": the indices are the samples
            }
        }
        pos += 4 * (size_t)h.colors;
    }
    uint64_t offset = h.offset;
    if (offset == 0) offset = pos;                                              // Pillow: `offset or self.fp.tell()`
    if (offset > 0xFFFFFFFFull) return;
    info.width = (int32_t)h.width;
    info.height = (int32_t)h.height;
    info.channels = h.bits == 16 ? 3 : 1;
    info.kind = kind;
    info.topdown = h.flip ? 1 : 0;
    info.stride = rle ? 0 : (uint32_t)((((uint64_t)h.width * h.bits + 31) >> 3) & ~3ull);
    if (rle && size > KE_BMPX_MAX_RLE_FILE) return;                            // the walk and its reader count the stream's bytes in 32 bits
    // the raw decoder wants every stored row whole but the last, of which it wants the pixels' bytes, not the padding
    const uint64_t rows_need = (uint64_t)info.stride * (h.height - 1) + ((h.width * h.bits + 7) >> 3);
    if (rle ? offset >= size : offset > size || rows_need > size - offset) {
        info.status = KE_BMPX_CORRUPT;                                          // (RLE: no stream at all)
        return;
    }
    info.data_off = (uint32_t)offset;
    info.status = KE_BMPX_OK;
}
