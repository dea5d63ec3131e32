// ke_webp_core.h -- lossy WebP (one VP8 key frame) decoding arithmetic shared by the HIP kernels (ke_webp.hip), the host parser
// (ke_webp_parse.h) and the CPU build the tests hold against Pillow (tests/_webp_cpu.cpp).  Plain C++ without allocation; KE_HD
// marks what the device compiles too.
//
// What is restated here is libwebp's decoder as Pillow drives it for `Image.open(path)` (WebPAnimDecoder, RGBA, default
// options) -- the decode step of the reference's batch hasher (src/core/fastsig.py:31-34) and of safe_load_image
// (src/utils/image_io.py:60-138):
//   boolean decoder    : RFC 6386 section 7 in libwebp's form (range - 1 kept, bits counted down); reading past the end of a
//                        partition yields one zero byte and marks the reader, and a marked reader fails the decode
//                        ("Premature end-of-file") -- KE_WEBP_CORRUPT here;
//   frame header       : section 9 (segments, filter, quantisers, partitions, probability updates);
//   modes and tokens   : sections 11 and 13, with the above / left non-zero contexts; dequantised coefficients are stored
//                        as libwebp stores them (int16), the Y2 block undone by the inverse WHT right away (section 14.3);
//   reconstruction     : section 14.4's IDCT, section 12's predictors with a key frame's edges (127 above, 129 left,
//                        above-right of the sub-blocks from the macroblock row above); prediction reads unfiltered pixels;
//   loop filter        : section 15, normal and simple, in macroblock raster order, inner edges skipped for macroblocks
//                        that are not B_PRED and have no non-zero coefficients (libwebp's reading of "no coefficients");
//   output             : libwebp's "fancy" 9-3-3-1 chroma upsampling and its 14-bit fixed-point VP8YUVToR/G/B.
// Blocks with a coefficient outside [-2048, 2048] after dequantisation are refused (KE_WEBP_UNSUPPORTED): no encoder writes
// them, and libwebp's C and SIMD transforms part ways there.
#pragma once

#include <stdint.h>

#ifndef KE_HD
#ifdef __HIPCC__
#define KE_HD __host__ __device__ __forceinline__
#define KE_HD_STATIC static __host__ __device__ __forceinline__
#else
#define KE_HD static inline
#define KE_HD_STATIC static inline
#endif
#endif

enum { KE_WEBP_OK = 0, KE_WEBP_UNSUPPORTED = 1, KE_WEBP_CORRUPT = 2 };

// The pixel cap: frames of more than this many 16x16 macroblocks (16.7 Mpx, e.g. 4096 x 4096) are left to Pillow.  The decoder's
// scratch is about 1.2 KB per macroblock (mode record, coefficients, unfiltered planes).
constexpr int kWebpMaxMbs = 65536;

enum { KE_B_DC = 0, KE_B_TM, KE_B_VE, KE_B_HE, KE_B_RD, KE_B_VR, KE_B_LD, KE_B_VL, KE_B_HD, KE_B_HU };

constexpr uint8_t kVp8Zigzag[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
constexpr uint8_t kVp8Bands[17] = {0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7, 0};   // the 17th: after the last coefficient
constexpr uint8_t kVp8Cat[4][12] = {{173, 148, 140, 0}, {176, 155, 140, 135, 0}, {180, 157, 141, 134, 130, 0},
                                    {254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129, 0}};
// sub-block mode tree (section 11.2) as libwebp walks it: a positive entry is the next node, -entry a leaf (the mode)
constexpr int8_t kVp8YModesIntra4[18] = {-KE_B_DC, 1, -KE_B_TM, 2, -KE_B_VE, 3, 4, 6, -KE_B_HE, 5, -KE_B_RD, -KE_B_VR, -KE_B_LD, 7,
                                         -KE_B_VL, 8, -KE_B_HD, -KE_B_HU};

// ---- boolean decoder (section 7) -----------------------------------------------------------------------------------------
struct KeVp8Bool {
    uint32_t pos, end;       // next byte, end of the partition (offsets into the file)
    uint32_t value;          // the bits not consumed yet: `bits + 8` of them
    int32_t bits;            // number of valid bits beyond 8; < 0: a byte is due
    uint32_t range;          // range - 1, in [127, 254]
    int32_t eof;             // read past the end (sticky)
};

KE_HD void ke_vp8_load(KeVp8Bool &b, const uint8_t *p) {
    if (b.pos < b.end) {
        b.bits += 8;
        b.value = (b.value << 8) | p[b.pos++];
    } else if (!b.eof) {                           // one zero byte past the end, then the decode fails
        b.value <<= 8;
        b.bits += 8;
        b.eof = 1;
    } else {
        b.bits = 0;
    }
}

KE_HD void ke_vp8_init(KeVp8Bool &b, const uint8_t *p, uint32_t pos, uint32_t end) {
    b.pos = pos; b.end = end; b.value = 0; b.bits = -8; b.range = 254; b.eof = 0;
    ke_vp8_load(b, p);
}

KE_HD int ke_vp8_bit(KeVp8Bool &b, const uint8_t *p, int prob) {
    uint32_t range = b.range;
    if (b.bits < 0) ke_vp8_load(b, p);
    const int pos = b.bits;
    const uint32_t split = (range * (uint32_t)prob) >> 8;
    const uint32_t value = b.value >> pos;
    const int bit = value > split;
    if (bit) {
        range -= split;
        b.value -= (split + 1) << pos;
    } else {
        range = split + 1;
    }
    const int shift = 7 ^ (31 - __builtin_clz(range));
    range <<= shift;
    b.bits -= shift;
    b.range = range - 1;
    return bit;
}

KE_HD uint32_t ke_vp8_value(KeVp8Bool &b, const uint8_t *p, int nbits) {
    uint32_t v = 0;
    while (nbits-- > 0) v |= (uint32_t)ke_vp8_bit(b, p, 0x80) << nbits;
    return v;
}

KE_HD int ke_vp8_signed_value(KeVp8Bool &b, const uint8_t *p, int nbits) {
    const int v = (int)ke_vp8_value(b, p, nbits);
    return ke_vp8_bit(b, p, 0x80) ? -v : v;
}

// ---- the per-image record the frame header becomes (ke_webp_parse.h fills it on the host) ---------------------------------
struct KeWebpHeader {
    int32_t status;
    int32_t width, height, mb_w, mb_h;
    int32_t meta;                      // the file carries an EXIF or XMP chunk (either can hold an orientation)
    uint32_t vp8_off, vp8_size;        // payload of the "VP8 " chunk inside the file
    KeVp8Bool p0;                      // partition 0 where the frame header ends (the modes follow)
    KeVp8Bool parts[8];                // the token partitions
    int32_t num_parts;
    int32_t update_map, use_skip, skip_p;
    uint8_t seg_probs[4];
    int16_t dq[4][6];                  // per segment: Y1 DC, Y1 AC, Y2 DC, Y2 AC, UV DC, UV AC
    int32_t filter_type;               // 0 off, 1 simple, 2 normal
    uint8_t f_limit[4][2], f_ilevel[4][2], f_hev[4][2];   // [segment][B_PRED]; limit 0: no filtering
    uint8_t probas[4][8][3][11];       // [type][band][context][node]
};

// One macroblock's modes as the token pass leaves them for reconstruction and the loop filter.
struct KeWebpMb {
    uint8_t imodes[16];                // B_PRED: the 16 sub-block modes; otherwise imodes[0] = the 16x16 mode
    uint8_t is_i4, uvmode, segment, inner;
};

// Spec data of RFC 6386 (the default coefficient probabilities of 13.5, their update probabilities of 13.4, the contextual
// sub-block mode probabilities of 11.5, the quantiser steps of 14.1), with the modes numbered as libwebp numbers them:
// B_DC, B_TM, B_VE, B_HE, B_RD, B_VR, B_LD, B_VL, B_HD, B_HU (the 16x16 / chroma DC, TM, V, H share the first four numbers).
constexpr uint8_t kVp8CoeffsProba0[4][8][3][11] = {
    {
        {
            {128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128},
            {128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128},
            {128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128}},
        {
            {253, 136, 254, 255, 228, 219, 128, 128, 128, 128, 128},
            {189, 129, 242, 255, 227, 213, 255, 219, 128, 128, 128},
            {106, 126, 227, 252, 214, 209, 255, 255, 128, 128, 128}},
        {
            {1, 98, 248, 255, 236, 226, 255, 255, 128, 128, 128},
            {181, 133, 238, 254, 221, 234, 255, 154, 128, 128, 128},
            {78, 134, 202, 247, 198, 180, 255, 219, 128, 128, 128}},
        {
            {1, 185, 249, 255, 243, 255, 128, 128, 128, 128, 128},
            {184, 150, 247, 255, 236, 224, 128, 128, 128, 128, 128},
            {77, 110, 216, 255, 236, 230, 128, 128, 128, 128, 128}},
        {
            {1, 101, 251, 255, 241, 255, 128, 128, 128, 128, 128},
            {170, 139, 241, 252, 236, 209, 255, 255, 128, 128, 128},
            {37, 116, 196, 243, 228, 255, 255, 255, 128, 128, 128}},
        {
            {1, 204, 254, 255, 245, 255, 128, 128, 128, 128, 128},
            {207, 160, 250, 255, 238, 128, 128, 128, 128, 128, 128},
            {102, 103, 231, 255, 211, 171, 128, 128, 128, 128, 128}},
        {
            {1, 152, 252, 255, 240, 255, 128, 128, 128, 128, 128},
            {177, 135, 243, 255, 234, 225, 128, 128, 128, 128, 128},
            {80, 129, 211, 255, 194, 224, 128, 128, 128, 128, 128}},
        {
            {1, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128},
            {246, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128},
            {255, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128}}},
    {
        {
            {198, 35, 237, 223, 193, 187, 162, 160, 145, 155, 62},
            {131, 45, 198, 221, 172, 176, 220, 157, 252, 221, 1},
            {68, 47, 146, 208, 149, 167, 221, 162, 255, 223, 128}},
        {
            {1, 149, 241, 255, 221, 224, 255, 255, 128, 128, 128},
            {184, 141, 234, 253, 222, 220, 255, 199, 128, 128, 128},
            {81, 99, 181, 242, 176, 190, 249, 202, 255, 255, 128}},
        {
            {1, 129, 232, 253, 214, 197, 242, 196, 255, 255, 128},
            {99, 121, 210, 250, 201, 198, 255, 202, 128, 128, 128},
            {23, 91, 163, 242, 170, 187, 247, 210, 255, 255, 128}},
        {
            {1, 200, 246, 255, 234, 255, 128, 128, 128, 128, 128},
            {109, 178, 241, 255, 231, 245, 255, 255, 128, 128, 128},
            {44, 130, 201, 253, 205, 192, 255, 255, 128, 128, 128}},
        {
            {1, 132, 239, 251, 219, 209, 255, 165, 128, 128, 128},
            {94, 136, 225, 251, 218, 190, 255, 255, 128, 128, 128},
            {22, 100, 174, 245, 186, 161, 255, 199, 128, 128, 128}},
        {
            {1, 182, 249, 255, 232, 235, 128, 128, 128, 128, 128},
            {124, 143, 241, 255, 227, 234, 128, 128, 128, 128, 128},
            {35, 77, 181, 251, 193, 211, 255, 205, 128, 128, 128}},
        {
            {1, 157, 247, 255, 236, 231, 255, 255, 128, 128, 128},
            {121, 141, 235, 255, 225, 227, 255, 255, 128, 128, 128},
            {45, 99, 188, 251, 195, 217, 255, 224, 128, 128, 128}},
        {
            {1, 1, 251, 255, 213, 255, 128, 128, 128, 128, 128},
            {203, 1, 248, 255, 255, 128, 128, 128, 128, 128, 128},
            {137, 1, 177, 255, 224, 255, 128, 128, 128, 128, 128}}},
    {
        {
            {253, 9, 248, 251, 207, 208, 255, 192, 128, 128, 128},
            {175, 13, 224, 243, 193, 185, 249, 198, 255, 255, 128},
            {73, 17, 171, 221, 161, 179, 236, 167, 255, 234, 128}},
        {
            {1, 95, 247, 253, 212, 183, 255, 255, 128, 128, 128},
            {239, 90, 244, 250, 211, 209, 255, 255, 128, 128, 128},
            {155, 77, 195, 248, 188, 195, 255, 255, 128, 128, 128}},
        {
            {1, 24, 239, 251, 218, 219, 255, 205, 128, 128, 128},
            {201, 51, 219, 255, 196, 186, 128, 128, 128, 128, 128},
            {69, 46, 190, 239, 201, 218, 255, 228, 128, 128, 128}},
        {
            {1, 191, 251, 255, 255, 128, 128, 128, 128, 128, 128},
            {223, 165, 249, 255, 213, 255, 128, 128, 128, 128, 128},
            {141, 124, 248, 255, 255, 128, 128, 128, 128, 128, 128}},
        {
            {1, 16, 248, 255, 255, 128, 128, 128, 128, 128, 128},
            {190, 36, 230, 255, 236, 255, 128, 128, 128, 128, 128},
            {149, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128}},
        {
            {1, 226, 255, 128, 128, 128, 128, 128, 128, 128, 128},
            {247, 192, 255, 128, 128, 128, 128, 128, 128, 128, 128},
            {240, 128, 255, 128, 128, 128, 128, 128, 128, 128, 128}},
        {
            {1, 134, 252, 255, 255, 128, 128, 128, 128, 128, 128},
            {213, 62, 250, 255, 255, 128, 128, 128, 128, 128, 128},
            {55, 93, 255, 128, 128, 128, 128, 128, 128, 128, 128}},
        {
            {128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128},
            {128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128},
            {128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128}}},
    {
        {
            {202, 24, 213, 235, 186, 191, 220, 160, 240, 175, 255},
            {126, 38, 182, 232, 169, 184, 228, 174, 255, 187, 128},
            {61, 46, 138, 219, 151, 178, 240, 170, 255, 216, 128}},
        {
            {1, 112, 230, 250, 199, 191, 247, 159, 255, 255, 128},
            {166, 109, 228, 252, 211, 215, 255, 174, 128, 128, 128},
            {39, 77, 162, 232, 172, 180, 245, 178, 255, 255, 128}},
        {
            {1, 52, 220, 246, 198, 199, 249, 220, 255, 255, 128},
            {124, 74, 191, 243, 183, 193, 250, 221, 255, 255, 128},
            {24, 71, 130, 219, 154, 170, 243, 182, 255, 255, 128}},
        {
            {1, 182, 225, 249, 219, 240, 255, 224, 128, 128, 128},
            {149, 150, 226, 252, 216, 205, 255, 171, 128, 128, 128},
            {28, 108, 170, 242, 183, 194, 254, 223, 255, 255, 128}},
        {
            {1, 81, 230, 252, 204, 203, 255, 192, 128, 128, 128},
            {123, 102, 209, 247, 188, 196, 255, 233, 128, 128, 128},
            {20, 95, 153, 243, 164, 173, 255, 203, 128, 128, 128}},
        {
            {1, 222, 248, 255, 216, 213, 128, 128, 128, 128, 128},
            {168, 175, 246, 252, 235, 205, 255, 255, 128, 128, 128},
            {47, 116, 215, 255, 211, 212, 255, 255, 128, 128, 128}},
        {
            {1, 121, 236, 253, 212, 214, 255, 255, 128, 128, 128},
            {141, 84, 213, 252, 201, 202, 255, 219, 128, 128, 128},
            {42, 80, 160, 240, 162, 185, 255, 205, 128, 128, 128}},
        {
            {1, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128},
            {244, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128},
            {238, 1, 255, 128, 128, 128, 128, 128, 128, 128, 128}}}};
constexpr uint8_t kVp8CoeffsUpdateProba[4][8][3][11] = {
    {
        {
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {176, 246, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {223, 241, 252, 255, 255, 255, 255, 255, 255, 255, 255},
            {249, 253, 253, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 244, 252, 255, 255, 255, 255, 255, 255, 255, 255},
            {234, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {253, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 246, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {239, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {254, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 248, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {251, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {251, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {254, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 254, 253, 255, 254, 255, 255, 255, 255, 255, 255},
            {250, 255, 254, 255, 254, 255, 255, 255, 255, 255, 255},
            {254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}}},
    {
        {
            {217, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {225, 252, 241, 253, 255, 255, 254, 255, 255, 255, 255},
            {234, 250, 241, 250, 253, 255, 253, 254, 255, 255, 255}},
        {
            {255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {223, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {238, 253, 254, 254, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 248, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {249, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 253, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {247, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {252, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {253, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 254, 253, 255, 255, 255, 255, 255, 255, 255, 255},
            {250, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}}},
    {
        {
            {186, 251, 250, 255, 255, 255, 255, 255, 255, 255, 255},
            {234, 251, 244, 254, 255, 255, 255, 255, 255, 255, 255},
            {251, 251, 243, 253, 254, 255, 254, 255, 255, 255, 255}},
        {
            {255, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {236, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {251, 253, 253, 254, 254, 255, 255, 255, 255, 255, 255}},
        {
            {255, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {254, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}}},
    {
        {
            {248, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {250, 254, 252, 254, 255, 255, 255, 255, 255, 255, 255},
            {248, 254, 249, 253, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 253, 253, 255, 255, 255, 255, 255, 255, 255, 255},
            {246, 253, 253, 255, 255, 255, 255, 255, 255, 255, 255},
            {252, 254, 251, 254, 254, 255, 255, 255, 255, 255, 255}},
        {
            {255, 254, 252, 255, 255, 255, 255, 255, 255, 255, 255},
            {248, 254, 253, 255, 255, 255, 255, 255, 255, 255, 255},
            {253, 255, 254, 254, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 251, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {245, 251, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {253, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 251, 253, 255, 255, 255, 255, 255, 255, 255, 255},
            {252, 253, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 252, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {249, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 254, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 255, 253, 255, 255, 255, 255, 255, 255, 255, 255},
            {250, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}},
        {
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255},
            {255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255}}}};
constexpr uint8_t kVp8BModesProba[10][10][9] = {
    {
        {231, 120, 48, 89, 115, 113, 120, 152, 112},
        {152, 179, 64, 126, 170, 118, 46, 70, 95},
        {175, 69, 143, 80, 85, 82, 72, 155, 103},
        {56, 58, 10, 171, 218, 189, 17, 13, 152},
        {114, 26, 17, 163, 44, 195, 21, 10, 173},
        {121, 24, 80, 195, 26, 62, 44, 64, 85},
        {144, 71, 10, 38, 171, 213, 144, 34, 26},
        {170, 46, 55, 19, 136, 160, 33, 206, 71},
        {63, 20, 8, 114, 114, 208, 12, 9, 226},
        {81, 40, 11, 96, 182, 84, 29, 16, 36}},
    {
        {134, 183, 89, 137, 98, 101, 106, 165, 148},
        {72, 187, 100, 130, 157, 111, 32, 75, 80},
        {66, 102, 167, 99, 74, 62, 40, 234, 128},
        {41, 53, 9, 178, 241, 141, 26, 8, 107},
        {74, 43, 26, 146, 73, 166, 49, 23, 157},
        {65, 38, 105, 160, 51, 52, 31, 115, 128},
        {104, 79, 12, 27, 217, 255, 87, 17, 7},
        {87, 68, 71, 44, 114, 51, 15, 186, 23},
        {47, 41, 14, 110, 182, 183, 21, 17, 194},
        {66, 45, 25, 102, 197, 189, 23, 18, 22}},
    {
        {88, 88, 147, 150, 42, 46, 45, 196, 205},
        {43, 97, 183, 117, 85, 38, 35, 179, 61},
        {39, 53, 200, 87, 26, 21, 43, 232, 171},
        {56, 34, 51, 104, 114, 102, 29, 93, 77},
        {39, 28, 85, 171, 58, 165, 90, 98, 64},
        {34, 22, 116, 206, 23, 34, 43, 166, 73},
        {107, 54, 32, 26, 51, 1, 81, 43, 31},
        {68, 25, 106, 22, 64, 171, 36, 225, 114},
        {34, 19, 21, 102, 132, 188, 16, 76, 124},
        {62, 18, 78, 95, 85, 57, 50, 48, 51}},
    {
        {193, 101, 35, 159, 215, 111, 89, 46, 111},
        {60, 148, 31, 172, 219, 228, 21, 18, 111},
        {112, 113, 77, 85, 179, 255, 38, 120, 114},
        {40, 42, 1, 196, 245, 209, 10, 25, 109},
        {88, 43, 29, 140, 166, 213, 37, 43, 154},
        {61, 63, 30, 155, 67, 45, 68, 1, 209},
        {100, 80, 8, 43, 154, 1, 51, 26, 71},
        {142, 78, 78, 16, 255, 128, 34, 197, 171},
        {41, 40, 5, 102, 211, 183, 4, 1, 221},
        {51, 50, 17, 168, 209, 192, 23, 25, 82}},
    {
        {138, 31, 36, 171, 27, 166, 38, 44, 229},
        {67, 87, 58, 169, 82, 115, 26, 59, 179},
        {63, 59, 90, 180, 59, 166, 93, 73, 154},
        {40, 40, 21, 116, 143, 209, 34, 39, 175},
        {47, 15, 16, 183, 34, 223, 49, 45, 183},
        {46, 17, 33, 183, 6, 98, 15, 32, 183},
        {57, 46, 22, 24, 128, 1, 54, 17, 37},
        {65, 32, 73, 115, 28, 128, 23, 128, 205},
        {40, 3, 9, 115, 51, 192, 18, 6, 223},
        {87, 37, 9, 115, 59, 77, 64, 21, 47}},
    {
        {104, 55, 44, 218, 9, 54, 53, 130, 226},
        {64, 90, 70, 205, 40, 41, 23, 26, 57},
        {54, 57, 112, 184, 5, 41, 38, 166, 213},
        {30, 34, 26, 133, 152, 116, 10, 32, 134},
        {39, 19, 53, 221, 26, 114, 32, 73, 255},
        {31, 9, 65, 234, 2, 15, 1, 118, 73},
        {75, 32, 12, 51, 192, 255, 160, 43, 51},
        {88, 31, 35, 67, 102, 85, 55, 186, 85},
        {56, 21, 23, 111, 59, 205, 45, 37, 192},
        {55, 38, 70, 124, 73, 102, 1, 34, 98}},
    {
        {125, 98, 42, 88, 104, 85, 117, 175, 82},
        {95, 84, 53, 89, 128, 100, 113, 101, 45},
        {75, 79, 123, 47, 51, 128, 81, 171, 1},
        {57, 17, 5, 71, 102, 57, 53, 41, 49},
        {38, 33, 13, 121, 57, 73, 26, 1, 85},
        {41, 10, 67, 138, 77, 110, 90, 47, 114},
        {115, 21, 2, 10, 102, 255, 166, 23, 6},
        {101, 29, 16, 10, 85, 128, 101, 196, 26},
        {57, 18, 10, 102, 102, 213, 34, 20, 43},
        {117, 20, 15, 36, 163, 128, 68, 1, 26}},
    {
        {102, 61, 71, 37, 34, 53, 31, 243, 192},
        {69, 60, 71, 38, 73, 119, 28, 222, 37},
        {68, 45, 128, 34, 1, 47, 11, 245, 171},
        {62, 17, 19, 70, 146, 85, 55, 62, 70},
        {37, 43, 37, 154, 100, 163, 85, 160, 1},
        {63, 9, 92, 136, 28, 64, 32, 201, 85},
        {75, 15, 9, 9, 64, 255, 184, 119, 16},
        {86, 6, 28, 5, 64, 255, 25, 248, 1},
        {56, 8, 17, 132, 137, 255, 55, 116, 128},
        {58, 15, 20, 82, 135, 57, 26, 121, 40}},
    {
        {164, 50, 31, 137, 154, 133, 25, 35, 218},
        {51, 103, 44, 131, 131, 123, 31, 6, 158},
        {86, 40, 64, 135, 148, 224, 45, 183, 128},
        {22, 26, 17, 131, 240, 154, 14, 1, 209},
        {45, 16, 21, 91, 64, 222, 7, 1, 197},
        {56, 21, 39, 155, 60, 138, 23, 102, 213},
        {83, 12, 13, 54, 192, 255, 68, 47, 28},
        {85, 26, 85, 85, 128, 128, 32, 146, 171},
        {18, 11, 7, 63, 144, 171, 4, 4, 246},
        {35, 27, 10, 146, 174, 171, 12, 26, 128}},
    {
        {190, 80, 35, 99, 180, 80, 126, 54, 45},
        {85, 126, 47, 87, 176, 51, 41, 20, 32},
        {101, 75, 128, 139, 118, 146, 116, 128, 85},
        {56, 41, 15, 176, 236, 85, 37, 9, 62},
        {71, 30, 17, 119, 118, 255, 17, 18, 138},
        {101, 38, 60, 138, 55, 70, 43, 26, 142},
        {146, 36, 19, 30, 171, 255, 97, 27, 20},
        {138, 45, 61, 62, 219, 1, 81, 188, 64},
        {32, 41, 20, 117, 151, 142, 20, 21, 163},
        {112, 19, 12, 61, 195, 128, 48, 4, 24}}};
constexpr uint8_t kVp8DcTable[128] = {
    4, 5, 6, 7, 8, 9, 10, 10, 11, 12, 13, 14, 15, 16, 17, 17,
    18, 19, 20, 20, 21, 21, 22, 22, 23, 23, 24, 25, 25, 26, 27, 28,
    29, 30, 31, 32, 33, 34, 35, 36, 37, 37, 38, 39, 40, 41, 42, 43,
    44, 45, 46, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58,
    59, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74,
    75, 76, 76, 77, 78, 79, 80, 81, 82, 83, 84, 85, 86, 87, 88, 89,
    91, 93, 95, 96, 98, 100, 101, 102, 104, 106, 108, 110, 112, 114, 116, 118,
    122, 124, 126, 128, 130, 132, 134, 136, 138, 140, 143, 145, 148, 151, 154, 157
};
constexpr uint16_t kVp8AcTable[128] = {
    4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19,
    20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35,
    36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51,
    52, 53, 54, 55, 56, 57, 58, 60, 62, 64, 66, 68, 70, 72, 74, 76,
    78, 80, 82, 84, 86, 88, 90, 92, 94, 96, 98, 100, 102, 104, 106, 108,
    110, 112, 114, 116, 119, 122, 125, 128, 131, 134, 137, 140, 143, 146, 149, 152,
    155, 158, 161, 164, 167, 170, 173, 177, 181, 185, 189, 193, 197, 201, 205, 209,
    213, 217, 221, 225, 229, 234, 239, 245, 249, 254, 259, 264, 269, 274, 279, 284
};

// ---- modes and tokens (sections 11, 13) ----------------------------------------------------------------------------------
KE_HD int ke_vp8_large_value(KeVp8Bool &b, const uint8_t *f, const uint8_t *p) {      // section 13.2: the token tree past "ONE"
    int v;
    if (!ke_vp8_bit(b, f, p[3])) {
        v = ke_vp8_bit(b, f, p[4]) ? 3 + ke_vp8_bit(b, f, p[5]) : 2;
    } else if (!ke_vp8_bit(b, f, p[6])) {
        if (!ke_vp8_bit(b, f, p[7])) {
            v = 5 + ke_vp8_bit(b, f, 159);
        } else {
            v = 7 + 2 * ke_vp8_bit(b, f, 165);
            v += ke_vp8_bit(b, f, 145);
        }
    } else {
        const int bit1 = ke_vp8_bit(b, f, p[8]);
        const int bit0 = ke_vp8_bit(b, f, p[9 + bit1]);
        const int cat = 2 * bit1 + bit0;
        v = 0;
        for (const uint8_t *tab = kVp8Cat[cat]; *tab; ++tab) v += v + ke_vp8_bit(b, f, *tab);
        v += 3 + (8 << cat);
    }
    return v;
}

// The tokens of one 4x4 block from position n on, dequantised into out[] (natural order, int16 as libwebp keeps them).
// Returns libwebp's "position after the last coefficient" (16 when a run of zeros reaches the end).  *maxabs grows to the
// largest magnitude stored.
KE_HD int ke_vp8_coeffs(KeVp8Bool &b, const uint8_t *f, const uint8_t (*bands)[3][11], int ctx, int dc_q, int ac_q, int n,
                        int16_t *out, int &maxabs) {
    const uint8_t *p = bands[kVp8Bands[n]][ctx];
    for (; n < 16; ++n) {
        if (!ke_vp8_bit(b, f, p[0])) return n;               // end of block
        while (!ke_vp8_bit(b, f, p[1])) {                     // a zero
            p = bands[kVp8Bands[++n]][0];
            if (n == 16) return 16;
        }
        const uint8_t (*next)[11] = bands[kVp8Bands[n + 1]];
        int v;
        if (!ke_vp8_bit(b, f, p[2])) {
            v = 1;
            p = next[1];
        } else {
            v = ke_vp8_large_value(b, f, p);
            p = next[2];
        }
        const int s = ke_vp8_bit(b, f, 0x80) ? -v : v;
        const int16_t q = (int16_t)(s * (n > 0 ? ac_q : dc_q));
        const int a = q < 0 ? -(int)q : q;
        maxabs = a > maxabs ? a : maxabs;
        out[kVp8Zigzag[n]] = q;
    }
    return 16;
}

KE_HD void ke_vp8_iwht(const int16_t *in, int16_t *out) {      // section 14.3; out[16 k] = DC of block k
    int tmp[16];
    for (int i = 0; i < 4; ++i) {
        const int a0 = in[0 + i] + in[12 + i], a1 = in[4 + i] + in[8 + i];
        const int a2 = in[4 + i] - in[8 + i], a3 = in[0 + i] - in[12 + i];
        tmp[0 + i] = a0 + a1;
        tmp[8 + i] = a0 - a1;
        tmp[4 + i] = a3 + a2;
        tmp[12 + i] = a3 - a2;
    }
    for (int i = 0; i < 4; ++i) {
        const int dc = tmp[0 + i * 4] + 3;
        const int a0 = dc + tmp[3 + i * 4], a1 = tmp[1 + i * 4] + tmp[2 + i * 4];
        const int a2 = tmp[1 + i * 4] - tmp[2 + i * 4], a3 = dc - tmp[3 + i * 4];
        out[64 * i + 0] = (int16_t)((a0 + a1) >> 3);
        out[64 * i + 16] = (int16_t)((a3 + a2) >> 3);
        out[64 * i + 32] = (int16_t)((a0 - a1) >> 3);
        out[64 * i + 48] = (int16_t)((a3 - a2) >> 3);
    }
}

KE_HD int ke_vp8_nz_code(int nz, int dc_nz) { return nz > 3 ? 3 : nz > 1 ? 2 : dc_nz; }

// Partition 0's modes and the token partitions of the whole frame, one macroblock after the other: mbs[mb_w * mb_h] and
// coeffs[384 per macroblock: 16 Y blocks, 4 U, 4 V, 16 each] are written; top[] is 8 bytes of scratch per macroblock column.
// Returns the image's status.
KE_HD int ke_webp_tokens(const KeWebpHeader &h, const uint8_t *f, KeWebpMb *mbs, int16_t *coeffs, uint8_t *top) {
    KeVp8Bool p0 = h.p0;
    KeVp8Bool parts[8];
    for (int k = 0; k < h.num_parts; ++k) parts[k] = h.parts[k];
    for (int x = 0; x < h.mb_w; ++x)
        for (int k = 0; k < 8; ++k) top[8 * x + k] = 0;      // [0..3] sub-block modes above (B_DC), [4] nz bits, [5] Y2 nz
    int maxabs = 0;
    for (int y = 0; y < h.mb_h; ++y) {
        KeVp8Bool tb = parts[y & (h.num_parts - 1)];
        uint8_t left[4] = {0, 0, 0, 0};
        uint32_t lnz = 0, ldc = 0;
        for (int x = 0; x < h.mb_w; ++x) {
            KeWebpMb m;
            uint8_t *t = top + 8 * x;
            // ---- modes (section 11)
            int seg = 0;
            if (h.update_map) seg = !ke_vp8_bit(p0, f, h.seg_probs[0]) ? ke_vp8_bit(p0, f, h.seg_probs[1]) : ke_vp8_bit(p0, f, h.seg_probs[2]) + 2;
            const int skip = h.use_skip ? ke_vp8_bit(p0, f, h.skip_p) : 0;
            const int is_i4 = !ke_vp8_bit(p0, f, 145);
            for (int k = 0; k < 16; ++k) m.imodes[k] = 0;
            if (!is_i4) {
                const int ymode = ke_vp8_bit(p0, f, 156) ? (ke_vp8_bit(p0, f, 128) ? KE_B_TM : KE_B_HE)
                                                         : (ke_vp8_bit(p0, f, 163) ? KE_B_VE : KE_B_DC);
                m.imodes[0] = (uint8_t)ymode;
                for (int k = 0; k < 4; ++k) t[k] = left[k] = (uint8_t)ymode;
            } else {
                for (int by = 0; by < 4; ++by) {
                    int ymode = left[by];
                    for (int bx = 0; bx < 4; ++bx) {
                        const uint8_t *prob = kVp8BModesProba[t[bx]][ymode];
                        int i = kVp8YModesIntra4[ke_vp8_bit(p0, f, prob[0])];
                        while (i > 0) i = kVp8YModesIntra4[2 * i + ke_vp8_bit(p0, f, prob[i])];
                        ymode = -i;
                        t[bx] = (uint8_t)ymode;
                        m.imodes[4 * by + bx] = (uint8_t)ymode;
                    }
                    left[by] = (uint8_t)ymode;
                }
            }
            m.uvmode = !ke_vp8_bit(p0, f, 142) ? KE_B_DC : !ke_vp8_bit(p0, f, 114) ? KE_B_VE : ke_vp8_bit(p0, f, 183) ? KE_B_TM : KE_B_HE;
            m.is_i4 = (uint8_t)is_i4;
            m.segment = (uint8_t)seg;
            // ---- residuals (section 13)
            int16_t *dst = coeffs + (size_t)(y * h.mb_w + x) * 384;
            for (int k = 0; k < 384; ++k) dst[k] = 0;
            uint32_t tnz = t[4], tdc = t[5];
            int nonzero = 0;
            if (!skip) {
                const int16_t *q = h.dq[seg];
                int first;
                const uint8_t (*ac_bands)[3][11];
                if (!is_i4) {
                    int16_t dc[16];
                    for (int k = 0; k < 16; ++k) dc[k] = 0;
                    int unused = 0;
                    const int nz = ke_vp8_coeffs(tb, f, h.probas[1], (int)(tdc + ldc), q[2], q[3], 0, dc, unused);
                    tdc = ldc = nz > 0;
                    ke_vp8_iwht(dc, dst);
                    for (int k = 0; k < 16; ++k) {
                        const int a = dst[16 * k] < 0 ? -(int)dst[16 * k] : dst[16 * k];
                        maxabs = a > maxabs ? a : maxabs;
                    }
                    first = 1;
                    ac_bands = h.probas[0];
                } else {
                    first = 0;
                    ac_bands = h.probas[3];
                }
                for (int by = 0; by < 4; ++by)
                    for (int bx = 0; bx < 4; ++bx) {
                        int16_t *blk = dst + 16 * (4 * by + bx);
                        const int ctx = (int)((lnz >> by) & 1) + (int)((tnz >> bx) & 1);
                        const int nz = ke_vp8_coeffs(tb, f, ac_bands, ctx, q[0], q[1], first, blk, maxabs);
                        const uint32_t flag = nz > first;
                        tnz = (tnz & ~(1u << bx)) | (flag << bx);
                        lnz = (lnz & ~(1u << by)) | (flag << by);
                        nonzero |= ke_vp8_nz_code(nz, blk[0] != 0);
                    }
                for (int ch = 0; ch < 2; ++ch)
                    for (int by = 0; by < 2; ++by)
                        for (int bx = 0; bx < 2; ++bx) {
                            int16_t *blk = dst + 256 + 64 * ch + 16 * (2 * by + bx);
                            const int tb_ = 4 + 2 * ch + bx, lb = 4 + 2 * ch + by;
                            const int ctx = (int)((lnz >> lb) & 1) + (int)((tnz >> tb_) & 1);
                            const int nz = ke_vp8_coeffs(tb, f, h.probas[2], ctx, q[4], q[5], 0, blk, maxabs);
                            const uint32_t flag = nz > 0;
                            tnz = (tnz & ~(1u << tb_)) | (flag << tb_);
                            lnz = (lnz & ~(1u << lb)) | (flag << lb);
                            nonzero |= ke_vp8_nz_code(nz, blk[0] != 0);
                        }
            } else {
                tnz = lnz = 0;
                if (!is_i4) tdc = ldc = 0;
            }
            t[4] = (uint8_t)tnz;
            t[5] = (uint8_t)tdc;
            m.inner = (uint8_t)(is_i4 || nonzero != 0);
            mbs[y * h.mb_w + x] = m;
            if (tb.eof || p0.eof) return KE_WEBP_CORRUPT;          // "Premature end-of-file": nothing is shown
        }
        parts[y & (h.num_parts - 1)] = tb;
    }
    return maxabs > 2048 ? KE_WEBP_UNSUPPORTED : KE_WEBP_OK;
}

// ---- reconstruction (sections 12, 14) ------------------------------------------------------------------------------------
KE_HD int ke_vp8_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// inverse DCT of one block added to the 4x4 prediction pred[] (row-major), result to dst (stride)
KE_HD void ke_vp8_idct_add(const int16_t *in, const uint8_t *pred, uint8_t *dst, int stride) {
    int C[16];
    for (int i = 0; i < 4; ++i) {
        const int a = in[i] + in[8 + i], b = in[i] - in[8 + i];
        const int c = ((in[4 + i] * 35468) >> 16) - (((in[12 + i] * 20091) >> 16) + in[12 + i]);
        const int d = (((in[4 + i] * 20091) >> 16) + in[4 + i]) + ((in[12 + i] * 35468) >> 16);
        C[4 * i + 0] = a + d;
        C[4 * i + 1] = b + c;
        C[4 * i + 2] = b - c;
        C[4 * i + 3] = a - d;
    }
    for (int i = 0; i < 4; ++i) {
        const int dc = C[i] + 4;
        const int a = dc + C[8 + i], b = dc - C[8 + i];
        const int c = ((C[4 + i] * 35468) >> 16) - (((C[12 + i] * 20091) >> 16) + C[12 + i]);
        const int d = (((C[4 + i] * 20091) >> 16) + C[4 + i]) + ((C[12 + i] * 35468) >> 16);
        dst[i * stride + 0] = (uint8_t)ke_vp8_clip8(pred[4 * i + 0] + ((a + d) >> 3));
        dst[i * stride + 1] = (uint8_t)ke_vp8_clip8(pred[4 * i + 1] + ((b + c) >> 3));
        dst[i * stride + 2] = (uint8_t)ke_vp8_clip8(pred[4 * i + 2] + ((b - c) >> 3));
        dst[i * stride + 3] = (uint8_t)ke_vp8_clip8(pred[4 * i + 3] + ((a - d) >> 3));
    }
}

KE_HD int ke_avg3(int a, int b, int c) { return (a + 2 * b + c + 2) >> 2; }
KE_HD int ke_avg2(int a, int b) { return (a + b + 1) >> 1; }

// One 4x4 sub-block prediction (section 12.3): A[0..7] above (4 + above-right), L[0..3] left, X above-left.  out: row-major.
KE_HD void ke_vp8_pred4(int mode, const int *A, const int *L, int X, uint8_t *o) {
#define KE_P(x, y) o[(x) + 4 * (y)]
    const int I = L[0], J = L[1], K = L[2], Ll = L[3];
    switch (mode) {
    case KE_B_DC: {
        int dc = 4;
        for (int i = 0; i < 4; ++i) dc += A[i] + L[i];
        for (int i = 0; i < 16; ++i) o[i] = (uint8_t)(dc >> 3);
        break;
    }
    case KE_B_TM:
        for (int y = 0; y < 4; ++y)
            for (int x = 0; x < 4; ++x) KE_P(x, y) = (uint8_t)ke_vp8_clip8(A[x] + L[y] - X);
        break;
    case KE_B_VE: {
        const int v0 = ke_avg3(X, A[0], A[1]), v1 = ke_avg3(A[0], A[1], A[2]), v2 = ke_avg3(A[1], A[2], A[3]), v3 = ke_avg3(A[2], A[3], A[4]);
        for (int y = 0; y < 4; ++y) { KE_P(0, y) = (uint8_t)v0; KE_P(1, y) = (uint8_t)v1; KE_P(2, y) = (uint8_t)v2; KE_P(3, y) = (uint8_t)v3; }
        break;
    }
    case KE_B_HE: {
        const int r[4] = {ke_avg3(X, I, J), ke_avg3(I, J, K), ke_avg3(J, K, Ll), ke_avg3(K, Ll, Ll)};
        for (int y = 0; y < 4; ++y)
            for (int x = 0; x < 4; ++x) KE_P(x, y) = (uint8_t)r[y];
        break;
    }
    case KE_B_RD:
        KE_P(0, 3) = (uint8_t)ke_avg3(J, K, Ll);
        KE_P(1, 3) = KE_P(0, 2) = (uint8_t)ke_avg3(I, J, K);
        KE_P(2, 3) = KE_P(1, 2) = KE_P(0, 1) = (uint8_t)ke_avg3(X, I, J);
        KE_P(3, 3) = KE_P(2, 2) = KE_P(1, 1) = KE_P(0, 0) = (uint8_t)ke_avg3(A[0], X, I);
        KE_P(3, 2) = KE_P(2, 1) = KE_P(1, 0) = (uint8_t)ke_avg3(A[1], A[0], X);
        KE_P(3, 1) = KE_P(2, 0) = (uint8_t)ke_avg3(A[2], A[1], A[0]);
        KE_P(3, 0) = (uint8_t)ke_avg3(A[3], A[2], A[1]);
        break;
    case KE_B_LD:
        KE_P(0, 0) = (uint8_t)ke_avg3(A[0], A[1], A[2]);
        KE_P(1, 0) = KE_P(0, 1) = (uint8_t)ke_avg3(A[1], A[2], A[3]);
        KE_P(2, 0) = KE_P(1, 1) = KE_P(0, 2) = (uint8_t)ke_avg3(A[2], A[3], A[4]);
        KE_P(3, 0) = KE_P(2, 1) = KE_P(1, 2) = KE_P(0, 3) = (uint8_t)ke_avg3(A[3], A[4], A[5]);
        KE_P(3, 1) = KE_P(2, 2) = KE_P(1, 3) = (uint8_t)ke_avg3(A[4], A[5], A[6]);
        KE_P(3, 2) = KE_P(2, 3) = (uint8_t)ke_avg3(A[5], A[6], A[7]);
        KE_P(3, 3) = (uint8_t)ke_avg3(A[6], A[7], A[7]);
        break;
    case KE_B_VR:
        KE_P(0, 0) = KE_P(1, 2) = (uint8_t)ke_avg2(X, A[0]);
        KE_P(1, 0) = KE_P(2, 2) = (uint8_t)ke_avg2(A[0], A[1]);
        KE_P(2, 0) = KE_P(3, 2) = (uint8_t)ke_avg2(A[1], A[2]);
        KE_P(3, 0) = (uint8_t)ke_avg2(A[2], A[3]);
        KE_P(0, 3) = (uint8_t)ke_avg3(K, J, I);
        KE_P(0, 2) = (uint8_t)ke_avg3(J, I, X);
        KE_P(0, 1) = KE_P(1, 3) = (uint8_t)ke_avg3(I, X, A[0]);
        KE_P(1, 1) = KE_P(2, 3) = (uint8_t)ke_avg3(X, A[0], A[1]);
        KE_P(2, 1) = KE_P(3, 3) = (uint8_t)ke_avg3(A[0], A[1], A[2]);
        KE_P(3, 1) = (uint8_t)ke_avg3(A[1], A[2], A[3]);
        break;
    case KE_B_VL:
        KE_P(0, 0) = (uint8_t)ke_avg2(A[0], A[1]);
        KE_P(1, 0) = KE_P(0, 2) = (uint8_t)ke_avg2(A[1], A[2]);
        KE_P(2, 0) = KE_P(1, 2) = (uint8_t)ke_avg2(A[2], A[3]);
        KE_P(3, 0) = KE_P(2, 2) = (uint8_t)ke_avg2(A[3], A[4]);
        KE_P(0, 1) = (uint8_t)ke_avg3(A[0], A[1], A[2]);
        KE_P(1, 1) = KE_P(0, 3) = (uint8_t)ke_avg3(A[1], A[2], A[3]);
        KE_P(2, 1) = KE_P(1, 3) = (uint8_t)ke_avg3(A[2], A[3], A[4]);
        KE_P(3, 1) = KE_P(2, 3) = (uint8_t)ke_avg3(A[3], A[4], A[5]);
        KE_P(3, 2) = (uint8_t)ke_avg3(A[4], A[5], A[6]);
        KE_P(3, 3) = (uint8_t)ke_avg3(A[5], A[6], A[7]);
        break;
    case KE_B_HD:
        KE_P(0, 0) = KE_P(2, 1) = (uint8_t)ke_avg2(I, X);
        KE_P(0, 1) = KE_P(2, 2) = (uint8_t)ke_avg2(J, I);
        KE_P(0, 2) = KE_P(2, 3) = (uint8_t)ke_avg2(K, J);
        KE_P(0, 3) = (uint8_t)ke_avg2(Ll, K);
        KE_P(3, 0) = (uint8_t)ke_avg3(A[0], A[1], A[2]);
        KE_P(2, 0) = (uint8_t)ke_avg3(X, A[0], A[1]);
        KE_P(1, 0) = KE_P(3, 1) = (uint8_t)ke_avg3(I, X, A[0]);
        KE_P(1, 1) = KE_P(3, 2) = (uint8_t)ke_avg3(J, I, X);
        KE_P(1, 2) = KE_P(3, 3) = (uint8_t)ke_avg3(K, J, I);
        KE_P(1, 3) = (uint8_t)ke_avg3(Ll, K, J);
        break;
    default:   // KE_B_HU
        KE_P(0, 0) = (uint8_t)ke_avg2(I, J);
        KE_P(2, 0) = KE_P(0, 1) = (uint8_t)ke_avg2(J, K);
        KE_P(2, 1) = KE_P(0, 2) = (uint8_t)ke_avg2(K, Ll);
        KE_P(1, 0) = (uint8_t)ke_avg3(I, J, K);
        KE_P(3, 0) = KE_P(1, 1) = (uint8_t)ke_avg3(J, K, Ll);
        KE_P(3, 1) = KE_P(1, 2) = (uint8_t)ke_avg3(K, Ll, Ll);
        KE_P(3, 2) = KE_P(2, 2) = KE_P(0, 3) = KE_P(1, 3) = KE_P(2, 3) = KE_P(3, 3) = (uint8_t)Ll;
        break;
    }
#undef KE_P
}

// The DC value of a whole-block prediction (16x16 luma or 8x8 chroma, section 12.2; n = 16 or 8) with the variant the
// macroblock's position asks for, as libwebp's CheckMode picks it.
KE_HD int ke_vp8_dc_value(const int *A, const int *L, int n, int mb_x, int mb_y) {
    const int sh = n == 16 ? 4 : 3;
    int dc = 0;
    if (mb_x > 0 && mb_y > 0) {
        for (int i = 0; i < n; ++i) dc += A[i] + L[i];
        return (dc + n) >> (sh + 1);
    }
    if (mb_y > 0) {
        for (int i = 0; i < n; ++i) dc += A[i];
        return (dc + (n >> 1)) >> sh;
    }
    if (mb_x > 0) {
        for (int i = 0; i < n; ++i) dc += L[i];
        return (dc + (n >> 1)) >> sh;
    }
    return 0x80;
}

KE_HD int ke_vp8_pred_block(int mode, const int *A, const int *L, int X, int dc, int px, int py) {
    switch (mode) {
    case KE_B_TM: return ke_vp8_clip8(A[px] + L[py] - X);
    case KE_B_VE: return A[px];
    case KE_B_HE: return L[py];
    default: return dc;
    }
}

// Reconstruction of macroblock (mb_x, mb_y) into the unfiltered planes Y (stride ys = 16 mb_w), U / V (stride uvs = 8 mb_w).
// Reads the unfiltered pixels of (mb_x - 1, mb_y), (mb_x - 1 .. mb_x + 1, mb_y - 1): whatever order keeps those ahead works.
KE_HD void ke_webp_recon_mb(const KeWebpMb &m, const int16_t *coeffs, uint8_t *Y, uint8_t *U, uint8_t *V, int mb_w, int mb_x,
                            int mb_y) {
    const int ys = 16 * mb_w, uvs = 8 * mb_w;
    uint8_t *y0 = Y + (size_t)16 * mb_y * ys + 16 * mb_x;
    int A[21], L[16], X;                                  // above (16 + above-right 4), left, above-left
    for (int i = 0; i < 20; ++i) A[i] = 127;
    X = mb_y > 0 ? (mb_x > 0 ? y0[-ys - 1] : 129) : 127;
    if (mb_y > 0) {
        for (int i = 0; i < 16; ++i) A[i] = y0[-ys + i];
        for (int i = 16; i < 20; ++i) A[i] = mb_x + 1 < mb_w ? y0[-ys + i] : y0[-ys + 15];
    }
    for (int i = 0; i < 16; ++i) L[i] = mb_x > 0 ? y0[i * ys - 1] : 129;
    A[20] = A[19];
    uint8_t pred[16];
    if (m.is_i4) {
        for (int n = 0; n < 16; ++n) {
            const int bx = n & 3, by = n >> 2;
            uint8_t *d = y0 + 4 * by * ys + 4 * bx;
            int a[8], l[4], x;
            for (int i = 0; i < 8; ++i)
                a[i] = by == 0 ? A[4 * bx + i] : (bx == 3 && i >= 4) ? A[16 + i - 4] : d[-ys + i];
            for (int i = 0; i < 4; ++i) l[i] = bx == 0 ? L[4 * by + i] : d[i * ys - 1];
            x = by == 0 ? (bx == 0 ? X : A[4 * bx - 1]) : (bx == 0 ? L[4 * by - 1] : d[-ys - 1]);
            ke_vp8_pred4(m.imodes[n], a, l, x, pred);
            ke_vp8_idct_add(coeffs + 16 * n, pred, d, ys);
        }
    } else {
        const int dc = ke_vp8_dc_value(A, L, 16, mb_x, mb_y);
        for (int n = 0; n < 16; ++n) {
            const int bx = n & 3, by = n >> 2;
            for (int i = 0; i < 16; ++i)
                pred[i] = (uint8_t)ke_vp8_pred_block(m.imodes[0], A, L, X, dc, 4 * bx + (i & 3), 4 * by + (i >> 2));
            ke_vp8_idct_add(coeffs + 16 * n, pred, y0 + 4 * by * ys + 4 * bx, ys);
        }
    }
    for (int ch = 0; ch < 2; ++ch) {
        uint8_t *c0 = (ch ? V : U) + (size_t)8 * mb_y * uvs + 8 * mb_x;
        for (int i = 0; i < 8; ++i) {
            A[i] = mb_y > 0 ? c0[-uvs + i] : 127;
            L[i] = mb_x > 0 ? c0[i * uvs - 1] : 129;
        }
        X = mb_y > 0 ? (mb_x > 0 ? c0[-uvs - 1] : 129) : 127;
        const int dc = ke_vp8_dc_value(A, L, 8, mb_x, mb_y);
        for (int n = 0; n < 4; ++n) {
            const int bx = n & 1, by = n >> 1;
            for (int i = 0; i < 16; ++i)
                pred[i] = (uint8_t)ke_vp8_pred_block(m.uvmode, A, L, X, dc, 4 * bx + (i & 3), 4 * by + (i >> 2));
            ke_vp8_idct_add(coeffs + 256 + 64 * ch + 16 * n, pred, c0 + 4 * by * uvs + 4 * bx, uvs);
        }
    }
}

// ---- loop filter (section 15, as libwebp's dsp writes it) -----------------------------------------------------------------
KE_HD int ke_vp8_sclip1(int v) { return v < -128 ? -128 : v > 127 ? 127 : v; }   // [-1020, 1020] -> [-128, 127]
KE_HD int ke_vp8_sclip2(int v) { return v < -16 ? -16 : v > 15 ? 15 : v; }       // [-112, 112] -> [-16, 15]
KE_HD int ke_vp8_abs(int v) { return v < 0 ? -v : v; }

KE_HD void ke_vp8_filter2(uint8_t *p, int step) {               // 4 pixels in, 2 out
    const int p1 = p[-2 * step], p0 = p[-step], q0 = p[0], q1 = p[step];
    const int a = 3 * (q0 - p0) + ke_vp8_sclip1(p1 - q1);
    const int a1 = ke_vp8_sclip2((a + 4) >> 3), a2 = ke_vp8_sclip2((a + 3) >> 3);
    p[-step] = (uint8_t)ke_vp8_clip8(p0 + a2);
    p[0] = (uint8_t)ke_vp8_clip8(q0 - a1);
}

KE_HD void ke_vp8_filter4(uint8_t *p, int step) {               // 4 pixels in, 4 out
    const int p1 = p[-2 * step], p0 = p[-step], q0 = p[0], q1 = p[step];
    const int a = 3 * (q0 - p0);
    const int a1 = ke_vp8_sclip2((a + 4) >> 3), a2 = ke_vp8_sclip2((a + 3) >> 3), a3 = (a1 + 1) >> 1;
    p[-2 * step] = (uint8_t)ke_vp8_clip8(p1 + a3);
    p[-step] = (uint8_t)ke_vp8_clip8(p0 + a2);
    p[0] = (uint8_t)ke_vp8_clip8(q0 - a1);
    p[step] = (uint8_t)ke_vp8_clip8(q1 - a3);
}

KE_HD void ke_vp8_filter6(uint8_t *p, int step) {               // 6 pixels in, 6 out
    const int p2 = p[-3 * step], p1 = p[-2 * step], p0 = p[-step], q0 = p[0], q1 = p[step], q2 = p[2 * step];
    const int a = ke_vp8_sclip1(3 * (q0 - p0) + ke_vp8_sclip1(p1 - q1));
    const int a1 = (27 * a + 63) >> 7, a2 = (18 * a + 63) >> 7, a3 = (9 * a + 63) >> 7;
    p[-3 * step] = (uint8_t)ke_vp8_clip8(p2 + a3);
    p[-2 * step] = (uint8_t)ke_vp8_clip8(p1 + a2);
    p[-step] = (uint8_t)ke_vp8_clip8(p0 + a1);
    p[0] = (uint8_t)ke_vp8_clip8(q0 - a1);
    p[step] = (uint8_t)ke_vp8_clip8(q1 - a2);
    p[2 * step] = (uint8_t)ke_vp8_clip8(q2 - a3);
}

KE_HD bool ke_vp8_hev(const uint8_t *p, int step, int thresh) {
    return ke_vp8_abs(p[-2 * step] - p[-step]) > thresh || ke_vp8_abs(p[step] - p[0]) > thresh;
}

KE_HD bool ke_vp8_needs_filter(const uint8_t *p, int step, int t) {
    return 4 * ke_vp8_abs(p[-step] - p[0]) + ke_vp8_abs(p[-2 * step] - p[step]) <= t;
}

KE_HD bool ke_vp8_needs_filter2(const uint8_t *p, int step, int t, int it) {
    const int p3 = p[-4 * step], p2 = p[-3 * step], p1 = p[-2 * step], p0 = p[-step];
    const int q0 = p[0], q1 = p[step], q2 = p[2 * step], q3 = p[3 * step];
    if (4 * ke_vp8_abs(p0 - q0) + ke_vp8_abs(p1 - q1) > t) return false;
    return ke_vp8_abs(p3 - p2) <= it && ke_vp8_abs(p2 - p1) <= it && ke_vp8_abs(p1 - p0) <= it && ke_vp8_abs(q3 - q2) <= it &&
           ke_vp8_abs(q2 - q1) <= it && ke_vp8_abs(q1 - q0) <= it;
}

// `size` pixels along an edge: hstride crosses the edge, vstride walks it.  edge: macroblock edge (6-tap) or inner (4-tap).
KE_HD void ke_vp8_filter_loop(uint8_t *p, int hstride, int vstride, int size, int thresh, int ithresh, int hev_t, bool edge) {
    const int thresh2 = 2 * thresh + 1;
    for (int i = 0; i < size; ++i, p += vstride) {
        if (!ke_vp8_needs_filter2(p, hstride, thresh2, ithresh)) continue;
        if (ke_vp8_hev(p, hstride, hev_t)) ke_vp8_filter2(p, hstride);
        else if (edge) ke_vp8_filter6(p, hstride);
        else ke_vp8_filter4(p, hstride);
    }
}

KE_HD void ke_vp8_simple_loop(uint8_t *p, int hstride, int vstride, int thresh) {
    const int thresh2 = 2 * thresh + 1;
    for (int i = 0; i < 16; ++i, p += vstride)
        if (ke_vp8_needs_filter(p, hstride, thresh2)) ke_vp8_filter2(p, hstride);
}

// The loop filter of macroblock (mb_x, mb_y) on the planes, in place: left edge, inner vertical edges, top edge, inner
// horizontal edges (libwebp's DoFilter).  Run in raster order over macroblocks, or in any order that keeps (mb_x - 1, mb_y)
// and (mb_x + 1, mb_y - 1) ahead -- those are the neighbours whose pixels overlap this one's.
KE_HD void ke_webp_filter_mb(const KeWebpHeader &h, const KeWebpMb &m, uint8_t *Y, uint8_t *U, uint8_t *V, int mb_x, int mb_y) {
    const int limit = h.f_limit[m.segment][m.is_i4];
    if (h.filter_type == 0 || limit == 0) return;
    const int ys = 16 * h.mb_w, uvs = 8 * h.mb_w;
    uint8_t *y0 = Y + (size_t)16 * mb_y * ys + 16 * mb_x;
    if (h.filter_type == 1) {
        if (mb_x > 0) ke_vp8_simple_loop(y0, 1, ys, limit + 4);
        if (m.inner)
            for (int k = 1; k < 4; ++k) ke_vp8_simple_loop(y0 + 4 * k, 1, ys, limit);
        if (mb_y > 0) ke_vp8_simple_loop(y0, ys, 1, limit + 4);
        if (m.inner)
            for (int k = 1; k < 4; ++k) ke_vp8_simple_loop(y0 + 4 * k * ys, ys, 1, limit);
        return;
    }
    const int il = h.f_ilevel[m.segment][m.is_i4], hev = h.f_hev[m.segment][m.is_i4];
    uint8_t *u0 = U + (size_t)8 * mb_y * uvs + 8 * mb_x, *v0 = V + (size_t)8 * mb_y * uvs + 8 * mb_x;
    if (mb_x > 0) {
        ke_vp8_filter_loop(y0, 1, ys, 16, limit + 4, il, hev, true);
        ke_vp8_filter_loop(u0, 1, uvs, 8, limit + 4, il, hev, true);
        ke_vp8_filter_loop(v0, 1, uvs, 8, limit + 4, il, hev, true);
    }
    if (m.inner) {
        for (int k = 1; k < 4; ++k) ke_vp8_filter_loop(y0 + 4 * k, 1, ys, 16, limit, il, hev, false);
        ke_vp8_filter_loop(u0 + 4, 1, uvs, 8, limit, il, hev, false);
        ke_vp8_filter_loop(v0 + 4, 1, uvs, 8, limit, il, hev, false);
    }
    if (mb_y > 0) {
        ke_vp8_filter_loop(y0, ys, 1, 16, limit + 4, il, hev, true);
        ke_vp8_filter_loop(u0, uvs, 1, 8, limit + 4, il, hev, true);
        ke_vp8_filter_loop(v0, uvs, 1, 8, limit + 4, il, hev, true);
    }
    if (m.inner) {
        for (int k = 1; k < 4; ++k) ke_vp8_filter_loop(y0 + 4 * k * ys, ys, 1, 16, limit, il, hev, false);
        ke_vp8_filter_loop(u0 + 4 * uvs, uvs, 1, 8, limit, il, hev, false);
        ke_vp8_filter_loop(v0 + 4 * uvs, uvs, 1, 8, limit, il, hev, false);
    }
}

// ---- output: libwebp's fancy upsampling + VP8YUVToR/G/B -------------------------------------------------------------------
KE_HD int ke_vp8_mult_hi(int v, int coeff) { return (v * coeff) >> 8; }
KE_HD int ke_vp8_yuv_clip(int v) { return (v & ~16383) == 0 ? (v >> 6) : v < 0 ? 0 : 255; }   // YUV_FIX2 = 6

// One chroma sample of output pixel (x, y): the planes (stride uvs) hold the decoded chroma; W x H is the frame.
KE_HD int ke_vp8_fancy(const uint8_t *C, int uvs, int W, int H, int x, int y) {
    int nr, fr;                                       // the nearer and the farther chroma row
    if (y == 0 || (y == H - 1 && !(H & 1))) {
        nr = fr = y >> 1;                             // first row, last row of an even height: the row mirrored
    } else if (y & 1) {
        nr = y >> 1; fr = nr + 1;
    } else {
        nr = y >> 1; fr = nr - 1;
    }
    const uint8_t *n = C + (size_t)nr * uvs, *f = C + (size_t)fr * uvs;
    if (x == 0 || (x == W - 1 && !(W & 1))) {
        const int c = x >> 1;
        return (3 * n[c] + f[c] + 2) >> 2;
    }
    const int a = x >> 1, b = (x & 1) ? a + 1 : a - 1;   // nearer / farther chroma column
    const int A = n[a], B = n[b], Cc = f[a], D = f[b];
    return (((A + D + 3 * (B + Cc) + 8) >> 3) + A) >> 1;
}

KE_HD void ke_webp_rgb_at(const uint8_t *Y, const uint8_t *U, const uint8_t *V, int mb_w, int W, int H, int x, int y, uint8_t *rgb) {
    const int yy = Y[(size_t)y * 16 * mb_w + x];
    const int u = ke_vp8_fancy(U, 8 * mb_w, W, H, x, y), v = ke_vp8_fancy(V, 8 * mb_w, W, H, x, y);
    const int yh = ke_vp8_mult_hi(yy, 19077);
    rgb[0] = (uint8_t)ke_vp8_yuv_clip(yh + ke_vp8_mult_hi(v, 26149) - 14234);
    rgb[1] = (uint8_t)ke_vp8_yuv_clip(yh - ke_vp8_mult_hi(u, 6419) - ke_vp8_mult_hi(v, 13320) + 8708);
    rgb[2] = (uint8_t)ke_vp8_yuv_clip(yh + ke_vp8_mult_hi(u, 33050) - 17685);
}
