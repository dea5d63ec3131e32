// ke_webpl_core.h -- lossless WebP (one VP8L bitstream) decoding arithmetic shared by the HIP kernels (ke_webpl.hip), the host
// parser (ke_webpl_parse.h) and the CPU build the tests hold against Pillow (tests/_webpl_cpu.cpp).  Plain C++ without
// allocation; KE_HD marks what the device compiles too.
//
// What is restated here is the published VP8L bitstream specification as libwebp decodes it for Pillow's `Image.open(path)`
// -- the decode step of the reference's batch hasher (src/core/fastsig.py:31-34) and of safe_load_image
// (src/utils/image_io.py:60-138):
//   bit reader        : least significant bit first; bits past the end read as zero and fail the decode once consumed;
//   prefix codes      : simple codes of 1-2 symbols (a symbol outside the alphabet is dropped), normal codes through the
//                       19-symbol code-length code with the repeat codes 16 / 17 / 18 and max_symbol; a code with exactly one
//                       used symbol costs zero bits, every other code has to be complete (Kraft sum exactly one);
//   groups            : five codes -- green + length prefixes + colour cache (256 + 24 + cache size), red, blue, alpha (256
//                       each), distance prefixes (40) --, selected per block by the entropy image of the main image;
//   colour cache      : 1-11 bits, hash 0x1e35a7bd * argb >> (32 - bits), fed by every pixel, copied ones included;
//   LZ77              : prefix + extra bits for length and distance, the 120 short distance codes mapped to 2-D neighbours;
//   transforms        : predictor (14 modes; 14 and 15 predict opaque black as mode 0 does), cross-colour, subtract-green,
//                       colour indexing with 1 / 2 / 4 / 8 pixels per packed green value; each at most once.
// Sub-images (transform data, entropy image, palette) are entropy-coded images without transforms or entropy image.
//
// Codes are kept in canonical form -- 16 counts and the used symbols in code order, read a bit at a time -- not as lookup
// tables: an image may carry tens of thousands of groups, and a group costs 40 bytes plus two bytes per used symbol this way.
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

enum { KE_WEBPL_OK = 0, KE_WEBPL_UNSUPPORTED = 1, KE_WEBPL_CORRUPT = 2 };

// The pixel cap: images of more than this many pixels (the lossy decoder's 16.7 Mpx) are left to Pillow.  The scratch is
// about 9.2 bytes per pixel plus 96 KiB (see ke_vp8l_scratch_words).
constexpr int64_t kWebplMaxPixels = (int64_t)65536 * 256;

enum { KE_VP8L_PREDICTOR = 0, KE_VP8L_CROSS_COLOUR = 1, KE_VP8L_SUBTRACT_GREEN = 2, KE_VP8L_COLOUR_INDEXING = 3 };

// distance codes 1..120 -> (dy << 4) | (8 - dx)
constexpr uint8_t kVp8lCodeToPlane[120] = {
    0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36, 0x3a,
    0x25, 0x2b, 0x48, 0x04, 0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34, 0x3c, 0x03,
    0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d, 0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67, 0x69, 0x12, 0x1e,
    0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e, 0x78, 0x01, 0x77, 0x79, 0x53, 0x5d, 0x11, 0x1f,
    0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52, 0x5e, 0x00, 0x74, 0x7c, 0x41,
    0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61, 0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70};
constexpr uint8_t kVp8lCodeLengthOrder[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};

KE_HD int ke_vp8l_subsample(int size, int bits) { return (size + (1 << bits) - 1) >> bits; }

// ---- bit reader -------------------------------------------------------------------------------------------------------------
struct KeVp8lBits {
    const uint8_t *p;
    uint32_t len, pos;       // bytes of the stream, next byte
    uint64_t val;            // the bits not consumed yet, lowest first
    int32_t nbits;           // how many of them, zero bits made up behind the stream's end included
    int32_t pad;             // ... how many were made up
};

KE_HD void ke_vp8l_bits_init(KeVp8lBits &b, const uint8_t *p, uint32_t len) {
    b.p = p; b.len = len; b.pos = 0; b.val = 0; b.nbits = 0; b.pad = 0;
}
KE_HD void ke_vp8l_fill(KeVp8lBits &b) {
    while (b.nbits <= 56) {
        uint64_t byte = 0;
        if (b.pos < b.len) byte = b.p[b.pos++];
        else b.pad += 8;
        b.val |= byte << b.nbits;
        b.nbits += 8;
    }
}
KE_HD uint32_t ke_vp8l_read(KeVp8lBits &b, int n) {              // n <= 32
    if (n == 0) return 0;
    ke_vp8l_fill(b);
    const uint32_t v = (uint32_t)(b.val & ((1ull << n) - 1ull));
    b.val >>= n;
    b.nbits -= n;
    return v;
}
KE_HD bool ke_vp8l_eos(const KeVp8lBits &b) { return b.pad > b.nbits; }   // made-up bits were consumed

// ---- prefix codes -----------------------------------------------------------------------------------------------------------
// The decoder's working memory is one array of 32-bit words: the pixels first, then a bump allocator.
struct KeVp8lArena {
    uint32_t *mem;
    uint32_t cap, used;      // words
};
KE_HD uint32_t ke_vp8l_alloc(KeVp8lArena &a, uint64_t words) {     // word offset, or 0: out of room
    if (words > (uint64_t)(a.cap - a.used)) return 0;
    const uint32_t at = a.used;
    a.used += (uint32_t)words;
    return at;
}

struct KeVp8lCode {
    uint32_t off;            // word offset of {uint16 count[16]; uint16 symbol[]}, or 0: the code has one symbol
    uint32_t single;         // ... this one, read with zero bits
};
struct KeVp8lGroup { KeVp8lCode c[5]; };    // green / red / blue / alpha / distance

KE_HD uint32_t ke_vp8l_symbol_raw(KeVp8lBits &b, const uint16_t *cnt, const uint16_t *sym) {
    ke_vp8l_fill(b);
    uint32_t bits = (uint32_t)b.val;
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int c = cnt[len];
        if (code - c < first) {
            b.val >>= len;
            b.nbits -= len;
            return sym[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    b.val >>= 15;                                                  // not reached: the code is complete
    b.nbits -= 15;
    return 0;
}
KE_HD uint32_t ke_vp8l_symbol(KeVp8lBits &b, const uint32_t *mem, const KeVp8lCode &c) {
    if (!c.off) return c.single;
    const uint16_t *cnt = (const uint16_t *)(mem + c.off);
    return ke_vp8l_symbol_raw(b, cnt, cnt + 16);
}

// counts per length, the number of used symbols, validity: one symbol, or a complete code
KE_HD int ke_vp8l_census(const uint8_t *lengths, int n, uint16_t *cnt, int &used, int &last) {
    for (int k = 0; k < 16; ++k) cnt[k] = 0;
    used = 0;
    last = 0;
    for (int s = 0; s < n; ++s)
        if (lengths[s]) { ++cnt[lengths[s]]; ++used; last = s; }
    if (used == 0) return KE_WEBPL_CORRUPT;
    if (used == 1) return KE_WEBPL_OK;
    uint32_t kraft = 0;
    for (int len = 1; len <= 15; ++len) kraft += (uint32_t)cnt[len] << (15 - len);
    return kraft == (1u << 15) ? KE_WEBPL_OK : KE_WEBPL_CORRUPT;
}
KE_HD void ke_vp8l_sort_symbols(const uint8_t *lengths, int n, const uint16_t *cnt, uint16_t *sym) {
    uint16_t at[16];
    at[0] = at[1] = 0;
    for (int len = 1; len < 15; ++len) at[len + 1] = (uint16_t)(at[len] + cnt[len]);
    for (int s = 0; s < n; ++s)
        if (lengths[s]) sym[at[lengths[s]]++] = (uint16_t)s;
}

// One prefix code of `alphabet` symbols read from the stream; lengths: room for `alphabet` bytes.
KE_HD int ke_vp8l_read_code(KeVp8lBits &b, KeVp8lArena &ar, int alphabet, uint8_t *lengths, KeVp8lCode &out) {
    for (int s = 0; s < alphabet; ++s) lengths[s] = 0;
    if (ke_vp8l_read(b, 1)) {                                      // simple code
        const int two = (int)ke_vp8l_read(b, 1);
        const int s0 = (int)ke_vp8l_read(b, ke_vp8l_read(b, 1) ? 8 : 1);
        if (s0 < alphabet) lengths[s0] = 1;
        if (two) {
            const int s1 = (int)ke_vp8l_read(b, 8);
            if (s1 < alphabet) lengths[s1] = 1;
        }
    } else {
        uint8_t cl[19];
        for (int k = 0; k < 19; ++k) cl[k] = 0;
        const int num = (int)ke_vp8l_read(b, 4) + 4;
        for (int k = 0; k < num; ++k) cl[kVp8lCodeLengthOrder[k]] = (uint8_t)ke_vp8l_read(b, 3);
        uint16_t ccnt[16], csym[19];
        int cused, clast;
        if (ke_vp8l_census(cl, 19, ccnt, cused, clast) != KE_WEBPL_OK) return KE_WEBPL_CORRUPT;
        ke_vp8l_sort_symbols(cl, 19, ccnt, csym);
        int max_symbol = alphabet;
        if (ke_vp8l_read(b, 1)) {
            const int nb = 2 + 2 * (int)ke_vp8l_read(b, 3);
            max_symbol = 2 + (int)ke_vp8l_read(b, nb);
            if (max_symbol > alphabet) return KE_WEBPL_CORRUPT;
        }
        int s = 0, prev = 8;
        while (s < alphabet) {
            if (max_symbol-- == 0) break;
            const int len = cused == 1 ? clast : (int)ke_vp8l_symbol_raw(b, ccnt, csym);
            if (len < 16) {
                lengths[s++] = (uint8_t)len;
                if (len) prev = len;
            } else {
                const int extra = len == 16 ? 2 : len == 17 ? 3 : 7, base = len == 18 ? 11 : 3;
                const int repeat = (int)ke_vp8l_read(b, extra) + base;
                if (s + repeat > alphabet) return KE_WEBPL_CORRUPT;
                const uint8_t v = (uint8_t)(len == 16 ? prev : 0);
                for (int k = 0; k < repeat; ++k) lengths[s++] = v;
            }
            if (ke_vp8l_eos(b)) return KE_WEBPL_CORRUPT;
        }
    }
    if (ke_vp8l_eos(b)) return KE_WEBPL_CORRUPT;
    uint16_t cnt[16];
    int used, last;
    if (ke_vp8l_census(lengths, alphabet, cnt, used, last) != KE_WEBPL_OK) return KE_WEBPL_CORRUPT;
    out.off = 0;
    out.single = (uint32_t)last;
    if (used == 1) return KE_WEBPL_OK;
    out.off = ke_vp8l_alloc(ar, (uint64_t)(32 + 2 * used + 3) / 4);
    if (!out.off) return KE_WEBPL_UNSUPPORTED;                     // more codes than the scratch was sized for: Pillow's
    uint16_t *dst = (uint16_t *)(ar.mem + out.off);
    for (int k = 0; k < 16; ++k) dst[k] = cnt[k];
    ke_vp8l_sort_symbols(lengths, alphabet, cnt, dst + 16);
    return KE_WEBPL_OK;
}

// `n` groups; returns the word offset of the KeVp8lGroup array through `at`
KE_HD int ke_vp8l_read_groups(KeVp8lBits &b, KeVp8lArena &ar, uint32_t n, int cache_bits, uint8_t *lengths, uint32_t &at) {
    at = ke_vp8l_alloc(ar, (uint64_t)n * (sizeof(KeVp8lGroup) / 4));
    if (!at) return KE_WEBPL_UNSUPPORTED;
    for (uint32_t g = 0; g < n; ++g)
        for (int j = 0; j < 5; ++j) {
            const int alphabet = j == 0 ? 256 + 24 + (cache_bits > 0 ? 1 << cache_bits : 0) : j == 4 ? 40 : 256;
            KeVp8lCode c;
            const int st = ke_vp8l_read_code(b, ar, alphabet, lengths, c);
            if (st != KE_WEBPL_OK) return st;
            ((KeVp8lGroup *)(ar.mem + at))[g].c[j] = c;
        }
    return KE_WEBPL_OK;
}

// ---- the pixels of one entropy-coded image ----------------------------------------------------------------------------------
KE_HD uint32_t ke_vp8l_prefix_value(KeVp8lBits &b, uint32_t sym) {            // length or distance code from its prefix symbol
    if (sym < 4) return sym + 1;
    const int extra = (int)(sym - 2) >> 1;
    const uint32_t offset = (2u + (sym & 1u)) << extra;
    return offset + ke_vp8l_read(b, extra) + 1;
}
KE_HD uint32_t ke_vp8l_plane_distance(int xsize, uint32_t code) {
    if (code > 120) return code - 120;
    const int e = kVp8lCodeToPlane[code - 1];
    const int dist = (e >> 4) * xsize + (8 - (e & 15));
    return dist >= 1 ? (uint32_t)dist : 1u;
}

struct KeVp8lEntropy {
    uint32_t groups;         // word offset of the groups
    uint32_t himg;           // word offset of the entropy image, 0: one group
    int32_t hbits, hw;       // its block size (bits) and width
    uint32_t cache;          // word offset of the colour cache, 0: none
    int32_t cache_bits;
};

KE_HD int ke_vp8l_decode_pixels(KeVp8lBits &b, uint32_t *mem, const KeVp8lEntropy &e, uint32_t *dst, int xs, int ys) {
    const uint32_t n = (uint32_t)xs * (uint32_t)ys;
    const KeVp8lGroup *groups = (const KeVp8lGroup *)(mem + e.groups);
    uint32_t *cache = e.cache ? mem + e.cache : nullptr;
    const int shift = 32 - e.cache_bits;
    uint32_t pos = 0;
    int x = 0, y = 0;
    while (pos < n) {
        const KeVp8lGroup &g = e.himg ? groups[(mem[e.himg + (uint32_t)(y >> e.hbits) * e.hw + (x >> e.hbits)] >> 8) & 0xffffu] : groups[0];
        const uint32_t s = ke_vp8l_symbol(b, mem, g.c[0]);
        if (s < 256) {
            const uint32_t r = ke_vp8l_symbol(b, mem, g.c[1]), bl = ke_vp8l_symbol(b, mem, g.c[2]), a = ke_vp8l_symbol(b, mem, g.c[3]);
            const uint32_t argb = (a << 24) | (r << 16) | (s << 8) | bl;
            dst[pos++] = argb;
            if (cache) cache[(0x1e35a7bdu * argb) >> shift] = argb;
            if (++x == xs) { x = 0; ++y; }
        } else if (s < 256 + 24) {
            const uint32_t len = ke_vp8l_prefix_value(b, s - 256);
            const uint32_t dsym = ke_vp8l_symbol(b, mem, g.c[4]);
            const uint32_t dist = ke_vp8l_plane_distance(xs, ke_vp8l_prefix_value(b, dsym));
            if (dist > pos || len > n - pos) return KE_WEBPL_CORRUPT;
            for (uint32_t k = 0; k < len; ++k, ++pos) {
                const uint32_t argb = dst[pos - dist];
                dst[pos] = argb;
                if (cache) cache[(0x1e35a7bdu * argb) >> shift] = argb;
            }
            x += (int)len;
            while (x >= xs) { x -= xs; ++y; }
        } else {
            if (!cache) return KE_WEBPL_CORRUPT;                   // (the alphabet has no such symbol then)
            const uint32_t argb = cache[s - (256 + 24)];
            dst[pos++] = argb;
            cache[(0x1e35a7bdu * argb) >> shift] = argb;
            if (++x == xs) { x = 0; ++y; }
        }
        if (ke_vp8l_eos(b)) return KE_WEBPL_CORRUPT;
    }
    return KE_WEBPL_OK;
}

KE_HD int ke_vp8l_read_cache(KeVp8lBits &b, KeVp8lArena &ar, KeVp8lEntropy &e) {
    e.cache = 0;
    e.cache_bits = 0;
    if (!ke_vp8l_read(b, 1)) return KE_WEBPL_OK;
    e.cache_bits = (int)ke_vp8l_read(b, 4);
    if (e.cache_bits < 1 || e.cache_bits > 11) return KE_WEBPL_CORRUPT;
    e.cache = ke_vp8l_alloc(ar, (uint64_t)1 << e.cache_bits);
    if (!e.cache) return KE_WEBPL_UNSUPPORTED;
    for (uint32_t k = 0; k < (1u << e.cache_bits); ++k) ar.mem[e.cache + k] = 0;
    return KE_WEBPL_OK;
}

// A sub-image (transform data, entropy image, palette): colour cache, one group, pixels.  What it allocated is given back.
KE_HD int ke_vp8l_sub_image(KeVp8lBits &b, KeVp8lArena &ar, uint8_t *lengths, uint32_t *dst, int xs, int ys) {
    const uint32_t mark = ar.used;
    KeVp8lEntropy e;
    e.himg = 0; e.hbits = 0; e.hw = 0;
    int st = ke_vp8l_read_cache(b, ar, e);
    if (st == KE_WEBPL_OK) st = ke_vp8l_read_groups(b, ar, 1, e.cache_bits, lengths, e.groups);
    if (st == KE_WEBPL_OK) st = ke_vp8l_decode_pixels(b, ar.mem, e, dst, xs, ys);
    ar.used = mark;
    return st;
}

// ---- the stream: header, transforms, entropy image, codes, pixels -----------------------------------------------------------
struct KeVp8lXform {
    int32_t type, bits;
    int32_t xsize;           // width of the image this transform yields
    uint32_t data;           // word offset of its sub-image (colour indexing: 256 colours, the unused ones transparent black)
};
struct KeVp8lPlan {
    int32_t ntrans;
    KeVp8lXform t[4];        // in the order of the stream: undone last to first
    uint32_t pix;            // word offset of the decoded pixels (they end where the full-size image ends)
    int32_t xsize;           // their width
};

// Worst case of the bump allocator beside the pixels: three sub-images of 4x4 blocks, palette, colour cache, the code-length
// buffer; and for the codes 64 KiB + 4 bytes per pixel (a stream with more groups than that holds goes to Pillow).
KE_HD uint64_t ke_vp8l_scratch_words(int w, int h) {
    const uint64_t px = (uint64_t)w * h, sub = (uint64_t)ke_vp8l_subsample(w, 2) * ke_vp8l_subsample(h, 2);
    return px + 3 * sub + 256 + 2048 + 600 + 16384 + px + 16;
}

// What follows the 5-byte header: transforms, colour cache, entropy image, codes, pixels, read from `b` as it stands.  The
// header is exactly 40 bits, so a stream without one -- the VP8L-coded plane of an ALPH chunk, whose size the container
// supplies (libwebp's VP8LDecodeAlphaHeader) -- starts here with a fresh reader.  mem / cap / plan as ke_vp8l_decode_stream.
KE_HD int ke_vp8l_decode_body(KeVp8lBits &b, int w, int h, uint32_t *mem, uint64_t cap, KeVp8lPlan &plan) {
    plan.ntrans = 0;
    KeVp8lArena ar;
    ar.mem = mem;
    ar.cap = (uint32_t)(cap > 0xffffffffull ? 0xffffffffull : cap);
    ar.used = (uint32_t)w * (uint32_t)h;
    if (ar.used >= ar.cap) return KE_WEBPL_UNSUPPORTED;
    const uint32_t lbuf = ke_vp8l_alloc(ar, (256 + 24 + 2048 + 3) / 4);
    if (!lbuf) return KE_WEBPL_UNSUPPORTED;
    uint8_t *lengths = (uint8_t *)(mem + lbuf);
    int xs = w, seen = 0;
    while (ke_vp8l_read(b, 1)) {
        const int type = (int)ke_vp8l_read(b, 2);
        if (seen & (1 << type)) return KE_WEBPL_CORRUPT;
        seen |= 1 << type;
        KeVp8lXform &t = plan.t[plan.ntrans];
        t.type = type; t.bits = 0; t.xsize = xs; t.data = 0;
        if (type == KE_VP8L_PREDICTOR || type == KE_VP8L_CROSS_COLOUR) {
            t.bits = 2 + (int)ke_vp8l_read(b, 3);
            const int sw = ke_vp8l_subsample(xs, t.bits), sh = ke_vp8l_subsample(h, t.bits);
            t.data = ke_vp8l_alloc(ar, (uint64_t)sw * sh);
            if (!t.data) return KE_WEBPL_UNSUPPORTED;
            const int st = ke_vp8l_sub_image(b, ar, lengths, mem + t.data, sw, sh);
            if (st != KE_WEBPL_OK) return st;
        } else if (type == KE_VP8L_COLOUR_INDEXING) {
            const int colours = (int)ke_vp8l_read(b, 8) + 1;
            t.bits = colours > 16 ? 0 : colours > 4 ? 1 : colours > 2 ? 2 : 3;
            t.data = ke_vp8l_alloc(ar, 256);
            if (!t.data) return KE_WEBPL_UNSUPPORTED;
            uint32_t *pal = mem + t.data;
            const int st = ke_vp8l_sub_image(b, ar, lengths, pal, colours, 1);
            if (st != KE_WEBPL_OK) return st;
            for (int k = 1; k < colours; ++k) {                    // delta-coded, channel by channel
                const uint32_t a = pal[k], c = pal[k - 1];
                pal[k] = (((a & 0xff00ff00u) + (c & 0xff00ff00u)) & 0xff00ff00u) | (((a & 0x00ff00ffu) + (c & 0x00ff00ffu)) & 0x00ff00ffu);
            }
            for (int k = colours; k < 256; ++k) pal[k] = 0;
            xs = ke_vp8l_subsample(xs, t.bits);
        }
        ++plan.ntrans;
        if (ke_vp8l_eos(b)) return KE_WEBPL_CORRUPT;
    }
    KeVp8lEntropy e;
    int st = ke_vp8l_read_cache(b, ar, e);
    if (st != KE_WEBPL_OK) return st;
    e.himg = 0; e.hbits = 0; e.hw = 0;
    uint32_t ngroups = 1;
    if (ke_vp8l_read(b, 1)) {                                      // the entropy image
        e.hbits = 2 + (int)ke_vp8l_read(b, 3);
        e.hw = ke_vp8l_subsample(xs, e.hbits);
        const int hh2 = ke_vp8l_subsample(h, e.hbits);
        e.himg = ke_vp8l_alloc(ar, (uint64_t)e.hw * hh2);
        if (!e.himg) return KE_WEBPL_UNSUPPORTED;
        st = ke_vp8l_sub_image(b, ar, lengths, mem + e.himg, e.hw, hh2);
        if (st != KE_WEBPL_OK) return st;
        uint32_t top = 0;
        for (uint32_t k = 0; k < (uint32_t)e.hw * hh2; ++k) {
            const uint32_t g = (mem[e.himg + k] >> 8) & 0xffffu;
            top = g > top ? g : top;
        }
        ngroups = top + 1;
    }
    if (ke_vp8l_eos(b)) return KE_WEBPL_CORRUPT;
    st = ke_vp8l_read_groups(b, ar, ngroups, e.cache_bits, lengths, e.groups);
    if (st != KE_WEBPL_OK) return st;
    plan.xsize = xs;
    plan.pix = (uint32_t)w * h - (uint32_t)xs * h;
    return ke_vp8l_decode_pixels(b, mem, e, mem + plan.pix, xs, h);
}

// mem: ke_vp8l_scratch_words(w, h) words; mem[0 .. w * h) will hold the pixels.  `p` is the VP8L chunk's payload.
KE_HD int ke_vp8l_decode_stream(const uint8_t *p, uint32_t len, int w, int h, uint32_t *mem, uint64_t cap, KeVp8lPlan &plan) {
    KeVp8lBits b;
    ke_vp8l_bits_init(b, p, len);
    plan.ntrans = 0;
    if (ke_vp8l_read(b, 8) != 0x2f) return KE_WEBPL_CORRUPT;
    const int hw = (int)ke_vp8l_read(b, 14) + 1, hh = (int)ke_vp8l_read(b, 14) + 1;
    ke_vp8l_read(b, 1);                                            // the alpha hint
    if (ke_vp8l_read(b, 3) != 0 || hw != w || hh != h) return KE_WEBPL_UNSUPPORTED;
    return ke_vp8l_decode_body(b, w, h, mem, cap, plan);
}

// ---- inverse transforms, per pixel ------------------------------------------------------------------------------------------
KE_HD uint32_t ke_vp8l_add(uint32_t a, uint32_t b) {
    return (((a & 0xff00ff00u) + (b & 0xff00ff00u)) & 0xff00ff00u) | (((a & 0x00ff00ffu) + (b & 0x00ff00ffu)) & 0x00ff00ffu);
}
KE_HD uint32_t ke_vp8l_avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xfefefefeu) >> 1) + (a & b); }
KE_HD int ke_vp8l_abs(int v) { return v < 0 ? -v : v; }
KE_HD uint32_t ke_vp8l_clip255(int v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }
KE_HD uint32_t ke_vp8l_select(uint32_t t, uint32_t l, uint32_t tl) {
    int d = 0;                                                     // sum over channels of |l - tl| - |t - tl|
    for (int s = 0; s < 32; s += 8) {
        const int a = (int)((t >> s) & 255u), bb = (int)((l >> s) & 255u), c = (int)((tl >> s) & 255u);
        d += ke_vp8l_abs(bb - c) - ke_vp8l_abs(a - c);
    }
    return d <= 0 ? t : l;
}
KE_HD uint32_t ke_vp8l_clamped_full(uint32_t c0, uint32_t c1, uint32_t c2) {
    uint32_t out = 0;
    for (int s = 0; s < 32; s += 8)
        out |= ke_vp8l_clip255((int)((c0 >> s) & 255u) + (int)((c1 >> s) & 255u) - (int)((c2 >> s) & 255u)) << s;
    return out;
}
KE_HD uint32_t ke_vp8l_clamped_half(uint32_t c0, uint32_t c1, uint32_t c2) {
    const uint32_t ave = ke_vp8l_avg2(c0, c1);
    uint32_t out = 0;
    for (int s = 0; s < 32; s += 8) {
        const int a = (int)((ave >> s) & 255u), bb = (int)((c2 >> s) & 255u);
        out |= ke_vp8l_clip255(a + (a - bb) / 2) << s;
    }
    return out;
}

// The predicted value of pixel (x, y) of an image `w` wide whose earlier pixels are final.  The above-right neighbour of a
// row's last pixel is the next pixel in memory: the first one of the current row.
KE_HD uint32_t ke_vp8l_predict(const uint32_t *pix, int w, int x, int y, const uint32_t *modes, int bits) {
    if (y == 0) return x == 0 ? 0xff000000u : pix[x - 1];
    const uint32_t *cur = pix + (size_t)y * w + x;
    if (x == 0) return cur[-w];
    const int mode = (int)((modes[(size_t)(y >> bits) * ke_vp8l_subsample(w, bits) + (x >> bits)] >> 8) & 15u);
    const uint32_t L = cur[-1], T = cur[-w], TL = cur[-w - 1], TR = cur[-w + 1];
    switch (mode) {
        case 1: return L;
        case 2: return T;
        case 3: return TR;
        case 4: return TL;
        case 5: return ke_vp8l_avg2(ke_vp8l_avg2(L, TR), T);
        case 6: return ke_vp8l_avg2(L, TL);
        case 7: return ke_vp8l_avg2(L, T);
        case 8: return ke_vp8l_avg2(TL, T);
        case 9: return ke_vp8l_avg2(T, TR);
        case 10: return ke_vp8l_avg2(ke_vp8l_avg2(L, TL), ke_vp8l_avg2(T, TR));
        case 11: return ke_vp8l_select(T, L, TL);
        case 12: return ke_vp8l_clamped_full(L, T, TL);
        case 13: return ke_vp8l_clamped_half(L, T, TL);
        default: return 0xff000000u;                               // 0, and the two unused values
    }
}

KE_HD int ke_vp8l_delta(uint32_t mult, uint32_t colour) { return ((int)(int8_t)mult * (int)(int8_t)colour) >> 5; }
KE_HD uint32_t ke_vp8l_cross_colour(uint32_t argb, uint32_t m) {          // m: the block's multipliers
    const uint32_t green = (argb >> 8) & 255u;
    uint32_t red = (argb >> 16) & 255u, blue = argb & 255u;
    red = (red + (uint32_t)ke_vp8l_delta(m & 255u, green)) & 255u;
    blue = (blue + (uint32_t)ke_vp8l_delta((m >> 8) & 255u, green)) & 255u;
    blue = (blue + (uint32_t)ke_vp8l_delta((m >> 16) & 255u, red)) & 255u;
    return (argb & 0xff00ff00u) | (red << 16) | blue;
}
KE_HD uint32_t ke_vp8l_add_green(uint32_t argb) {
    const uint32_t g = (argb >> 8) & 255u;
    return (argb & 0xff00ff00u) | ((((argb & 0x00ff00ffu) + ((g << 16) | g)) & 0x00ff00ffu));
}
// pixel x of a row whose packed values start at `row`
KE_HD uint32_t ke_vp8l_colour_index(const uint32_t *row, int x, int bits, const uint32_t *palette) {
    const int per = 8 >> bits;                                     // bits per index
    const uint32_t packed = (row[x >> bits] >> 8) & 255u;
    return palette[(packed >> ((x & ((1 << bits) - 1)) * per)) & ((1u << per) - 1u)];
}
