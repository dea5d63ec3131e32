// ke_tiffc_core.h -- compressed TIFF: the stream arithmetic shared by the HIP kernels (ke_tiffc.hip) and the CPU build the tests
// hold against Pillow (tests/_tiffc_cpu.cpp).  Replaces `Image.open(path)` + pixel access of the reference's batch hasher
// (src/core/fastsig.py:31-34) for the strips of LZW (Compression 5) and PackBits (32773) files, which Pillow hands to libtiff.
// Every strip is a stream of its own: it yields the `want` = rows x width x samples bytes of its rows, before the predictor.
//
// LZW as libtiff's LZWDecode reads it: codes MSB-first, 9 to 12 bits; 256 clears the table, 257 ends the data, 258 is the
// first free code; the width grows "early" -- when the next free code reaches 511, 1023, 2047; a code needs all its bits
// inside the strip's bytes; the strip is over when it has yielded its bytes, whatever follows.  A code beyond the next free
// one, the end code or the end of the bytes before the last byte is out: libtiff fails the strip (Pillow raises), CORRUPT
// here.  Two things libtiff decodes are left to it (UNSUPPORTED): a strip that does not open with a clear code (libtiff
// starts from a phantom previous string) and codes that go on after the table's last entry, 4095, without a clear code
// (libtiff allows 1 024 more).  A dictionary entry is kept as in ke_gif_core.h: (where its string was last written, its
// length) -- the string of a new entry is the previous string plus the first character of the current one, and those lie next
// to each other in the output, so expanding a code is a copy from earlier output.
//
// PackBits as libtiff's PackBitsDecode reads it, a whole strip at a time (runs may cross rows): a header n in 0..127 is n + 1
// literal bytes, -127..-1 the next byte 1 - n times, -128 nothing.  A run or a literal that would pass the strip's last byte is
// cut there (libtiff warns and does the same); bytes that end before the strip is full: CORRUPT.
//
// Predictor 2 (horizontal differencing, 8-bit): per row and per sample a running sum modulo 256, stride = samples per pixel.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define KE_TIFFC_HD __host__ __device__ __forceinline__
#else
#define KE_TIFFC_HD static inline
#endif

enum { KE_TIFFC_OK = 0, KE_TIFFC_UNSUPPORTED = 1, KE_TIFFC_CORRUPT = 2 };
enum { KE_TIFFC_LZW = 5, KE_TIFFC_PACKBITS = 32773 };
enum { KE_TIFFC_MAX_STRIP = 1 << 23 };     // bytes a strip yields: a copy's distance has 23 bits in the record (ke_lz_copies.h)

// Src: byte(pos) of the strip, asked for ascending positions below `end`.  Dict: set(code, pos, len), get(code, pos, len).
// Sink: literal(byte), copy(from, len) -- both append.
template <typename Src, typename Dict, typename Sink>
KE_TIFFC_HD int ke_tiffc_lzw(Src &src, uint32_t pos, uint32_t end, uint32_t want, Dict &dict, Sink &sink) {
    uint32_t next = 258, nbits = 9;
    uint32_t bitbuf = 0, bitcount = 0;
    uint32_t out = 0, last_pos = 0, last_len = 0;
    bool fresh = false, opened = false;     // fresh: the next code is the first after a clear code
    while (out < want) {
        while (bitcount < nbits) {
            if (pos >= end) return KE_TIFFC_CORRUPT;               // libtiff: "not terminated with EOI code"
            bitbuf = (bitbuf << 8) | src.byte(pos++);
            bitcount += 8;
        }
        const uint32_t c = (bitbuf >> (bitcount - nbits)) & ((1u << nbits) - 1u);
        bitcount -= nbits;
        if (c == 256) {
            next = 258;
            nbits = 9;
            fresh = opened = true;
            continue;
        }
        if (!opened) return KE_TIFFC_UNSUPPORTED;
        if (c == 257) return KE_TIFFC_CORRUPT;                     // "Not enough data at scanline"
        const uint32_t at = out;
        uint32_t len = 1;
        if (fresh) {
            if (c > 257) return KE_TIFFC_CORRUPT;
            sink.literal((uint8_t)c);
            fresh = false;
        } else {
            if (next >= 4096) return KE_TIFFC_UNSUPPORTED;
            if (c < 256) {
                sink.literal((uint8_t)c);
            } else {
                if (c > next) return KE_TIFFC_CORRUPT;             // "Using code not yet in table"
                uint32_t from = last_pos;
                len = last_len + 1;
                if (c != next) dict.get(c, from, len);
                const uint32_t take = len < want - out ? len : want - out;
                sink.copy(from, take);
            }
            dict.set(next, last_pos, last_len + 1);
            ++next;
            if (next == (1u << nbits) - 1u && nbits < 12) ++nbits;
        }
        last_pos = at;
        last_len = len;
        out += len;
    }
    return KE_TIFFC_OK;
}

template <typename Src, typename Sink>
KE_TIFFC_HD int ke_tiffc_packbits(Src &src, uint32_t pos, uint32_t end, uint32_t want, Sink &sink) {
    uint32_t out = 0;
    while (pos < end && out < want) {
        const uint32_t h = src.byte(pos++);
        if (h == 128) continue;
        if (h > 128) {
            uint32_t run = 257 - h;
            if (run > want - out) run = want - out;
            if (pos >= end) break;
            const uint8_t b = (uint8_t)src.byte(pos++);
            sink.literal(b);
            if (run == 2) sink.literal(b);
            else if (run > 2) sink.copy(out, run - 1);             // the byte just written, repeated: a copy at distance 1
            out += run;
        } else {
            uint32_t n = h + 1;
            if (n > want - out) n = want - out;
            if (end - pos < n) break;
            for (uint32_t k = 0; k < n; ++k) sink.literal((uint8_t)src.byte(pos++));
            out += n;
        }
    }
    return out == want ? KE_TIFFC_OK : KE_TIFFC_CORRUPT;           // "Not enough data for scanline"
}

// bytes of four samples added lane by lane, each modulo 256
KE_TIFFC_HD uint32_t ke_tiffc_add4(uint32_t a, uint32_t b) { return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u); }
