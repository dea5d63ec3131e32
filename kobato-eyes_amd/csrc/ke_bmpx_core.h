// ke_bmpx_core.h -- RLE, 1 / 4-bit and 16-bit BMP files: the arithmetic shared by the HIP kernels (ke_bmpx.hip) and the CPU build the
// tests hold against Pillow (tests/_bmpx_cpu.cpp).  Replaces `Image.open(path)` + pixel access of the reference's batch hasher
// (src/core/fastsig.py:31-34) for the BMP files ke_bmp_parse.h leaves out and ke_bmpx_parse.h takes.
//
// The RLE walk restates BmpImagePlugin.BmpRleDecoder.decode state for state -- Pillow is the yardstick, also where it departs
// from the format's description: the decoder appends to one linear buffer (`pos` = its length) and keeps a column `x`;
//   (n, v), n > 0      a run of n pixels of v (RLE4: the two nibbles of v in turn, the high one first), cut to max(0, W - x): a
//                      run that passes the row's end does not wrap, and later runs in that row write nothing;
//   (0, 0)             end of line: zeros up to the next multiple of W (none if pos is on one), x = 0;
//   (0, 1)             end of bitmap: the walk ends;
//   (0, 2, right, up)  right + up * W zeros, then x = pos % W; the walk ends if the two bytes are missing;
//   (0, n), n >= 3     absolute: RLE8 n bytes, RLE4 n / 2 bytes of two pixels each (an odd n yields n - 1 pixels) -- not cut to
//                      the row: it spills into the next one, and x += n grows past W; a short read ends the walk after its
//                      bytes; then one byte is skipped if the position IN THE FILE is odd.
// The walk runs while pos < W * H and ends at a missing byte.  pos < W * H at its end: Pillow raises "not enough image data"
// (CORRUPT); otherwise the first W * H entries are the picture, row r of them the picture's row H - 1 - r (r in a top-down
// file), and what lies beyond them is dropped.  The walker writes no pixel: it hands runs and literals, cut to W * H, to a sink.
//
// 16-bit pixels: Pillow's BGR;15 / BGR;16 unpackers expand a field of n bits as floor(v * 255 / (2^n - 1)).
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define KE_BMPX_HD __host__ __device__ __forceinline__
#define KE_BMPX_MEMBER __host__ __device__ __forceinline__
#else
#define KE_BMPX_HD static inline
#define KE_BMPX_MEMBER inline
#endif

enum { KE_BMPX_OK = 0, KE_BMPX_UNSUPPORTED = 1, KE_BMPX_CORRUPT = 2 };
// what a file's pixel data is
enum { KE_BMPX_RLE8 = 1, KE_BMPX_RLE4 = 2, KE_BMPX_P1 = 3, KE_BMPX_P4 = 4, KE_BMPX_RGB555 = 5, KE_BMPX_RGB565 = 6 };

// Src: byte(p) of the stream, p < n, asked in ascending order (not every p is asked for: a literal's bytes are stepped over).
// Sink: run(pos, len, v) -- len pixels of v from pos on; literal(pos, len, p) -- len pixels from the stream's bytes at p on.
// n: the bytes from the data offset to the file's end; abs0: the data offset (its parity decides the skip behind a literal).
template <typename Src, typename Sink>
KE_BMPX_HD int ke_bmpx_walk(Src &src, uint32_t n, uint32_t abs0, uint32_t W, uint32_t WH, bool rle4, Sink &sink) {
    uint32_t pos = 0, p = 0;
    uint64_t x = 0;
    while (pos < WH) {
        if (n - p < 2) break;
        const uint32_t a = src.byte(p), b = src.byte(p + 1);
        p += 2;
        if (a) {
            uint32_t num = a;
            if (x + num > W) num = x < W ? (uint32_t)(W - x) : 0;
            if (num) sink.run(pos, num < WH - pos ? num : WH - pos, b);
            pos += num;
            x += num;
        } else if (b == 0) {
            const uint32_t r = pos % W;
            if (r) pos += W - r;
            x = 0;
        } else if (b == 1) {
            break;
        } else if (b == 2) {
            if (n - p < 2) break;
            const uint32_t right = src.byte(p), up = src.byte(p + 1);
            p += 2;
            pos += right + up * W;
            x = pos % W;
        } else {
            const uint32_t count = rle4 ? b >> 1 : b;
            const uint32_t have = count < n - p ? count : n - p;
            const uint32_t pixels = rle4 ? 2 * have : have;
            if (pixels) sink.literal(pos, pixels < WH - pos ? pixels : WH - pos, p);
            pos += pixels;
            p += have;
            if (have < count) break;
            x += b;
            if (((abs0 + p) & 1u) && p < n) ++p;
        }
    }
    return pos >= WH ? KE_BMPX_OK : KE_BMPX_CORRUPT;
}

// The sink of ke_bmpx_codes, compiled for the host too (tests/_bmpx_cpu.cpp hands the records back): what the walk yields,
// written down for ke_bmpx_expand.  Every code of the stream is at least two bytes and yields at most one record, so a file has
// room for (bytes from the data offset on) / 2 of them; one more is counted, not written.
struct alignas(16) KeBmpxRec {
    uint32_t pos, len;                   // entries [pos, pos + len) of the walk's buffer, inside [0, W * H)
    uint32_t literal;                    // 0: a run of `arg`; 1: a literal whose bytes start at `arg` in the stream
    uint32_t arg;
};

struct KeBmpxRecSink {
    KeBmpxRec *rec;
    uint32_t nrec, max_rec;
    KE_BMPX_MEMBER void put(uint32_t pos, uint32_t len, uint32_t literal, uint32_t arg) {
        if (nrec < max_rec) {
            KeBmpxRec r;
            r.pos = pos; r.len = len; r.literal = literal; r.arg = arg;
            rec[nrec] = r;
        }
        ++nrec;
    }
    KE_BMPX_MEMBER void run(uint32_t pos, uint32_t len, uint32_t v) { put(pos, len, 0u, v); }
    KE_BMPX_MEMBER void literal(uint32_t pos, uint32_t len, uint32_t p) { put(pos, len, 1u, p); }
};

// pixel k of a run of v / of a literal whose bytes start at s
KE_BMPX_HD uint32_t ke_bmpx_run_index(uint32_t v, uint32_t k, bool rle4) { return rle4 ? (k & 1u ? v & 15u : v >> 4) : v; }
template <typename Bytes>
KE_BMPX_HD uint32_t ke_bmpx_literal_index(const Bytes &s, uint32_t k, bool rle4) {
    if (!rle4) return s[k];
    const uint32_t b = s[k >> 1];
    return k & 1u ? b & 15u : b >> 4;
}

// where entry i of the walk's buffer lies in the picture (bytes from the plane's start)
KE_BMPX_HD uint32_t ke_bmpx_place(uint32_t i, uint32_t W, uint32_t H, bool topdown) {
    const uint32_t r = i / W, c = i - r * W;
    return (topdown ? r : H - 1 - r) * W + c;
}

// index x of a stored 1-bit / 4-bit row: the most significant bit or nibble first
KE_BMPX_HD uint32_t ke_bmpx_p1(const uint8_t *row, uint32_t x) { return (row[x >> 3] >> (7 - (x & 7u))) & 1u; }
KE_BMPX_HD uint32_t ke_bmpx_p4(const uint8_t *row, uint32_t x) { return (row[x >> 1] >> (x & 1u ? 0 : 4)) & 15u; }

// a 16-bit pixel -> R | G << 8 | B << 16
KE_BMPX_HD uint32_t ke_bmpx_rgb16(uint32_t v, bool is565) {
    const uint32_t b = ((v & 31u) * 255u) / 31u;
    const uint32_t g = is565 ? (((v >> 5) & 63u) * 255u) / 63u : (((v >> 5) & 31u) * 255u) / 31u;
    const uint32_t r = is565 ? (((v >> 11) & 31u) * 255u) / 31u : (((v >> 10) & 31u) * 255u) / 31u;
    return r | (g << 8) | (b << 16);
}
