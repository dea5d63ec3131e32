// ke_lz_records.h -- the sink the two LZW walkers write through (ke_gif.hip, ke_tiffc.hip), one for both, and compiled for the
// host too (oracle/keyes_gif_cpu.cpp, tests/_tiffc_cpu.cpp: an entry each that hands the records back) so that the CPU tests
// hold its splitting: a literal goes to its place, a string that lies in the output already is recorded as copies for
// ke_lz_make_copies (ke_lz_copies.h, length bias 2) -- {destination, distance << 9 | (length - 2)} -- not made.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define KE_LZ_HD __host__ __device__ __forceinline__
typedef uint2 KeLzRec;
#else
#define KE_LZ_HD inline
struct KeLzRec { uint32_t x, y; };
#endif

constexpr uint32_t kKeLzMaxCopy = 511 + 2;        // the record's length field

struct KeLzRecSink {
    uint8_t *bytes;                               // the stream's output (a GIF frame's indices, a TIFF strip's plane)
    KeLzRec *rec;
    uint32_t out, nrec;
    KE_LZ_HD void literal(uint8_t b) { bytes[out++] = b; }
    KE_LZ_HD void copy(uint32_t from, uint32_t len) {
        const uint32_t dist = out - from;
        // A copied string has at least 2 characters; only the stream's last one can be cut to 1 -- it is recorded as 2, the
        // second byte lands in the slack behind the output.  Pieces of at most 513, none of them a single byte.
        if (len == 1) len = 2;
        while (len) {
            const uint32_t take = len > kKeLzMaxCopy ? (len - kKeLzMaxCopy == 1 ? kKeLzMaxCopy - 1 : kKeLzMaxCopy) : len;
            KeLzRec r;
            r.x = out;
            r.y = (dist << 9) | (take - 2);
            rec[nrec++] = r;
            out += take;
            len -= take;
        }
    }
};
