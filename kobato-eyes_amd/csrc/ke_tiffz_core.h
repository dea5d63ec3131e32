// ke_tiffz_core.h -- the one piece of arithmetic the decoder of deflate TIFF files (ke_tiffz.hip) does not take from the PNG path
// (ke_png_core.h: ke_inflate_zlib) or from the LZW / PackBits one (ke_tiffc_core.h): the Adler-32 (RFC 1950) of a strip's plane
// summed by the 64 lanes of one wave, in 32-bit words.  Compiled for the host too (tests/_tiffz_cpu.cpp), where the lanes are a
// loop, and held against zlib there at the lengths at which a 32-bit sum first overflows.
//
//   adler = s2 << 16 | s1,   s1 = 1 + sum of b[j],   s2 = n + sum of (n - j) * b[j]   (mod 65521, j = 0 .. n-1)
//
// Lane l takes the 16-byte chunks l, l + 64, ...: per chunk the sum S of its bytes (<= 4 080) and the sum of k * b[k] over its
// 16 places (<= 30 600).  (n - j) is carried modulo 65521 -- it goes down by 1 024 per step --, so a term (n - j0) * S stays
// below 2^28 and eight of them fit a 32-bit word: the weighted sum is reduced every eighth step.  The two plain sums cannot
// overflow: a strip yields at most KE_TIFFC_MAX_STRIP = 2^23 bytes, 8 192 chunks per lane.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define KE_TIFFZ_HD __host__ __device__ __forceinline__
#else
#define KE_TIFFZ_HD static inline
#endif

enum { KE_TIFFZ_ADLER_MOD = 65521 };

struct KeTiffzAdlerLane { uint32_t s1, s2; };      // this lane's share of the two sums, each below 65521

// p: the plane, readable in whole 16-byte chunks up to the chunk that holds byte n - 1 (bytes at n and beyond are masked out)
KE_TIFFZ_HD KeTiffzAdlerLane ke_tiffz_adler_lane(const uint8_t *p, uint32_t n, uint32_t lane) {
    const uint32_t M = KE_TIFFZ_ADLER_MOD;
    uint32_t a = 0, c = 0, s2 = 0, step = 0;
    uint32_t j0 = 16 * lane;
    uint32_t w = j0 < n ? (n - j0) % M : 0;               // (n - j0) mod 65521
    for (; j0 < n; j0 += 1024, ++step) {
        uint32_t x[4];
        __builtin_memcpy(x, p + j0, 16);
        const uint32_t have = n - j0;                       // bytes of this chunk inside the plane
        uint32_t sum = 0, weighted = 0;
        for (int q = 0; q < 4; ++q) {
            const uint32_t left = have > 4u * q ? have - 4u * q : 0u;
            const uint32_t v = left >= 4 ? x[q] : left == 0 ? 0u : (x[q] & ((1u << (8 * left)) - 1u));
            const uint32_t b0 = v & 255u, b1 = (v >> 8) & 255u, b2 = (v >> 16) & 255u, b3 = v >> 24;
            const uint32_t s = b0 + b1 + b2 + b3;
            sum += s;
            weighted += 4u * q * s + b1 + 2 * b2 + 3 * b3;
        }
        a += sum;
        c += weighted;
        s2 += w * sum;
        if ((step & 7) == 7) s2 %= M;
        w = w >= 1024 ? w - 1024 : w + M - 1024;
    }
    KeTiffzAdlerLane r;
    r.s1 = a % M;
    r.s2 = (s2 % M + M - c % M) % M;
    return r;
}

// s1, s2: the lanes' shares added up (64 values below 65521 each)
KE_TIFFZ_HD uint32_t ke_tiffz_adler_join(uint32_t n, uint32_t s1, uint32_t s2) {
    const uint32_t M = KE_TIFFZ_ADLER_MOD;
    return (((n % M + s2) % M) << 16) | ((1u + s1) % M);
}
