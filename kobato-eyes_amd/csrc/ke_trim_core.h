// ke_trim_core.h -- the content box of a picture (include/keyes.h, ke_content_boxes) as pure functions, shared by the HIP
// kernels (ke_trim.hip) and by the host build the tests hold against the definition (tests/_trim_core_cpu.cpp).
//
// A pixel DIFFERS when max over c of |p[c] - ref[c]| > tolerance, ref = pixel (0, 0), the fourth byte of a 4-channel
// pixel ignored.  Per byte that is "p outside [lo, hi]", lo = max(ref - tol, 0), hi = min(ref + tol, 255), and the ignored
// byte has [0, 255].  A row is read as aligned 16-byte vectors of four dwords; the four bytes of a dword are tested at
// once in two halves of 16-bit fields (bytes 0, 2 and bytes 1, 3):  hi + 256 - p  keeps bit 8 iff p <= hi,  p + 256 - lo
// keeps bit 8 iff p >= lo, no borrow or carry crosses a field.  The channel of a dword's first byte is its PHASE; the
// bounds of a dword, spread into fields, are a KeTrimPat per phase, made once per image.
//
// Walking a row: a vector starts at byte p0 = 16 j - lead of the row (lead = the row's address & 15), so p0 may be
// negative and p0 + 16 may pass the row's end: ke_trim_range_mask cuts those bytes off.  The phase of dword k of that
// vector is (p0 + 4 k) mod channels; for 3 channels 4 = 16 = 64 * 16 = 1 (mod 3), so the phase goes up by one from dword
// to dword and from one 64-vector stride to the next, which is how the kernel turns three patterns round in registers.
#pragma once

#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define KE_TRIM_HD __host__ __device__ static inline
#else
#define KE_TRIM_HD static inline
#endif

// Rows of one work item (image, band of rows).  32: a 512 x 512 RGB image is 16 items of 48 KiB, one 4032 x 3024 image 95
// items, so a single large image still reaches a third of the chip's compute units and a batch of them all.
#define KE_TRIM_BAND_ROWS 32
#define KE_TRIM_VEC 16          // bytes of one aligned vector read
#define KE_TRIM_MIN_SIDE 8      // a box qualifies for a trimmed hash from this side up

#define KE_TRIM_FIELDS 0x00FF00FFu
#define KE_TRIM_BIT8 0x01000100u

struct KeTrimPat {
    uint32_t ae, be;   // bytes 0 and 2:  hi + 256,  256 - lo
    uint32_t ao, bo;   // bytes 1 and 3
};

// bounds of the four bytes of a dword whose first byte is channel `phase` (0 <= phase < ch)
KE_TRIM_HD KeTrimPat ke_trim_pat(const uint8_t ref[4], int tol, int ch, int phase) {
    uint32_t a[4], b[4];
    for (int i = 0; i < 4; ++i) {
        const int c = (phase + i) % ch;
        int lo = 0, hi = 255;
        if (c < 3) {
            const int r = c == 0 ? ref[0] : (c == 1 ? ref[1] : ref[2]);   // constant indices: the array stays in registers
            lo = r - tol < 0 ? 0 : r - tol;
            hi = r + tol > 255 ? 255 : r + tol;
        }
        a[i] = (uint32_t)(hi + 256);
        b[i] = (uint32_t)(256 - lo);
    }
    KeTrimPat p;
    p.ae = a[0] | a[2] << 16;
    p.be = b[0] | b[2] << 16;
    p.ao = a[1] | a[3] << 16;
    p.bo = b[1] | b[3] << 16;
    return p;
}

// which of the four bytes of x lie outside their bounds: bit i = byte i
KE_TRIM_HD uint32_t ke_trim_diff4(uint32_t x, KeTrimPat p) {
    const uint32_t xe = x & KE_TRIM_FIELDS, xo = (x >> 8) & KE_TRIM_FIELDS;
    const uint32_t in_e = (p.ae - xe) & (xe + p.be) & KE_TRIM_BIT8;      // bit 8 / 24: byte 0 / 2 inside
    const uint32_t in_o = (p.ao - xo) & (xo + p.bo) & KE_TRIM_BIT8;      // byte 1 / 3 inside
    const uint32_t out = ((in_e >> 8) | (in_o >> 7)) ^ 0x00030003u;      // bits 0, 1, 16, 17 = bytes 0, 1, 2, 3 outside
    return (out | out >> 14) & 0xFu;
}

// the bytes of a vector at row byte p0 that belong to a row of row_bytes: bit i = byte i
KE_TRIM_HD uint32_t ke_trim_range_mask(int64_t p0, int64_t row_bytes) {
    const int s = p0 < 0 ? (int)-p0 : 0;
    const int e = row_bytes - p0 < KE_TRIM_VEC ? (int)(row_bytes - p0) : KE_TRIM_VEC;
    if (e <= s) return 0;
    return ((1u << e) - 1u) & ~((1u << s) - 1u);
}

// The 16 bytes at a (a multiple of 16) as four little-endian dwords.  Only a vector that reaches outside the image's own
// bytes [s, s_end) -- the first and the last of an image -- is put together from the bytes inside; the rest of it is 0.
KE_TRIM_HD void ke_trim_load_vec(const uint8_t *a, const uint8_t *s, const uint8_t *s_end, uint32_t v[4]) {
    if (a >= s && a + KE_TRIM_VEC <= s_end) {
#ifdef __HIP_DEVICE_COMPILE__
        const uint4 q = *(const uint4 *)a;
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
#else
        memcpy(v, a, KE_TRIM_VEC);
#endif
        return;
    }
    for (int k = 0; k < 4; ++k) {
        uint32_t w = 0;
        for (int b = 0; b < 4; ++b)
            if (a + 4 * k + b >= s && a + 4 * k + b < s_end) w |= (uint32_t)a[4 * k + b] << (8 * b);
        v[k] = w;
    }
}

// running bounds of the differing bytes one lane saw: byte-in-row index and row index
struct KeTrimAcc {
    int32_t bmin, bmax, ymin, ymax;
};

KE_TRIM_HD KeTrimAcc ke_trim_acc_empty() {
    KeTrimAcc a;
    a.bmin = a.ymin = INT32_MAX;
    a.bmax = a.ymax = -1;
    return a;
}

KE_TRIM_HD int ke_trim_ctz(uint32_t m) {
#ifdef __HIP_DEVICE_COMPILE__
    return __ffs((int)m) - 1;
#else
    return __builtin_ctz(m);
#endif
}
KE_TRIM_HD int ke_trim_top(uint32_t m) {
#ifdef __HIP_DEVICE_COMPILE__
    return 31 - __clz((int)m);
#else
    return 31 - __builtin_clz(m);
#endif
}

// the differing bytes `mask` (bit i = byte i, already cut to the row) of the vector at row byte p0 of row y
KE_TRIM_HD void ke_trim_acc_vec(KeTrimAcc *a, uint32_t mask, int32_t p0, int32_t y) {
    if (!mask) return;
    const int32_t lo = p0 + ke_trim_ctz(mask), hi = p0 + ke_trim_top(mask);
    a->bmin = lo < a->bmin ? lo : a->bmin;
    a->bmax = hi > a->bmax ? hi : a->bmax;
    a->ymin = y < a->ymin ? y : a->ymin;
    a->ymax = y > a->ymax ? y : a->ymax;
}

KE_TRIM_HD void ke_trim_acc_merge(KeTrimAcc *a, KeTrimAcc b) {
    a->bmin = b.bmin < a->bmin ? b.bmin : a->bmin;
    a->bmax = b.bmax > a->bmax ? b.bmax : a->bmax;
    a->ymin = b.ymin < a->ymin ? b.ymin : a->ymin;
    a->ymax = b.ymax > a->ymax ? b.ymax : a->ymax;
}

// One vector of a row: the differing bytes of v (dword k tested against pat[k]), cut to the row, into the lane's bounds.
KE_TRIM_HD void ke_trim_vec(KeTrimAcc *a, const uint32_t v[4], KeTrimPat p0, KeTrimPat p1, KeTrimPat p2, KeTrimPat p3, int32_t at,
                            int32_t row_bytes, int32_t y) {
    const uint32_t m = ke_trim_diff4(v[0], p0) | ke_trim_diff4(v[1], p1) << 4 | ke_trim_diff4(v[2], p2) << 8 | ke_trim_diff4(v[3], p3) << 12;
    ke_trim_acc_vec(a, m & ke_trim_range_mask(at, row_bytes), at, y);
}

// bounds of differing bytes -> box (x0, y0, x1, y1); four zeros when no byte differed.  The one division by channels.
KE_TRIM_HD void ke_trim_box(KeTrimAcc a, int ch, int32_t box[4]) {
    if (a.ymax < 0) {
        box[0] = box[1] = box[2] = box[3] = 0;
        return;
    }
    box[0] = a.bmin / ch;
    box[1] = a.ymin;
    box[2] = a.bmax / ch + 1;
    box[3] = a.ymax + 1;
}

KE_TRIM_HD int ke_trim_bands(int h) { return (h + KE_TRIM_BAND_ROWS - 1) / KE_TRIM_BAND_ROWS; }

// phase of the vector at row byte `at` (>= -15): the channel of its first byte
KE_TRIM_HD int ke_trim_phase(int32_t at, int ch) { return (int)((at + 48) % ch); }

// A box qualifies for a trimmed hash when it exists, both sides are at least KE_TRIM_MIN_SIDE, and it cuts at least 2 %
// off one axis -- a one-pixel trim would only double the plain hash's edges.
KE_TRIM_HD int ke_trim_qualifies(int w, int h, const int32_t box[4]) {
    const int64_t bw = (int64_t)box[2] - box[0], bh = (int64_t)box[3] - box[1];
    if (bw <= 0 || bh <= 0) return 0;
    if (bw < KE_TRIM_MIN_SIDE || bh < KE_TRIM_MIN_SIDE) return 0;
    return ((int64_t)w - bw) * 50 >= w || ((int64_t)h - bh) * 50 >= h;
}
