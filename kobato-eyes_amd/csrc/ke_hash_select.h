// Which single-pass hash kernel a shape gets: the one table of the kernels' instantiations, and the pure function that
// lists the rows to try for a shape, in order.  No HIP, no context, no device: ke_hash.hip expands the same list a
// second time to attach each row's kernel, and a host-only program can include this file to see what a shape is given.
#pragma once
#include <cstdint>

enum { KE_SP_MX = 0, KE_SP_WIDE = 1 };   // ke_phash_fused_mx: 256 threads, 32-row tiles; ke_phash_fused_wide: 512 threads, 16-row tiles

// Operand steps (64 pixels each) of the narrow kernel per 64-pixel bucket of the row length: KS of W64.
constexpr int kKeMxSteps[13] = {0, 0, 2, 2, 3, 3, 4, 5, 5, 6, 6, 7, 8};

// X(family, six template arguments in the kernel's order, first width, last width)
//   mx   <W64, KS, DH, GEN, C, UNAL>     wide <KSH, QPT, DH, KDW, C, UNAL>
// C: bytes per pixel.  UNAL: rows that do not end on a 4-pixel boundary (RGB, pHash leg only).  DH: both hashes in one
// pass over the pixels.  Within a family and a (C, UNAL, DH) the first row in list order that takes the width is the one.
#define KE_MX_GEN(X, B, DH, C, UNAL) X(mx, B, kKeMxSteps[B], DH, true, C, UNAL, 64 * (B - 1) + 1, 64 * B)   // run-time row length
#define KE_MX_EXACT(X, B, KS, DH) X(mx, B, KS, DH, false, 3, false, 64 * B, 64 * B)                          // compile-time row length
#define KE_MX_GEN_2_8(X, DH, C, UNAL) \
    KE_MX_GEN(X, 2, DH, C, UNAL) KE_MX_GEN(X, 3, DH, C, UNAL) KE_MX_GEN(X, 4, DH, C, UNAL) KE_MX_GEN(X, 5, DH, C, UNAL) \
    KE_MX_GEN(X, 6, DH, C, UNAL) KE_MX_GEN(X, 7, DH, C, UNAL) KE_MX_GEN(X, 8, DH, C, UNAL)
#define KE_MX_GEN_2_10(X, C, UNAL) KE_MX_GEN_2_8(X, false, C, UNAL) KE_MX_GEN(X, 9, false, C, UNAL) KE_MX_GEN(X, 10, false, C, UNAL)
#define KE_WIDE_TO_2048(X, DH, KDW3, KDW4, KDW5, C) \
    X(wide, 3, 8, DH, KDW3, C, false, 65, 1024) X(wide, 4, 12, DH, KDW4, C, false, 1025, 1536) X(wide, 5, 16, DH, KDW5, C, false, 1537, 2048)

#define KE_SINGLE_PASS_ROWS(X) \
    /* RGB rows that do not end on a 4-pixel boundary, up to 704 pixels; then the wide kernel up to 1024.  Wider ones */ \
    /* stay on the banded kernel (funnel-shift loader): measured 3.9 TB/s here at 1599 pixels against 5.3 there */ \
    KE_MX_GEN_2_10(X, 3, true) KE_MX_GEN(X, 11, false, 3, true) \
    X(wide, 3, 8, false, 1, 3, true, 65, 1024) \
    /* RGB, pHash + dHash, rows up to 512 pixels: widths with their own instantiation, then any other multiple of 4 */ \
    KE_MX_EXACT(X, 4, 3, true) KE_MX_EXACT(X, 6, 4, true) KE_MX_EXACT(X, 8, 5, true) \
    KE_MX_GEN_2_8(X, true, 3, false) \
    /* RGB, pHash alone; 768 has its own step count, and 708..764 have no row: 8 operand steps do not fit the register */ \
    /* file beside the pixel loads */ \
    KE_MX_EXACT(X, 4, 3, false) KE_MX_EXACT(X, 6, 4, false) KE_MX_EXACT(X, 8, 5, false) KE_MX_EXACT(X, 10, 6, false) \
    KE_MX_EXACT(X, 12, 7, false) \
    KE_MX_GEN_2_10(X, 3, false) KE_MX_GEN(X, 11, false, 3, false) \
    /* 1-byte pixels: the luma step is a sign flip, 4-byte loads */ \
    KE_MX_GEN_2_10(X, 1, false) KE_MX_GEN(X, 11, false, 1, false) KE_MX_GEN(X, 12, false, 1, false) \
    /* RGBX / RGBA rows, up to 640 pixels */ \
    KE_MX_GEN_2_10(X, 4, false) \
    /* wide rows, both hashes in one pass (RGB) */ \
    KE_WIDE_TO_2048(X, true, 2, 3, 4, 3) \
    /* wide rows, pHash alone; RGB goes on to 2816 (2560x1440-class rows: below the strip kernel's range) */ \
    KE_WIDE_TO_2048(X, false, 1, 1, 1, 4) \
    KE_WIDE_TO_2048(X, false, 1, 1, 1, 1) \
    KE_WIDE_TO_2048(X, false, 1, 1, 1, 3) X(wide, 6, 20, false, 1, 3, false, 2049, 2560) X(wide, 7, 22, false, 1, 3, false, 2561, 2816)

struct KeSpRow {
    int family;
    int t[6];          // the template arguments, in the kernel's order
    int w_lo, w_hi;    // row lengths the instantiation takes
    int channels() const { return t[4]; }
    bool unal() const { return t[5] != 0; }
    bool dh() const { return t[2] != 0; }
};

#define KE_SP_ROW_mx KE_SP_MX
#define KE_SP_ROW_wide KE_SP_WIDE
#define KE_SP_ROW(F, A0, A1, A2, A3, A4, A5, LO, HI) {KE_SP_ROW_##F, {A0, A1, A2, A3, A4, A5}, LO, HI},
constexpr KeSpRow kKeSpRows[] = {KE_SINGLE_PASS_ROWS(KE_SP_ROW)};
#undef KE_SP_ROW
constexpr int kKeSpRowCount = (int)(sizeof(kKeSpRows) / sizeof(kKeSpRows[0]));

// What the choice depends on.  base_dword: the group's base pointer is a multiple of 4; stride_dword: the group has an
// offset array, or its stride is a multiple of 4; misaligned: some image of a ragged group does not start on a dword
// boundary (the callers check every offset); band_plan: the kernels run per band of rows, not one workgroup per image.
struct KeSpShape {
    int w, h, channels;
    bool misaligned, base_dword, stride_dword;
    bool want_d, band_plan;
};

constexpr int kKeSpMaxCandidates = 4;

// Taller than 100 widths: from there Pillow's Image.resize shrinks vertically first, where the target is shorter
inline bool ke_taller_than_100_widths(int w, int h) { return (int64_t)h > (int64_t)w * 100; }

// The rows (indices into kKeSpRows) to try for a shape, in order; 0 when no single-pass kernel takes it.  The caller
// launches the first row that does not decline (KE_EUNSUPPORTED: coefficient tables or LDS needs beyond the row).  A
// row with DH covers both hashes; the others leave dHash to the caller.
inline int ke_single_pass_candidates(const KeSpShape &s, int out[kKeSpMaxCandidates]) {
    const int w = s.w, h = s.h, c = s.channels;
    const bool unal = w % 4 != 0;                  // rows that do not end on a 4-pixel boundary: RGB, pHash leg only
    if (s.misaligned) return 0;                    // the banded funnel-shift loader takes such a group
    if (w <= 64 || w > (unal ? 1024 : c == 3 ? 2816 : 2048) || h == 32 || h < 16 || (unal && c != 3) ||
        (!s.band_plan && h > 4096) || ke_taller_than_100_widths(w, h) || (!unal && (!s.base_dword || !s.stride_dword)) ||
        (int64_t)w * h * c >= (1LL << 31))
        return 0;
    const bool both = s.want_d && h != 8 && c == 3 && !unal;
    int n = 0;
    auto add = [&](int family, bool dh) {          // the family's row for this shape, if it has one
        for (int r = 0; r < kKeSpRowCount; ++r) {
            const KeSpRow &row = kKeSpRows[r];
            if (row.family == family && row.dh() == dh && row.channels() == c && row.unal() == unal && w >= row.w_lo && w <= row.w_hi) {
                out[n++] = r;
                return true;
            }
        }
        return false;
    };
    // the wide kernel takes what the narrow one leaves: rows above its reach, and unaligned rows after it
    const bool wide = unal || w > (c == 4 ? 640 : c == 1 ? 768 : both ? 512 : 704);
    if (both) {                                    // pHash + dHash in one pass over the pixels
        // when both legs do not fit one workgroup per image the call ends here: per band they do (one pass)
        if ((add(KE_SP_MX, true) || (wide && add(KE_SP_WIDE, true))) && !s.band_plan) return n;
    }
    // both hashes of RGB rows of 516..768 pixels: the wide kernel has a dHash leg for them, the narrow one does not; it
    // comes last, for pHash alone, when the wide kernel could not take the rows (LDS)
    const bool narrow_last = both && w > 512;
    if (!narrow_last) add(KE_SP_MX, false);
    if (wide) add(KE_SP_WIDE, false);
    if (narrow_last) add(KE_SP_MX, false);
    return n;
}
