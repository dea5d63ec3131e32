// csrc/ke_trim_core.h without a GPU: the content box of a picture, driven by host loops the way ke_content_boxes_kernel
// walks -- band by band, a wave per row, a lane per aligned 16-byte vector, three patterns turned round from vector to
// vector.  tests/test_trim_core_cpu.py builds this file as a shared object (the tr_* functions, held against the NumPy
// definition and the Pillow recipe) and, with -fsanitize=address,undefined, as a program: `main` runs the same sweep against
// the definition spelled out here, with every buffer ending exactly where its picture ends.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ke_trim_core.h"

extern "C" {

int tr_band_rows() { return KE_TRIM_BAND_ROWS; }

int tr_qualifies(int w, int h, const int32_t *box) { return ke_trim_qualifies(w, h, box); }

// The kernel's walk.  px may start on any byte.  Returns the number of faults: a vector that reaches outside the picture's
// bytes and is neither the first nor the last vector of the picture (the aligned vectors that hold its first and last byte).
int64_t tr_content_box(const uint8_t *px, int w, int h, int ch, int tol, int32_t *box) {
    const uint8_t *s = px, *s_end = px + (size_t)w * h * ch;
    const uint8_t *v_first = s - ((uintptr_t)s & (KE_TRIM_VEC - 1)), *v_last = s_end - 1 - ((uintptr_t)(s_end - 1) & (KE_TRIM_VEC - 1));
    const int32_t row_bytes = w * ch;
    uint8_t ref[4] = {0, 0, 0, 0};
    for (int c = 0; c < ch; ++c) ref[c] = s[c];
    KeTrimPat pats[4];
    for (int t = 0; t < 4; ++t) pats[t] = ke_trim_pat(ref, tol, ch, t % ch);
    int64_t faults = 0;
    int32_t g[4] = {INT32_MAX, INT32_MAX, 0, 0};                    // the image's box in global memory
    for (int band = 0; band < ke_trim_bands(h); ++band) {
        const int y0 = band * KE_TRIM_BAND_ROWS, y1 = y0 + KE_TRIM_BAND_ROWS < h ? y0 + KE_TRIM_BAND_ROWS : h;
        std::vector<KeTrimAcc> acc(256, ke_trim_acc_empty());       // a lane's registers
        for (int wave = 0; wave < 4; ++wave)
            for (int y = y0 + wave; y < y1; y += 4) {
                const uint8_t *row = s + (size_t)y * row_bytes;
                const int lead = (int)((uintptr_t)row & (KE_TRIM_VEC - 1));
                const int nv = (lead + row_bytes + KE_TRIM_VEC - 1) / KE_TRIM_VEC;
                for (int lane = 0; lane < 64 && lane < nv; ++lane) {
                    const int f0 = ke_trim_phase(KE_TRIM_VEC * lane - lead, ch);
                    KeTrimPat p0 = pats[f0], p1 = pats[(f0 + 4) % ch], p2 = pats[(f0 + 8) % ch];
                    for (int j = lane; j < nv; j += 64) {
                        const int32_t at = KE_TRIM_VEC * j - lead;
                        const uint8_t *a = row + at;
                        if ((a < s || a + KE_TRIM_VEC > s_end) && a != v_first && a != v_last) ++faults;
                        uint32_t v[4];
                        ke_trim_load_vec(a, s, s_end, v);
                        ke_trim_vec(&acc[(size_t)(wave * 64 + lane)], v, p0, p1, p2, p0, at, row_bytes, y);
                        if (ch == 3) {
                            const KeTrimPat t = p0;
                            p0 = p1; p1 = p2; p2 = t;
                        }
                    }
                }
            }
        KeTrimAcc all = ke_trim_acc_empty();
        for (const KeTrimAcc &a : acc) ke_trim_acc_merge(&all, a);
        if (all.ymax >= 0) {                                         // the item's four atomics
            int32_t b[4];
            ke_trim_box(all, ch, b);
            g[0] = b[0] < g[0] ? b[0] : g[0];
            g[1] = b[1] < g[1] ? b[1] : g[1];
            g[2] = b[2] > g[2] ? b[2] : g[2];
            g[3] = b[3] > g[3] ? b[3] : g[3];
        }
    }
    if (g[2] == 0) g[0] = g[1] = 0;
    memcpy(box, g, sizeof g);
    return faults;
}

}  // extern "C"

#ifdef TRIM_CORE_MAIN
// the definition, pixel by pixel
static void box_by_definition(const uint8_t *px, int w, int h, int ch, int tol, int32_t box[4]) {
    int x0 = w, y0 = h, x1 = 0, y1 = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int most = 0;
            for (int c = 0; c < ch && c < 3; ++c) {
                const int d = abs((int)px[((size_t)y * w + x) * ch + c] - (int)px[c]);
                most = d > most ? d : most;
            }
            if (most > tol) {
                x0 = x < x0 ? x : x0;
                y0 = y < y0 ? y : y0;
                x1 = x + 1 > x1 ? x + 1 : x1;
                y1 = y + 1 > y1 ? y + 1 : y1;
            }
        }
    box[0] = x1 ? x0 : 0;
    box[1] = x1 ? y0 : 0;
    box[2] = x1;
    box[3] = x1 ? y1 : 0;
}

int main() {
    const int B = KE_TRIM_BAND_ROWS;
    const int widths[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 21, 22, 43}, heights[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, B - 1, B, B + 1, 2 * B + 3};
    const int tols[] = {0, 1, 48, 254, 255};
    uint32_t seed = 20261020u;
    auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    long cases = 0;
    for (int w : widths)
        for (int h : heights)
            for (int ch : {1, 3, 4})
                for (int align = 0; align < 16; ++align) {
                    // the picture ends where its allocation ends, and starts `align` past a multiple of 16
                    const size_t bytes = (size_t)w * h * ch, pad = (size_t)align;
                    uint8_t *base = (uint8_t *)malloc(pad + bytes);
                    uint8_t *px = base + pad;
                    if (((uintptr_t)px & 15) != (uintptr_t)align) { printf("alignment %d not reached\n", align); return 1; }
                    // a border within the tolerance of its corner, content anywhere inside a random rectangle
                    const int rx0 = (int)(next() % (unsigned)w), ry0 = (int)(next() % (unsigned)h);
                    const int rx1 = rx0 + 1 + (int)(next() % (unsigned)(w - rx0)), ry1 = ry0 + 1 + (int)(next() % (unsigned)(h - ry0));
                    uint8_t bg[4] = {(uint8_t)next(), (uint8_t)next(), (uint8_t)next(), (uint8_t)next()};
                    for (int y = 0; y < h; ++y)
                        for (int x = 0; x < w; ++x)
                            for (int c = 0; c < ch; ++c) {
                                uint8_t *p = px + ((size_t)y * w + x) * ch + c;
                                if (x >= rx0 && x < rx1 && y >= ry0 && y < ry1 && next() % 3 == 0) {
                                    *p = (uint8_t)next();
                                } else {
                                    int v = bg[c] + (int)(next() % 3) - 1;          // the corner's colour, +-1
                                    *p = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
                                }
                            }
                    for (int tol : tols) {
                        int32_t got[4], want[4];
                        if (tr_content_box(px, w, h, ch, tol, got) != 0) { printf("a vector outside the picture: %dx%dx%d align %d\n", w, h, ch, align); return 1; }
                        box_by_definition(px, w, h, ch, tol, want);
                        if (memcmp(got, want, sizeof got) != 0) {
                            printf("%dx%dx%d align %d tol %d: got (%d, %d, %d, %d), want (%d, %d, %d, %d)\n", w, h, ch, align, tol, got[0], got[1], got[2],
                                   got[3], want[0], want[1], want[2], want[3]);
                            return 1;
                        }
                        ++cases;
                    }
                    free(base);
                }
    printf("ok %ld\n", cases);
    return 0;
}
#endif
