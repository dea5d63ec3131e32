// csrc/ke_ssim_plan.h without a GPU: the launch plan of the SSIM kernels over a sweep of shapes.
// tests/test_ssim_plan_cpu.py builds this file as a shared object (sp_plan_many runs the header on a list of widths and writes
// each plan out as ten int64 words; the test holds them against the rules written out again in Python) and, with
// -fsanitize=address,undefined, as a program: `main` walks the same sweep and checks what every plan must satisfy, whatever the
// rules make of it.
#include <cstdint>
#include <cstdio>

#include "ke_ssim_plan.h"

extern "C" {

// out[10 * i ..]: kernel, px, aligned, col_blocks, block_cols, band_rows, bands, items_per_pair, n_items, why
void sp_plan_many(const int32_t *w, int64_t n, int32_t h, int32_t channels, int64_t n_pairs, int32_t base_mod4, int32_t exact_mode,
                  int64_t *out) {
    for (int64_t i = 0; i < n; ++i) {
        const KeSsimPlan p = ke_ssim_plan(w[i], h, channels, n_pairs, base_mod4, exact_mode != 0);
        const int64_t words[10] = {p.kernel, p.px, p.aligned, p.col_blocks, p.block_cols, p.band_rows, p.bands, p.items_per_pair, p.n_items, p.why};
        for (int k = 0; k < 10; ++k) out[10 * i + k] = words[k];
    }
}

}  // extern "C"

#ifdef SSIM_PLAN_MAIN
namespace {

int64_t failures = 0;

void expect(bool ok, const char *what, int w, int h, int ch, int64_t pairs, int base, int exact) {
    if (ok) return;
    if (++failures <= 20) std::printf("%s: w %d h %d channels %d pairs %lld base %d exact %d\n", what, w, h, ch, (long long)pairs, base, exact);
}

}  // namespace

int main() {
    const int heights[] = {7, 8, 12, 13, 14, 20, 21, 69, 70, 71, 132, 133, 134, 512};
    const int64_t pair_counts[] = {1, 2, 39, 2048, 3200, 8192, 11700};
    const int chans[] = {1, 3, 4};
    int64_t plans = 0;
    for (int w = 1; w <= 3100; ++w)
        for (int h : heights)
            for (int ch : chans)
                for (int64_t pairs : pair_counts)
                    for (int base = 0; base < 4; ++base)
                        for (int exact = 0; exact < 2; ++exact) {
#define EXPECT(cond) expect((cond), #cond, w, h, ch, pairs, base, exact)
                            const KeSsimPlan p = ke_ssim_plan(w, h, ch, pairs, base, exact != 0);
                            ++plans;
                            if (w < 7) {
                                EXPECT(p.kernel == KE_SSIM_NAN && p.px == -1 && p.n_items == -1);
                                EXPECT(ke_ssim_plan(h, w, ch, pairs, base, exact != 0).kernel == KE_SSIM_NAN);
                                continue;
                            }
                            EXPECT(p.kernel == KE_SSIM_EXACT_KERNEL || p.kernel == KE_SSIM_FAST_KERNEL);
                            EXPECT(p.px == 4 || p.px == 8);
                            EXPECT(p.col_blocks >= 1 && (int64_t)(p.col_blocks - 1) * p.block_cols < w - 6 && w - 6 <= (int64_t)p.col_blocks * p.block_cols);
                            EXPECT(!p.aligned || p.block_cols % 4 == 0 || p.col_blocks == 1);
                            EXPECT(p.block_cols >= 1 && p.block_cols <= 64 * p.px - 6);
                            EXPECT(p.aligned == (p.why == KE_SSIM_AL_TAKEN) && p.why >= KE_SSIM_AL_TAKEN && p.why <= KE_SSIM_AL_BLOCKS);
                            EXPECT(!p.aligned || (w % 4 == 0 && base == 0));
                            if (p.kernel == KE_SSIM_FAST_KERNEL) EXPECT(p.band_rows % 7 == 0 && p.band_rows >= 14 && p.band_rows <= 126);
                            else EXPECT(p.band_rows == 64);
                            EXPECT(p.bands >= 1 && (int64_t)(p.bands - 1) * p.band_rows < h - 6 && h - 6 <= (int64_t)p.bands * p.band_rows);
                            EXPECT((int64_t)(w - 6) * (h - 6) >= 4096 || p.kernel == KE_SSIM_EXACT_KERNEL);
                            EXPECT(!exact || p.kernel == KE_SSIM_EXACT_KERNEL);
                            EXPECT(p.items_per_pair == p.col_blocks * p.bands && p.n_items == pairs * p.items_per_pair);
#undef EXPECT
                        }
    if (failures) {
        std::printf("%lld failures\n", (long long)failures);
        return 1;
    }
    std::printf("ok %lld\n", (long long)plans);
    return 0;
}
#endif
