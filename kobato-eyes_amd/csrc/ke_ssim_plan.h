// ke_ssim_plan.h -- how ke_launch_ssim (ke_ssim.hip) cuts a launch of SSIM pairs into waves: a pure host function of the
// shape, so that it compiles with any C++ compiler and is tested without a GPU (tests/test_ssim_plan_cpu.py).
//
// One wave scores one (pair, column block, row band).  A lane owns px = 4 or 8 neighbouring columns, so a wave spans 64*px
// columns of which 64*px - 6 are interior ones (a 7x7 window needs 3 columns on either side): 250 or 506.
//   px         the choice that leaves the fewest idle lanes: 8 iff ceil((w-6)/506) * 506 < ceil((w-6)/250) * 250 (ties -> 4,
//              which holds two waves per SIMD more easily)
//   aligned    the loader that reads whole dwords needs dword-aligned quads of pixels: the width a multiple of 4, the image
//              base and the image size multiples of 4, and every block starting on a multiple of 4 -- one block, or blocks of
//              248 / 504 columns where those do not add a block.  Otherwise the funnel-shift loader reads any alignment.
//   kernel     images of fewer than 4096 windows always take the exact kernel: skimage's float32 intermediates can be off by
//              up to ~1e-4 in a single window of a bright, nearly flat image (uxx - ux*ux cancels); over thousands of windows
//              that averages far below 1e-5, in a 7x7 image (one window) it is the whole score, and such images cost nothing
//              either way.  So does every image in exact mode (ke_ssim_set_mode); the others take the fast kernel.  A side
//              under 7 has no window: NaN.
//   band_rows  exact: 64 interior rows per wave.  Fast: rows are taken seven at a time, so a band is 7*G interior rows, G as
//              large as leaves about 8 waves per SIMD of work in the launch (each band re-reads 6 halo rows) within 2..18,
//              then lowered to the smallest G >= 2 that needs no more bands (the bands come out equal).
#pragma once

#include <cstdint>

enum { KE_SSIM_NAN = 0, KE_SSIM_EXACT_KERNEL = 1, KE_SSIM_FAST_KERNEL = 2 };
// why the aligned loader was or was not taken
enum { KE_SSIM_AL_TAKEN = 0, KE_SSIM_AL_WIDTH = 1, KE_SSIM_AL_BASE = 2, KE_SSIM_AL_BLOCKS = 3 };
// the words of ke_last_ssim_plan
enum { KE_SP_KERNEL = 0, KE_SP_PX, KE_SP_ALIGNED, KE_SP_COL_BLOCKS, KE_SP_BLOCK_COLS, KE_SP_BAND_ROWS, KE_SP_BANDS, KE_SP_WHY, KE_SP_COUNT };

constexpr int kSsimExactBandRows = 64;     // interior rows per wave of the exact kernel
constexpr int kSsimMinFastWindows = 4096;  // fewer windows: the exact kernel whatever the mode

struct KeSsimPlan {
    int kernel = KE_SSIM_NAN;
    int px = -1, aligned = -1;             // everything below: -1 for KE_SSIM_NAN
    int col_blocks = -1, block_cols = -1;  // blocks of interior columns and their width
    int band_rows = -1, bands = -1;        // interior rows per wave and bands per image
    int items_per_pair = -1;               // col_blocks * bands waves per pair
    int64_t n_items = -1;                  // waves in the launch
    int why = -1;                          // KE_SSIM_AL_*
};

// base_mod4: the address of the first image modulo 4.  exact_mode: ke_ssim_set_mode(KE_SSIM_EXACT).
inline KeSsimPlan ke_ssim_plan(int w, int h, int channels, int64_t n_pairs, int base_mod4, bool exact_mode) {
    KeSsimPlan p;
    if (w < 7 || h < 7) return p;          // skimage raises for images smaller than the window
    const int cb4 = (w - 6 + 249) / 250, cb8 = (w - 6 + 505) / 506;
    p.px = ((int64_t)cb8 * 506 < (int64_t)cb4 * 250) ? 8 : 4;
    p.col_blocks = p.px == 8 ? cb8 : cb4;
    p.block_cols = 64 * p.px - 6;
    p.why = w % 4 != 0 ? KE_SSIM_AL_WIDTH : (base_mod4 != 0 || ((uint64_t)w * (uint64_t)h * (uint64_t)channels) % 4 != 0) ? KE_SSIM_AL_BASE : KE_SSIM_AL_TAKEN;
    if (p.why == KE_SSIM_AL_TAKEN && p.col_blocks > 1) {
        const int bca = p.block_cols & ~3;
        if ((w - 6 + bca - 1) / bca == p.col_blocks) p.block_cols = bca; else p.why = KE_SSIM_AL_BLOCKS;
    }
    p.aligned = p.why == KE_SSIM_AL_TAKEN;
    const bool exact = exact_mode || (int64_t)(w - 6) * (h - 6) < kSsimMinFastWindows;
    p.kernel = exact ? KE_SSIM_EXACT_KERNEL : KE_SSIM_FAST_KERNEL;
    p.band_rows = kSsimExactBandRows;
    if (!exact) {
        const int64_t groups_total = (h - 6 + 6) / 7;
        int64_t G = groups_total * n_pairs * p.col_blocks / 8192;
        G = G < 2 ? 2 : G > 18 ? 18 : G;
        const int64_t nb = (groups_total + G - 1) / G;
        G = (groups_total + nb - 1) / nb;  // equalise the bands
        if (G < 2) G = 2;                  // a single group of rows: still one band, named by the smallest band the plan has
        p.band_rows = (int)(7 * G);
    }
    p.bands = (h - 6 + p.band_rows - 1) / p.band_rows;
    p.items_per_pair = p.col_blocks * p.bands;
    p.n_items = n_pairs * p.items_per_pair;
    return p;
}
