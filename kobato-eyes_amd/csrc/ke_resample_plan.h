// How the resample kernels of ke_hash.hip are launched: one pure function per path, from the facts the decision depends
// on -- the group's shape, the target, a few numbers of the tap tables, the CU count, the two environment switches -- to a
// plan struct or a reason to decline.  No HIP, no context, no getenv: ke_hash.hip fetches the tables, calls the plan,
// reserves scratch, copies plan fields and device pointers into the kernel's argument struct and launches; a host-only
// program can include this file to see what a shape is given (tests/test_resample_plan_cpu.py).  Where a path needs a
// table that depends on an earlier choice the function comes in two steps.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "ke_coeffs.h"
#include "ke_hash_select.h"

// KE_FUSED_MIN_IMAGES and KE_VTILE_VALU, as the entry points of ke_hash.hip read them at every call.
struct KeHashSwitches {
    bool fused_min_set = false;      // KE_FUSED_MIN_IMAGES is set ...
    int64_t fused_min_images = 0;    // ... to this
    bool vtile_valu = false;         // KE_VTILE_VALU is set
};

// A group of equally sized images.  base_dword: the base pointer is a multiple of 4; stride_dword: so is the stride.
struct KePlanShape {
    int w, h, channels;
    int64_t n;
    bool misaligned, base_dword, stride_dword, has_offsets;
};

// Why a path does not take a shape.  ke_hash.hip maps every one to KE_EUNSUPPORTED.
enum KeDecline {
    KE_PLAN_OK = 0,
    KE_DECLINE_ONE_LAUNCH,        // any path: more workgroups than one launch takes
    // ke_plan_hband
    KE_DECLINE_HB_VERTICAL_FIRST, // Pillow's vertical-first rule
    KE_DECLINE_HB_SHAPE,          // under 4 pixels, over 16384 x 65536, 2 GiB or more
    KE_DECLINE_HB_WINDOW,         // a window beyond 32 chunks of 32 dwords
    KE_DECLINE_HB_ROW,            // a row of more than 2048 quads
    KE_DECLINE_HB_LDS,            // two tile buffers and the staged band over 64 KiB
    // ke_plan_vtile
    KE_DECLINE_VT_LDS,            // VALU form: one column over 64 KiB
    // ke_plan_strips
    KE_DECLINE_ST_TARGET,         // neither 32 x 32 nor 9 x 8
    KE_DECLINE_ST_SHAPE,          // not packed RGB rows of 2052.. pixels that end on a quad, too tall, identity vertical axis
    KE_DECLINE_ST_ADDRESS,        // 2 GiB or more, or images off a dword boundary
    KE_DECLINE_ST_STEPS,          // more than 6 operand steps per wave
    KE_DECLINE_ST_TABLE,          // the operand table came out another way
    KE_DECLINE_ST_LAST_STRIP,     // a nearly empty last strip
    KE_DECLINE_ST_SWITCH,         // KE_FUSED_MIN_IMAGES asks for a larger group
    KE_DECLINE_ST_FILL,           // too few workgroups to fill the chip
    // ke_plan_sp_bands
    KE_DECLINE_SPB_SHAPE,         // too tall for its width, or under 16 rows
    // ke_plan_fused
    KE_DECLINE_FU_WIDTH,          // the row of the kernel table does not take this row length
    KE_DECLINE_FU_TABLE,          // the operand table has other step counts
    KE_DECLINE_FU_DH_TABLE,       // so has the dHash leg's
    KE_DECLINE_FU_LDS,            // over 150 KB of LDS
    KE_DECLINE_FU_BANDS_FIT,      // over 80 KB whole, under it per band: the caller runs the kernel per band
    KE_DECLINE_COUNT
};

// ---- shared rules ------------------------------------------------------------------------------------------------
// Pitch of one transposed output column in the global scratch hs[img][column][pitch]: the vertical windows (span) and the
// rows + 4 fit, a multiple of 8, and 8 more for the kernels that read whole dword pairs.
inline int ke_column_pitch(int span, int h) { return ((std::max(span, h + 4) + 7) & ~7) + 8; }

inline bool ke_fits_one_launch(int64_t workgroups) { return workgroups <= 0x7fffffffLL; }

// first-pass scratch of a call is held to 512 MB: images per chunk at `per_image` bytes each
inline int64_t ke_chunk_images(size_t per_image) { return std::max<int64_t>(1, (int64_t)(((size_t)512 << 20) / per_image)); }
// The banded path needs 32*H bytes of scratch per image, the generic passes up to W*H: ke_launch_hash_group sizes its
// chunks for the former (the generic passes re-chunk themselves, KeGenericPlan::max_n)
inline size_t ke_hash_scratch_per_image(int h) { return (size_t)40 * (std::max(h, 32) + 1024); }
inline size_t ke_resize_scratch_per_image(int ow, int oh, int h) { return (size_t)(ow + 8) * (std::max(h, oh) + 1024); }

// The single-pass kernels give one workgroup a whole image, so a small group of large images cannot fill the chip that
// way; such a group runs the same kernels per band of rows (a single image is spread over the whole GPU).  Measured
// crossover on MI355X: about 200 images at 512x512 and 1024^2, 500-700 at 2048^2, none below ~400 KB per image.
// KE_FUSED_MIN_IMAGES overrides the threshold (tests set it to 1 to reach the one-workgroup-per-image form with a few
// images).
inline int64_t ke_fused_min_images(int64_t image_bytes, const KeHashSwitches &sw) {
    if (sw.fused_min_set) return sw.fused_min_images;
    return image_bytes < 400 * 1024 ? 1 : image_bytes < (8 << 20) ? 192 : 512;
}

// ---- ke_hband: the banded horizontal pass ---------------------------------------------------------------------------
struct KeHbandChunks {
    KeDecline why;
    int best_log2;     // log2(chunks per output): ke_plan_hband wants the chunk table built for 1 << best_log2, 8
};

// Chunks per output: the power of two that wastes the fewest padded dwords, chunk <= 32 dwords; when the virtual columns
// of all outputs do not fit the 256 lanes, the outputs are split over several launches.  ndw: of the horizontal axis.
inline KeHbandChunks ke_plan_hband_chunks(const KePlanShape &g, int ow, int oh, int ndw) {
    if (ke_taller_than_100_widths(g.w, g.h) && oh < g.h) return {KE_DECLINE_HB_VERTICAL_FIRST, -1};
    if ((int64_t)g.w * g.h < 4 || g.w > 16384 || g.h > 65536 || (int64_t)g.w * g.h * g.channels >= (1LL << 31)) return {KE_DECLINE_HB_SHAPE, -1};
    int best_log2 = -1, best_waste = 1 << 30;
    for (int l = 0; l <= 5; ++l) {
        const int cpo = 1 << l, ndwc = (((ndw + cpo - 1) / cpo) + 7) & ~7;
        if (ndwc > 32) continue;
        const int launches = (ow * cpo + 255) / 256;
        const int waste = cpo * ndwc - ndw + (ndwc > 24 ? 8 : 0) + 1000 * (launches - 1);   // mild preference for <= 24 (3 waves/SIMD)
        if (waste < best_waste) { best_waste = waste; best_log2 = l; }
    }
    if (best_log2 < 0) return {KE_DECLINE_HB_WINDOW, -1};
    return {KE_PLAN_OK, best_log2};
}

struct KeHbandPlan {
    KeDecline why;
    int best_log2;
    int qr, lp, rt, band_rows, bands, bp;   // as in KeBandArgs
    int per_launch;                         // outputs whose virtual columns fit 256 lanes
    int launches;                           // ke_hband_launch(plan, ow, 0 .. launches - 1)
    int lt_half, hp;
    size_t lds, scratch_bytes;
    bool aligned;                           // the dword loader, not the funnel shift
};

// cspan: of the chunk table; vspan: span of the vertical axis
inline KeHbandPlan ke_plan_hband(const KePlanShape &g, int ow, int best_log2, int cspan, int vspan) {
    KeHbandPlan p{};
    p.best_log2 = best_log2;
    p.qr = (g.w + 3) / 4;
    if (p.qr > 2048) { p.why = KE_DECLINE_HB_ROW; return p; }
    p.lp = (4 * p.qr + 7) & ~7;
    p.rt = std::max(1, std::min(2048 / p.qr, g.h));
    // Rows per workgroup.  Upper bounds: about 2 MB of pixels (amortises the tap-plane loads of a workgroup; measured
    // 4-6 % over 512 KB bands), 480 rows and 24 KB of LDS for the band's staged output bytes.  The image is then cut
    // into EQUAL bands (a short last band leaves its CU idle at the end), each a whole number of 4-tile groups so that
    // bands start on a multiple of 4 rows.
    const int unit = 4 * p.rt;
    p.per_launch = std::min(ow, 256 >> best_log2);
    int64_t cap_rows = std::max<int64_t>(unit, ((int64_t)(2048 << 10) / ((int64_t)g.w * g.channels)) / unit * unit);
    cap_rows = std::min<int64_t>(cap_rows, std::max(unit, 480 / unit * unit));
    cap_rows = std::min<int64_t>(cap_rows, std::max<int64_t>(unit, ((24 * 1024) / p.per_launch - 8) / unit * unit));
    // small groups still have to fill the chip: aim for at least ~3000 workgroups per launch (4 per SIMD slot)
    const int64_t min_bands = std::min<int64_t>((3072 + g.n - 1) / g.n, (g.h + unit - 1) / unit);
    if (min_bands > 1) cap_rows = std::min<int64_t>(cap_rows, std::max<int64_t>(unit, ((g.h + min_bands - 1) / min_bands + unit - 1) / unit * unit));
    const int64_t want_bands = (g.h + cap_rows - 1) / cap_rows;
    const int64_t rows = std::min<int64_t>(cap_rows, (((g.h + want_bands - 1) / want_bands + unit - 1) / unit) * unit);
    p.band_rows = (int)rows;
    p.bands = (g.h + p.band_rows - 1) / p.band_rows;
    p.bp = ((p.band_rows + 3) & ~3) + 4;
    const int tile_bytes = p.rt * p.lp + std::max(0, cspan - p.lp) + 16;
    p.lt_half = (tile_bytes + 15) & ~15;
    p.lds = 2 * (size_t)p.lt_half + (size_t)p.per_launch * p.bp;
    if (p.lds > 64 * 1024) { p.why = KE_DECLINE_HB_LDS; return p; }
    p.hp = ke_column_pitch(vspan, g.h);
    p.scratch_bytes = (size_t)g.n * ow * p.hp + 8192;     // + slack: ke_vtile_mx reads whole steps
    if (!ke_fits_one_launch((int64_t)g.n * p.bands)) { p.why = KE_DECLINE_ONE_LAUNCH; return p; }
    // "aligned" = every row starts on a quad boundary of the packed stream (w % 4 == 0) and every image starts on a
    // dword boundary, so a quad is DW whole dwords and the last quad of the image ends with the image.  Other widths, and
    // ragged batches in which some image starts off a dword boundary, take the funnel-shift loader.
    p.aligned = g.w % 4 == 0 && !g.misaligned;
    p.launches = (ow + p.per_launch - 1) / p.per_launch;
    return p;
}

struct KeHbandLaunch {
    int out_first, nout, vcp_log2;
};

inline KeHbandLaunch ke_hband_launch(const KeHbandPlan &p, int ow, int i) {
    KeHbandLaunch l;
    l.out_first = i * p.per_launch;
    l.nout = std::min(p.per_launch, ow - l.out_first);
    int vcp = 1, vl = 0;
    while (vcp < (l.nout << p.best_log2)) { vcp <<= 1; ++vl; }
    l.vcp_log2 = vl;
    return l;
}

// ---- ke_vtile_mx / ke_vtile: the vertical taps of the banded paths ----------------------------------------------------
inline bool ke_vtile_on_mx(int oh, const KeHashSwitches &sw) { return oh <= 128 && !sw.vtile_valu; }

struct KeVtilePlan {
    KeDecline why;
    bool on_mx;
    int nt;                   // matrix cores: column tiles, n * mx_tiles * nt waves, four to a workgroup
    int64_t items, blocks;
    int cg;                   // VALU: columns staged in LDS per round
    size_t lds;
};

// mx_tiles: KeMxTable::tiles of the vertical axis (read only where ke_vtile_on_mx says so)
inline KeVtilePlan ke_plan_vtile(int ow, int oh, int hp, int64_t n, const KeHashSwitches &sw, int mx_tiles) {
    KeVtilePlan p{};
    p.on_mx = ke_vtile_on_mx(oh, sw);
    if (p.on_mx) {
        p.nt = (ow + 15) / 16;
        p.items = n * mx_tiles * p.nt;
        p.blocks = (p.items + 3) / 4;
        if (!ke_fits_one_launch(p.blocks)) p.why = KE_DECLINE_ONE_LAUNCH;
        return p;
    }
    p.cg = std::max(1, std::min(ow, (48 * 1024) / hp));
    p.lds = (size_t)p.cg * hp;
    if (p.lds > 64 * 1024) p.why = KE_DECLINE_VT_LDS;
    return p;
}

// ---- ke_hstrips: rows wider than 2048 pixels --------------------------------------------------------------------------
constexpr int kKeStripWidth = 2048;                  // strip width in pixels: 16 rows of it are one LDS buffer
constexpr int kKeStripPitch = kKeStripWidth + 16;    // LDS pitch of a strip row (129 x 16 B: conflict-free operand rows)

struct KeStripSteps {
    KeDecline why;
    int nt, parts, ksh;       // ke_plan_strips wants the operand table built for parts * ksh steps, 64-aligned
};

// (32 x 32) or (8 x 9) tile of packed RGB images 2816..5300 pixels wide.  bounds: of the horizontal axis.
inline KeStripSteps ke_plan_strips_steps(const KePlanShape &g, int ow, int oh, const int32_t *bounds) {
    if (!((ow == 32 && oh == 32) || (ow == 9 && oh == 8))) return {KE_DECLINE_ST_TARGET, 0, 0, 0};
    if (g.misaligned || g.channels != 3 || g.w % 4 || g.w <= 2048 || ke_taller_than_100_widths(g.w, g.h) || g.h == oh) return {KE_DECLINE_ST_SHAPE, 0, 0, 0};
    if ((int64_t)g.w * g.h * 3 >= (1LL << 31) || !g.base_dword || !(g.has_offsets || g.stride_dword)) return {KE_DECLINE_ST_ADDRESS, 0, 0, 0};
    const int nt = (ow + 15) / 16, parts = 16 / nt;
    // natural step count with 64-aligned bases decides the instantiation
    int ks = 0;
    for (int j = 0; j < nt; ++j) {
        int lo = g.w, hi = 0;
        for (int o = 16 * j; o < std::min(16 * j + 16, ow); ++o) { lo = std::min(lo, bounds[2 * o]); hi = std::max(hi, bounds[2 * o] + bounds[2 * o + 1]); }
        ks = std::max(ks, (hi - (lo & ~63) + 63) / 64);
    }
    const int ksh = std::max((ks + parts - 1) / parts, 3);
    if (ksh > 6) return {KE_DECLINE_ST_STEPS, nt, parts, ksh};
    return {KE_PLAN_OK, nt, parts, ksh};
}

struct KeStripPlan {
    KeDecline why;
    int nstrips, band_rows, bands, bp;   // as in KeStripArgs
    int base0, base1;
    int x_off, hb_off, hp;
    size_t lds, scratch_bytes;
};

// mx: the operand table built for the steps; vspan: span of the vertical axis
inline KeStripPlan ke_plan_strips(const KePlanShape &g, int ow, const KeStripSteps &s, const KeMxTable &mx, int vspan, int cu_count,
                                  const KeHashSwitches &sw) {
    KeStripPlan p{};
    if (mx.tiles != s.nt || mx.ks != s.parts * s.ksh || mx.base[0] % 64 || (s.nt == 2 && mx.base[1] % 64)) { p.why = KE_DECLINE_ST_TABLE; return p; }
    p.nstrips = (g.w + kKeStripWidth - 1) / kKeStripWidth;
    // a nearly empty last strip costs a full strip of load slots: rows that leave less than 3/8 of one stay banded
    if (g.w - (p.nstrips - 1) * kKeStripWidth < 768) { p.why = KE_DECLINE_ST_LAST_STRIP; return p; }
    // bands of up to 256 rows, equal, multiples of 16; only worth it when the bands fill the chip
    const int64_t want_bands = (g.h + 255) / 256;
    p.band_rows = (int)((((g.h + want_bands - 1) / want_bands) + 15) / 16 * 16);
    p.bands = (g.h + p.band_rows - 1) / p.band_rows;
    // few workgroups cannot fill the chip: such groups keep the banded kernel (smaller bands, up to 3072 workgroups);
    // KE_FUSED_MIN_IMAGES, when set, decides instead (as for the single-pass kernels)
    if (sw.fused_min_set) {
        if (g.n < sw.fused_min_images) { p.why = KE_DECLINE_ST_SWITCH; return p; }
    } else if (g.n * p.bands < 2 * (int64_t)cu_count) {
        p.why = KE_DECLINE_ST_FILL;
        return p;
    }
    p.base0 = mx.base[0]; p.base1 = s.nt == 2 ? mx.base[1] : 0;
    p.bp = p.band_rows + 4;
    p.lds = 2 * (size_t)16 * kKeStripPitch;
    p.x_off = (int)p.lds; p.lds += (size_t)2 * s.nt * (s.parts - 1) * 1024;
    p.hb_off = (int)p.lds; p.lds += (size_t)ow * p.bp;
    p.hp = ke_column_pitch(vspan, g.h);
    p.scratch_bytes = (size_t)g.n * ow * p.hp + 8192;
    if (!ke_fits_one_launch((int64_t)g.n * p.bands)) p.why = KE_DECLINE_ONE_LAUNCH;
    return p;
}

// ---- the single-pass kernels per band of rows -----------------------------------------------------------------------
// Band mode of the single-pass kernels (see KeFusedArgs::bands): how a group is cut, and the pitches of the columns.
struct KeSpBandPlan {
    KeDecline why;
    int bands, band_rows;
    int hs_hp, hsd_hp;
    size_t scratch_bytes;
};

// want_d: the 9 x 8 tile is asked for too; vspan / vdspan: spans of the vertical axes to 32 and (with want_d) to 8 rows
inline KeSpBandPlan ke_plan_sp_bands(const KePlanShape &g, bool want_d, int vspan, int vdspan, int cu_count) {
    KeSpBandPlan p{};
    if (ke_taller_than_100_widths(g.w, g.h) || g.h < 16) { p.why = KE_DECLINE_SPB_SHAPE; return p; }
    // bands: at most 1024 rows (32 KB of columns in LDS), and enough of them that the launch has ~4 workgroups per CU
    const int64_t fill = (4 * (int64_t)cu_count + g.n - 1) / g.n;
    // ... and short enough that two workgroups share a CU (80 KB each) where the kernel's fixed LDS allows it
    const bool both = want_d && g.channels == 3;
    const int64_t fixed = (g.w <= 768 && !(both && g.w > 512)) ? 64 * (int64_t)(g.w + 32) + (both ? 4096 : 0)
                                                               : 32 * (int64_t)(g.w + 32) + 12288 + (both ? 14336 : 0);
    int64_t max_rows = (80 * 1024 - fixed) / (both ? 41 : 32) / 32 * 32 - 32;
    if (max_rows < 128) max_rows = 1024;
    max_rows = std::min<int64_t>(max_rows, 1024);
    const int64_t bands = std::max<int64_t>((g.h + max_rows - 1) / max_rows, std::min<int64_t>(fill, (g.h + 63) / 64));
    p.band_rows = (int)(((g.h + bands - 1) / bands + 31) / 32 * 32);
    p.bands = (g.h + p.band_rows - 1) / p.band_rows;
    p.hs_hp = ke_column_pitch(vspan, g.h);
    p.hsd_hp = want_d ? ke_column_pitch(vdspan, g.h) : 8;
    p.scratch_bytes = (size_t)g.n * (32 * (size_t)p.hs_hp + (want_d ? 9 * (size_t)p.hsd_hp : 0)) + 8192;
    return p;
}

// ---- the single-pass kernels (rows of ke_hash_select.h) ---------------------------------------------------------------
constexpr int kKeTileRowsMx = 32, kKeTileRowsWide = 16;   // rows per tile of ke_phash_fused_mx and ke_phash_fused_wide

struct KeFusedSteps {
    KeDecline why;
    int ks;        // operand steps per output tile: a quarter per wave, or KS -- the table is built for at least these
    int ksd;       // dHash steps: the whole row in eight parts of KDW steps, or in two halves of KD = ceil(W64 / 2) steps
};

inline KeFusedSteps ke_plan_fused_steps(int r, int W) {
    const KeSpRow &row = kKeSpRows[r];
    const bool wide = row.family == KE_SP_WIDE;
    KeFusedSteps s{KE_PLAN_OK, wide ? 4 * row.t[0] : row.t[1], wide ? 8 * row.t[3] : 2 * ((row.t[0] + 1) / 2)};
    if ((W % 4 != 0) != row.unal() || (wide ? kKeTileRowsWide * ((W + 3) / 4) > 512 * row.t[1] : W < row.w_lo || W > row.w_hi)) s.why = KE_DECLINE_FU_WIDTH;
    return s;
}

struct KeFusedPlan {
    KeDecline why;
    int qw, qw_inv, lp, lt_half, hp, hpd, x_off;   // as in KeFusedArgs
    int row_bytes;
    int threads;
    int64_t workgroups;
    size_t lds;
    bool raise_lds_limit;                          // over the 64 KiB a kernel gets without the attribute
};

// LDS of a single-pass workgroup: two luma tile buffers, the 32 transposed columns (pitch hp), the 9 of the dHash leg (pitch
// hpd) and the exchange area X behind them: the wide kernel's waves always meet there (12 KB, and 14 KB more for the dHash
// leg), the narrow kernel's only for its dHash leg (4 KB).  *x_off: where X begins (0 without one).
inline size_t ke_fused_lds(bool wide, bool DH, int lt_half, int hp, int hpd, int *x_off) {
    size_t lds = (size_t)2 * lt_half + (size_t)32 * hp;
    if (!wide) lds = std::max<size_t>(lds, 4096);
    if (DH) lds += (size_t)9 * hpd;
    *x_off = 0;
    if (wide || DH) {
        lds = (lds + 15) & ~(size_t)15;
        *x_off = (int)lds;
        lds += wide ? 2 * 2 * 3 * 1024 + (DH ? 2 * 7 * 1024 : 0) : 4096;
    }
    return lds;
}

// Row r of the table on images of W x h; bands: NULL for one workgroup per image.  mx: operands of the 32-output horizontal
// axis at KeFusedSteps::ks; vspan: span of the vertical axis to 32 rows.  For a row with a dHash leg, mxd: operands of the
// 9-output axis at ksd; vd: the vertical axis to 8 rows in 3 chunks.
inline KeFusedPlan ke_plan_fused(int r, int W, int h, int64_t n, const KeFusedSteps &s, const KeMxTable &mx, int vspan, const KeMxTable *mxd,
                                 const KeChunkTable *vd, const KeSpBandPlan *bands) {
    const KeSpRow &row = kKeSpRows[r];
    const bool wide = row.family == KE_SP_WIDE, DH = row.dh();
    const int C = row.channels();
    const int rt = wide ? kKeTileRowsWide : kKeTileRowsMx;
    const bool exact = !wide && !row.t[3];                             // compile-time row length
    KeFusedPlan p{};
    p.threads = wide ? 512 : 256;
    if (mx.tiles != 2 || mx.ks != s.ks) { p.why = KE_DECLINE_FU_TABLE; return p; }
    const int rows_padded = bands ? bands->band_rows : ((h + rt - 1) / rt) * rt;
    // one tile buffer: rt padded rows + the part of the last row's operand window that overhangs the row
    const int overhang = std::max(0, std::max(std::max(mx.base[0], mx.base[1]) + 64 * s.ks, DH ? 64 * s.ksd : 0) - W);
    p.qw = (W + 3) / 4;
    p.row_bytes = W * C;
    p.qw_inv = (int)(uint32_t)((0x100000000ull + (uint64_t)p.qw - 1) / (uint64_t)p.qw);
    // row pitch: an odd number of 16-byte units, so the 16 rows of an operand land in distinct bank groups
    p.lp = exact ? W + 16 : (((W + 15) / 16 + 1) | 1) * 16;
    p.lt_half = (rt * p.lp + overhang + 15) & ~15;
    p.hp = ((std::max(bands ? 0 : vspan, rows_padded) + 7) & ~7) + 8;
    p.hpd = 8;
    if (DH) {
        if (mxd->tiles != 1 || mxd->base[0] != 0 || mxd->ks != s.ksd) { p.why = KE_DECLINE_FU_DH_TABLE; return p; }
        p.hpd = ((std::max(bands ? 0 : vd->cspan, rows_padded) + 7) & ~7) + 8;
    }
    p.lds = ke_fused_lds(wide, DH, p.lt_half, p.hp, p.hpd, &p.x_off);
    // up to 80 KB two workgroups share a CU.  A tall image (its 32 x H transposed columns) would need more and run one
    // per CU; if cutting it into bands brings the columns back under that line, decline: the caller then runs this
    // kernel per band (measured 5.4-6.0 TB/s against 3.9-4.9 for one workgroup per CU)
    if (p.lds > 150 * 1024) { p.why = KE_DECLINE_FU_LDS; return p; }
    if (!bands && p.lds > 80 * 1024 && p.lds - (size_t)(32 * (p.hp - 136)) - (DH ? (size_t)(9 * (p.hpd - 136)) : 0) <= 80 * 1024) { p.why = KE_DECLINE_FU_BANDS_FIT; return p; }
    p.raise_lds_limit = p.lds > 64 * 1024;
    p.workgroups = n * (bands ? bands->bands : 1);
    if (!ke_fits_one_launch(p.workgroups)) p.why = KE_DECLINE_ONE_LAUNCH;
    return p;
}

// ---- the tail of the single-pass kernels: the vertical taps on the matrix cores -----------------------------------------
// One workgroup per image: behind the row loop four waves turn the transposed columns into the 32 x 32 tile, one 16 x 16
// block each, out of the KeMxTable of the vertical axis; with a dHash leg each wave also takes a quarter of the 8-output
// axis' operand steps.  The steps are issued in fixed groups, so the tables are built for rounded step counts:
constexpr int kKeTailStepGroup = 3, kKeTailDStepGroup = 2;
// ... of the 32-output axis, from the count its table has unpadded (ke_build_mx with min_ks = 0)
inline int ke_fused_tail_steps(int natural_ks) { return (natural_ks + kKeTailStepGroup - 1) / kKeTailStepGroup * kKeTailStepGroup; }
// ... of the 8-output axis: four equal parts, each a whole number of groups
inline int ke_fused_tail_dsteps(int natural_ks) {
    const int per_wave = ((natural_ks + 3) / 4 + kKeTailDStepGroup - 1) / kKeTailDStepGroup * kKeTailDStepGroup;
    return 4 * per_wave;
}

struct KeFusedTailPlan {
    bool on_mx;              // false: the dot-product tail, and the plan stays as ke_plan_fused made it
    int hp, hpd, x_off;      // on_mx: these replace the KeFusedPlan's
    size_t lds;
    bool raise_lds_limit;
    int ks, kdq;             // operand steps per 16-row block of the tile; dHash steps per wave
};

// p: what ke_plan_fused answered for row r without bands.  vmx: the vertical 32-output axis at ke_fused_tail_steps; vdmx
// (rows with a dHash leg): the vertical 8-output axis at ke_fused_tail_dsteps.  A step reads 64 rows of every column,
// and the steps of a block run to base + 64 * ks whatever the image's height: rows past it meet zero taps, but the
// columns are lengthened so that every read stays inside the column area.  The pitch becomes an odd number of 16-byte
// units: 16-byte reads, and the 16 columns of an operand (and of the row loop's dword stores) in distinct banks.  Where
// the longer columns would cost the second workgroup of a CU (80 KB each) or pass the kernel's LDS, the shape keeps the
// dot-product tail; so it does under KE_VTILE_VALU.
inline KeFusedTailPlan ke_plan_fused_tail(int r, const KeFusedPlan &p, const KeMxTable &vmx, const KeMxTable *vdmx, const KeHashSwitches &sw) {
    const KeSpRow &row = kKeSpRows[r];
    const bool wide = row.family == KE_SP_WIDE, DH = row.dh();
    KeFusedTailPlan t{false, p.hp, p.hpd, p.x_off, p.lds, p.raise_lds_limit, 0, 0};
    if (sw.vtile_valu || vmx.tiles != 2 || vmx.ks % kKeTailStepGroup) return t;
    if (DH && (!vdmx || vdmx->tiles != 1 || vdmx->base[0] != 0 || vdmx->ks % (4 * kKeTailDStepGroup))) return t;
    auto odd16 = [](int bytes) { return (((bytes + 15) / 16) | 1) * 16; };
    const int hp = odd16(std::max(p.hp, std::max(vmx.base[0], vmx.base[1]) + 64 * vmx.ks));
    const int hpd = DH ? odd16(std::max(p.hpd, 64 * vdmx->ks)) : p.hpd;
    int x_off = 0;
    const size_t lds = ke_fused_lds(wide, DH, p.lt_half, hp, hpd, &x_off);
    if (lds > 150 * 1024 || (p.lds <= 80 * 1024 && lds > 80 * 1024)) return t;
    return {true, hp, hpd, x_off, lds, lds > 64 * 1024, vmx.ks, DH ? vdmx->ks / 4 : 0};
}

// ---- ke_resample_pass: two single-axis passes in Pillow's order -------------------------------------------------------
struct KeGenericPlan {
    bool vertical_first;      // Pillow's Image.resize shrinks very tall, narrow images vertically first (PIL/Image.py)
    int mid_w, mid_h;         // the image between the passes
    size_t mid_bytes;
    int64_t max_n;            // images per round: bounds the first-pass scratch
    int b0, b1;               // workgroups per image of the first and the second pass
};

inline KeGenericPlan ke_plan_generic(int w, int h, int ow, int oh) {
    KeGenericPlan p;
    p.vertical_first = ke_taller_than_100_widths(w, h) && oh < h;
    p.mid_w = p.vertical_first ? w : ow;
    p.mid_h = p.vertical_first ? oh : h;
    p.mid_bytes = (size_t)p.mid_w * p.mid_h;
    p.max_n = ke_chunk_images(p.mid_bytes);
    p.b0 = (int)((p.mid_bytes + 255) / 256);
    p.b1 = (ow * oh + 255) / 256;
    return p;
}
