// The pair scan's tiling and the part of it that a scan "from first_new" covers: which tiles exist, which workgroup
// ordinal is which tile, how many pairs a tile and a shard stand for.  Plain integer arithmetic without HIP types, for
// the kernel (ke_scan.hip), for the host's closed form beside it and for the host-only programs (tests/_scan_region_cpu.cpp,
// tests/_scan_cross_cpu.cpp).  The cross region of ke_hamming_scan_cross has its functions at the end of the file.
//
// The table is [library | added]: positions first_new .. n-1 are new, and the region is the pairs i < j with
// j >= first_new.  Over the 1024 x 1024 tiling of the upper triangle that is a trapezoid: with cc0 = first_new / kKeScanCols,
// row block rb owns the column chunks max(kKeScanCPR * rb, cc0) .. ncc-1 -- the first `rect` row blocks a rectangle of
// `width` = ncc - cc0 chunks each, the ones below them their rows of the triangle.  first_new = 0 is the whole triangle.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define KE_REGION_FN __host__ __device__ inline
#else
#define KE_REGION_FN inline
#endif

constexpr int kKeScanTile = 1024;                          // rows per workgroup ...
constexpr int kKeScanCols = 1024;                          // ... against this many columns
constexpr int kKeScanCPR = kKeScanTile / kKeScanCols;      // column chunks per row block

struct KeScanRegion {
    int64_t n, first_new;
    int64_t nb, ncc;        // row blocks, column chunks of the whole table
    int64_t cc0;            // the chunk first_new lies in
    int64_t rect, width;    // row blocks 0 .. rect-1 own `width` chunks each, from cc0
    int64_t rect_tiles;     // rect * width: ordinals below it are the rectangle's
    int64_t tri_base;       // ordinal of tile (rect, kKeScanCPR * rect) in the whole triangle's enumeration
    int64_t n_tiles;
};

// tiles of the whole triangle in front of row block rb
KE_REGION_FN int64_t ke_tri_offset(int64_t rb, int64_t ncc) { return rb * ncc - (int64_t)kKeScanCPR * rb * (rb - 1) / 2; }

KE_REGION_FN KeScanRegion ke_scan_region(int64_t n, int64_t first_new) {
    KeScanRegion r;
    r.n = n; r.first_new = first_new;
    r.nb = (n + kKeScanTile - 1) / kKeScanTile;
    r.ncc = (n + kKeScanCols - 1) / kKeScanCols;
    r.cc0 = first_new / kKeScanCols;
    if (first_new >= n) {                                   // nothing new: no tile (cc0 may lie past the last chunk)
        r.rect = r.width = r.rect_tiles = r.tri_base = r.n_tiles = 0;
        return r;
    }
    const int64_t split = r.cc0 / kKeScanCPR + 1;           // first row block whose own diagonal chunk lies right of cc0
    r.rect = split < r.nb ? split : r.nb;
    r.width = r.ncc - r.cc0;
    r.rect_tiles = r.rect * r.width;
    r.tri_base = ke_tri_offset(r.rect, r.ncc);
    r.n_tiles = r.rect_tiles + ke_tri_offset(r.nb, r.ncc) - r.tri_base;
    return r;
}

// ordinal of row block rb's first tile in the region's enumeration (rb = nb: the tile count)
KE_REGION_FN int64_t ke_region_offset(const KeScanRegion &r, int64_t rb) {
    return rb <= r.rect ? rb * r.width : r.rect_tiles + ke_tri_offset(rb, r.ncc) - r.tri_base;
}

// Tile ordinal t of the whole triangle (row-major, row block rb owns chunks kKeScanCPR * rb .. ncc-1) -> (rb, cc): the
// quadratic offset(rb) <= t inverted with a float estimate and an exact integer fix-up.
KE_REGION_FN void ke_tri_tile(int64_t t, int64_t nb, int64_t ncc, int64_t *rb_out, int64_t *cc_out) {
    const double hc = 0.5 * kKeScanCPR, bq = (double)ncc + hc;
    int64_t rb = (int64_t)floor((bq - sqrt(fmax(bq * bq - 4.0 * hc * (double)t, 0.0))) / (2.0 * hc));
    if (rb < 0) rb = 0;
    if (rb >= nb) rb = nb - 1;
    while (rb > 0 && ke_tri_offset(rb, ncc) > t) --rb;
    while (rb + 1 < nb && ke_tri_offset(rb + 1, ncc) <= t) ++rb;
    *rb_out = rb;
    *cc_out = (int64_t)kKeScanCPR * rb + (t - ke_tri_offset(rb, ncc));
}

// Tile ordinal t in [0, n_tiles) of the region -> (rb, cc): a division inside the rectangle, below it the triangle's
// inversion on the ordinal the tile has there.
KE_REGION_FN void ke_region_tile(const KeScanRegion &r, int64_t t, int64_t *rb_out, int64_t *cc_out) {
    if (t < r.rect_tiles) {
        *rb_out = t / r.width;
        *cc_out = r.cc0 + t % r.width;
        return;
    }
    ke_tri_tile(t - r.rect_tiles + r.tri_base, r.nb, r.ncc, rb_out, cc_out);
}

// pairs i < j, j >= first_new, that tile (rb, cc) of the region stands for: column j meets min(rows, j - row0) rows
KE_REGION_FN int64_t ke_region_tile_pairs(const KeScanRegion &r, int64_t rb, int64_t cc) {
    const int64_t row0 = rb * kKeScanTile, col0 = cc * kKeScanCols;
    const int64_t rows = r.n - row0 < kKeScanTile ? r.n - row0 : kKeScanTile;
    const int64_t jlo = (col0 > r.first_new ? col0 : r.first_new) - row0;
    const int64_t jhi = (col0 + kKeScanCols < r.n ? col0 + kKeScanCols : r.n) - row0;
    if (jhi <= jlo || jlo < 0) return 0;
    // sum over d in [0, m) of min(rows, d)
    const int64_t blo = jlo <= rows ? jlo * (jlo - 1) / 2 : rows * (rows - 1) / 2 + (jlo - rows) * rows;
    const int64_t bhi = jhi <= rows ? jhi * (jhi - 1) / 2 : rows * (rows - 1) / 2 + (jhi - rows) * rows;
    return bhi - blo;
}

// tiles of the region dealt to shard part_index of part_count (tile t goes to shard t mod part_count)
KE_REGION_FN int64_t ke_region_shard_tiles(const KeScanRegion &r, int part_index, int part_count) {
    return r.n_tiles > part_index ? (r.n_tiles - part_index + part_count - 1) / part_count : 0;
}

// Pairs of the region that shard part_index of part_count stands for, in O(row blocks): of a row block's tiles only the
// diagonal ones, the one first_new lies in and the last one are partial, the rest are rows x kKeScanCols rectangles and
// are counted by how many of their ordinals fall to the shard.
KE_REGION_FN uint64_t ke_region_shard_pairs(const KeScanRegion &r, int part_index, int part_count) {
    uint64_t pairs = 0;
    for (int64_t rb = 0; rb < r.nb && r.n_tiles > 0; ++rb) {
        const int64_t off = ke_region_offset(r, rb);
        const int64_t start = rb < r.rect ? r.cc0 : (int64_t)kKeScanCPR * rb;
        const int64_t rows = r.n - rb * kKeScanTile < kKeScanTile ? r.n - rb * kKeScanTile : kKeScanTile;
        for (int64_t cc = start; cc < r.ncc; ++cc) {
            const int64_t t = off + (cc - start);
            const bool whole = cc >= (int64_t)kKeScanCPR * (rb + 1) && cc > r.cc0 && cc < r.ncc - 1;
            if (whole) {                                    // chunks cc .. ncc-2 are all whole: ordinals [t, t_last)
                const int64_t t_last = off + (r.ncc - 1 - start);
                const int64_t below_last = t_last <= part_index ? 0 : (t_last - part_index + part_count - 1) / part_count;
                const int64_t below_t = t <= part_index ? 0 : (t - part_index + part_count - 1) / part_count;
                pairs += (uint64_t)(below_last - below_t) * (uint64_t)(rows * kKeScanCols);
                cc = r.ncc - 2;                             // the loop goes on with the last chunk
                continue;
            }
            if (t % part_count == part_index) pairs += (uint64_t)ke_region_tile_pairs(r, rb, cc);
        }
    }
    return pairs;
}

// ---- the cross region: the table is [library | queries] and only the pairs i < first_new <= j are wanted, the queries are
// not compared with each other.  Over the same tiling that is the rectangle of row blocks 0 .. ceil(first_new / kKeScanTile) - 1
// against the column chunks cc0 .. ncc-1, row-major; nothing of the triangle below it.  first_new = 0 or n: no tile.
KE_REGION_FN KeScanRegion ke_cross_region(int64_t n, int64_t first_new) {
    KeScanRegion r;
    r.n = n; r.first_new = first_new;
    r.nb = (n + kKeScanTile - 1) / kKeScanTile;
    r.ncc = (n + kKeScanCols - 1) / kKeScanCols;
    r.cc0 = first_new / kKeScanCols;
    r.tri_base = 0;
    if (first_new <= 0 || first_new >= n) {
        r.rect = r.width = r.rect_tiles = r.n_tiles = 0;
        return r;
    }
    r.rect = (first_new + kKeScanTile - 1) / kKeScanTile;
    r.width = r.ncc - r.cc0;
    r.rect_tiles = r.n_tiles = r.rect * r.width;
    return r;
}

// Tile ordinal t in [0, n_tiles) of the cross region -> (rb, cc)
KE_REGION_FN void ke_cross_tile(const KeScanRegion &r, int64_t t, int64_t *rb_out, int64_t *cc_out) {
    *rb_out = t / r.width;
    *cc_out = r.cc0 + t % r.width;
}

// pairs i < first_new <= j that tile (rb, cc) of the cross region stands for: its rows below first_new times its columns
// from first_new on (every such pair has i < j)
KE_REGION_FN int64_t ke_cross_tile_pairs(const KeScanRegion &r, int64_t rb, int64_t cc) {
    const int64_t row0 = rb * kKeScanTile, col0 = cc * kKeScanCols;
    const int64_t rows = (row0 + kKeScanTile < r.first_new ? row0 + kKeScanTile : r.first_new) - row0;
    const int64_t jlo = col0 > r.first_new ? col0 : r.first_new;
    const int64_t jhi = col0 + kKeScanCols < r.n ? col0 + kKeScanCols : r.n;
    if (rows <= 0 || jhi <= jlo) return 0;
    return rows * (jhi - jlo);
}

// Pairs of the cross region that shard part_index of part_count stands for (tile t goes to shard t mod part_count), in
// O(row blocks): of a row block's tiles only the one first_new lies in and the last one have fewer than kKeScanCols columns.
KE_REGION_FN uint64_t ke_cross_shard_pairs(const KeScanRegion &r, int part_index, int part_count) {
    uint64_t pairs = 0;
    for (int64_t rb = 0; rb < r.rect && r.n_tiles > 0; ++rb) {
        const int64_t off = rb * r.width;
        const int64_t t_last = off + r.width - 1;
        if (off % part_count == part_index) pairs += (uint64_t)ke_cross_tile_pairs(r, rb, r.cc0);
        if (r.width < 2) continue;
        if (t_last % part_count == part_index) pairs += (uint64_t)ke_cross_tile_pairs(r, rb, r.ncc - 1);
        // chunks cc0+1 .. ncc-2 are whole: ordinals [off + 1, t_last)
        const int64_t t = off + 1;
        const int64_t below_last = t_last <= part_index ? 0 : (t_last - part_index + part_count - 1) / part_count;
        const int64_t below_t = t <= part_index ? 0 : (t - part_index + part_count - 1) / part_count;
        pairs += (uint64_t)(below_last - below_t) * (uint64_t)ke_cross_tile_pairs(r, rb, r.cc0 + 1);
    }
    return pairs;
}
