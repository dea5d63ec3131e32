// ke_scan_plan.h -- what ke_launch_scan (ke_scan.hip) reserves and launches for one pair scan: a pure host function of the
// call's shape and the two environment settings, so that it compiles with any C++ compiler and is tested without a GPU
// (tests/test_scan_plan_cpu.py).
//
//   kind          KE_SCAN_ALL: the pairs i < j; KE_SCAN_FROM: those with j >= first_new; KE_SCAN_CROSS: i < first_new <= j.
//                 FROM with first_new = 0 is ALL and launches ALL's kernels.
//   region        ke_cross_region for CROSS, else ke_scan_region (ke_scan_region.h); tile t of its enumeration belongs to shard
//                 t mod part_count: my_tiles of them and `pairs` pairs to this shard, which counters[0] must come to.
//   exact         every pair within the threshold is an edge: the tile kernel alone, no bucket pair cap, no bucket pair count,
//                 so no histogram, no sort and no bucket kernel whatever else the call asks for.
//   table         bands of at most 24 bits get a histogram of band_count << band_bits bins when something needs the bucket
//                 sizes (need_hist: the bucket path, the cap, the count); wider bands get a sort per band instead (wide_sort:
//                 the cap or the count), which needs n < 2^32.
//   buckets       the bucket kernels are launched beside the tile kernel and the device picks one (ke_bucket_offsets): a table
//                 of at most kScanBucketMaxBins bins and n < 2^32, not KE_SCAN_MODE=tiles, and n >= kScanBucketMinN unless
//                 KE_SCAN_MODE=buckets.  The device takes them when the walked bucket pairs are at most bucket_threshold =
//                 region_pairs / kScanBucketRatio (ALL) or / kScanBucketRatioFrom (FROM, CROSS) and no walked bucket is longer than
//                 kBucketLongest (ke_scan.hip); region_pairs is what the tile kernel would visit over all shards.  buckets_allowed = false
//                 is the plan for a call whose sort buffer (sort_bytes) could not be reserved.
//   hist_pairs    without the bucket path the count comes from a kernel of its own over the histogram.
//   state         [counters, path, longest bucket: kScanStateBytes | block sums: kScanBlockSumBytes | histogram], one memset.
//   slices        a launch holds fewer than 2^32 threads: kScanMaxLaunchTiles tiles.  An exact scan launches its my_tiles
//                 in consecutive slices of at most KE_SCAN_TILES_PER_LAUNCH (default and ceiling: kScanMaxLaunchTiles); slot s
//                 of a slice that starts at slot s0 is tile part_index + (s0 + s) * part_count.  Every other scan is one
//                 slice, refused beyond 2^31 - 1 tiles.  Beyond kScanMaxLaunchTiles only a part of that grid runs and the call
//                 ends at the caller's check of counters[0]; the cross scan is refused there instead where the tile kernel is
//                 its only path.
#pragma once

#include <cstddef>
#include <cstdint>

#include "ke_scan_region.h"

enum KeScanKind { KE_SCAN_ALL = 0, KE_SCAN_FROM = 1, KE_SCAN_CROSS = 2 };
enum { KE_SCAN_AUTO = 0, KE_SCAN_FORCE_TILES = 1, KE_SCAN_FORCE_BUCKETS = 2 };   // KE_SCAN_MODE
// why a call is refused (KE_EUNSUPPORTED)
enum { KE_SCAN_FITS = 0, KE_SCAN_WIDE_NEEDS_32_BITS, KE_SCAN_TOO_MANY_TILES, KE_SCAN_CROSS_OVER_ONE_LAUNCH };

// The rule between the paths (set from the sweeps recorded there): below kScanBucketMinN both paths cost about
// their launches.  The bucket kernels walk every bucket of the
// table however thin the region is, so their time does not shrink with it while the tile kernel's does: between the rows of the
// record (tiles ahead at region pairs / bucket pairs = 33 and 312, level at 325, buckets ahead from 2 978) kScanBucketRatioFrom sits
// at the geometric middle.
constexpr unsigned long long kScanBucketRatio = 6000;
constexpr int64_t kScanBucketMinN = 50000;
constexpr unsigned long long kScanBucketRatioFrom = 1000;
constexpr size_t kScanBucketMaxBins = (size_t)1 << 18;
constexpr size_t kScanStateBytes = 128, kScanBlockSumBytes = 1024;
constexpr int kScanThreads = 512;                                    // of a tile's workgroup
constexpr int64_t kScanMaxLaunchTiles = 0xffffffffLL / kScanThreads;

struct KeScanShape {
    int64_t n = 0, first_new = 0;
    KeScanKind kind = KE_SCAN_ALL;
    int part_index = 0, part_count = 1;
    int band_bits = 16, band_count = 4;
    int64_t bucket_pair_cap = 0;
    bool exact = false, want_bucket_pairs = false;
    bool buckets_allowed = true;
};

struct KeScanKnobs {
    int forced = KE_SCAN_AUTO;       // KE_SCAN_MODE
    int64_t tiles_per_launch = 0;    // KE_SCAN_TILES_PER_LAUNCH; outside 1 .. kScanMaxLaunchTiles - 1: kScanMaxLaunchTiles
};

struct KeScanSlice {
    int64_t first_tile, count;       // the tile of the launch's first workgroup; its grid
};

struct KeScanPlan {
    KeScanKind kind;
    KeScanRegion region;
    int part_index, part_count;
    int64_t n_tiles, my_tiles;
    uint64_t pairs, region_pairs, bucket_threshold;
    uint64_t cap;                    // the bucket pair cap in force, 0: none
    bool table, buckets, need_hist, hist_pairs, wide_sort;
    size_t bins, sort_bytes, hist_at, state_bytes, exp_bytes;
    int64_t slice_tiles, n_slices;
    int refusal;                     // KE_SCAN_FITS or why not; the messages print n, my_tiles and kScanThreads
};

inline KeScanPlan ke_scan_plan(const KeScanShape &s, const KeScanKnobs &k) {
    KeScanPlan p;
    const uint64_t n = (uint64_t)s.n, f = (uint64_t)s.first_new;
    p.kind = s.kind == KE_SCAN_FROM && s.first_new == 0 ? KE_SCAN_ALL : s.kind;
    const bool cross = p.kind == KE_SCAN_CROSS;
    p.region = cross ? ke_cross_region(s.n, s.first_new) : ke_scan_region(s.n, s.first_new);
    p.part_index = s.part_index; p.part_count = s.part_count;
    p.n_tiles = p.region.n_tiles;
    p.my_tiles = ke_region_shard_tiles(p.region, s.part_index, s.part_count);
    p.pairs = cross ? ke_cross_shard_pairs(p.region, s.part_index, s.part_count) : ke_region_shard_pairs(p.region, s.part_index, s.part_count);
    p.region_pairs = cross ? f * (n - f) : n * (n - 1) / 2 - (f ? f * (f - 1) / 2 : 0);
    p.bucket_threshold = p.region_pairs / (p.kind == KE_SCAN_ALL ? kScanBucketRatio : kScanBucketRatioFrom);
    p.cap = !s.exact && s.bucket_pair_cap > 0 ? (uint64_t)s.bucket_pair_cap : 0;
    const bool want_bucket_pairs = !s.exact && s.want_bucket_pairs;
    p.table = s.band_bits <= 24;
    p.bins = p.table ? (size_t)s.band_count << s.band_bits : 0;
    p.buckets = s.buckets_allowed && !s.exact && p.table && p.bins <= kScanBucketMaxBins && s.n <= 0xffffffffLL &&
                k.forced != KE_SCAN_FORCE_TILES && (k.forced == KE_SCAN_FORCE_BUCKETS || s.n >= kScanBucketMinN);
    // [sorted hashes 8 B | sorted positions 4 B] per band and hash, and the per-bin offsets
    p.sort_bytes = p.buckets ? (size_t)s.band_count * (size_t)s.n * 12 + p.bins * sizeof(uint32_t) : 0;
    p.need_hist = p.table && (p.buckets || p.cap > 0 || want_bucket_pairs);
    p.hist_pairs = p.need_hist && !p.buckets && want_bucket_pairs;
    p.wide_sort = !p.table && (p.cap > 0 || want_bucket_pairs);
    p.hist_at = kScanStateBytes + kScanBlockSumBytes;
    p.state_bytes = (p.hist_at + (p.need_hist ? p.bins * sizeof(uint32_t) : 0) + 15) & ~(size_t)15;
    p.exp_bytes = (size_t)p.region.nb * kKeScanTile * 64;         // the kernel reads whole tiles: operands beyond n are zero
    p.slice_tiles = !s.exact ? p.my_tiles : k.tiles_per_launch > 0 && k.tiles_per_launch < kScanMaxLaunchTiles ? k.tiles_per_launch : kScanMaxLaunchTiles;
    p.n_slices = p.my_tiles > 0 ? (p.my_tiles + p.slice_tiles - 1) / p.slice_tiles : 0;
    p.refusal = p.wide_sort && s.n > 0xffffffffLL                                          ? KE_SCAN_WIDE_NEEDS_32_BITS
                : !s.exact && p.my_tiles > 0x7fffffffLL                                    ? KE_SCAN_TOO_MANY_TILES
                : !s.exact && cross && !p.buckets && p.my_tiles > kScanMaxLaunchTiles ? KE_SCAN_CROSS_OVER_ONE_LAUNCH
                                                                                           : KE_SCAN_FITS;
    return p;
}

// slice i of [0, n_slices)
inline KeScanSlice ke_scan_slice(const KeScanPlan &p, int64_t i) {
    const int64_t s0 = i * p.slice_tiles, left = p.my_tiles - s0;
    return {p.part_index + s0 * p.part_count, left < p.slice_tiles ? left : p.slice_tiles};
}
