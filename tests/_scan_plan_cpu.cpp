// ke_scan_plan.h compiled for the CPU with the sanitizers on: what tests/test_scan_plan_cpu.py builds and runs.
// Every plan of the lists in main() is held to expectations written out here from the rules the header states -- region and
// shard, the bucket rule's yardstick, which of histogram / bucket kernels / hist-pairs / wide sort run, the sizes of the
// buffers, the refusals -- and its slices are walked slot by slot.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "ke_scan_plan.h"

static int failures = 0;
static const char *what = "";
static char where[256];

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond) && ++failures <= 20) std::printf("FAIL %s: %s [%s]\n", what, #cond, where); \
    } while (0)

static const int64_t kTwo32 = (int64_t)1 << 32;
static const int64_t kMaxLaunch = 8388607;             // 0xffffffff / 512

// the walk over the slices of a plan, slot by slot where that is affordable
static void walk_slices(const KeScanPlan &p, const KeScanShape &s, int64_t limit) {
    what = "slices";
    const int64_t want_slices = p.my_tiles == 0 ? 0 : s.exact ? (p.my_tiles + limit - 1) / limit : 1;
    CHECK(p.n_slices == want_slices);
    int64_t slot = 0;
    for (int64_t i = 0; i < p.n_slices; ++i) {
        const KeScanSlice sl = ke_scan_slice(p, i);
        CHECK(sl.count >= 1);
        CHECK(!s.exact || sl.count <= limit);
        CHECK(sl.first_tile == s.part_index + slot * s.part_count);
        if (p.my_tiles <= 20000) {
            for (int64_t k = 0; k < sl.count; ++k, ++slot) {
                const int64_t tile = sl.first_tile + k * s.part_count;     // what workgroup k of the launch computes
                CHECK(tile == s.part_index + slot * s.part_count);
                CHECK(tile < p.n_tiles);
            }
        } else {
            slot += sl.count;
        }
    }
    CHECK(slot == p.my_tiles);                         // every slot once, in order, none beyond
}

struct Bands { int bits, count; };

static int one_plan(const KeScanShape &s, const KeScanKnobs &k, uint64_t shard_pairs, int64_t shard_tiles, int64_t region_tiles) {
    std::snprintf(where, sizeof where, "n=%lld f=%lld kind=%d shard=%d/%d bands=%dx%d cap=%lld exact=%d want=%d allowed=%d forced=%d per=%lld",
                  (long long)s.n, (long long)s.first_new, (int)s.kind, s.part_index, s.part_count, s.band_bits, s.band_count,
                  (long long)s.bucket_pair_cap, (int)s.exact, (int)s.want_bucket_pairs, (int)s.buckets_allowed, k.forced,
                  (long long)k.tiles_per_launch);
    const KeScanPlan p = ke_scan_plan(s, k);
    const uint64_t n = (uint64_t)s.n, f = (uint64_t)s.first_new;
    const bool cross = s.kind == KE_SCAN_CROSS, all = s.kind == KE_SCAN_ALL || (s.kind == KE_SCAN_FROM && s.first_new == 0);

    what = "region";
    CHECK(p.kind == (all ? KE_SCAN_ALL : s.kind));
    CHECK(p.n_tiles == region_tiles && p.region.n_tiles == region_tiles);
    CHECK(p.region.n == s.n && p.region.first_new == s.first_new);
    CHECK(p.my_tiles == shard_tiles);
    CHECK(p.pairs == shard_pairs);
    const uint64_t region_pairs = cross ? f * (n - f) : n * (n - 1) / 2 - (f ? f * (f - 1) / 2 : 0);
    CHECK(p.region_pairs == region_pairs);
    if (s.part_count == 1) CHECK(p.pairs == region_pairs);
    CHECK(p.bucket_threshold == region_pairs / (all ? 6000u : 1000u));

    what = "paths";
    const uint64_t cap = !s.exact && s.bucket_pair_cap > 0 ? (uint64_t)s.bucket_pair_cap : 0;
    const bool want = !s.exact && s.want_bucket_pairs;
    const bool table = s.band_bits <= 24;
    const size_t bins = table ? (size_t)s.band_count << s.band_bits : 0;
    const bool buckets = s.buckets_allowed && !s.exact && table && bins <= 262144 && s.n <= 4294967295LL && k.forced != 1 &&
                         (k.forced == 2 || s.n >= 50000);
    const bool need_hist = table && (buckets || cap > 0 || want);
    CHECK(p.cap == cap);
    CHECK(p.table == table && p.bins == bins);
    CHECK(p.buckets == buckets);
    CHECK(p.need_hist == need_hist);
    CHECK(p.hist_pairs == (need_hist && !buckets && want));
    CHECK(p.wide_sort == (!table && (cap > 0 || want)));
    if (s.exact) CHECK(!p.buckets && !p.need_hist && !p.hist_pairs && !p.wide_sort && p.cap == 0);

    what = "sizes";
    CHECK(p.sort_bytes == (buckets ? (size_t)s.band_count * (size_t)s.n * 12 + bins * 4 : 0));
    CHECK(p.hist_at == 1152);
    CHECK(p.state_bytes == ((1152 + (need_hist ? bins * 4 : 0) + 15) / 16) * 16);
    CHECK(p.exp_bytes == (size_t)((s.n + 1023) / 1024) * 1024 * 64);
    if (s.exact) CHECK(p.sort_bytes == 0 && p.state_bytes == 1152);

    what = "refusal";
    const int refusal = !table && (cap > 0 || want) && s.n > 4294967295LL ? KE_SCAN_WIDE_NEEDS_32_BITS
                        : !s.exact && shard_tiles > 2147483647LL          ? KE_SCAN_TOO_MANY_TILES
                        : !s.exact && cross && !buckets && shard_tiles > kMaxLaunch ? KE_SCAN_CROSS_OVER_ONE_LAUNCH
                                                                           : KE_SCAN_FITS;
    CHECK(p.refusal == refusal);

    const int64_t limit = k.tiles_per_launch >= 1 && k.tiles_per_launch < kMaxLaunch ? k.tiles_per_launch : kMaxLaunch;
    walk_slices(p, s, limit);
    return p.refusal;
}

// tiles of the region, counted from its definition: row block rb owns the chunks from max(rb, first_new / 1024) on (ALL, FROM), the
// row blocks that hold a row below first_new own the chunks from first_new's on (CROSS)
static int64_t count_tiles(int64_t n, int64_t f, KeScanKind kind) {
    const int64_t nb = (n + 1023) / 1024, c0 = f / 1024;
    if (kind == KE_SCAN_CROSS) return f <= 0 || f >= n ? 0 : ((f + 1023) / 1024) * (nb - c0);
    if (f >= n) return 0;
    const int64_t rect = c0 + 1 < nb ? c0 + 1 : nb;         // row blocks 0 .. c0 own nb - c0 chunks each, row block rb > c0 owns nb - rb
    return rect * (nb - c0) + (nb - rect) * (nb - rect + 1) / 2;
}

int main() {
    int cases = 0;
    const int64_t sizes[] = {2, 1023, 1024, 1025, 2049, 5000, 49999, 50000, 4193280, 4193281, kTwo32};
    const int shards[][2] = {{0, 1}, {0, 3}, {2, 3}, {7, 8}};
    const Bands bands[] = {{16, 4}, {17, 3}, {24, 2}, {25, 2}, {1, 64}};
    const int64_t per_launch[] = {0, 1, 3, 8, (int64_t)1 << 40};
    for (int64_t n : sizes) {
        const bool huge = n == kTwo32;                      // a triangle's pair count walks 4 million row blocks there: few cases
        for (KeScanKind kind : {KE_SCAN_ALL, KE_SCAN_FROM, KE_SCAN_CROSS}) {
            for (int64_t f : {(int64_t)0, (int64_t)1, (int64_t)1024, (int64_t)1025, n - 1, n}) {
                if (f > n || (kind == KE_SCAN_ALL && f != 0) || (huge && (kind == KE_SCAN_FROM || (f != 0 && f != 1025)))) continue;
                const int64_t region_tiles = count_tiles(n, f, kind);
                for (const auto &sh : shards) {
                    if (huge && sh[1] != 1) continue;
                    // the shard's part by the rules: tiles sh[0], sh[0] + sh[1], ... of the enumeration; its pairs from the region's functions
                    const int64_t shard_tiles = region_tiles > sh[0] ? (region_tiles - sh[0] + sh[1] - 1) / sh[1] : 0;
                    const KeScanRegion r = kind == KE_SCAN_CROSS ? ke_cross_region(n, f) : ke_scan_region(n, f);
                    const uint64_t shard_pairs = kind == KE_SCAN_CROSS ? ke_cross_shard_pairs(r, sh[0], sh[1]) : ke_region_shard_pairs(r, sh[0], sh[1]);
                    for (const Bands &b : bands)
                        for (int forced : {KE_SCAN_AUTO, KE_SCAN_FORCE_TILES, KE_SCAN_FORCE_BUCKETS})
                            for (int64_t cap : {(int64_t)0, (int64_t)5})
                                for (int flags = 0; flags < 8; ++flags) {
                                    if (huge && (forced != KE_SCAN_AUTO || (flags & 4) || (b.bits != 25 && (b.bits != 16 || kind != KE_SCAN_CROSS)))) continue;
                                    KeScanShape s;
                                    s.n = n; s.first_new = f; s.kind = kind;
                                    s.part_index = sh[0]; s.part_count = sh[1];
                                    s.band_bits = b.bits; s.band_count = b.count;
                                    s.bucket_pair_cap = cap;
                                    s.want_bucket_pairs = flags & 1; s.exact = flags & 2; s.buckets_allowed = !(flags & 4);
                                    KeScanKnobs k;
                                    k.forced = forced;
                                    // every slice size where the plan has slices to cut and they can be walked; the default elsewhere
                                    for (int64_t per : per_launch) {
                                        if (per != 0 && !(s.exact && forced == KE_SCAN_AUTO && cap == 0 && b.bits == 16)) continue;
                                        if (per != 0 && per <= 8 && shard_tiles > 20000) continue;
                                        k.tiles_per_launch = per;
                                        one_plan(s, k, shard_pairs, shard_tiles, region_tiles);
                                        ++cases;
                                    }
                                }
                }
            }
        }
    }

    // The boundaries by name.  where[] is one_plan's.
    what = "named";
    KeScanShape s;
    KeScanKnobs k;
    auto plan = [&](int64_t n, int64_t f, KeScanKind kind) {
        s.n = n; s.first_new = f; s.kind = kind;
        std::snprintf(where, sizeof where, "n=%lld f=%lld kind=%d", (long long)n, (long long)f, (int)kind);
        return ke_scan_plan(s, k);
    };
    // kBucketMinN, and KE_SCAN_MODE=buckets below it
    CHECK(!plan(49999, 0, KE_SCAN_ALL).buckets && plan(50000, 0, KE_SCAN_ALL).buckets);
    k.forced = KE_SCAN_FORCE_BUCKETS;
    CHECK(plan(5000, 0, KE_SCAN_ALL).buckets && plan(5000, 0, KE_SCAN_ALL).sort_bytes == (size_t)4 * 5000 * 12 + 262144 * 4);
    k.forced = KE_SCAN_FORCE_TILES;
    CHECK(!plan(50000, 0, KE_SCAN_ALL).buckets);
    k.forced = KE_SCAN_AUTO;
    // 2^18 bins is the last table with buckets; 393 216 bins still have a histogram when something needs it
    s.band_bits = 17; s.band_count = 3; s.bucket_pair_cap = 5;
    CHECK(!plan(50000, 0, KE_SCAN_ALL).buckets && plan(50000, 0, KE_SCAN_ALL).need_hist && plan(50000, 0, KE_SCAN_ALL).bins == 393216);
    s.bucket_pair_cap = 0;
    CHECK(!plan(50000, 0, KE_SCAN_ALL).need_hist && plan(50000, 0, KE_SCAN_ALL).state_bytes == 1152);
    // the re-plan after a refused sort buffer: no buckets, and the histogram only if the cap or the count still needs it
    s.band_bits = 16; s.band_count = 4; s.buckets_allowed = false;
    CHECK(!plan(50000, 0, KE_SCAN_ALL).buckets && !plan(50000, 0, KE_SCAN_ALL).need_hist && plan(50000, 0, KE_SCAN_ALL).sort_bytes == 0);
    s.want_bucket_pairs = true;
    CHECK(plan(50000, 0, KE_SCAN_ALL).need_hist && plan(50000, 0, KE_SCAN_ALL).hist_pairs);
    s.buckets_allowed = true;
    CHECK(plan(50000, 0, KE_SCAN_ALL).need_hist && !plan(50000, 0, KE_SCAN_ALL).hist_pairs);
    s.want_bucket_pairs = false;
    // 2^32 hashes: no bucket path; wide bands with a cap or the count are refused, without them and under exact they are not
    // (cross scans: their shard's pair count walks the library's row blocks only)
    CHECK(plan(kTwo32 - 1, 1025, KE_SCAN_CROSS).buckets && !plan(kTwo32, 1025, KE_SCAN_CROSS).buckets);
    s.band_bits = 25; s.band_count = 2;
    CHECK(plan(kTwo32, 1025, KE_SCAN_CROSS).refusal == KE_SCAN_FITS && !plan(kTwo32, 1025, KE_SCAN_CROSS).wide_sort);
    s.bucket_pair_cap = 5;
    CHECK(plan(kTwo32, 1025, KE_SCAN_CROSS).refusal == KE_SCAN_WIDE_NEEDS_32_BITS);
    CHECK(plan(kTwo32 - 1, 1025, KE_SCAN_CROSS).refusal == KE_SCAN_FITS && plan(kTwo32 - 1, 1025, KE_SCAN_CROSS).wide_sort);
    s.bucket_pair_cap = 0; s.want_bucket_pairs = true;
    CHECK(plan(kTwo32, 1025, KE_SCAN_CROSS).refusal == KE_SCAN_WIDE_NEEDS_32_BITS);
    s.exact = true;
    CHECK(plan(kTwo32, 1025, KE_SCAN_CROSS).refusal == KE_SCAN_FITS);
    s.want_bucket_pairs = false;
    s.exact = false; s.bucket_pair_cap = 0; s.band_bits = 16; s.band_count = 4;
    // too many tiles for one launch: 65 536 row blocks are 2^31 + 32 768 tiles of the triangle, 65 535 are 2^31 - 32 768
    CHECK(plan(65535 * 1024, 0, KE_SCAN_ALL).my_tiles == 2147450880LL && plan(65535 * 1024, 0, KE_SCAN_ALL).refusal == KE_SCAN_FITS);
    CHECK(plan(65535 * 1024 + 1, 0, KE_SCAN_ALL).my_tiles == 2147516416LL && plan(65535 * 1024 + 1, 0, KE_SCAN_ALL).refusal == KE_SCAN_TOO_MANY_TILES);
    CHECK(plan(65535 * 1024 + 1, 1, KE_SCAN_FROM).refusal == KE_SCAN_TOO_MANY_TILES);
    s.part_count = 2;
    CHECK(plan(65535 * 1024 + 1, 0, KE_SCAN_ALL).refusal == KE_SCAN_FITS);
    s.part_count = 1; s.exact = true;
    CHECK(plan(65535 * 1024 + 1, 0, KE_SCAN_ALL).refusal == KE_SCAN_FITS && plan(65535 * 1024 + 1, 0, KE_SCAN_ALL).n_slices == 257);
    s.exact = false;
    // the cross scan over one launch: [1024 | 8 388 607 x 1024] is one row block against 8 388 607 chunks, one more query adds a chunk.
    // Refused only where the tile kernel is the only path; the banded ALL and FROM scans of 4 193 281 keep their one slice.
    const int64_t q = kMaxLaunch * 1024;
    k.forced = KE_SCAN_FORCE_TILES;
    CHECK(plan(1024 + q, 1024, KE_SCAN_CROSS).my_tiles == kMaxLaunch && plan(1024 + q, 1024, KE_SCAN_CROSS).refusal == KE_SCAN_FITS);
    CHECK(plan(1025 + q, 1024, KE_SCAN_CROSS).my_tiles == kMaxLaunch + 1 && plan(1025 + q, 1024, KE_SCAN_CROSS).refusal == KE_SCAN_CROSS_OVER_ONE_LAUNCH);
    s.exact = true;
    CHECK(plan(1025 + q, 1024, KE_SCAN_CROSS).refusal == KE_SCAN_FITS && plan(1025 + q, 1024, KE_SCAN_CROSS).n_slices == 2);
    s.exact = false;
    // below 2^32 hashes the bucket path stands beside the tile kernel and the call goes through: three row blocks against
    // 2 796 202 chunks fit, against 2 796 203 they do not
    const int64_t three = 3 * 1024, wide = 2796203;
    CHECK(plan((3 + wide - 1) * 1024, three, KE_SCAN_CROSS).my_tiles == kMaxLaunch - 1 && plan((3 + wide - 1) * 1024, three, KE_SCAN_CROSS).refusal == KE_SCAN_FITS);
    CHECK(plan((3 + wide - 1) * 1024 + 1, three, KE_SCAN_CROSS).my_tiles == kMaxLaunch + 2 && plan((3 + wide - 1) * 1024 + 1, three, KE_SCAN_CROSS).refusal == KE_SCAN_CROSS_OVER_ONE_LAUNCH);
    k.forced = KE_SCAN_AUTO;
    CHECK(plan((3 + wide - 1) * 1024 + 1, three, KE_SCAN_CROSS).buckets && plan((3 + wide - 1) * 1024 + 1, three, KE_SCAN_CROSS).refusal == KE_SCAN_FITS);
    s.buckets_allowed = false;
    CHECK(plan((3 + wide - 1) * 1024 + 1, three, KE_SCAN_CROSS).refusal == KE_SCAN_CROSS_OVER_ONE_LAUNCH);
    s.buckets_allowed = true;
    k.forced = KE_SCAN_FORCE_TILES;
    CHECK(plan(4193280, 0, KE_SCAN_ALL).my_tiles == 8386560 && plan(4193281, 0, KE_SCAN_ALL).my_tiles == 8390656);
    CHECK(plan(4193281, 0, KE_SCAN_ALL).refusal == KE_SCAN_FITS && plan(4193281, 0, KE_SCAN_ALL).n_slices == 1);
    CHECK(ke_scan_slice(plan(4193281, 0, KE_SCAN_ALL), 0).count == 8390656);
    CHECK(plan(4193281, 1, KE_SCAN_FROM).refusal == KE_SCAN_FITS && plan(4193281, 1, KE_SCAN_FROM).n_slices == 1);
    s.exact = true;
    CHECK(plan(4193280, 0, KE_SCAN_ALL).n_slices == 1 && plan(4193281, 0, KE_SCAN_ALL).n_slices == 2);
    CHECK(ke_scan_slice(plan(4193281, 0, KE_SCAN_ALL), 1).count == 8390656 - kMaxLaunch);
    // the setting is clamped to what one launch holds
    k.tiles_per_launch = kMaxLaunch + 1;
    CHECK(plan(4193281, 0, KE_SCAN_ALL).n_slices == 2 && ke_scan_slice(plan(4193281, 0, KE_SCAN_ALL), 0).count == kMaxLaunch);
    k.tiles_per_launch = kMaxLaunch - 1;
    CHECK(ke_scan_slice(plan(4193281, 0, KE_SCAN_ALL), 0).count == kMaxLaunch - 1 && ke_scan_slice(plan(4193281, 0, KE_SCAN_ALL), 1).count == 2050);
    k.tiles_per_launch = -3;
    CHECK(ke_scan_slice(plan(4193281, 0, KE_SCAN_ALL), 0).count == kMaxLaunch);
    ++cases;

    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("ok cases=%d\n", cases);
    return 0;
}
