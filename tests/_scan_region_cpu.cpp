// ke_scan_region.h compiled for the CPU with the sanitizers on: what tests/test_scan_region_cpu.py builds and runs.
// For every (n, first_new, part_count) of the lists below: the map t -> (rb, cc) hits every tile of the region once and
// no other, the shards' tile counts add up, every shard's closed-form pair count equals the sum over its tiles, and the
// shards together stand for n (n - 1) / 2 - f (f - 1) / 2 pairs.  Small tables are also enumerated pair by pair.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ke_scan_region.h"

static int failures = 0;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++failures <= 20) {                       \
                std::printf("FAIL %s: ", #cond);          \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

static void one_case(int64_t n, int64_t f, bool pair_by_pair) {
    const KeScanRegion r = ke_scan_region(n, f);
    const int64_t nb = (n + kKeScanTile - 1) / kKeScanTile, ncc = (n + kKeScanCols - 1) / kKeScanCols;
    CHECK(r.nb == nb && r.ncc == ncc, "n=%lld f=%lld", (long long)n, (long long)f);
    // the region's tiles by the issue's definition
    std::vector<char> want((size_t)(nb * ncc), 0), seen((size_t)(nb * ncc), 0);
    int64_t want_tiles = 0;
    if (f < n)
        for (int64_t rb = 0; rb < nb; ++rb)
            for (int64_t cc = (kKeScanCPR * rb > f / kKeScanCols ? kKeScanCPR * rb : f / kKeScanCols); cc < ncc; ++cc) {
                want[(size_t)(rb * ncc + cc)] = 1;
                ++want_tiles;
            }
    CHECK(r.n_tiles == want_tiles, "n=%lld f=%lld tiles %lld want %lld", (long long)n, (long long)f, (long long)r.n_tiles, (long long)want_tiles);
    CHECK(ke_region_offset(r, nb) == r.n_tiles || r.n_tiles == 0, "n=%lld f=%lld offset(nb)", (long long)n, (long long)f);
    std::vector<int64_t> tile_pairs((size_t)(nb * ncc), 0);
    std::vector<int64_t> ordinal_pairs((size_t)r.n_tiles, 0);
    for (int64_t t = 0; t < r.n_tiles; ++t) {
        int64_t rb = -1, cc = -1;
        ke_region_tile(r, t, &rb, &cc);
        const bool inside = rb >= 0 && rb < nb && cc >= 0 && cc < ncc;
        CHECK(inside, "n=%lld f=%lld t=%lld -> (%lld, %lld)", (long long)n, (long long)f, (long long)t, (long long)rb, (long long)cc);
        if (!inside) continue;
        const size_t at = (size_t)(rb * ncc + cc);
        CHECK(want[at], "n=%lld f=%lld t=%lld -> (%lld, %lld) outside the region", (long long)n, (long long)f, (long long)t, (long long)rb, (long long)cc);
        CHECK(!seen[at], "n=%lld f=%lld t=%lld -> (%lld, %lld) twice", (long long)n, (long long)f, (long long)t, (long long)rb, (long long)cc);
        CHECK(ke_region_offset(r, rb) <= t && t < ke_region_offset(r, rb + 1), "n=%lld f=%lld t=%lld offset", (long long)n, (long long)f, (long long)t);
        seen[at] = 1;
        ordinal_pairs[(size_t)t] = tile_pairs[at] = ke_region_tile_pairs(r, rb, cc);
    }
    if (pair_by_pair) {
        std::vector<int64_t> brute((size_t)(nb * ncc), 0);
        for (int64_t j = f; j < n; ++j)
            for (int64_t i = 0; i < j; ++i) ++brute[(size_t)((i / kKeScanTile) * ncc + j / kKeScanCols)];
        for (size_t at = 0; at < brute.size(); ++at) {
            CHECK(!brute[at] || want[at], "n=%lld f=%lld tile %zu holds pairs outside the region", (long long)n, (long long)f, at);
            CHECK(brute[at] == tile_pairs[at], "n=%lld f=%lld tile %zu: %lld pairs, closed form %lld", (long long)n, (long long)f, at,
                  (long long)brute[at], (long long)tile_pairs[at]);
        }
    }
    const uint64_t un = (uint64_t)n, uf = (uint64_t)f;
    const uint64_t closed = (n ? un * (un - 1) / 2 : 0) - (f ? uf * (uf - 1) / 2 : 0);
    const int part_counts[] = {1, 3, 8};
    for (int pc : part_counts) {
        uint64_t sum = 0;
        int64_t tiles = 0;
        for (int pi = 0; pi < pc; ++pi) {
            uint64_t by_tile = 0;
            for (int64_t t = pi; t < r.n_tiles; t += pc) by_tile += (uint64_t)ordinal_pairs[(size_t)t];
            const uint64_t got = ke_region_shard_pairs(r, pi, pc);
            CHECK(got == by_tile, "n=%lld f=%lld shard %d/%d: %llu, over its tiles %llu", (long long)n, (long long)f, pi, pc,
                  (unsigned long long)got, (unsigned long long)by_tile);
            sum += got;
            tiles += ke_region_shard_tiles(r, pi, pc);
        }
        CHECK(sum == closed, "n=%lld f=%lld parts=%d: %llu pairs, closed form %llu", (long long)n, (long long)f, pc,
              (unsigned long long)sum, (unsigned long long)closed);
        CHECK(tiles == r.n_tiles, "n=%lld f=%lld parts=%d: %lld tiles of %lld", (long long)n, (long long)f, pc, (long long)tiles, (long long)r.n_tiles);
    }
}

int main() {
    const int64_t sizes[] = {1, 2, 1023, 1024, 1025, 2048, 2049, 3000, 5121, ((int64_t)1 << 20) + 1};
    int cases = 0;
    for (int64_t n : sizes) {
        const int64_t firsts[] = {0, 1, 15, 16, 17, 1023, 1024, 1025, n - 1, n};
        for (int64_t f : firsts) {
            if (f < 0 || f > n) continue;
            one_case(n, f, n <= 5121);
            ++cases;
        }
    }
    // first_new = 0 is the whole triangle: the region's map is the triangle's
    {
        const KeScanRegion r = ke_scan_region(5121, 0);
        for (int64_t t = 0; t < r.n_tiles; ++t) {
            int64_t a, b, c, d;
            ke_region_tile(r, t, &a, &b);
            ke_tri_tile(t, r.nb, r.ncc, &c, &d);
            CHECK(a == c && b == d, "t=%lld", (long long)t);
        }
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("ok cases=%d\n", cases);
    return 0;
}
