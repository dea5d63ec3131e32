// The cross region of ke_scan_region.h (the pairs i < first_new <= j of a table [library | queries]) compiled for the CPU:
// what tests/test_turned_cpu.py builds and runs, once plainly and once with the sanitizers on.
// usage: scan_cross_cpu FIRST_NEW...   (the list of tests/_scan_from_cases.py; n - 1 is added for every n)
// For every n of the list below and every first_new that fits: every pair i < first_new <= j lies in exactly one
// enumerated tile and no enumerated tile lies outside the table's tiling, the tile pair counts are the pair-by-pair
// counts and add up to first_new * (n - first_new), and the shard sums for 1, 3 and 8 parts equal the sums over the
// shards' tiles and add up to the same.
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

static void one_case(int64_t n, int64_t f) {
    const KeScanRegion r = ke_cross_region(n, f);
    const int64_t nb = (n + kKeScanTile - 1) / kKeScanTile, ncc = (n + kKeScanCols - 1) / kKeScanCols;
    CHECK(r.nb == nb && r.ncc == ncc, "n=%lld f=%lld", (long long)n, (long long)f);
    std::vector<int64_t> brute((size_t)(nb * ncc), 0), tile_pairs((size_t)(nb * ncc), 0);
    std::vector<char> seen((size_t)(nb * ncc), 0);
    for (int64_t j = f; j < n; ++j)
        for (int64_t i = 0; i < f; ++i) ++brute[(size_t)((i / kKeScanTile) * ncc + j / kKeScanCols)];
    std::vector<int64_t> ordinal_pairs((size_t)r.n_tiles, 0);
    for (int64_t t = 0; t < r.n_tiles; ++t) {
        int64_t rb = -1, cc = -1;
        ke_cross_tile(r, t, &rb, &cc);
        const bool inside = rb >= 0 && rb < nb && cc >= 0 && cc < ncc;
        CHECK(inside, "n=%lld f=%lld t=%lld -> (%lld, %lld)", (long long)n, (long long)f, (long long)t, (long long)rb, (long long)cc);
        if (!inside) continue;
        const size_t at = (size_t)(rb * ncc + cc);
        CHECK(!seen[at], "n=%lld f=%lld t=%lld -> (%lld, %lld) twice", (long long)n, (long long)f, (long long)t, (long long)rb, (long long)cc);
        seen[at] = 1;
        // the kernel's row blocks and chunks: rows below first_new, chunks from first_new's on
        CHECK(rb * kKeScanTile < f && (cc + 1) * kKeScanCols > f, "n=%lld f=%lld t=%lld -> (%lld, %lld) outside the rectangle", (long long)n,
              (long long)f, (long long)t, (long long)rb, (long long)cc);
        ordinal_pairs[(size_t)t] = tile_pairs[at] = ke_cross_tile_pairs(r, rb, cc);
    }
    uint64_t total = 0;
    for (size_t at = 0; at < brute.size(); ++at) {
        CHECK(!brute[at] || seen[at], "n=%lld f=%lld tile %zu holds pairs and is not enumerated", (long long)n, (long long)f, at);
        CHECK(brute[at] == tile_pairs[at], "n=%lld f=%lld tile %zu: %lld pairs, closed form %lld", (long long)n, (long long)f, at,
              (long long)brute[at], (long long)tile_pairs[at]);
        total += (uint64_t)tile_pairs[at];
    }
    const uint64_t closed = (uint64_t)f * (uint64_t)(n - f);
    CHECK(total == closed, "n=%lld f=%lld: tiles stand for %llu pairs, closed form %llu", (long long)n, (long long)f,
          (unsigned long long)total, (unsigned long long)closed);
    if (f == 0 || f == n) CHECK(r.n_tiles == 0, "n=%lld f=%lld: %lld tiles of an empty region", (long long)n, (long long)f, (long long)r.n_tiles);
    const int part_counts[] = {1, 3, 8};
    for (int pc : part_counts) {
        uint64_t sum = 0;
        for (int pi = 0; pi < pc; ++pi) {
            uint64_t by_tile = 0;
            for (int64_t t = pi; t < r.n_tiles; t += pc) by_tile += (uint64_t)ordinal_pairs[(size_t)t];
            const uint64_t got = ke_cross_shard_pairs(r, pi, pc);
            CHECK(got == by_tile, "n=%lld f=%lld shard %d/%d: %llu, over its tiles %llu", (long long)n, (long long)f, pi, pc,
                  (unsigned long long)got, (unsigned long long)by_tile);
            sum += got;
        }
        CHECK(sum == closed, "n=%lld f=%lld parts=%d: %llu pairs, closed form %llu", (long long)n, (long long)f, pc,
              (unsigned long long)sum, (unsigned long long)closed);
    }
}

int main(int argc, char **argv) {
    const int64_t sizes[] = {1, 2, 1023, 1024, 1025, 2500, 5000};
    int cases = 0;
    for (int64_t n : sizes) {
        std::vector<int64_t> firsts;
        for (int k = 1; k < argc; ++k) firsts.push_back(std::atoll(argv[k]));
        firsts.push_back(n - 1);
        for (int64_t f : firsts) {
            if (f < 0 || f > n) continue;
            one_case(n, f);
            ++cases;
        }
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("ok cases=%d\n", cases);
    return 0;
}
