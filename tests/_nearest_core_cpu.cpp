// Host build of csrc/ke_nearest_core.h for tests/test_nearest_core_cpu.py: the cut, the sort key and the two-pass walk of
// ke_hamming_nearest driven by host loops the way the kernel runs them -- a segment per wave, whole blocks then steps, a column of
// the histogram per thread, the ties placed by rank, the keys through the bitonic network.  With -DNEAREST_CORE_MAIN the same
// source is a program that holds the walk against the definition spelled out in C++ (built with AddressSanitizer and UBSan by
// the test; every buffer ends where its data ends).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "ke_nearest_core.h"

static int popcount64(uint64_t x) { return __builtin_popcountll(x); }

// One query the kernel's way.  Returns the number of things that must never happen (a key written outside its slots, a wave
// that finds more or fewer entries than pass 1 counted for it); the outputs are as ke_hamming_nearest's for one query.
static int64_t walk_one(const uint64_t *hashes, const int64_t *ids, int64_t n, uint64_t query, int has_qid, int64_t qid, int32_t k,
                        int32_t max_distance, int64_t *index_out, int32_t *distance_out, int32_t *count_out, int64_t *within_out,
                        uint32_t *histogram_out) {
    int64_t faults = 0;
    const bool with_ids = ids && has_qid;
    std::vector<uint32_t> hist((size_t)KE_NEAREST_BINS * KE_NEAREST_THREADS, 0u);
    for (int w = 0; w < KE_NEAREST_WAVES; ++w) {                                       // pass 1
        const int64_t lo = ke_nearest_seg_lo(n, w), hi = ke_nearest_seg_hi(n, w);
        if ((hi - lo) > ke_nearest_seg_len(n) || lo > hi || (w == 0 && lo != 0) || (w == KE_NEAREST_WAVES - 1 && hi != n)) ++faults;
        const int64_t full = ke_nearest_full_end((uint32_t)lo, (uint32_t)hi);
        if (full < lo || full > hi || (full - lo) % (2 * KE_NEAREST_BLOCK) || hi - full >= 2 * KE_NEAREST_BLOCK) ++faults;
        auto count = [&](int64_t p, int l) {
            if (p < lo || p >= hi) { ++faults; return; }
            if (with_ids && ids[p] == qid) return;
            hist[ke_nearest_hist_at((uint32_t)popcount64(hashes[p] ^ query), (uint32_t)(w * KE_NEAREST_LANES + l))] += 1;
        };
        for (int64_t base = lo; base < full; base += KE_NEAREST_BLOCK)                  // whole blocks: a lane owns neighbours
            for (int l = 0; l < KE_NEAREST_LANES; ++l)
                for (int u = 0; u < KE_NEAREST_STEPS; ++u) count(ke_nearest_slot_position(1, (uint32_t)base, (uint32_t)l, u), l);
        for (int64_t base = full; base < hi; base += KE_NEAREST_LANES)                  // the rest, a step at a time
            for (int l = 0; l < KE_NEAREST_LANES; ++l)
                if (base + l < hi) count(base + l, l);
    }
    uint32_t seg[KE_NEAREST_BINS][KE_NEAREST_WAVES], tot[KE_NEAREST_BINS];
    for (int b = 0; b < KE_NEAREST_BINS; ++b) {
        tot[b] = 0;
        for (int w = 0; w < KE_NEAREST_WAVES; ++w) {
            seg[b][w] = 0;
            for (int l = 0; l < KE_NEAREST_LANES; ++l) seg[b][w] += hist[ke_nearest_hist_at((uint32_t)b, (uint32_t)(w * KE_NEAREST_LANES + l))];
            tot[b] += seg[b][w];
        }
    }
    const KeNearestCut cut = ke_nearest_cut(tot, k, max_distance);
    const uint32_t dstar = (uint32_t)cut.dstar, take = (uint32_t)cut.take, n_below = (uint32_t)(cut.count - cut.take);
    std::vector<uint64_t> keys((size_t)ke_nearest_sort_len(cut.count), ~0ull);       // no more slots than the sort needs
    std::vector<uint8_t> written(keys.size(), 0);
    uint32_t cursor = 0;
    for (int w = KE_NEAREST_WAVES - 1; w >= 0; --w) {                                  // pass 2: the waves in any order
        const int64_t lo = ke_nearest_seg_lo(n, w), hi = ke_nearest_seg_hi(n, w);
        uint32_t taken = take, mine = 0;
        if (take > 0) {
            taken = 0;
            for (int v = 0; v < w; ++v) taken += seg[dstar][v];
        }
        for (uint32_t b = 0; b < dstar; ++b) mine += seg[b][w];
        // one step of 64 positions, the lanes in order: what a ballot and its prefix count give
        auto step = [&](int64_t base) {
            uint32_t ties = 0, found = 0;
            for (int l = 0; l < KE_NEAREST_LANES; ++l) {
                const int64_t p = base + l;
                if (p >= hi) continue;
                if (with_ids && ids[p] == qid) continue;
                const uint32_t d = (uint32_t)popcount64(hashes[p] ^ query);
                if (d < dstar) {
                    const uint32_t slot = cursor++;
                    if (slot >= n_below || written[slot]) { ++faults; continue; }
                    keys[slot] = ke_nearest_key(d, (uint32_t)p);
                    written[slot] = 1;
                    ++found;
                } else if (d == dstar) {
                    const uint32_t rank = taken + ties++;
                    if (rank < take) {
                        if (n_below + rank >= keys.size() || written[n_below + rank]) { ++faults; continue; }
                        keys[n_below + rank] = ke_nearest_key(d, (uint32_t)p);
                        written[n_below + rank] = 1;
                    }
                }
            }
            if (found > mine) ++faults;
            mine -= std::min(found, mine);
            taken += ties;
        };
        const int64_t full = ke_nearest_full_end((uint32_t)lo, (uint32_t)hi);
        for (int64_t base = lo; base < full && (mine > 0 || taken < take); base += 2 * KE_NEAREST_BLOCK)   // pairs of blocks, both always
            for (int u = 0; u < 2 * KE_NEAREST_STEPS; ++u) {
                if (ke_nearest_slot_position(0, (uint32_t)base, 0, u % KE_NEAREST_STEPS) + (u / KE_NEAREST_STEPS) * KE_NEAREST_BLOCK !=
                    (uint32_t)(base + u * KE_NEAREST_LANES)) ++faults;
                step(base + u * KE_NEAREST_LANES);
            }
        for (int64_t base = full; base < hi && (mine > 0 || taken < take); base += KE_NEAREST_LANES) step(base);
        if (mine != 0) ++faults;                       // the segment ended before the wave had what pass 1 promised
    }
    for (int32_t j = 0; j < cut.count; ++j) faults += !written[(size_t)j];
    const int32_t len = (int32_t)keys.size();
    for (int32_t size = 2; size <= len; size <<= 1)
        for (int32_t stride = size >> 1; stride > 0; stride >>= 1)
            for (int32_t t = 0; t < len / 2; ++t) {
                const int32_t a = ke_nearest_bitonic_lo(t, stride), b = a + stride;
                if ((keys[(size_t)a] > keys[(size_t)b]) == (bool)ke_nearest_bitonic_up(a, size)) std::swap(keys[(size_t)a], keys[(size_t)b]);
            }
    for (int32_t j = 0; j < k; ++j) {
        const bool has = j < cut.count;
        index_out[j] = has ? (int64_t)ke_nearest_key_position(keys[(size_t)j]) : -1;
        distance_out[j] = has ? (int32_t)ke_nearest_key_distance(keys[(size_t)j]) : -1;
    }
    *count_out = cut.count;
    if (within_out) *within_out = ke_nearest_within(tot, max_distance);
    if (histogram_out)
        for (int b = 0; b < KE_NEAREST_BINS; ++b) histogram_out[b] = b <= max_distance ? tot[b] : 0u;
    return faults;
}

extern "C" {

void nr_cut(const uint32_t *hist, int32_t k, int32_t max_distance, int32_t out[3]) {
    const KeNearestCut c = ke_nearest_cut(hist, k, max_distance);
    out[0] = c.dstar;
    out[1] = c.take;
    out[2] = c.count;
}
int64_t nr_within(const uint32_t *hist, int32_t max_distance) { return ke_nearest_within(hist, max_distance); }
uint64_t nr_key(uint32_t distance, uint32_t position) { return ke_nearest_key(distance, position); }
uint32_t nr_key_distance(uint64_t key) { return ke_nearest_key_distance(key); }
uint32_t nr_key_position(uint64_t key) { return ke_nearest_key_position(key); }
int32_t nr_max_k(void) { return KE_NEAREST_K_LIMIT; }
int32_t nr_threads(void) { return KE_NEAREST_THREADS; }
int64_t nr_seg_lo(int64_t n, int32_t wave) { return ke_nearest_seg_lo(n, wave); }
int64_t nr_seg_hi(int64_t n, int32_t wave) { return ke_nearest_seg_hi(n, wave); }
int64_t nr_walk(const uint64_t *hashes, const int64_t *ids, int64_t n, uint64_t query, int32_t has_qid, int64_t qid, int32_t k,
                int32_t max_distance, int64_t *index_out, int32_t *distance_out, int32_t *count_out, int64_t *within_out,
                uint32_t *histogram_out) {
    return walk_one(hashes, ids, n, query, has_qid, qid, k, max_distance, index_out, distance_out, count_out, within_out, histogram_out);
}

}  // extern "C"

#ifdef NEAREST_CORE_MAIN
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {                                   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main() {
    const int64_t sizes[] = {1, 255, 256, 257, 1025};
    const int32_t ks[] = {1, 2, 7, 64, 1024};
    const int32_t limits[] = {0, 5, 31, 64};
    long cases = 0;
    for (int64_t n : sizes)
        for (int flavour = 0; flavour < 3; ++flavour) {   // random; all equal to the query; near the query with every id equal pairs
            const uint64_t query = rng();
            uint64_t *hashes = new uint64_t[(size_t)n];
            int64_t *ids = new int64_t[(size_t)n];
            for (int64_t i = 0; i < n; ++i) {
                uint64_t h = flavour == 1 ? query : rng();
                if (flavour == 2) {
                    h = query;
                    for (int b = (int)(rng() % 13); b > 0; --b) h ^= 1ull << (rng() % 64);
                }
                hashes[i] = h;
                ids[i] = i / 2;
            }
            for (int32_t k : ks)
                for (int32_t limit : limits)
                    for (int with_ids = 0; with_ids < 2; ++with_ids) {
                        const int64_t qid = (n - 1) / 2;
                        std::vector<std::pair<int32_t, int64_t>> want;               // the definition
                        uint32_t want_hist[KE_NEAREST_BINS] = {0};
                        for (int64_t i = 0; i < n; ++i) {
                            const int32_t d = popcount64(hashes[i] ^ query);
                            if (d > limit || (with_ids && ids[i] == qid)) continue;
                            want.push_back({d, i});
                            want_hist[d] += 1;
                        }
                        std::sort(want.begin(), want.end());
                        int64_t *index = new int64_t[(size_t)k];
                        int32_t *distance = new int32_t[(size_t)k];
                        uint32_t *hist = new uint32_t[KE_NEAREST_BINS];
                        int32_t count = -7;
                        int64_t within = -7;
                        const int64_t faults = walk_one(hashes, with_ids ? ids : nullptr, n, query, with_ids, qid, k, limit, index, distance,
                                                        &count, &within, hist);
                        bool ok = faults == 0 && within == (int64_t)want.size() && count == (int32_t)std::min<size_t>((size_t)k, want.size());
                        for (int32_t j = 0; ok && j < k; ++j)
                            ok = j < count ? (index[j] == want[(size_t)j].second && distance[j] == want[(size_t)j].first)
                                           : (index[j] == -1 && distance[j] == -1);
                        for (int b = 0; ok && b < KE_NEAREST_BINS; ++b) ok = hist[b] == want_hist[b];
                        delete[] index;
                        delete[] distance;
                        delete[] hist;
                        if (!ok) {
                            std::printf("mismatch n=%lld flavour=%d k=%d limit=%d ids=%d faults=%lld\n", (long long)n, flavour, k, limit, with_ids,
                                        (long long)faults);
                            return 1;
                        }
                        ++cases;
                    }
            delete[] hashes;
            delete[] ids;
        }
    std::printf("ok %ld\n", cases);
    return 0;
}
#endif
