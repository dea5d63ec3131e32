// ke_nearest_core.h -- the arithmetic of ke_hamming_nearest (include/keyes.h) as pure functions, shared by the HIP kernel
// (ke_nearest.hip) and by the host build the tests hold against the definition (tests/_nearest_core_cpu.cpp).
//
// One query against a table of n hashes.  S = the entries within max_distance of the query that the id rule does not take
// out; the answer is the first min(k, |S|) of S by (distance, position).  The kernel never sorts S: it counts S by distance
// (65 bins), finds from the counts the distance d* at which the k-th entry lies (THE CUT), then collects every entry below d*
// and the first `take` entries AT d* in position order, and sorts those k keys or fewer.
//
// THE WALK.  The table is cut into KE_NEAREST_WAVES contiguous segments of ke_nearest_seg_len(n) positions (a multiple of 64),
// one per wave of the workgroup; a wave reads its segment front to back: first whole blocks of KE_NEAREST_BLOCK positions, two
// at a time (one is in flight while the other is worked on), up to ke_nearest_full_end; then the rest, fewer than two blocks,
// 64 positions a step.  In pass 2 lane l of a step holds the position base + l, so that a ballot is in position order; in
// the blocks of pass 1, where only the wave's sums matter, a lane holds two neighbouring positions (ke_nearest_slot_position).
// Both passes cover the same segments, so pass 1 leaves in the columns of wave w exactly the counts of segment w: the entries at
// d* that lie before a wave's segment, and the entries below d* inside it, are known before pass 2 starts, and the waves of
// pass 2 never wait for one another.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define KE_NEAREST_HD __host__ __device__ static inline
#else
#define KE_NEAREST_HD static inline
#endif

#define KE_NEAREST_BINS 65         // distances 0..64
#define KE_NEAREST_WAVES 4         // waves of a workgroup = segments of the table
#define KE_NEAREST_LANES 64
#define KE_NEAREST_THREADS (KE_NEAREST_WAVES * KE_NEAREST_LANES)
#ifndef KE_NEAREST_STEPS
#define KE_NEAREST_STEPS 8         // steps of 64 positions in one block of the walk: 512 positions, 4 KiB of hashes per wave
#endif
#define KE_NEAREST_BLOCK (KE_NEAREST_STEPS * KE_NEAREST_LANES)
#define KE_NEAREST_K_LIMIT 1024    // KE_NEAREST_MAX_K of include/keyes.h: the keys of one query fit 8 KiB of LDS

struct KeNearestCut {
    int32_t dstar;   // every entry of S below this distance is taken; max_distance + 1 when all of S is
    int32_t take;    // entries taken AT dstar, the first ones in position order; 0 when all of S is taken
    int32_t count;   // min(k, |S|) = entries below dstar + take
};

// hist[d] = entries of S at distance d, KE_NEAREST_BINS of them (bins above max_distance do not count).  Every bin is read
// whatever the answer, and nothing is branched on: on the device the 65 reads are under way together.
KE_NEAREST_HD KeNearestCut ke_nearest_cut(const uint32_t *hist, int32_t k, int32_t max_distance) {
    KeNearestCut c;
    c.dstar = max_distance + 1;
    c.take = 0;
    int64_t below = 0;     // entries of S below d, while the cut has not been found; then frozen
    int found = 0;
    for (int32_t d = 0; d < KE_NEAREST_BINS; ++d) {
        const int64_t here = d <= max_distance ? (int64_t)hist[d] : 0;
        const int hit = !found && below + here >= k;
        c.dstar = hit ? d : c.dstar;
        c.take = hit ? (int32_t)(k - below) : c.take;
        found |= hit;
        below += found ? 0 : here;
    }
    c.count = found ? k : (int32_t)below;
    return c;
}

// |S| from the same counts
KE_NEAREST_HD int64_t ke_nearest_within(const uint32_t *hist, int32_t max_distance) {
    int64_t s = 0;
    for (int32_t d = 0; d < KE_NEAREST_BINS; ++d) s += d <= max_distance ? (int64_t)hist[d] : 0;
    return s;
}

// the sort key: ascending keys are (distance ascending, position ascending)
KE_NEAREST_HD uint64_t ke_nearest_key(uint32_t distance, uint32_t position) { return (uint64_t)distance << 32 | position; }
KE_NEAREST_HD uint32_t ke_nearest_key_distance(uint64_t key) { return (uint32_t)(key >> 32); }
KE_NEAREST_HD uint32_t ke_nearest_key_position(uint64_t key) { return (uint32_t)key; }

// positions of one segment: ceil(n / waves) rounded up to whole steps of 64
KE_NEAREST_HD int64_t ke_nearest_seg_len(int64_t n) {
    const int64_t per = (int64_t)KE_NEAREST_WAVES * KE_NEAREST_LANES;
    return (n + per - 1) / per * KE_NEAREST_LANES;
}
KE_NEAREST_HD int64_t ke_nearest_seg_lo(int64_t n, int wave) {
    const int64_t at = ke_nearest_seg_len(n) * wave;
    return at < n ? at : n;
}
KE_NEAREST_HD int64_t ke_nearest_seg_hi(int64_t n, int wave) { return ke_nearest_seg_lo(n, wave + 1); }

// where the whole pairs of blocks of the segment [lo, hi) end
KE_NEAREST_HD uint32_t ke_nearest_full_end(uint32_t lo, uint32_t hi) { return lo + (hi - lo) / (2u * KE_NEAREST_BLOCK) * (2u * KE_NEAREST_BLOCK); }
// The position of slot u (0 .. KE_NEAREST_STEPS - 1) of a lane in the block at `base`.  paired (pass 1): slots 2 j and 2 j + 1 are
// neighbours, one 16-byte load; otherwise (pass 2) slot u is step u, lane = position mod 64.
KE_NEAREST_HD uint32_t ke_nearest_slot_position(int paired, uint32_t base, uint32_t lane, int u) {
    return paired ? base + (uint32_t)(u >> 1) * 2u * KE_NEAREST_LANES + 2u * lane + (uint32_t)(u & 1) : base + (uint32_t)u * KE_NEAREST_LANES + lane;
}

// the word of (bin, thread) in the workgroup's histogram: a column per thread, so the bank is the lane whatever the bin
KE_NEAREST_HD uint32_t ke_nearest_hist_at(uint32_t bin, uint32_t thread) { return bin * KE_NEAREST_THREADS + thread; }

// keys the bitonic network sorts for `count` entries: the next power of two, the rest padded with ~0
KE_NEAREST_HD int32_t ke_nearest_sort_len(int32_t count) {
    int32_t p = 1;
    while (p < count) p <<= 1;
    return p;
}
// compare-exchange t of the step (size, stride) of a bitonic network: the lower index of the pair and its direction
KE_NEAREST_HD int32_t ke_nearest_bitonic_lo(int32_t t, int32_t stride) { return 2 * t - (t & (stride - 1)); }
KE_NEAREST_HD int ke_nearest_bitonic_up(int32_t lo, int32_t size) { return (lo & size) == 0; }
