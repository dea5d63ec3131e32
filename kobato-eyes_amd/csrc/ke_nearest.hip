// ke_nearest.hip -- ke_hamming_nearest (include/keyes.h): for every query the k nearest entries of a table of 64-bit hashes by
// Hamming distance, ties by position, with no band predicate.  The arithmetic -- the cut, the sort key, the walk -- is
// ke_nearest_core.h; this file is the kernel and the call around it.
//
// One workgroup of 256 lanes per query, two passes over the table, each wave over its own contiguous segment:
//   pass 1  counts the entries of S by distance.  A shared 65-bin histogram would serialise: distances of unrelated hashes
//           crowd into bins 26..38, so the 64 lanes of a wave would hit a handful of words.  Every lane has its own column
//           instead (hist[bin * 256 + thread], 65 KiB): the bank is the lane whatever the bin, no two lanes ever share a word,
//           and the increment is one LDS add that returns nothing.  The query's words are wave-uniform, so a pair costs two
//           xor, two bit counts (the second accumulating) and that add.
//           Whole blocks of 512 positions go two at a time through two register buffers, one in flight while the other is
//           counted; a lane loads two neighbouring hashes at once.
//   the cut is reduced from the columns per (bin, wave), which also tells every wave how many entries at d* lie before its
//           segment and how many entries below d* lie inside it.
//   pass 2  walks again.  Entries below d* (fewer than k) go through an LDS cursor in any order; of the entries at d* the
//           first `take` in position order are placed by rank: a ballot and a prefix count inside the wave, a running count
//           along the segment, the start from the cut's per-wave counts.  A wave stops once it has found what pass 1 promised.
//   then    a bitonic network sorts the min(k, |S|) keys in LDS and the row is written with ordinary vector stores.
// A table of n equal hashes therefore never needs more than k slots.  LDS: 65 KiB + 8 KiB of keys + 1.3 KiB: two workgroups
// on a compute unit.
#include "ke_internal.h"
#include "ke_nearest_core.h"

namespace {

constexpr int NEAREST_STEPS = KE_NEAREST_STEPS;
constexpr uint32_t NEAREST_BLOCK = KE_NEAREST_BLOCK;

template <bool IDS>
struct Block {
    uint64_t h[NEAREST_STEPS];
    int64_t id[IDS ? NEAREST_STEPS : 1];
};

typedef uint64_t HashPair __attribute__((ext_vector_type(2), aligned(8)));   // two neighbouring hashes, one 16-byte load

template <bool IDS, bool PAIRED>
__device__ inline void load_block(Block<IDS> &b, const uint64_t *__restrict__ hashes, const int64_t *__restrict__ ids, uint32_t base, uint32_t lane) {
#pragma unroll
    for (int u = 0; u < NEAREST_STEPS; u += PAIRED ? 2 : 1) {
        const uint32_t p = ke_nearest_slot_position(PAIRED, base, lane, u);
        if (PAIRED) {
            const HashPair two = *(const HashPair *)(hashes + p);
            b.h[u] = two.x;
            b.h[u + 1] = two.y;
            if (IDS) {
                const HashPair id = *(const HashPair *)(ids + p);
                b.id[u] = (int64_t)id.x;
                b.id[u + 1] = (int64_t)id.y;
            }
        } else {
            b.h[u] = hashes[p];
            if (IDS) b.id[u] = ids[p];
        }
    }
}

template <bool IDS>
__global__ __launch_bounds__(KE_NEAREST_THREADS) void ke_nearest_kernel(
    const uint64_t *__restrict__ hashes, const int64_t *__restrict__ ids, uint32_t n, const uint64_t *__restrict__ queries,
    const int64_t *__restrict__ query_ids, int64_t first_query, int32_t k, int32_t max_distance, int64_t *__restrict__ index_out,
    int32_t *__restrict__ distance_out, int32_t *__restrict__ count_out, int64_t *__restrict__ within_out,
    uint32_t *__restrict__ histogram_out) {
    __shared__ uint32_t hist[KE_NEAREST_BINS * KE_NEAREST_THREADS];
    __shared__ uint64_t keys[KE_NEAREST_K_LIMIT];
    __shared__ uint32_t seg[KE_NEAREST_BINS * KE_NEAREST_WAVES];   // entries of S per (bin, segment)
    __shared__ uint32_t tot[KE_NEAREST_BINS];
    __shared__ uint32_t cursor;

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int64_t q = first_query + blockIdx.x;
    const uint64_t qh = queries[q];
    int64_t qid = 0;
    if (IDS) qid = query_ids[q];
    const uint32_t lo = (uint32_t)ke_nearest_seg_lo(n, wave), hi = (uint32_t)ke_nearest_seg_hi(n, wave);
    const uint32_t full = ke_nearest_full_end(lo, hi);   // whole pairs of blocks end here; fewer than 1024 positions follow

    // ---- pass 1 -------------------------------------------------------------------------------------------------------
    for (uint32_t b = 0; b < KE_NEAREST_BINS; ++b) hist[ke_nearest_hist_at(b, tid)] = 0;   // the lane's own column: no barrier
    if (tid == 0) cursor = 0;
    // Whole blocks in pairs, two buffers: the loads of one block are under way while the other is counted.  Both are used on
    // every round -- a buffer used under a condition has its loads moved under it --, and past the last pair the even block is
    // asked for again at its old place rather than branched round.
    if (lo < full) {
        const uint32_t last = full - 2 * NEAREST_BLOCK;
        auto count_block = [&](const Block<IDS> &b) {
#pragma unroll
            for (int u = 0; u < NEAREST_STEPS; ++u)
                if (!IDS || b.id[u] != qid) atomicAdd(&hist[ke_nearest_hist_at((uint32_t)__popcll(b.h[u] ^ qh), tid)], 1u);
        };
        Block<IDS> even, odd;
        load_block<IDS, true>(even, hashes, ids, lo, lane);
        for (uint32_t base = lo; base < full; base += 2 * NEAREST_BLOCK) {
            load_block<IDS, true>(odd, hashes, ids, base + NEAREST_BLOCK, lane);
            count_block(even);
            load_block<IDS, true>(even, hashes, ids, min(base + 2 * NEAREST_BLOCK, last), lane);
            count_block(odd);
        }
    }
    for (uint32_t p = full + lane; p < hi; p += KE_NEAREST_LANES)
        if (!IDS || ids[p] != qid) atomicAdd(&hist[ke_nearest_hist_at((uint32_t)__popcll(hashes[p] ^ qh), tid)], 1u);
    __syncthreads();

    // ---- the cut ------------------------------------------------------------------------------------------------------
    // A thread per (bin, segment) adds the 64 columns of that segment, each lane starting at its own column: the lanes of a read
    // fall on different banks, and the 64 reads of a thread do not wait for one another.
    for (uint32_t pair = tid; pair < KE_NEAREST_BINS * KE_NEAREST_WAVES; pair += KE_NEAREST_THREADS) {
        const uint32_t first = ke_nearest_hist_at(pair / KE_NEAREST_WAVES, (pair % KE_NEAREST_WAVES) * KE_NEAREST_LANES);
        uint32_t s = 0;
#pragma unroll 16
        for (uint32_t j = 0; j < KE_NEAREST_LANES; ++j) s += hist[first + ((lane + j) & (KE_NEAREST_LANES - 1))];
        seg[pair] = s;
    }
    __syncthreads();
    if (tid < KE_NEAREST_BINS) {
        uint32_t s = 0;
        for (int w = 0; w < KE_NEAREST_WAVES; ++w) s += seg[tid * KE_NEAREST_WAVES + w];
        tot[tid] = s;
    }
    __syncthreads();
    const KeNearestCut cut = ke_nearest_cut(tot, k, max_distance);
    const uint32_t dstar = (uint32_t)cut.dstar, take = (uint32_t)cut.take, n_below = (uint32_t)(cut.count - cut.take);
    uint32_t taken = take, mine = 0;   // entries at d* before this wave's segment (take = 0: none wanted); entries below d* inside it
    if (take > 0) {
        taken = 0;
        for (int w = 0; w < wave; ++w) taken += seg[dstar * KE_NEAREST_WAVES + w];
    }
#pragma unroll
    for (uint32_t b = 0; b < KE_NEAREST_BINS; ++b) mine += b < dstar ? seg[b * KE_NEAREST_WAVES + wave] : 0u;   // every read asked for at once
    taken = __builtin_amdgcn_readfirstlane(taken);   // the same in every lane: the walk's exit test is a scalar one
    mine = __builtin_amdgcn_readfirstlane(mine);

    // ---- pass 2 -------------------------------------------------------------------------------------------------------
    // one step of 64 positions in position order: lane l holds position p, `in` = inside the segment and not excluded
    auto step = [&](uint64_t h, uint32_t p, bool in) {
        const uint32_t d = (uint32_t)__popcll(h ^ qh);
        const bool below = in && d < dstar, tie = in && d == dstar;
        const uint64_t m_below = __ballot(below), m_tie = __ballot(tie);
        if (below) {
            const uint32_t slot = atomicAdd(&cursor, 1u);
            if (slot < n_below) keys[slot] = ke_nearest_key(d, p);
        }
        if (tie) {
            const uint32_t rank = taken + __builtin_amdgcn_mbcnt_hi((uint32_t)(m_tie >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m_tie, 0u));
            if (rank < take) keys[n_below + rank] = ke_nearest_key(d, p);
        }
        const uint32_t found = (uint32_t)__popcll(m_below);
        mine = found < mine ? mine - found : 0;
        taken += (uint32_t)__popcll(m_tie);
    };
    if (lo < full && (mine > 0 || taken < take)) {
        const uint32_t last = full - 2 * NEAREST_BLOCK;
        auto place_block = [&](const Block<IDS> &b, uint32_t base) {
#pragma unroll
            for (int u = 0; u < NEAREST_STEPS; ++u) step(b.h[u], ke_nearest_slot_position(0, base, lane, u), !IDS || b.id[u] != qid);
        };
        Block<IDS> even, odd;
        load_block<IDS, false>(even, hashes, ids, lo, lane);
        for (uint32_t base = lo; base < full && (mine > 0 || taken < take); base += 2 * NEAREST_BLOCK) {
            load_block<IDS, false>(odd, hashes, ids, base + NEAREST_BLOCK, lane);
            place_block(even, base);
            load_block<IDS, false>(even, hashes, ids, min(base + 2 * NEAREST_BLOCK, last), lane);
            place_block(odd, base + NEAREST_BLOCK);       // nothing is left for it to take when the wave has all it wants
        }
    }
    for (uint32_t base = full; base < hi && (mine > 0 || taken < take); base += KE_NEAREST_LANES) {
        const uint32_t p = base + lane;
        const bool in = p < hi;
        step(in ? hashes[p] : 0, p, in && (!IDS || ids[p] != qid));
    }
    __syncthreads();

    // ---- sort and write -----------------------------------------------------------------------------------------------
    const int32_t count = cut.count, len = ke_nearest_sort_len(count);
    for (int32_t j = count + (int32_t)tid; j < len; j += KE_NEAREST_THREADS) keys[j] = ~0ull;
    for (int32_t size = 2; size <= len; size <<= 1)
        for (int32_t stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int32_t t = (int32_t)tid; t < len / 2; t += KE_NEAREST_THREADS) {
                const int32_t a = ke_nearest_bitonic_lo(t, stride), b = a + stride;
                const uint64_t ka = keys[a], kb = keys[b];
                if ((ka > kb) == (bool)ke_nearest_bitonic_up(a, size)) {
                    keys[a] = kb;
                    keys[b] = ka;
                }
            }
        }
    __syncthreads();
    const size_t row = (size_t)q * (size_t)k;
    for (int32_t j = (int32_t)tid; j < k; j += KE_NEAREST_THREADS) {
        const bool has = j < count;
        const uint64_t key = has ? keys[j] : 0;
        index_out[row + j] = has ? (int64_t)ke_nearest_key_position(key) : -1;
        distance_out[row + j] = has ? (int32_t)ke_nearest_key_distance(key) : -1;
    }
    if (tid == 0) {
        count_out[q] = count;
        if (within_out) within_out[q] = ke_nearest_within(tot, max_distance);
    }
    if (histogram_out && tid < KE_NEAREST_BINS) histogram_out[(size_t)q * KE_NEAREST_BINS + tid] = (int32_t)tid <= max_distance ? tot[tid] : 0u;
}

}  // namespace

static_assert(KE_NEAREST_K_LIMIT == KE_NEAREST_MAX_K, "the kernel's key slots are the header's limit");

KE_API int ke_hamming_nearest(ke_ctx *ctx, const uint64_t *hashes, const int64_t *ids, int64_t n, const uint64_t *queries,
                              const int64_t *query_ids, int64_t m, int32_t k, int32_t max_distance, int64_t *index_out,
                              int32_t *distance_out, int32_t *count_out, int64_t *within_out, uint32_t *histogram_out) {
    if (!ctx) return KE_EINVAL;
    if (k < 1 || k > KE_NEAREST_MAX_K) return ke_fail(ctx, KE_EINVAL, "k %d outside [1, %d]", k, KE_NEAREST_MAX_K);
    if (max_distance < 0 || max_distance > 64) return ke_fail(ctx, KE_EINVAL, "max_distance %d outside [0, 64]", max_distance);
    if (n < 0 || n > INT32_MAX) return ke_fail(ctx, KE_EINVAL, "n %lld outside [0, 2^31 - 1]", (long long)n);
    if (m < 0) return ke_fail(ctx, KE_EINVAL, "m %lld is negative", (long long)m);
    if (n > 0 && !hashes) return ke_fail(ctx, KE_EINVAL, "hashes is NULL");
    if (m == 0) return KE_OK;
    if (!queries) return ke_fail(ctx, KE_EINVAL, "queries is NULL");
    if (!index_out || !distance_out || !count_out) return ke_fail(ctx, KE_EINVAL, "index_out / distance_out / count_out is NULL");
    KE_HIP(ctx, hipSetDevice(ctx->device));
    const bool with_ids = n > 0 && ids && query_ids;

    // the host's inputs share one staging buffer, the host's outputs another; 8-byte arrays first
    const void *d_in[4];
    {
        const void *src[4] = {n > 0 ? hashes : nullptr, with_ids ? ids : nullptr, queries, with_ids ? query_ids : nullptr};
        const size_t bytes[4] = {(size_t)n * 8, (size_t)n * 8, (size_t)m * 8, (size_t)m * 8};
        size_t at[4], total = 0;
        for (int i = 0; i < 4; ++i) {
            at[i] = total;
            if (src[i] && !ke_is_device_ptr(src[i])) total += bytes[i];
        }
        void *base = nullptr;
        if (total) KE_TRY(ke_reserve(ctx, KE_BUF_NEAREST_IN, total, &base));
        for (int i = 0; i < 4; ++i) {
            d_in[i] = src[i];
            if (!src[i] || ke_is_device_ptr(src[i])) continue;
            d_in[i] = (uint8_t *)base + at[i];
            KE_HIP(ctx, hipMemcpyAsync((void *)d_in[i], src[i], bytes[i], hipMemcpyHostToDevice, ctx->stream));
        }
    }
    void *dst[5] = {index_out, within_out, distance_out, count_out, histogram_out}, *d_out[5];
    const size_t out_bytes[5] = {(size_t)m * k * 8, (size_t)m * 8, (size_t)m * k * 4, (size_t)m * 4, (size_t)m * KE_NEAREST_BINS * 4};
    bool staged[5];
    {
        size_t at[5], total = 0;
        for (int i = 0; i < 5; ++i) {
            at[i] = total;
            staged[i] = dst[i] && !ke_is_device_ptr(dst[i]);
            if (staged[i]) total += (out_bytes[i] + 7) & ~(size_t)7;
        }
        void *base = nullptr;
        if (total) KE_TRY(ke_reserve(ctx, KE_BUF_NEAREST_OUT, total, &base));
        for (int i = 0; i < 5; ++i) d_out[i] = staged[i] ? (void *)((uint8_t *)base + at[i]) : dst[i];
    }

    ke_time_begin(ctx, KE_T_NEAREST);
    const int64_t per_launch = (int64_t)1 << 30;   // workgroups of one launch
    for (int64_t q0 = 0; q0 < m; q0 += per_launch) {
        const dim3 grid((unsigned)std::min<int64_t>(per_launch, m - q0)), block(KE_NEAREST_THREADS);
        if (with_ids)
            hipLaunchKernelGGL(ke_nearest_kernel<true>, grid, block, 0, ctx->stream, (const uint64_t *)d_in[0], (const int64_t *)d_in[1],
                               (uint32_t)n, (const uint64_t *)d_in[2], (const int64_t *)d_in[3], q0, k, max_distance, (int64_t *)d_out[0],
                               (int32_t *)d_out[2], (int32_t *)d_out[3], (int64_t *)d_out[1], (uint32_t *)d_out[4]);
        else
            hipLaunchKernelGGL(ke_nearest_kernel<false>, grid, block, 0, ctx->stream, (const uint64_t *)d_in[0], (const int64_t *)nullptr,
                               (uint32_t)n, (const uint64_t *)d_in[2], (const int64_t *)nullptr, q0, k, max_distance, (int64_t *)d_out[0],
                               (int32_t *)d_out[2], (int32_t *)d_out[3], (int64_t *)d_out[1], (uint32_t *)d_out[4]);
        KE_HIP(ctx, hipGetLastError());
    }
    ke_time_end(ctx, KE_T_NEAREST);
    for (int i = 0; i < 5; ++i)
        if (staged[i]) KE_HIP(ctx, hipMemcpyAsync(dst[i], d_out[i], out_bytes[i], hipMemcpyDeviceToHost, ctx->stream));
    KE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KE_OK;
}
