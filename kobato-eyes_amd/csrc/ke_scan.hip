// ke_scan.hip -- K4: all-pairs Hamming candidate scan for gfx950.
//
// Replaces the bucket build + in-bucket pair loop of DuplicateScanner.build_clusters
// (src/dup/scanner.py:227-299).  The pair space i<j is cut into 1024 x 1024 tiles of the upper
// triangle; a workgroup owns one tile.
//
// The Hamming distance itself runs on the matrix cores: with every hash written out as 128 one-bit
// values [bits of x | bits of ~x], <row(x), row(y)> = popc(x & y) + popc(~x & ~y) = 64 - popc(x ^ y), so one
// v_mfma_scale_f32_16x16x128_f8f6f4 with fp4 (E2M1) operands -- bit 1 = 1.0, exact, sums <= 64 exact in
// f32 -- yields the 256 similarities of 16 x 16 hashes in 16 cycles.  A pre-pass expands the hashes once
// (64 B each, already in operand order); a wave keeps the operands of 128 row hashes in registers and
// walks the tile's columns out of LDS: 8 MFMAs per 16 columns, then one running maximum over the 32
// results per lane.  Only when a 128 x 16 block holds a similarity >= 64 - threshold does the wave
// re-inspect it and apply the full predicate (band lanes, ids, size ratio, bucket cap) to the original
// 64-bit hashes and append edges through one atomic cursor.  The VALU version of the same loop
// (2 xor + 2 popcount + min per pair) topped out at 7-8 Tpairs/s on VALU issue.
//
// Tables whose band buckets hold few pairs and no long bucket skip all of that: the bucket kernels further down visit only the
// pairs inside buckets, and the choice between the two paths is made per call on the device (kPathWord).
#include <cmath>

#include <hipcub/hipcub.hpp>

#include "ke_internal.h"

namespace {

constexpr int kThreads = kScanThreads;      // 8 waves
constexpr int kRT = 8;                      // 16-hash row tiles per wave
constexpr int kTile = 8 * kRT * 16;         // 1024 rows per workgroup ...
constexpr int kCols = 1024;                 // ... against 1024 columns
static_assert(kTile == kKeScanTile && kCols == kKeScanCols, "ke_scan_region.h describes this tiling");
constexpr int kCPR = kTile / kCols;         // column chunks per row block
constexpr int kChunk = 256;                 // columns staged in LDS at a time (16 operand tiles, 16 KB)

typedef int ke_v8i __attribute__((ext_vector_type(8)));
typedef int ke_v4i __attribute__((ext_vector_type(4)));
typedef float ke_v4f __attribute__((ext_vector_type(4)));

struct ScanArgs {
    const uint64_t *hashes;
    const ke_v4i *expanded;  // operand tiles: [hash / 16][lane = group * 16 + hash % 16] x 16 B, zero beyond n
    const int64_t *ids;
    const int64_t *sizes;
    int64_t n;
    int nb;                 // row blocks
    int ncc;                // column chunks
    int64_t first_tile;     // ordinal of this launch's first tile in the triangle enumeration
    int64_t tile_step;
    int64_t n_tiles;        // total tiles in the triangle
    int threshold, band_bits, band_count;
    double size_ratio;
    const uint32_t *hist;   // nullable: band_count tables of 2^band_bits bucket sizes (band_bits <= 24) ...
    const uint32_t *blen;   // ... or, for wider bands, the size of hash i's bucket in band b at blen[b * n + i]
    unsigned long long cap;
    ke_edge *edges;
    int64_t capacity;
    unsigned long long *counters;  // [0] pairs, [1] sum of shared bands, [2] edges, [3] bucket pairs, [4] path (kPathWord)
    int exact;              // ke_hamming_scan_exact: a pair that shares no band is an edge as well, with bands = 0
};

// counters[kPathWord]: 0 = the all-pairs tile kernel does the scan, 1 = the bucket kernels do.  Zeroed with the counters,
// written once per call on the device (ke_bucket_offsets) before any kernel that reads it; each path's kernels return at
// their first instruction when it names the other.  counters[kLongestWord]: longest bucket the reference would walk.
constexpr int kPathWord = 4, kLongestWord = 5;

__device__ __forceinline__ int popc64(uint32_t lo, uint32_t hi) { return __popc(lo) + __popc(hi); }

// Full predicate for one pair that already passed popcount <= threshold: true when the pair is an edge, with its bands
// mask and the number of bands it shares (both 0 for an edge that only an exact scan keeps).  only_band >= 0 (bucket path,
// which meets a pair once per band it shares): true only when that band is the lowest one counted here, so that the pair
// appears once.  The index is kept beside the mask because bands >= 31 share the mask's bit 31.
__device__ bool pair_is_edge(const ScanArgs &a, int64_t gi, int64_t gj, uint64_t x, uint64_t y, int only_band, int *bands_out,
                             int *shared_out) {
    if (gi >= gj || gj >= a.n) return false;
    if (a.ids && a.ids[gi] == a.ids[gj]) return false;                 // src/dup/scanner.py:266
    if (a.sizes && a.size_ratio > 0.0) {                               // :358-370
        const int64_t sa = a.sizes[gi], sb = a.sizes[gj];
        if (sa > 0 && sb > 0) {
            const int64_t small = sa < sb ? sa : sb, large = sa < sb ? sb : sa;
            if (!((double)small / (double)large >= a.size_ratio)) return false;
        }
    }
    const uint64_t d = x ^ y;
    const uint64_t mask = a.band_bits >= 64 ? ~0ull : ((1ull << a.band_bits) - 1ull);
    int bands = 0, shared = 0, first = -1;
    for (int b = 0; b < a.band_count; ++b) {
        const int sh = b * a.band_bits;
        if (((d >> sh) & mask) != 0) continue;
        if (a.cap) {                                                   // KE_DUP_BUCKET_PAIR_CAP, :262-263
            const unsigned long long len = a.hist ? a.hist[((size_t)b << a.band_bits) + (size_t)((x >> sh) & mask)]
                                                  : a.blen[(size_t)b * (size_t)a.n + (size_t)gi];
            if (len * (len - 1) / 2 > a.cap) continue;
        }
        bands |= 1 << (b < 31 ? b : 31);
        if (first < 0) first = b;
        ++shared;
    }
    if (!shared && !a.exact) return false;
    if (only_band >= 0 && first != only_band) return false;
    *bands_out = bands; *shared_out = shared;
    return true;
}

__device__ void consider_pair(const ScanArgs &a, int64_t gi, int64_t gj, uint64_t x, uint64_t y, int pc, int only_band = -1) {
    int bands, shared;
    if (!pair_is_edge(a, gi, gj, x, y, only_band, &bands, &shared)) return;
    atomicAdd(&a.counters[1], (unsigned long long)shared);
    const unsigned long long slot = atomicAdd(&a.counters[2], 1ull);
    if ((int64_t)slot < a.capacity) {
        ke_edge e;
        e.a = gi; e.b = gj; e.h = pc; e.bands = bands;
        a.edges[slot] = e;
    }
}

// 8 bits -> 8 E2M1 nibbles (bit n -> nibble n = 0b0010 = 1.0 or 0)
__device__ __forceinline__ uint32_t spread8(uint32_t b) {
    uint32_t t = (b | (b << 12)) & 0x000F000Fu;
    t = (t | (t << 6)) & 0x03030303u;
    t = (t | (t << 3)) & 0x11111111u;
    return t << 1;
}

// Operand image of the hashes.  Lane group g of a 16-hash tile holds 32 of the 128 values of each hash:
// g = 0, 1: bits 0..31 / 32..63 of x; g = 2, 3: the same bits of ~x.  A and B operands use the same image
// (the k <-> (group, nibble) map of the instruction is the same for both, so any fixed order works).
__global__ __launch_bounds__(256) void ke_scan_expand(const uint64_t *__restrict__ hashes, int64_t n, int64_t n_pad,
                                                       ke_v4i *__restrict__ out, const unsigned long long *path) {
    if (*path) return;                                             // the bucket kernels do this call's scan
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;     // = tile * 64 + lane
    if (e >= n_pad * 4) return;
    const int64_t i = (e >> 6) * 16 + (e & 15);
    const int g = (int)(e >> 4) & 3;
    ke_v4i v = {0, 0, 0, 0};
    if (i < n) {
        const uint64_t x = g < 2 ? hashes[i] : ~hashes[i];
        const uint32_t half = (uint32_t)(x >> (32 * (g & 1)));
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (int)spread8((half >> (8 * k)) & 0xFFu);
    }
    out[e] = v;
}

// The tile kernel's body.  kMode = KE_SCAN_ALL is ke_scan_tiles, the whole triangle; kFrom is ke_scan_tiles_from, a scan
// from first_new: the tile comes from the enumeration of the trapezoid of tiles that hold a pair with j >= first_new
// (region, ke_scan_region.h) and the columns below first_new are left out -- whole chunks and 16-column blocks by where
// the loops start (wave-uniform), the lanes of the block first_new lies in at the rare path.  Every kFrom branch is
// compile-time, region is not read without it.
// kMode = KE_SCAN_CROSS is ke_scan_tiles_cross, the pairs i < first_new <= j of a table [library | queries]: the region is the
// rectangle of row blocks that hold a row below first_new against the chunks from first_new's on (ke_cross_region), the
// columns are cut as for kFrom, and the rows at or beyond first_new are left out -- a wave whose 128 rows all lie there
// walks no block but still meets the others at every barrier of the chunk loop, a single such row is dropped per lane at
// the rare path.  Every kCross branch is compile-time too.
template <KeScanKind kMode>
__device__ __forceinline__ void scan_tiles_body(const ScanArgs a, const KeScanRegion region) {
    constexpr bool kCross = kMode == KE_SCAN_CROSS, kFrom = kMode != KE_SCAN_ALL;   // kFrom: the columns start at first_new
    __shared__ ke_v4i s_b[2][kChunk / 16 * 64];      // two chunks of 16 operand tiles
    if (a.counters[kPathWord]) return;               // the bucket kernels do this call's scan
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t t = a.first_tile + (int64_t)blockIdx.x * a.tile_step;
    if (t >= a.n_tiles) return;
    int64_t rb, cc;
    if constexpr (kCross) {
        ke_cross_tile(region, t, &rb, &cc);
    } else if constexpr (kFrom) {
        ke_region_tile(region, t, &rb, &cc);         // the same inversion behind the region's rectangle (ke_scan_region.h)
    } else {
        ke_tri_tile(t, a.nb, a.ncc, &rb, &cc);       // the whole triangle, row-major
    }
    const int64_t row0 = rb * kTile, col0 = cc * kCols;
    const int64_t wrow0 = row0 + (int64_t)wv * (kRT * 16);          // this wave's 128 rows
    if constexpr (kCross) {
        // pairs i < first_new <= j of this tile: over the shards first_new (n - first_new)
        if (tid == 0) atomicAdd(&a.counters[0], (unsigned long long)ke_cross_tile_pairs(region, rb, cc));
    } else if constexpr (kFrom) {
        // pairs i < j, j >= first_new of this tile: over the shards n (n - 1) / 2 - f (f - 1) / 2
        if (tid == 0) atomicAdd(&a.counters[0], (unsigned long long)ke_region_tile_pairs(region, rb, cc));
    } else if (tid == 0) {
        // pairs i < j < n this tile stands for, counted where they are evaluated: the shards' counts must add up to
        // n (n - 1) / 2 (counters[0]; the host checks it against its own arithmetic)
        const int64_t rows = min((int64_t)kTile, a.n - row0), cols = min((int64_t)kCols, a.n - col0);
        const unsigned long long pairs = cc == kCPR * rb ? (unsigned long long)(rows * (rows - 1) / 2) : (unsigned long long)(rows * cols);
        atomicAdd(&a.counters[0], pairs);
    }

    // row operands: registers for the whole tile (only dwords 0..3 of an fp4 operand are read)
    ke_v8i ra[kRT];
#pragma unroll
    for (int r = 0; r < kRT; ++r) {
        const ke_v4i v = a.expanded[(wrow0 / 16 + r) * 64 + lane];
        ra[r] = ke_v8i{v[0], v[1], v[2], v[3], 0, 0, 0, 0};
    }
    // The similarities are small non-negative integers held as floats, so their bit patterns order like
    // integers: the running maximum is an integer max (a float max would first canonicalise every input).
    const int thr_bits = __float_as_int((float)(64 - a.threshold));
    const int nchunks = (int)((min((int64_t)kCols, a.n - col0) + kChunk - 1) / kChunk);
    // the first chunk to walk: (kFrom) the one first_new lies in; a tile of the region has a column >= first_new, so
    // c_lo < nchunks
    int c_lo = 0;
    if constexpr (kFrom) {
        const int64_t skip = (region.first_new - col0) / kChunk;            // whole chunks below first_new (cc = cc0 only)
        c_lo = skip > 0 ? (int)skip : 0;
    }
    // column operands: 16 KB per chunk, two 16-byte pieces per thread, next chunk in flight during the products
    const ke_v4i *cbase = a.expanded + (col0 / 16) * 64;
    ke_v4i pre0 = cbase[c_lo * (kChunk / 16 * 64) + tid], pre1 = cbase[c_lo * (kChunk / 16 * 64) + kThreads + tid];
    s_b[c_lo & 1][tid] = pre0;
    s_b[c_lo & 1][kThreads + tid] = pre1;
    // every load so far has landed from here on: without this hipcc re-waits for the row operands inside the
    // loop with counts that also drain the column prefetch issued at the top of each iteration
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    __syncthreads();
    for (int c = c_lo; c < nchunks; ++c) {
        {   // unconditional (the last iteration re-reads its own chunk): a guarded load is waited for at once
            const int cn = c + 1 < nchunks ? c + 1 : c;
            pre0 = cbase[cn * (kChunk / 16 * 64) + tid];
            pre1 = cbase[cn * (kChunk / 16 * 64) + kThreads + tid];
        }
        const ke_v4i *bt = s_b[c & 1];
        // diagonal tiles: a 128 x 16 block whose every column index is below the wave's first row holds no pair i < j --
        // the wave starts at the first block that can (wave-uniform)
        const int64_t below = wrow0 - (col0 + (int64_t)c * kChunk) - 15;
        int ct0 = below < 0 ? 0 : (int)min((int64_t)(kChunk / 16), below / 16 + 1);
        if constexpr (kFrom) {   // and at the first block that reaches first_new
            const int64_t before = region.first_new - (col0 + (int64_t)c * kChunk);
            if (before > 0) ct0 = max(ct0, (int)min((int64_t)(kChunk / 16), before / 16));
        }
        if constexpr (kCross) {  // a wave whose rows are all queries has no block to walk (wave-uniform); it stays for the barriers
            if (wrow0 >= region.first_new) ct0 = kChunk / 16;
        }
        for (int ct = ct0; ct < kChunk / 16; ++ct) {
            const ke_v4i bv = bt[ct * 64 + lane];
            const ke_v8i b = {bv[0], bv[1], bv[2], bv[3], 0, 0, 0, 0};
            ke_v4f acc[kRT];
#pragma unroll
            for (int r = 0; r < kRT; ++r)
                acc[r] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(ra[r], b, ke_v4f{0, 0, 0, 0}, 4, 4, 0, 0, 0, 0);
            int m = 0;
#pragma unroll
            for (int r = 0; r < kRT; ++r) {
                m = max(max(m, __float_as_int(acc[r][0])), __float_as_int(acc[r][1]));
                m = max(max(m, __float_as_int(acc[r][2])), __float_as_int(acc[r][3]));
            }
            if (__ballot(m >= thr_bits) != 0ull) {
                // Rare: collect which of this lane's 32 results qualify into a bit mask, then walk the mask with the
                // original hashes (result map: lane l holds rows 4(l>>4) + i of row tile r, column l & 15).
                uint32_t hits = 0;
#pragma unroll
                for (int r = 0; r < kRT; ++r)
#pragma unroll
                    for (int i = 0; i < 4; ++i) hits |= __float_as_int(acc[r][i]) >= thr_bits ? 1u << (4 * r + i) : 0u;
                const int64_t gj = col0 + (int64_t)c * kChunk + ct * 16 + (lane & 15);
                if (gj >= a.n) hits = 0;
                if constexpr (kFrom) { if (gj < region.first_new) hits = 0; }
                const uint64_t y = hits ? a.hashes[gj] : 0ull;
                while (hits) {
                    const int k = __ffs(hits) - 1;
                    hits &= hits - 1;
                    const int64_t gi = wrow0 + (k >> 2) * 16 + 4 * (lane >> 4) + (k & 3);
                    bool take = gi < gj;
                    if constexpr (kCross) take = take && gi < region.first_new;
                    if (take) {
                        const uint64_t x = a.hashes[gi];
                        consider_pair(a, gi, gj, x, y, __popcll(x ^ y));
                    }
                }
            }
        }
        s_b[(c + 1) & 1][tid] = pre0;
        s_b[(c + 1) & 1][kThreads + tid] = pre1;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void ke_scan_tiles(const ScanArgs a, const KeScanRegion region) {
    scan_tiles_body<KE_SCAN_ALL>(a, region);
}

__global__ __launch_bounds__(kThreads) void ke_scan_tiles_from(const ScanArgs a, const KeScanRegion region) {
    scan_tiles_body<KE_SCAN_FROM>(a, region);
}

__global__ __launch_bounds__(kThreads) void ke_scan_tiles_cross(const ScanArgs a, const KeScanRegion region) {
    scan_tiles_body<KE_SCAN_CROSS>(a, region);
}

__global__ void ke_band_hist(const uint64_t *__restrict__ hashes, int64_t n, int band_bits, int band_count,
                             uint32_t *__restrict__ hist) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t x = hashes[i];
    const uint64_t mask = (1ull << band_bits) - 1ull;
    for (int b = 0; b < band_count; ++b) atomicAdd(&hist[((size_t)b << band_bits) + (size_t)((x >> (b * band_bits)) & mask)], 1u);
}

// sum over buckets of C(len, 2) for the buckets the reference would walk (len >= 2, pairs <= cap when a cap is set):
// its "pairs total" funnel counter before the same-file-id exclusion (src/dup/scanner.py:258-270)
__global__ void ke_hist_pairs(const uint32_t *__restrict__ hist, size_t bins, unsigned long long cap, unsigned long long *out) {
    unsigned long long s = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < bins; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long len = hist[i];
        const unsigned long long p = len * (len - 1) / 2;
        if (len >= 2 && (!cap || p <= cap)) s += p;
    }
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d);
    __shared__ unsigned long long part[4];                    // one atomic per workgroup: thousands to one address serialise
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0 && (part[0] | part[1] | part[2] | part[3])) atomicAdd(out, part[0] + part[1] + part[2] + part[3]);
}

// ---- bucket path: visit only the pairs that share a bucket -----------------------------------------------------------
// consider_pair drops every pair that shares no band, so an edge exists only inside a bucket of some band -- the
// reference's own candidate generation (src/dup/scanner.py:227-290).  The positions are counting-sorted by band value per
// band (histogram -> exclusive offsets -> scatter of (hash, position)), then one thread per slot of a sorted run compares
// its hash with the later members of its bucket.  Tables up to kScanBucketMaxBins bins: one 1024-bin block per workgroup of the two histogram
// passes, at most 256 block sums, so a workgroup of ke_bucket_offsets adds its predecessors' sums with one value per thread.
constexpr int kBinsPerBlock = 1024;
// The rule between the paths (ke_scan_plan.h plans with it, DESIGN section 5 has the sweeps it was set from): buckets when the
// table has at least kBucketMinN hashes, the walked bucket pairs are at most 1/kBucketRatio of all pairs (1/kBucketRatioFrom of
// the region's for a scan from first_new or a cross scan) and no walked bucket is longer than kBucketLongest (one thread walks
// the rest of its bucket; checked on the device, ke_bucket_offsets), else tiles.  The host's three are stated here as well, where
// the tables of the GPU tests read them, and held to the plan's.
constexpr unsigned long long kBucketRatio = 6000, kBucketLongest = 260;
constexpr int64_t kBucketMinN = 50000;
constexpr unsigned long long kBucketRatioFrom = 1000;
static_assert(kBucketRatio == kScanBucketRatio && kBucketMinN == kScanBucketMinN && kBucketRatioFrom == kScanBucketRatioFrom,
              "ke_scan_plan.h plans with these");
static_assert(kScanBucketMaxBins / kBinsPerBlock * sizeof(uint32_t) == kScanBlockSumBytes, "ke_scan_plan.h sizes the block sums");

__device__ __forceinline__ unsigned long long block_sum_256(unsigned long long v, unsigned long long *s4) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return s4[0] + s4[1] + s4[2] + s4[3];
}

// per 1024-bin block: members (for the offsets), C(len, 2) over the walked buckets (counters[3], as ke_hist_pairs) and the
// longest walked bucket
__global__ __launch_bounds__(256) void ke_bucket_stats(const uint32_t *__restrict__ hist, size_t bins, unsigned long long cap,
                                                        uint32_t *__restrict__ block_sums, unsigned long long *state) {
    unsigned long long members = 0, pairs = 0, longest = 0;
    for (int k = 0; k < kBinsPerBlock / 256; ++k) {
        const size_t i = (size_t)blockIdx.x * kBinsPerBlock + (size_t)k * 256 + threadIdx.x;
        if (i >= bins) break;
        const unsigned long long len = hist[i];
        const unsigned long long p = len * (len - 1) / 2;
        members += len;
        if (len >= 2 && (!cap || p <= cap)) { pairs += p; longest = len > longest ? len : longest; }
    }
    __shared__ unsigned long long s_m[4], s_p[4], s_l[4];
    members = block_sum_256(members, s_m);
    pairs = block_sum_256(pairs, s_p);
    for (int d = 32; d > 0; d >>= 1) { const unsigned long long o = __shfl_down(longest, d); longest = o > longest ? o : longest; }
    if ((threadIdx.x & 63) == 0) s_l[threadIdx.x >> 6] = longest;
    __syncthreads();
    if (threadIdx.x == 0) {
        block_sums[blockIdx.x] = (uint32_t)members;
        if (pairs) atomicAdd(&state[3], pairs);
        longest = max(max(s_l[0], s_l[1]), max(s_l[2], s_l[3]));
        if (longest) atomicMax(&state[kLongestWord], longest);
    }
}

// Chooses the path (every workgroup evaluates the same rule on the same words; workgroup 0 publishes it for the later
// kernels and, in bucket mode, adds the pairs this shard stands for to counters[0] -- the host's closed form, which the
// tile kernel would have counted tile by tile) and, in bucket mode, turns the histogram into exclusive offsets.  Offsets
// are taken modulo 2^32 over the whole table: band b's run starts at b * n, and (offset - b * n) mod 2^32 is the place
// inside the band's run for every n < 2^32.
__global__ __launch_bounds__(256) void ke_bucket_offsets(const uint32_t *__restrict__ hist, size_t bins,
                                                          const uint32_t *__restrict__ block_sums, uint32_t *__restrict__ offsets,
                                                          unsigned long long *state, int forced, unsigned long long pairs_limit,
                                                          unsigned long long shard_pairs) {
    const bool buckets = forced == 2 || (state[3] <= pairs_limit && state[kLongestWord] <= kBucketLongest);
    if (!buckets) return;                          // the path word stays 0: tiles
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (blockIdx.x == 0 && tid == 0) {
        state[kPathWord] = 1;
        state[0] = shard_pairs;
    }
    __shared__ unsigned long long s_b[4];
    __shared__ uint32_t s_w[4];
    const uint32_t base = (uint32_t)block_sum_256(tid < (int)blockIdx.x ? block_sums[tid] : 0u, s_b);
    const size_t i0 = (size_t)blockIdx.x * kBinsPerBlock + (size_t)tid * 4;
    uint32_t v[4], mine = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = i0 + k < bins ? hist[i0 + k] : 0u; mine += v[k]; }
    uint32_t inc = mine;                           // inclusive scan over the wave, then over the four waves
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(inc, d); if (lane >= d) inc += t; }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint32_t run = base + inc - mine;
    for (int w = 0; w < wv; ++w) run += s_w[w];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i0 + k < bins) offsets[i0 + k] = run;
        run += v[k];
    }
}

// Counting sort per band: slot b * n + place holds a member's hash and its position, so that a bucket is one contiguous run
// of hashes.  The order inside a run is whatever the atomics give.
__global__ void ke_bucket_scatter(const uint64_t *__restrict__ hashes, int64_t n, int band_bits, int band_count,
                                  uint32_t *__restrict__ offsets, uint64_t *__restrict__ sorted_hash, uint32_t *__restrict__ sorted_pos,
                                  const unsigned long long *state) {
    if (!state[kPathWord]) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t x = hashes[i];
    const uint64_t mask = (1ull << band_bits) - 1ull;
    for (int b = 0; b < band_count; ++b) {
        const uint32_t slot = atomicAdd(&offsets[((size_t)b << band_bits) + (size_t)((x >> (b * band_bits)) & mask)], 1u);
        const uint32_t place = slot - (uint32_t)((uint64_t)b * (uint64_t)n);
        if ((int64_t)place < n) {
            sorted_hash[(size_t)b * (size_t)n + place] = x;
            sorted_pos[(size_t)b * (size_t)n + place] = (uint32_t)i;
        }
    }
}

// One thread per slot of a band's sorted run: its hash against the later slots of the run for as long as their band value is
// its own, all of it read from neighbouring addresses (lane l walks slots l + 1, l + 2, ... beside lane l + 1's).  The
// scatter's order inside a run differs from rank to rank, so the shards cannot divide the slots: every shard walks all of
// them (cheap) and a pair belongs to the shard named by its two positions.  A bucket over the pair cap is skipped as a whole
// (src/dup/scanner.py:262-263).
// A workgroup takes kPairSlots slots of one band (blockIdx.y) and collects its edges in LDS: one add per workgroup to the
// edge cursor and to the shared-bands sum.  On a uniform table the edges are few and far apart, one in a wave at most, so
// consider_pair's two adds per edge all went to one address one by one: 13 000 of them were the 120 us this kernel took at
// n = 100 000.  Edges beyond the staging buffer (skewed tables, where a wave's adds combine) go through consider_pair.
constexpr int kPairSlots = 1024, kPairStage = 256;

// kFrom (ke_bucket_pairs_from): a pair is kept only when its later position is at least first_new; its shard stays
// (lo + hi) mod part_count.  KE_SCAN_CROSS (ke_bucket_pairs_cross): only when lo < first_new <= hi as well.
template <KeScanKind kMode>
__device__ __forceinline__ void bucket_pairs_body(const ScanArgs a, const uint64_t *__restrict__ sorted_hash,
                                                  const uint32_t *__restrict__ sorted_pos, int part_index, int part_count,
                                                  int64_t first_new) {
    if (!a.counters[kPathWord]) return;
    __shared__ ke_edge s_edges[kPairStage];
    __shared__ unsigned int s_count, s_shared;
    __shared__ unsigned long long s_base;
    if (threadIdx.x == 0) { s_count = 0; s_shared = 0; }
    __syncthreads();
    const int b = blockIdx.y, sh = b * a.band_bits;
    const uint64_t mask = (1ull << a.band_bits) - 1ull;
    const uint64_t *run = sorted_hash + (size_t)b * (size_t)a.n;
    const uint32_t *pos = sorted_pos + (size_t)b * (size_t)a.n;
    for (int c = 0; c < kPairSlots / 256; ++c) {
        const int64_t r = (int64_t)blockIdx.x * kPairSlots + c * 256 + threadIdx.x;
        if (r >= a.n) break;
        const uint64_t x = run[r], key = (x >> sh) & mask;
        if (a.cap) {
            const unsigned long long len = a.hist[((size_t)b << a.band_bits) + (size_t)key];
            if (len * (len - 1) / 2 > a.cap) continue;
        }
        int64_t pi = -1;
        for (int64_t k = r + 1; k < a.n; ++k) {
            const uint64_t y = run[k];
            if (((y >> sh) & mask) != key) break;
            const int pc = __popcll(x ^ y);
            if (pc > a.threshold) continue;
            if (pi < 0) pi = pos[r];
            const int64_t pj = pos[k];
            const int64_t lo = pi < pj ? pi : pj, hi = pi < pj ? pj : pi;
            if (hi >= a.n || (lo + hi) % part_count != part_index) continue;
            if constexpr (kMode != KE_SCAN_ALL) { if (hi < first_new) continue; }
            if constexpr (kMode == KE_SCAN_CROSS) { if (lo >= first_new) continue; }
            const uint64_t xl = pi < pj ? x : y, xh = pi < pj ? y : x;
            int bands, shared;
            if (!pair_is_edge(a, lo, hi, xl, xh, b, &bands, &shared)) continue;
            const unsigned int at = atomicAdd(&s_count, 1u);
            if (at < (unsigned)kPairStage) {
                atomicAdd(&s_shared, (unsigned)shared);
                ke_edge e;
                e.a = lo; e.b = hi; e.h = pc; e.bands = bands;
                s_edges[at] = e;
            } else {
                consider_pair(a, lo, hi, xl, xh, pc, b);
            }
        }
    }
    __syncthreads();
    const unsigned int staged = s_count < (unsigned)kPairStage ? s_count : (unsigned)kPairStage;
    if (staged == 0) return;
    if (threadIdx.x == 0) {
        atomicAdd(&a.counters[1], (unsigned long long)s_shared);
        s_base = atomicAdd(&a.counters[2], (unsigned long long)staged);
    }
    __syncthreads();
    for (unsigned int i = threadIdx.x; i < staged; i += 256)
        if ((int64_t)(s_base + i) < a.capacity) a.edges[s_base + i] = s_edges[i];
}

__global__ __launch_bounds__(256) void ke_bucket_pairs(const ScanArgs a, const uint64_t *__restrict__ sorted_hash,
                                                        const uint32_t *__restrict__ sorted_pos, int part_index, int part_count,
                                                        int64_t first_new) {
    bucket_pairs_body<KE_SCAN_ALL>(a, sorted_hash, sorted_pos, part_index, part_count, first_new);
}

__global__ __launch_bounds__(256) void ke_bucket_pairs_from(const ScanArgs a, const uint64_t *__restrict__ sorted_hash,
                                                             const uint32_t *__restrict__ sorted_pos, int part_index, int part_count,
                                                             int64_t first_new) {
    bucket_pairs_body<KE_SCAN_FROM>(a, sorted_hash, sorted_pos, part_index, part_count, first_new);
}

__global__ __launch_bounds__(256) void ke_bucket_pairs_cross(const ScanArgs a, const uint64_t *__restrict__ sorted_hash,
                                                              const uint32_t *__restrict__ sorted_pos, int part_index, int part_count,
                                                              int64_t first_new) {
    bucket_pairs_body<KE_SCAN_CROSS>(a, sorted_hash, sorted_pos, part_index, part_count, first_new);
}

// Wide bands (2^band_bits bins do not fit a table): the band values are sorted together with their positions and the
// run lengths are read off the sorted keys.
__global__ void ke_band_keys(const uint64_t *__restrict__ hashes, int64_t n, int shift, uint64_t mask, uint64_t *__restrict__ keys,
                             uint32_t *__restrict__ pos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = (hashes[i] >> shift) & mask;
    pos[i] = (uint32_t)i;
}

// thread i starts a run iff keys[i] != keys[i-1]; it walks to the end of its run, writes the length to every member's
// slot and adds the run's pairs.  Runs are short unless the corpus is degenerate (then the walk is long but correct).
__global__ void ke_run_lengths(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ pos, int64_t n, unsigned long long cap,
                               uint32_t *__restrict__ blen, unsigned long long *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i > 0 && keys[i - 1] == keys[i]) return;
    int64_t e = i + 1;
    while (e < n && keys[e] == keys[i]) ++e;
    const unsigned long long len = (unsigned long long)(e - i);
    for (int64_t k = i; k < e; ++k) blen[pos[k]] = (uint32_t)len;
    const unsigned long long p = len * (len - 1) / 2;
    if (len >= 2 && (!cap || p <= cap)) atomicAdd(out, p);
}

// ---- the "size=" funnel counter (src/dup/scanner.py:268-270, 358-370): bucket pairs that pass the size filter ----------
// Positions sorted by size once; per band a stable sort by band value then leaves every bucket contiguous with its sizes
// ascending, and a member's partners are the earlier members whose size is large enough -- found by a binary search whose
// test is the reference's own float division (smaller / larger >= ratio, monotone in the smaller size).
__global__ void ke_size_keys(const int64_t *__restrict__ sizes, int64_t n, uint64_t *__restrict__ keys, uint32_t *__restrict__ pos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t s = sizes[i];
    keys[i] = s > 0 ? (uint64_t)s : 0ull;                     // a missing / non-positive size passes with everyone
    pos[i] = (uint32_t)i;
}

__global__ void ke_band_keys_of(const uint64_t *__restrict__ hashes, const uint32_t *__restrict__ order, int64_t n, int shift,
                                uint64_t mask, uint64_t *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = (hashes[order[i]] >> shift) & mask;
}

__global__ void ke_run_flags(const uint64_t *__restrict__ keys, int64_t n, uint32_t *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// rank[i] = number of the run position i lies in (inclusive sum of the flags, minus one); starts[r] = first position of run r
__global__ void ke_run_starts(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ rank1, int64_t n, uint32_t *__restrict__ starts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == 0 || keys[i] != keys[i - 1]) starts[rank1[i] - 1] = (uint32_t)i;
    if (i == n - 1) starts[rank1[i]] = (uint32_t)n;
}

__global__ void ke_size_pairs(const uint64_t *__restrict__ sz, const uint32_t *__restrict__ rank1, const uint32_t *__restrict__ starts,
                              int64_t n, double ratio, unsigned long long cap, unsigned long long *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long c = 0;
    if (i < n) {
        const uint32_t r = rank1[i] - 1;
        const int64_t st = starts[r], en = starts[r + 1], m = en - st;
        if (m >= 2 && (!cap || (unsigned long long)m * (unsigned long long)(m - 1) / 2 <= cap)) {
            const uint64_t si = sz[i];
            if (si == 0) {
                c = (unsigned long long)(i - st);             // every earlier member is size-free as well
            } else {
                int64_t lo = st, hi = i;                      // first member with a positive size
                while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (sz[mid] == 0) lo = mid + 1; else hi = mid; }
                const int64_t free_n = lo - st;
                hi = i;                                       // first positive member j < i with sz[j] / si >= ratio
                const double larger = (double)si;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if ((double)sz[mid] / larger >= ratio) hi = mid; else lo = mid + 1;
                }
                c = (unsigned long long)(i - lo) + (unsigned long long)free_n;
            }
        }
    }
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0 && (part[0] | part[1] | part[2] | part[3])) atomicAdd(out, part[0] + part[1] + part[2] + part[3]);
}

}  // namespace

int ke_launch_band_pairs_after_size(ke_ctx *ctx, const uint64_t *d_hashes, const int64_t *d_sizes, int64_t n, int band_bits,
                                    int band_count, double ratio, int64_t bucket_pair_cap, unsigned long long *d_out) {
    if (n > 0x7fffffffLL) return ke_fail(ctx, KE_EUNSUPPORTED, "the size funnel counter needs n < 2^31");
    const unsigned long long cap = bucket_pair_cap > 0 ? (unsigned long long)bucket_pair_cap : 0ull;
    size_t t_size = 0, t_band = 0, t_scan = 0;
    KE_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, t_size, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                                   (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, 0, 64, ctx->stream));
    KE_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, t_band, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                                   (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)n, 0, band_bits, ctx->stream));
    KE_HIP(ctx, hipcub::DeviceScan::InclusiveSum(nullptr, t_scan, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, ctx->stream));
    const size_t temp_bytes = std::max(t_size, std::max(t_band, t_scan));
    const size_t kb = ((size_t)n * 8 + 255) & ~(size_t)255, pb = ((size_t)(n + 1) * 4 + 255) & ~(size_t)255;
    void *scratch;
    KE_TRY(ke_reserve(ctx, KE_BUF_SCAN_AUX, 4 * kb + 4 * pb + temp_bytes + 256, &scratch));
    uint8_t *sp = (uint8_t *)scratch;
    uint64_t *k_a = (uint64_t *)sp, *k_b = (uint64_t *)(sp + kb), *sz_sorted = (uint64_t *)(sp + 2 * kb), *sz_band = (uint64_t *)(sp + 3 * kb);
    uint32_t *p_a = (uint32_t *)(sp + 4 * kb), *order = (uint32_t *)(sp + 4 * kb + pb), *rank1 = (uint32_t *)(sp + 4 * kb + 2 * pb),
             *starts = (uint32_t *)(sp + 4 * kb + 3 * pb);
    void *temp = sp + 4 * kb + 4 * pb;
    const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
    const uint64_t mask = band_bits >= 64 ? ~0ull : ((1ull << band_bits) - 1ull);
    hipLaunchKernelGGL(ke_size_keys, grid, blk, 0, ctx->stream, d_sizes, n, k_a, p_a);
    size_t tb = temp_bytes;
    KE_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(temp, tb, (const uint64_t *)k_a, sz_sorted, (const uint32_t *)p_a, order, (int)n, 0, 64, ctx->stream));
    for (int b = 0; b < band_count; ++b) {
        hipLaunchKernelGGL(ke_band_keys_of, grid, blk, 0, ctx->stream, d_hashes, (const uint32_t *)order, n, b * band_bits, mask, k_a);
        tb = temp_bytes;
        KE_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(temp, tb, (const uint64_t *)k_a, k_b, (const uint64_t *)sz_sorted, sz_band, (int)n, 0,
                                                       band_bits, ctx->stream));
        uint32_t *flags = p_a;                                // the positions are not needed again
        hipLaunchKernelGGL(ke_run_flags, grid, blk, 0, ctx->stream, (const uint64_t *)k_b, n, flags);
        tb = temp_bytes;
        KE_HIP(ctx, hipcub::DeviceScan::InclusiveSum(temp, tb, (const uint32_t *)flags, rank1, (int)n, ctx->stream));
        hipLaunchKernelGGL(ke_run_starts, grid, blk, 0, ctx->stream, (const uint64_t *)k_b, (const uint32_t *)rank1, n, starts);
        hipLaunchKernelGGL(ke_size_pairs, grid, blk, 0, ctx->stream, (const uint64_t *)sz_band, (const uint32_t *)rank1,
                           (const uint32_t *)starts, n, ratio, cap, d_out);
        KE_HIP(ctx, hipGetLastError());
    }
    return KE_OK;
}

// Plan, reserve, launch: what runs and how large its buffers are is ke_scan_plan.h's business.  KE_SCAN_MODE=auto|tiles|buckets
// (auto lets the device choose per call, the other two force a path; buckets still means tiles where the plan has no bucket
// path; must be the same on every rank of a sharded scan) and KE_SCAN_TILES_PER_LAUNCH are read once per process.
int ke_launch_scan(ke_ctx *ctx, const KeScanRequest &rq, unsigned long long **d_counters_out, unsigned long long *pairs_evaluated) {
    static const KeScanKnobs knobs = [] {
        const char *mode = std::getenv("KE_SCAN_MODE"), *per = std::getenv("KE_SCAN_TILES_PER_LAUNCH");
        KeScanKnobs k;
        k.forced = !mode ? KE_SCAN_AUTO : !std::strcmp(mode, "tiles") ? KE_SCAN_FORCE_TILES : !std::strcmp(mode, "buckets") ? KE_SCAN_FORCE_BUCKETS : KE_SCAN_AUTO;
        k.tiles_per_launch = per ? std::atoll(per) : 0;
        return k;
    }();
    // by KeScanKind; KE_SCAN_ALL launches what a scan always did: its kernels read neither the region nor first_new
    static constexpr void (*tile_kernels[])(ScanArgs, KeScanRegion) = {ke_scan_tiles, ke_scan_tiles_from, ke_scan_tiles_cross};
    static constexpr void (*pair_kernels[])(ScanArgs, const uint64_t *, const uint32_t *, int, int, int64_t) = {
        ke_bucket_pairs, ke_bucket_pairs_from, ke_bucket_pairs_cross};
    const int64_t n = rq.n;
    KeScanShape shape;
    shape.n = n; shape.first_new = rq.first_new; shape.kind = rq.kind;
    shape.part_index = rq.part_index; shape.part_count = rq.part_count;
    shape.band_bits = rq.band_bits; shape.band_count = rq.band_count;
    shape.bucket_pair_cap = rq.bucket_pair_cap;
    shape.exact = rq.exact; shape.want_bucket_pairs = rq.want_bucket_pairs;
    KeScanPlan p = ke_scan_plan(shape, knobs);
    // [sorted hashes | per-bin offsets | sorted positions]; a table too large for it is scanned by the tile kernel
    void *srt = nullptr;
    if (p.buckets && ke_reserve(ctx, KE_BUF_SCAN_SORT, p.sort_bytes, &srt) != KE_OK) {
        (void)hipGetLastError();
        ctx->err.clear();                          // not a failure of this call: the tile kernel needs no such buffer
        shape.buckets_allowed = false;
        p = ke_scan_plan(shape, knobs);
    }
    switch (p.refusal) {
    case KE_SCAN_WIDE_NEEDS_32_BITS: return ke_fail(ctx, KE_EUNSUPPORTED, "bands wider than 24 bits need n < 2^32");
    case KE_SCAN_TOO_MANY_TILES: return ke_fail(ctx, KE_EUNSUPPORTED, "too many tiles for one launch");
    case KE_SCAN_CROSS_OVER_ONE_LAUNCH:
        return ke_fail(ctx, KE_EUNSUPPORTED, "%lld tiles of %d threads do not fit one launch", (long long)p.my_tiles, kThreads);
    }
    *pairs_evaluated = p.pairs;
    ScanArgs a;
    a.hashes = rq.hashes; a.ids = rq.ids; a.sizes = (rq.size_ratio > 0.0) ? rq.sizes : nullptr;
    a.n = n;
    a.nb = (int)p.region.nb;
    a.ncc = (int)p.region.ncc;
    a.n_tiles = p.n_tiles;
    a.first_tile = rq.part_index;
    a.tile_step = rq.part_count;
    a.threshold = rq.threshold; a.band_bits = rq.band_bits; a.band_count = rq.band_count;
    a.size_ratio = rq.size_ratio;
    a.hist = nullptr; a.blen = nullptr;
    a.cap = p.cap;
    a.exact = rq.exact ? 1 : 0;
    a.edges = rq.edges; a.capacity = rq.capacity;
    const size_t slots = (size_t)rq.band_count * (size_t)n;
    uint64_t *sorted_hash = (uint64_t *)srt;
    uint32_t *offsets = (uint32_t *)(sorted_hash + slots), *sorted_pos = offsets + p.bins;
    // One allocation, one memset: [counters, path, longest bucket | block sums | histogram]
    void *st;
    KE_TRY(ke_reserve(ctx, KE_BUF_SCAN_CNT, p.state_bytes, &st));
    unsigned long long *state = (unsigned long long *)st;
    uint32_t *block_sums = (uint32_t *)((uint8_t *)st + kScanStateBytes), *hist = (uint32_t *)((uint8_t *)st + p.hist_at);
    a.counters = state;
    *d_counters_out = state;
    void *exp;
    KE_TRY(ke_reserve(ctx, KE_BUF_SCAN_EXP, p.exp_bytes, &exp));
    a.expanded = (const ke_v4i *)exp;
    ke_time_begin(ctx, KE_T_SCAN);
    KE_HIP(ctx, hipMemsetAsync(st, 0, p.state_bytes, ctx->stream));
    const dim3 per_hash((unsigned)((n + 255) / 256)), blk(256);
    // Bucket sizes per band: needed by the bucket path and the pair cap, and they give the reference's "pairs total"
    // counter (counters[3]).
    if (p.need_hist) {
        hipLaunchKernelGGL(ke_band_hist, per_hash, blk, 0, ctx->stream, rq.hashes, n, rq.band_bits, rq.band_count, hist);
        KE_HIP(ctx, hipGetLastError());
        a.hist = hist;
    }
    if (p.buckets) {
        const dim3 blocks((unsigned)((p.bins + kBinsPerBlock - 1) / kBinsPerBlock));
        hipLaunchKernelGGL(ke_bucket_stats, blocks, blk, 0, ctx->stream, (const uint32_t *)hist, p.bins, a.cap, block_sums, state);
        hipLaunchKernelGGL(ke_bucket_offsets, blocks, blk, 0, ctx->stream, (const uint32_t *)hist, p.bins, (const uint32_t *)block_sums,
                           offsets, state, knobs.forced, (unsigned long long)p.bucket_threshold, (unsigned long long)p.pairs);
        hipLaunchKernelGGL(ke_bucket_scatter, per_hash, blk, 0, ctx->stream, rq.hashes, n, rq.band_bits, rq.band_count, offsets,
                           sorted_hash, sorted_pos, (const unsigned long long *)state);
        hipLaunchKernelGGL(pair_kernels[p.kind], dim3((unsigned)((n + kPairSlots - 1) / kPairSlots), (unsigned)rq.band_count), blk, 0,
                           ctx->stream, a, (const uint64_t *)sorted_hash, (const uint32_t *)sorted_pos, rq.part_index, rq.part_count,
                           rq.first_new);
        KE_HIP(ctx, hipGetLastError());
    }
    if (p.hist_pairs) {
        const unsigned blocks = (unsigned)std::min<size_t>((p.bins + 1023) / 1024, 256);
        hipLaunchKernelGGL(ke_hist_pairs, dim3(blocks), blk, 0, ctx->stream, (const uint32_t *)hist, p.bins, a.cap, state + 3);
        KE_HIP(ctx, hipGetLastError());
    }
    if (p.wide_sort) {
        // sort (band value, position) per band; scratch: keys in/out, positions in/out, per-hash lengths, cub temp storage
        size_t temp_bytes = 0;
        KE_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                                       (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, 0, rq.band_bits, ctx->stream));
        const size_t kb = ((size_t)n * 8 + 255) & ~(size_t)255, pb = ((size_t)n * 4 + 255) & ~(size_t)255;
        void *scratch, *lens;
        KE_TRY(ke_reserve(ctx, KE_BUF_SCAN_AUX, 2 * kb + 2 * pb + temp_bytes + 256, &scratch));
        KE_TRY(ke_reserve(ctx, KE_BUF_SCAN_HIST, (size_t)rq.band_count * n * sizeof(uint32_t), &lens));
        uint8_t *sp = (uint8_t *)scratch;
        uint64_t *k_in = (uint64_t *)sp, *k_out = (uint64_t *)(sp + kb);
        uint32_t *p_in = (uint32_t *)(sp + 2 * kb), *p_out = (uint32_t *)(sp + 2 * kb + pb);
        void *temp = sp + 2 * kb + 2 * pb;
        const uint64_t mask = rq.band_bits >= 64 ? ~0ull : ((1ull << rq.band_bits) - 1ull);
        for (int b = 0; b < rq.band_count; ++b) {
            hipLaunchKernelGGL(ke_band_keys, per_hash, blk, 0, ctx->stream, rq.hashes, n, b * rq.band_bits, mask, k_in, p_in);
            KE_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, k_in, k_out, p_in, p_out, (int)n, 0, rq.band_bits, ctx->stream));
            hipLaunchKernelGGL(ke_run_lengths, per_hash, blk, 0, ctx->stream, k_out, p_out, n, a.cap, (uint32_t *)lens + (size_t)b * n,
                               state + 3);
            KE_HIP(ctx, hipGetLastError());
        }
        a.blen = (const uint32_t *)lens;
    }
    if (p.n_slices > 0) {
        const int64_t n_pad = p.region.nb * kTile;
        hipLaunchKernelGGL(ke_scan_expand, dim3((unsigned)((n_pad * 4 + 255) / 256)), blk, 0, ctx->stream, rq.hashes, n, n_pad,
                           (ke_v4i *)exp, (const unsigned long long *)(state + kPathWord));
    }
    // one workgroup per tile: splitting a thin region's tiles over 2 or 4 workgroups was measured and did not pay (DESIGN
    // section 5).  Only first_tile moves from slice to slice; the tiles count their pairs into counters[0] as ever, and the
    // caller's closed-form check covers all slices together.
    for (int64_t i = 0; i < p.n_slices; ++i) {
        const KeScanSlice slice = ke_scan_slice(p, i);
        a.first_tile = slice.first_tile;
        hipLaunchKernelGGL(tile_kernels[p.kind], dim3((unsigned)slice.count), dim3(kThreads), 0, ctx->stream, a, p.region);
        KE_HIP(ctx, hipGetLastError());
    }
    ke_time_end(ctx, KE_T_SCAN);
    return KE_OK;
}
