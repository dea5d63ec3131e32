// ke_internal.h -- shared declarations of libkeyes_hip.so (gfx950 only, no CPU fallback).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/keyes.h"
#include "ke_coeffs.h"
#include "ke_scan_plan.h"
#include "ke_ssim_plan.h"
#include "ke_view_plan.h"

#define KE_API extern "C" __attribute__((visibility("default")))

struct KeDevBuf {
    void *ptr = nullptr;
    size_t bytes = 0;
};

enum { KE_T_HASH = 0, KE_T_SCAN = 1, KE_T_SSIM = 2, KE_T_SYNTH = 3, KE_T_JPEG = 4, KE_T_TRIM_BOX = 5, KE_T_TRIM_CROP = 6, KE_T_TRIM_LUMA = 7, KE_T_VIEW_LUMA = 8, KE_T_NEAREST = 9, KE_T_COUNT = 10 };
enum {
    KE_BUF_PIXELS = 0,   // staged input images
    KE_BUF_TMP,          // first-pass output of the generic resampler
    KE_BUF_TILE32,
    KE_BUF_TILE98,
    KE_BUF_OUT0,         // staged outputs
    KE_BUF_OUT1,
    KE_BUF_OUT2,         // staged tie margins
    KE_BUF_META,         // offsets / out_idx arrays
    KE_BUF_SCAN_IN,
    KE_BUF_SCAN_AUX,
    KE_BUF_SCAN_EDGES,
    KE_BUF_SCAN_CNT,     // scan state, zeroed by one memset per call: counters, path word, block sums, band histogram
    KE_BUF_SCAN_HIST,    // wide bands only: per-hash bucket lengths
    KE_BUF_SCAN_SORT,    // bucket path: hashes sorted by band value band by band, per-bin offsets, their positions
    KE_BUF_SCAN_EXP,     // hashes expanded to matrix-core operands (64 B each)
    KE_BUF_SSIM_IN,
    KE_BUF_SSIM_AUX,
    KE_BUF_COMM,         // gathered hash shards before they are put back into corpus order
    KE_BUF_COMM_EDGES,   // edge records: [send | world x recv]
    KE_BUF_JPEG_TABLES,  // Huffman tables of a JPEG batch
    KE_BUF_TURN_TILES,   // ke_hash_images_turned: the 32x32 tiles of a call's images, group after group
    KE_BUF_TRIM_BOXES,   // ke_content_boxes: the boxes of a call's images, 16 B each
    KE_BUF_TRIM_CROPS,   // ke_hash_images_trimmed: the packed crops of one chunk of qualifying images
    KE_BUF_VIEW_LUMA,    // the pair calls: the luma planes of a call's made views, 1 B/px per distinct (image, box, orientation)
    KE_BUF_NEAREST_IN,   // ke_hamming_nearest: the host's arrays among [hashes | ids | queries | query_ids]
    KE_BUF_NEAREST_OUT,  // ke_hamming_nearest: the host's arrays among [index | within | distance | count | histogram]
    KE_BUF_COUNT
};

// Pinned staging (north-star step 1): producers (decode threads) write pixels straight into page-locked host buffers;
// a submit enqueues the H2D copy on a copy stream and the hash kernels behind an event on the compute stream, so the copy
// of batch k+1 overlaps the kernels of batch k and the host never blocks between batches.
constexpr int KE_MAX_STAGE_SLOTS = 4;
struct KeStageSlot {
    uint8_t *h_px = nullptr, *d_px = nullptr;        // pinned pixels and their device twin
    uint64_t *h_meta = nullptr, *d_meta = nullptr;   // per size group: [byte offsets | output slots]
    uint64_t *h_ph = nullptr, *h_dh = nullptr, *d_ph = nullptr, *d_dh = nullptr;
    float *h_mg = nullptr, *d_mg = nullptr;
    hipEvent_t copied = nullptr, done = nullptr;
    bool in_flight = false;
    bool px_external = false;                         // h_px is the caller's memory, registered with the runtime
    uint64_t *user_ph = nullptr, *user_dh = nullptr;  // where the results go when the slot is waited for
    float *user_mg = nullptr;
    int64_t n = 0;
};
struct KeStage {
    size_t bytes = 0;
    int64_t max_images = 0;
    int n_slots = 0, next = 0;
    hipStream_t copy_stream = nullptr;
    KeStageSlot slot[KE_MAX_STAGE_SLOTS];
};

struct ke_ctx {
    int device = 0;
    int cu_count = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    KeDevBuf buf[KE_BUF_COUNT];
    std::map<std::tuple<int, int, uint32_t, uint32_t>, KeAxisCoeffs *> coeffs;   // key: (in_size, out_size * 4 + filter, bits of in0, in1)
    hipEvent_t ev0[KE_T_COUNT] = {}, ev1[KE_T_COUNT] = {};
    bool ev_valid[KE_T_COUNT] = {};
    KeStage *stage = nullptr;
    hipStream_t side[2] = {nullptr, nullptr};   // side streams of the ragged hash call: neighbouring size groups overlap their tails
    hipEvent_t side_fork = nullptr, side_join[2] = {nullptr, nullptr};
    int64_t edge_slots = 1024;       // edges carried by one record of ke_allgather_edges (follows the largest list seen)
    void *h_comm = nullptr;          // pinned landing zone of the gathered edge records
    size_t h_comm_bytes = 0;
    void *h_meta = nullptr;          // page-locked per-image records of a decode batch on their way to the device
    size_t h_meta_bytes = 0;
    int scan_path = -1;              // path of the last ke_hamming_scan: 0 tiles, 1 buckets (ke_last_scan_path)
    int32_t resize_plan[8] = {-1, -1, -1, -1, -1, -1, -1, -1};   // of the last group of ke_launch_resize_group (ke_last_resize_plan)
    int32_t ssim_plan[KE_SP_COUNT] = {-1, -1, -1, -1, -1, -1, -1, -1};   // of the last ke_launch_ssim (ke_last_ssim_plan)
    bool ssim_exact = false;         // ke_ssim_set_mode: false = integer-sum kernel (default), true = fp64-carry kernel
    float *margin_cur = nullptr;     // device array the hash kernels of the CURRENT call write tie margins to (slot = hash slot)
    int64_t decode_sub_batches = 0;  // sub-batches the last ke_decode_sub_batches worked its images off in (ke_last_decode_sub_batches)
    int64_t jpeg_files_split = 0, jpeg_split_lanes = 0;   // of the last JPEG decode call: files decoded interval-wise, their lanes (ke_jpeg_last_split)
    bool dct_tables_ready = false;   // __constant__ tables are per device: uploaded once per context
};

// error helpers ------------------------------------------------------------------------------
int ke_fail(ke_ctx *ctx, int code, const char *fmt, ...);
#define KE_HIP(ctx, call)                                                                        \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return ke_fail((ctx), KE_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                           __FILE__, __LINE__);                                                  \
    } while (0)
#define KE_TRY(expr)            \
    do {                        \
        int rc_ = (expr);       \
        if (rc_ != KE_OK) return rc_; \
    } while (0)

// memory helpers (ke_api.hip) ------------------------------------------------------------------
bool ke_is_device_ptr(const void *p);
int ke_reserve(ke_ctx *ctx, int which, size_t bytes, void **out);
// Returns in *dev a device pointer holding `bytes` of `p` (p itself if it already is device memory,
// else a staged copy in buffer `which`).
int ke_to_device(ke_ctx *ctx, const void *p, size_t bytes, int which, const void **dev);
// taps of one axis; (in0, in1) = source interval (Pillow's box), in1 < 0 means the whole axis
const KeAxisCoeffs *ke_get_coeffs(ke_ctx *ctx, int in_size, int out_size, int filter = KE_FILTER_LANCZOS, float in0 = 0.0f,
                                  float in1 = -1.0f);
const KeChunkTable *ke_get_chunks(ke_ctx *ctx, const KeAxisCoeffs *c, int cpo, int ndwc_multiple = 4);
// min_ks: build with at least this many steps per tile (zero operands past the window); a cached table keeps its own
// align64: every tile's first tap column is a multiple of 64 (the strip kernel cuts rows at multiples of 64)
const KeMxTable *ke_get_mx(ke_ctx *ctx, const KeAxisCoeffs *c, int min_ks = 0, bool align64 = false);
void ke_time_begin(ke_ctx *ctx, int kind);
void ke_time_end(ke_ctx *ctx, int kind);

// kernel launchers (one per .hip file) ------------------------------------------------------------
struct KeHashGroup {
    const uint8_t *pixels;     // device
    const uint64_t *offsets;   // device, nullable (then image k is at k*stride)
    uint64_t stride;
    const int64_t *out_idx;    // device, nullable (then output slot k)
    int64_t n;
    int w, h, channels;
    bool misaligned = false;   // some image of the group starts at an address that is not a multiple of 4
};
// Images [first, first + count) of a group.  With out_idx == NULL a slot is the position in the group: the caller keeps
// that true for the part by offsetting its output pointers.
inline KeHashGroup ke_sub_group(const KeHashGroup &g, int64_t first, int64_t count) {
    KeHashGroup s = g;
    s.n = count;
    if (g.offsets) s.offsets = g.offsets + first; else s.pixels = g.pixels + (size_t)first * g.stride;
    if (g.out_idx) s.out_idx = g.out_idx + first;
    return s;
}
// fused_stream (nullable): where the scratch-free one-workgroup-per-image kernel of the group may run instead of ctx->stream
int ke_launch_hash_group(ke_ctx *ctx, const KeHashGroup &g, uint64_t *d_phash, uint64_t *d_dhash,
                         uint8_t *d_tile32_out, uint8_t *d_tile98_out, hipStream_t fused_stream = nullptr);
// the eight turned pHashes of n 32x32 tiles (device): tile k -> d_turned[(d_out_idx ? d_out_idx[k] : k) * 8 + 0..7]
int ke_launch_tiles_turned(ke_ctx *ctx, const uint8_t *d_tile32, const int64_t *d_out_idx, int64_t n, uint64_t *d_turned);
// luma + resize of a group to (oh x ow) u8 tiles with the given filter (banded path, generic fallback)
// box = {x0, y0, x1, y1} source rectangle (Pillow's resize box), NULL = the whole image
// ctx->resize_plan holds what was launched for the last group, written from the plans of the path that ran (ke_last_resize_plan):
enum { KE_RP_BANDED = 0, KE_RP_CPO, KE_RP_NDWC, KE_RP_LAUNCHES, KE_RP_BANDS, KE_RP_FUNNEL, KE_RP_VMX, KE_RP_VFIRST, KE_RP_COUNT };
int ke_launch_resize_group(ke_ctx *ctx, const KeHashGroup &g, int ow, int oh, int filter, uint8_t *d_tiles,
                           const float *box = nullptr);
// the made views of the pair calls (job structs: ke_view_plan.h): the luma plane of a box of each image (ke_trim.hip), and of an
// orientation of a box of each image (ke_turn.hip; `timer`: the KE_T_* that times the launches, or -1).  The box lies inside its
// image, the job table goes through KE_BUF_META and the stream is drained before the call returns
int ke_launch_crop_luma(ke_ctx *ctx, const uint8_t *d_src, const KeCropLumaJob *jobs, int64_t n, uint8_t *d_dst);
int ke_launch_view_luma(ke_ctx *ctx, const uint8_t *d_src, const KeViewJob *jobs, int64_t n, uint8_t *d_dst, int timer);
int ke_launch_tile_ahash(ke_ctx *ctx, const uint8_t *d_tiles, int64_t n, int grid, int tile, uint64_t *d_bits);
int ke_launch_sad_pairs(ke_ctx *ctx, const uint8_t *d_thumbs, int64_t pixels, const int64_t *d_pa, const int64_t *d_pb,
                        int64_t n_pairs, uint64_t *d_out);
int ke_launch_band_pairs_after_size(ke_ctx *ctx, const uint64_t *d_hashes, const int64_t *d_sizes, int64_t n, int band_bits,
                                    int band_count, double ratio, int64_t bucket_pair_cap, unsigned long long *d_out);
// One pair scan.  The four ke_hamming_scan* calls fill it with their caller's pointers (host or device), ke_launch_scan gets it
// with device pointers; what is launched for it: ke_scan_plan.h
struct KeScanRequest {
    const uint64_t *hashes = nullptr;
    const int64_t *ids = nullptr, *sizes = nullptr;   // nullable
    int64_t n = 0, first_new = 0;
    KeScanKind kind = KE_SCAN_ALL;
    int part_index = 0, part_count = 1;
    int threshold = 0, band_bits = 0, band_count = 0;
    double size_ratio = 0.0;
    int64_t bucket_pair_cap = 0;
    bool exact = false;               // ke_hamming_scan_exact: pairs that share no band are edges as well
    ke_edge *edges = nullptr;
    int64_t capacity = 0;
    bool want_bucket_pairs = false;   // counters[3] is wanted
};
int ke_launch_scan(ke_ctx *ctx, const KeScanRequest &rq, unsigned long long **d_counters_out, unsigned long long *pairs_evaluated);
constexpr int KE_SCAN_STATE_WORDS = 5;   // what ke_hamming_scan reads back: counters [0..3] and the path word
// ctx->ssim_plan holds the KE_SP_* words of the plan (ke_ssim_plan.h) that the last call launched (ke_last_ssim_plan)
int ke_launch_ssim(ke_ctx *ctx, const uint8_t *d_images, int w, int h, int channels, const int64_t *d_pa,
                   const int64_t *d_pb, int64_t n_pairs, double *d_out);
int ke_launch_synth_rgb(ke_ctx *ctx, uint64_t seed, int64_t first, const int64_t *d_indices, int64_t n, int w, int h,
                        uint8_t *d_out);
int ke_launch_synth_hashes(ke_ctx *ctx, uint64_t seed, int64_t n, uint64_t *d_out);

// Host-side loops over the files of a batch (header parsing): [0, n) cut into contiguous ranges, one per thread; fn(lo, hi, t).
// KE_HOST_THREADS overrides the thread count (default: the hardware's, at most 16, at least 256 items per thread).
template <typename Fn>
static inline int ke_parallel_ranges(int64_t n, Fn fn) {
    int want = (int)std::thread::hardware_concurrency();
    if (const char *e = std::getenv("KE_HOST_THREADS")) want = std::atoi(e);
    int nt = (int)std::min<int64_t>(std::max(want, 1), std::min<int64_t>(16, n / 256));
    if (nt <= 1) { fn((int64_t)0, n, 0); return 1; }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back([=]() { fn(n * t / nt, n * (t + 1) / nt, t); });
    for (auto &x : th) x.join();
    return nt;
}
