// ke_gif.hip -- the first frame of GIF files decoded on the GPU: the decode step in front of the hash path for the
// fourth of the formats the reference ranks as keepers (src/dup/scanner.py:16-28).  Replaces `Image.open(path)` + pixel access of
// the reference's batch hasher (src/core/fastsig.py:31-34); what leaves is the luma `convert("L")` makes of the frame, which is
// what the reference's hashes see (src/sig/phash.py:25).  The arithmetic is ke_gif_core.h's (held against Pillow on the CPU).
//
//   ke_gif_codes    ONE THREAD PER IMAGE walks the code stream (it is sequential by construction).  A code below the clear
//                   code is a pixel and goes to its place; any other is a string that lies in the output already -- recorded as
//                   a copy (ke_gif_core.h), not made: a lane that waited for its own earlier stores would stall the other 63.
//                   The dictionary (4 096 x {where, how long}) is a slice of HBM per image; the file's bytes come through a
//                   16-byte register window that is refilled one step ahead.
//   ke_gif_copies   ONE WAVE PER IMAGE makes the recorded copies, 64 per round (ke_lz_copies.h, the PNG path's).
//   ke_gif_rows     index -> luma through the frame's table, rows put where an interlaced frame wants them.
#include <algorithm>
#include <vector>

#include "ke_decode_batch.h"

#include "ke_gif_core.h"
#include "ke_lz_copies.h"
#include "ke_lz_records.h"
#include "ke_lz_window.h"

namespace {

struct KeGifDev {
    uint64_t file_off;     // the file inside the uploaded bytes
    uint64_t idx_off;      // the frame's indices (width * height bytes) inside the scratch
    uint64_t rec_off;      // this image's copy records (8 bytes each; a copy covers at least 2 pixels)
    uint64_t out_off;      // bytes into the caller's pixel buffer
    uint32_t file_size, data_off;
    int32_t width, height, bits, interlace;
    uint8_t lut[256];
};

__global__ __launch_bounds__(64) void ke_gif_codes(const KeGifDev *__restrict__ imgs, int64_t n, const uint8_t *__restrict__ files,
                                                 uint8_t *__restrict__ indices, uint2 *__restrict__ records, uint2 *__restrict__ dicts,
                                                 int32_t *__restrict__ status, uint32_t *__restrict__ nrec) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const KeGifDev &d = imgs[i];
    WindowSrc src;
    src.file = files + d.file_off;
    src.limit = d.file_size;
    src.start(d.data_off);
    HbmDict dict{dicts + (size_t)i * 4096};
    KeLzRecSink sink{indices + d.idx_off, records + d.rec_off, 0, 0};
    const uint32_t want = (uint32_t)d.width * (uint32_t)d.height;
    status[i] = ke_gif_lzw(src, d.data_off, d.file_size, d.bits, want, dict, sink);
    nrec[i] = sink.nrec;
}

__global__ __launch_bounds__(64) void ke_gif_copies(const KeGifDev *__restrict__ imgs, uint8_t *__restrict__ indices,
                                                    const uint2 *__restrict__ records, const int32_t *__restrict__ status,
                                                    const uint32_t *__restrict__ nrec) {
    const int64_t i = blockIdx.x;
    if (status[i] != KE_GIF_OK) return;
    const KeGifDev &d = imgs[i];
    ke_lz_make_copies(indices + d.idx_off, records + d.rec_off, nrec[i], 2u);       // a copied string has at least 2 characters
}

constexpr int kRowsPerBlock = 8;

__global__ __launch_bounds__(256) void ke_gif_rows(const KeGifDev *__restrict__ imgs, const uint8_t *__restrict__ indices,
                                                   const int32_t *__restrict__ status, uint8_t *__restrict__ out, int rows) {
    __shared__ uint8_t s_lut[256];
    const int64_t i = blockIdx.x;
    const KeGifDev &d = imgs[i];
    const int k0 = blockIdx.y * rows;
    if (status[i] != KE_GIF_OK || k0 >= d.height) return;
    s_lut[threadIdx.x] = d.lut[threadIdx.x];
    __syncthreads();
    const int W = d.width, k1 = min(k0 + rows, d.height);
    for (int k = k0; k < k1; ++k) {                        // k: the row as it was decoded
        const uint8_t *src = indices + d.idx_off + (size_t)k * W;
        uint8_t *dst = out + d.out_off + (size_t)ke_gif_row(k, d.height, d.interlace) * W;
        for (int x = threadIdx.x; x < W; x += 256) dst[x] = s_lut[src[x]];
    }
}

}  // namespace

KE_API int ke_gif_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                        int32_t *heights, int32_t *channels, int32_t *status_out) {
    return ke_probe_each(files, offsets, sizes, n, widths, heights, channels, status_out,
                         [](const uint8_t *file, size_t size, int32_t &w, int32_t &h, int32_t &c, int32_t &st) {
                             KeGifInfo info;
                             ke_parse_gif(file, size, info);
                             w = info.width; h = info.height; c = info.channels; st = info.status;
                         });
}

KE_API int ke_gif_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out) {
    return ke_caveats_none(files, offsets, sizes, n, flags_out);       // (the decoder yields luma: only the hashing seams take it)
}

KE_API int ke_gif_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                         uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out) {
    KE_TRY(ke_decode_check_args(ctx, files, offsets, sizes, n, pixels_out, out_offsets, status_out, "the files' containers are walked"));
    if (n == 0) return KE_OK;
    struct Item { KeGifDev d; int64_t which; };
    std::vector<Item> items;
    items.reserve((size_t)n);
    uint64_t lo = ~0ull, hi = 0;
    std::vector<KeGifInfo> infos((size_t)n);                     // the containers are walked on the host's threads
    ke_parallel_ranges(n, [&](int64_t a, int64_t b, int) {
        for (int64_t i = a; i < b; ++i) ke_parse_gif(files + offsets[i], (size_t)sizes[i], infos[(size_t)i]);
    });
    for (int64_t i = 0; i < n; ++i) {
        const KeGifInfo &info = infos[(size_t)i];
        status_out[i] = info.status;
        if (info.status != KE_GIF_OK) continue;
        Item it;
        it.which = i;
        it.d.file_off = offsets[i];
        it.d.out_off = out_offsets[i];
        it.d.file_size = (uint32_t)sizes[i];
        it.d.data_off = info.data_off;
        it.d.width = info.width; it.d.height = info.height; it.d.bits = info.bits; it.d.interlace = info.interlace;
        std::memcpy(it.d.lut, info.lut, 256);
        lo = std::min(lo, offsets[i]);
        hi = std::max(hi, offsets[i] + sizes[i]);
        items.push_back(it);
    }
    if (items.empty()) return KE_OK;
    // lanes of one wave finish together at best: neighbours in the batch should have streams of like length
    std::stable_sort(items.begin(), items.end(), [](const Item &a, const Item &b) { return a.d.file_size > b.d.file_size; });
    std::vector<KeGifDev> devs;
    KeStreamGuard guard;                                           // after the host vectors it waits for
    void *d_files;
    KE_TRY(ke_upload_files(ctx, guard, files, lo, hi, KE_BUF_PIXELS, 256, &d_files));
    // sub-batches bounded by scratch: indices (1 B per pixel) + copy records (8 B per 2 pixels at worst) + 32 KB of dictionary
    uint64_t budget;
    KE_TRY(ke_scratch_budget(ctx, {KE_BUF_SSIM_IN, KE_BUF_TMP, KE_BUF_SSIM_AUX}, (uint64_t)2 << 30, (uint64_t)160 << 30, nullptr,
                             KE_BUDGET_ENV_LOWERS, &budget));
    uint64_t idx_bytes = 0, nrecs = 0;
    int max_height = 0;
    auto take = [&](size_t k, bool fresh) {
        if (fresh) {
            idx_bytes = nrecs = 0;
            max_height = 0;
            devs.clear();
        }
        Item &it = items[k];
        const uint64_t px = (uint64_t)it.d.width * it.d.height;
        const uint64_t ib = (px + 64 + 15) & ~15ull, rc = px / 2 + 2;
        if (!fresh && idx_bytes + ib + (nrecs + rc) * 8 + (uint64_t)(devs.size() + 1) * 32768 > budget) return false;
        it.d.file_off -= lo;
        it.d.idx_off = idx_bytes;
        it.d.rec_off = nrecs;
        idx_bytes += ib;
        nrecs += rc;
        max_height = std::max(max_height, it.d.height);
        devs.push_back(it.d);
        return true;
    };
    auto launch = [&](size_t m, const int32_t **status, size_t *words) {
        void *d_imgs, *d_idx, *d_rec, *d_dict, *d_status, *d_nrec;
        KE_TRY(ke_reserve(ctx, KE_BUF_META, m * sizeof(KeGifDev), &d_imgs));
        KE_TRY(ke_reserve(ctx, KE_BUF_TMP, (size_t)idx_bytes + 128, &d_idx));
        KE_TRY(ke_reserve(ctx, KE_BUF_SSIM_AUX, (size_t)nrecs * 8, &d_rec));
        KE_TRY(ke_reserve(ctx, KE_BUF_SSIM_IN, m * 32768, &d_dict));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT0, m * 4, &d_status));
        KE_TRY(ke_reserve(ctx, KE_BUF_TILE32, m * 4, &d_nrec));
        KE_HIP(ctx, hipMemcpyAsync(d_imgs, devs.data(), m * sizeof(KeGifDev), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(ke_gif_codes, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, ctx->stream, (const KeGifDev *)d_imgs, (int64_t)m, (const uint8_t *)d_files,
                           (uint8_t *)d_idx, (uint2 *)d_rec, (uint2 *)d_dict, (int32_t *)d_status, (uint32_t *)d_nrec);
        hipLaunchKernelGGL(ke_gif_copies, dim3((unsigned)m), dim3(64), 0, ctx->stream, (const KeGifDev *)d_imgs, (uint8_t *)d_idx,
                           (const uint2 *)d_rec, (const int32_t *)d_status, (const uint32_t *)d_nrec);
        const KeRowTiles tiles = ke_row_tiles(max_height, kRowsPerBlock);
        hipLaunchKernelGGL(ke_gif_rows, dim3((unsigned)m, tiles.grid_y), dim3(256), 0, ctx->stream,
                           (const KeGifDev *)d_imgs, (const uint8_t *)d_idx, (const int32_t *)d_status, pixels_out, tiles.rows);
        *status = (const int32_t *)d_status;
        *words = m;
        return (int)KE_OK;
    };
    KE_TRY(ke_decode_sub_batches(ctx, items.size(), take, launch,
                                 [&](size_t at, size_t k, size_t, const int32_t *st) { status_out[items[at].which] = st[k]; }));
    guard.disarm();
    return KE_OK;
}
