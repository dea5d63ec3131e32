// ke_webpl.hip -- lossless WebP files (one VP8L bitstream) decoded on the GPU: the decode step in front of the hash path (SURVEY
// 8 f2) for the WebP files the reference ranks among its keepers (src/dup/scanner.py:16-28).  Replaces `Image.open(path)` + pixel
// access of the reference's batch hasher (src/core/fastsig.py:31-34) for the files ke_webpl_parse.h takes; the arithmetic is
// ke_webpl_core.h's (held against Pillow on the CPU).  The container and the 5-byte header are read on the host's threads.
//
//   ke_webpl_entropy    ONE THREAD PER IMAGE walks the stream: transforms' sub-images, colour cache, entropy image, the prefix
//                       codes of every group, then the ARGB words of the image (literals, cache hits, LZ77 copies).  The
//                       stream is serial, and the colour cache makes a later symbol depend on the values of copied pixels,
//                       so the copies cannot be put off as ke_png_inflate puts them off; neighbours in a wave are sorted to
//                       like stream lengths instead.
//   ke_webpl_transform  ONE WORKGROUP PER IMAGE undoes the transforms, last to first.  Predictor: rows as a skewed wavefront,
//                       (x, y) at step x + 2y -- after (x - 1, y) and (x + 1, y - 1) --, one lane per row of a step.
//                       Cross-colour and subtract-green: a lane per pixel.  Colour indexing with packed pixels: row by row
//                       towards the front of the buffer, the packed rows lying behind where their pixels go.
//   ke_webpl_output     one thread per pixel: RGB or RGBA bytes at the caller's offsets.
#include <algorithm>
#include <vector>

#include "ke_decode_batch.h"
#include "ke_webpl_launch.h"
#include "ke_webpl_transform.h"

namespace {

__global__ __launch_bounds__(64) void ke_webpl_entropy_k(const KeWebplDev *__restrict__ imgs, int64_t n, const uint8_t *__restrict__ files,
                                                        uint8_t *__restrict__ scratch, KeVp8lPlan *__restrict__ plans,
                                                        int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const KeWebplDev &d = imgs[i];
    KeVp8lPlan plan;
    status[i] = ke_vp8l_decode_stream(files + d.file_off + d.h.off, d.h.size, d.h.width, d.h.height, (uint32_t *)(scratch + d.scratch_off),
                                      d.scratch_words, plan);
    plans[i] = plan;
}

constexpr int kTransformThreads = 256;

__global__ __launch_bounds__(kTransformThreads) void ke_webpl_transform_k(const KeWebplDev *__restrict__ imgs, uint8_t *__restrict__ scratch,
                                                                         const KeVp8lPlan *__restrict__ plans,
                                                                         const int32_t *__restrict__ status) {
    const int64_t i = blockIdx.x;
    if (status[i] != KE_WEBPL_OK) return;
    const KeWebplDev &d = imgs[i];
    ke_vp8l_undo_transforms_wg<kTransformThreads>((uint32_t *)(scratch + d.scratch_off), plans[i], d.h.width, d.h.height, (int)threadIdx.x);
}

constexpr int kRowsPerBlock = 8;

__global__ __launch_bounds__(256) void ke_webpl_output_k(const KeWebplDev *__restrict__ imgs, const uint8_t *__restrict__ scratch,
                                                        const int32_t *__restrict__ status, uint8_t *__restrict__ out, int rows) {
    const int64_t i = blockIdx.x;
    const KeWebplDev &d = imgs[i];
    const int y0 = blockIdx.y * rows;
    if (status[i] != KE_WEBPL_OK || y0 >= d.h.height) return;
    const int W = d.h.width, ch = d.h.channels;
    const uint32_t *pix = (const uint32_t *)(scratch + d.scratch_off);     // the finished image lies at the front
    const size_t lo = (size_t)y0 * W, hi = (size_t)min(y0 + rows, d.h.height) * W;
    for (size_t j = lo + threadIdx.x; j < hi; j += 256) ke_vp8l_store(pix[j], out + d.out_off + j * ch, ch);
}

}  // namespace

int ke_webpl_launch_images(ke_ctx *ctx, const KeWebplDev *d_imgs, int64_t m, const uint8_t *d_files, uint8_t *d_scratch, KeVp8lPlan *d_plans,
                           int32_t *d_status) {
    hipLaunchKernelGGL(ke_webpl_entropy_k, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, ctx->stream, d_imgs, m, d_files, d_scratch, d_plans, d_status);
    hipLaunchKernelGGL(ke_webpl_transform_k, dim3((unsigned)m), dim3(kTransformThreads), 0, ctx->stream, d_imgs, d_scratch, (const KeVp8lPlan *)d_plans,
                       (const int32_t *)d_status);
    return KE_OK;
}

KE_API int ke_webpl_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                          int32_t *heights, int32_t *channels, int32_t *status_out) {
    return ke_probe_each(files, offsets, sizes, n, widths, heights, channels, status_out,
                         [](const uint8_t *file, size_t size, int32_t &w, int32_t &h, int32_t &c, int32_t &st) {
                             KeWebplHeader hd;
                             ke_parse_webpl(file, size, hd);
                             w = hd.width; h = hd.height; c = hd.channels; st = hd.status;
                         });
}

KE_API int ke_webpl_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out) {
    // An EXIF chunk or an XMP packet may carry an orientation the reference's loader applies (flagged without reading it);
    // an RGBA file is composited over white by it.
    return ke_caveats_each(files, offsets, sizes, n, flags_out, [](const uint8_t *file, size_t size) {
        KeWebplHeader h;
        ke_parse_webpl(file, size, h);
        return (h.meta ? KE_CAVEAT_ORIENTATION : 0) | (h.channels == 4 ? KE_CAVEAT_TRANSPARENCY : 0);
    });
}

KE_API int ke_webpl_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                           uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out) {
    KE_TRY(ke_decode_check_args(ctx, files, offsets, sizes, n, pixels_out, out_offsets, status_out, "the files' headers are parsed"));
    if (n == 0) return KE_OK;
    std::vector<KeWebplDev> items((size_t)n);
    ke_parallel_ranges(n, [&](int64_t a, int64_t b, int) {
        for (int64_t i = a; i < b; ++i) ke_parse_webpl(files + offsets[i], (size_t)sizes[i], items[(size_t)i].h);
    });
    std::vector<int64_t> which;
    which.reserve((size_t)n);
    uint64_t lo = ~0ull, hi = 0;
    for (int64_t i = 0; i < n; ++i) {
        KeWebplDev &d = items[(size_t)i];
        status_out[i] = d.h.status;
        if (d.h.status != KE_WEBPL_OK) continue;
        d.file_off = offsets[i];
        d.out_off = out_offsets[i];
        d.scratch_words = ke_vp8l_scratch_words(d.h.width, d.h.height);
        lo = std::min(lo, offsets[i]);
        hi = std::max(hi, offsets[i] + sizes[i]);
        which.push_back(i);
    }
    if (which.empty()) return KE_OK;
    // lanes of one wave finish together at best: neighbours in the batch should have streams of like length
    std::stable_sort(which.begin(), which.end(), [&](int64_t a, int64_t b) { return sizes[a] > sizes[b]; });
    std::vector<KeWebplDev> devs;
    KeStreamGuard guard;                                           // after the host vectors it waits for
    void *d_files;
    KE_TRY(ke_upload_files(ctx, guard, files, lo, hi, KE_BUF_PIXELS, 256, &d_files));
    // sub-batches bounded by scratch: about 9.2 bytes per pixel and 96 KiB per image
    uint64_t budget;                                                // KE_WEBP_SCRATCH_BYTES: a smaller one (tests: many sub-batches)
    KE_TRY(ke_scratch_budget(ctx, {KE_BUF_SSIM_IN}, (uint64_t)2 << 30, (uint64_t)160 << 30, "KE_WEBP_SCRATCH_BYTES", KE_BUDGET_ENV_LOWERS, &budget));
    uint64_t bytes = 0;
    int max_height = 0;
    auto take = [&](size_t k, bool fresh) {
        if (fresh) {
            bytes = 0;
            max_height = 0;
            devs.clear();
        }
        KeWebplDev d = items[(size_t)which[k]];
        const uint64_t need = (d.scratch_words * 4 + 15) & ~15ull;
        if (!fresh && bytes + need > budget) return false;
        d.file_off -= lo;
        d.scratch_off = bytes;
        bytes += need;
        max_height = std::max(max_height, d.h.height);
        devs.push_back(d);
        return true;
    };
    auto launch = [&](size_t m, const int32_t **status, size_t *words) {
        void *d_imgs, *d_scratch, *d_status, *d_plans;
        KE_TRY(ke_reserve(ctx, KE_BUF_META, m * sizeof(KeWebplDev), &d_imgs));
        KE_TRY(ke_reserve(ctx, KE_BUF_SSIM_IN, (size_t)bytes + 64, &d_scratch));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT0, m * 4, &d_status));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT1, m * sizeof(KeVp8lPlan), &d_plans));
        KE_HIP(ctx, hipMemcpyAsync(d_imgs, devs.data(), m * sizeof(KeWebplDev), hipMemcpyHostToDevice, ctx->stream));
        KE_TRY(ke_webpl_launch_images(ctx, (const KeWebplDev *)d_imgs, (int64_t)m, (const uint8_t *)d_files, (uint8_t *)d_scratch, (KeVp8lPlan *)d_plans,
                                      (int32_t *)d_status));
        const KeRowTiles tiles = ke_row_tiles(max_height, kRowsPerBlock);
        hipLaunchKernelGGL(ke_webpl_output_k, dim3((unsigned)m, tiles.grid_y), dim3(256), 0, ctx->stream,
                           (const KeWebplDev *)d_imgs, (const uint8_t *)d_scratch, (const int32_t *)d_status, pixels_out, tiles.rows);
        *status = (const int32_t *)d_status;
        *words = m;
        return (int)KE_OK;
    };
    KE_TRY(ke_decode_sub_batches(ctx, which.size(), take, launch,
                                 [&](size_t at, size_t k, size_t, const int32_t *st) { status_out[which[at]] = st[k]; }));
    guard.disarm();
    return KE_OK;
}
