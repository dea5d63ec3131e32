// ke_webp.hip -- lossy WebP files (one VP8 key frame) decoded on the GPU: the decode step in front of the hash path
// for the WebP files the reference ranks among its keepers (src/dup/scanner.py:16-28).  Replaces `Image.open(path)` + pixel
// access of the reference's batch hasher (src/core/fastsig.py:31-34) for the files ke_webp_parse.h takes; the arithmetic is
// ke_webp_core.h's (held against Pillow on the CPU).  The container and the frame header -- with its ~1 000 probability
// updates -- are read on the host's threads, as the other formats' headers are.
//
//   ke_webp_tokens   ONE THREAD PER IMAGE walks partition 0 (modes) and the token partitions (both are serial by
//                    construction): per macroblock a mode record and 384 dequantised coefficients (the Y2 block undone).
//   ke_webp_recon    ONE WAVE PER IMAGE: reconstruction, then the loop filter, both over macroblocks in wavefront order --
//                    (x, y) at step x + 2y, after (x - 1, y) and (x + 1, y - 1) -- one lane per macroblock of a step.
//                    Prediction reads the unfiltered planes, so the filter runs once the whole frame is reconstructed.
//   ke_webp_colour   one thread per output pixel: fancy upsampling + YUV -> RGB, packed RGB where the hash kernels want it.
#include <algorithm>
#include <vector>

#include "ke_decode_batch.h"
#include "ke_webp_launch.h"

namespace {

__device__ __forceinline__ void ke_webp_layout(const KeWebpDev &d, uint8_t *scratch, int16_t *&coeffs, uint8_t *&planes, KeWebpMb *&mbs) {
    const size_t nmb = (size_t)d.h.mb_w * d.h.mb_h;
    coeffs = (int16_t *)(scratch + d.scratch_off);
    planes = scratch + d.scratch_off + nmb * 768;
    mbs = (KeWebpMb *)(planes + nmb * 384);
}

__global__ __launch_bounds__(64) void ke_webp_tokens_k(const KeWebpDev *__restrict__ imgs, int64_t n, const uint8_t *__restrict__ files,
                                                      uint8_t *__restrict__ scratch, int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const KeWebpDev &d = imgs[i];
    int16_t *coeffs;
    uint8_t *planes;
    KeWebpMb *mbs;
    ke_webp_layout(d, scratch, coeffs, planes, mbs);
    status[i] = ke_webp_tokens(d.h, files + d.file_off, mbs, coeffs, planes);   // the planes hold the columns' contexts meanwhile
}

__global__ __launch_bounds__(64) void ke_webp_recon_k(const KeWebpDev *__restrict__ imgs, uint8_t *__restrict__ scratch,
                                                     const int32_t *__restrict__ status) {
    const int64_t i = blockIdx.x;
    if (status[i] != KE_WEBP_OK) return;
    const KeWebpDev &d = imgs[i];
    int16_t *coeffs;
    uint8_t *planes;
    KeWebpMb *mbs;
    ke_webp_layout(d, scratch, coeffs, planes, mbs);
    const int mb_w = d.h.mb_w, mb_h = d.h.mb_h;
    const size_t nmb = (size_t)mb_w * mb_h;
    uint8_t *Y = planes, *U = planes + nmb * 256, *V = U + nmb * 64;
    const int steps = mb_w + 2 * (mb_h - 1);
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && d.h.filter_type == 0) break;
        for (int t = 0; t < steps; ++t) {
            // macroblocks (t - 2y, y) of this step: y from max(0, ceil((t - mb_w + 1) / 2)) to min(mb_h - 1, t / 2)
            const int ylo = t - mb_w + 1 > 0 ? (t - mb_w + 2) >> 1 : 0, yhi = min(mb_h - 1, t >> 1);
            for (int y = ylo + (int)threadIdx.x; y <= yhi; y += 64) {
                const int x = t - 2 * y;
                const KeWebpMb &m = mbs[y * mb_w + x];
                if (pass == 0) ke_webp_recon_mb(m, coeffs + (size_t)(y * mb_w + x) * 384, Y, U, V, mb_w, x, y);
                else ke_webp_filter_mb(d.h, m, Y, U, V, x, y);
            }
            __syncthreads();
        }
    }
}

constexpr int kRowsPerBlock = 8;

__global__ __launch_bounds__(256) void ke_webp_colour_k(const KeWebpDev *__restrict__ imgs, const uint8_t *__restrict__ scratch,
                                                       const int32_t *__restrict__ status, uint8_t *__restrict__ out, int rows) {
    const int64_t i = blockIdx.x;
    const KeWebpDev &d = imgs[i];
    const int y0 = blockIdx.y * rows;
    if (status[i] != KE_WEBP_OK || y0 >= d.h.height) return;
    const int W = d.h.width, H = d.h.height, mb_w = d.h.mb_w;
    const size_t nmb = (size_t)mb_w * d.h.mb_h;
    const uint8_t *Y = scratch + d.scratch_off + nmb * 768, *U = Y + nmb * 256, *V = U + nmb * 64;
    const int y1 = min(y0 + rows, H);
    for (int y = y0; y < y1; ++y)
        for (int x = threadIdx.x; x < W; x += 256) {
            uint8_t rgb[3];
            ke_webp_rgb_at(Y, U, V, mb_w, W, H, x, y, rgb);
            uint8_t *o = out + d.out_off + ((size_t)y * W + x) * 3;
            o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
        }
}

}  // namespace

int ke_webp_launch_frames(ke_ctx *ctx, const KeWebpDev *d_imgs, int64_t m, const uint8_t *d_files, uint8_t *d_scratch, int32_t *d_status) {
    hipLaunchKernelGGL(ke_webp_tokens_k, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, ctx->stream, d_imgs, m, d_files, d_scratch, d_status);
    hipLaunchKernelGGL(ke_webp_recon_k, dim3((unsigned)m), dim3(64), 0, ctx->stream, d_imgs, d_scratch, (const int32_t *)d_status);
    return KE_OK;
}

KE_API int ke_webp_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                         int32_t *heights, int32_t *channels, int32_t *status_out) {
    return ke_probe_each(files, offsets, sizes, n, widths, heights, channels, status_out,
                         [](const uint8_t *file, size_t size, int32_t &w, int32_t &h, int32_t &c, int32_t &st) {
                             KeWebpHeader hd;                        // container + frame tag: the decode call parses the rest
                             ke_webp_frame_tag(file, size, hd);
                             w = hd.width; h = hd.height; c = 3; st = hd.status;
                         });
}

KE_API int ke_webp_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out) {
    // An EXIF chunk -- or an XMP packet, whose tiff:Orientation Pillow's getexif() reads too -- may carry an orientation the
    // reference's loader applies: flagged without reading it (the loader decides).
    return ke_caveats_each(files, offsets, sizes, n, flags_out, [](const uint8_t *file, size_t size) {
        uint32_t off, bytes;
        int cw, ch, meta;
        ke_webp_container(file, size, off, bytes, cw, ch, meta);
        return meta ? KE_CAVEAT_ORIENTATION : 0;
    });
}

KE_API int ke_webp_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                          uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out) {
    KE_TRY(ke_decode_check_args(ctx, files, offsets, sizes, n, pixels_out, out_offsets, status_out, "the files' headers are parsed"));
    if (n == 0) return KE_OK;
    std::vector<KeWebpDev> items((size_t)n);                       // the headers are parsed on the host's threads
    ke_parallel_ranges(n, [&](int64_t a, int64_t b, int) {
        for (int64_t i = a; i < b; ++i) ke_parse_webp(files + offsets[i], (size_t)sizes[i], items[(size_t)i].h);
    });
    std::vector<int64_t> which;
    which.reserve((size_t)n);
    uint64_t lo = ~0ull, hi = 0;
    for (int64_t i = 0; i < n; ++i) {
        KeWebpDev &d = items[(size_t)i];
        status_out[i] = d.h.status;
        if (d.h.status != KE_WEBP_OK) continue;
        d.file_off = offsets[i];
        d.out_off = out_offsets[i];
        lo = std::min(lo, offsets[i]);
        hi = std::max(hi, offsets[i] + sizes[i]);
        which.push_back(i);
    }
    if (which.empty()) return KE_OK;
    // lanes of one wave finish together at best: neighbours in the batch should have streams of like length
    std::stable_sort(which.begin(), which.end(), [&](int64_t a, int64_t b) { return sizes[a] > sizes[b]; });
    std::vector<KeWebpDev> devs;
    KeStreamGuard guard;                                           // after the host vectors it waits for
    void *d_files;
    KE_TRY(ke_upload_files(ctx, guard, files, lo, hi, KE_BUF_PIXELS, 256, &d_files));
    // sub-batches bounded by scratch: 1 172 B per macroblock
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
        KeWebpDev d = items[(size_t)which[k]];
        const uint64_t need = ke_webp_frame_scratch(d.h);
        if (!fresh && bytes + need > budget) return false;
        d.file_off -= lo;
        d.scratch_off = bytes;
        bytes += need;
        max_height = std::max(max_height, d.h.height);
        devs.push_back(d);
        return true;
    };
    auto launch = [&](size_t m, const int32_t **status, size_t *words) {
        void *d_imgs, *d_scratch, *d_status;
        KE_TRY(ke_reserve(ctx, KE_BUF_META, m * sizeof(KeWebpDev), &d_imgs));
        KE_TRY(ke_reserve(ctx, KE_BUF_SSIM_IN, (size_t)bytes + 64, &d_scratch));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT0, m * 4, &d_status));
        KE_HIP(ctx, hipMemcpyAsync(d_imgs, devs.data(), m * sizeof(KeWebpDev), hipMemcpyHostToDevice, ctx->stream));
        KE_TRY(ke_webp_launch_frames(ctx, (const KeWebpDev *)d_imgs, (int64_t)m, (const uint8_t *)d_files, (uint8_t *)d_scratch, (int32_t *)d_status));
        const KeRowTiles tiles = ke_row_tiles(max_height, kRowsPerBlock);
        hipLaunchKernelGGL(ke_webp_colour_k, dim3((unsigned)m, tiles.grid_y), dim3(256), 0, ctx->stream,
                           (const KeWebpDev *)d_imgs, (const uint8_t *)d_scratch, (const int32_t *)d_status, pixels_out, tiles.rows);
        *status = (const int32_t *)d_status;
        *words = m;
        return (int)KE_OK;
    };
    KE_TRY(ke_decode_sub_batches(ctx, which.size(), take, launch,
                                 [&](size_t at, size_t k, size_t, const int32_t *st) { status_out[which[at]] = st[k]; }));
    guard.disarm();
    return KE_OK;
}
