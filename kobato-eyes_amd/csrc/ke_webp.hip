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
#include <cstdlib>
#include <vector>

#include "ke_internal.h"
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
    if (n < 0 || (n > 0 && (!files || !offsets || !sizes || !widths || !heights || !channels || !status_out))) return KE_EINVAL;
    ke_parallel_ranges(n, [=](int64_t lo, int64_t hi, int) {
        for (int64_t i = lo; i < hi; ++i) {
            KeWebpHeader h;                                         // container + frame tag: the decode call parses the rest
            ke_webp_frame_tag(files + offsets[i], (size_t)sizes[i], h);
            widths[i] = h.width; heights[i] = h.height; channels[i] = 3;
            status_out[i] = h.status;
        }
    });
    return KE_OK;
}

KE_API int ke_webp_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out) {
    if (n < 0 || (n > 0 && (!files || !offsets || !sizes || !flags_out))) return KE_EINVAL;
    // An EXIF chunk -- or an XMP packet, whose tiff:Orientation Pillow's getexif() reads too -- may carry an orientation the
    // reference's loader applies: flagged without reading it (the loader decides).
    ke_parallel_ranges(n, [=](int64_t lo, int64_t hi, int) {
        for (int64_t i = lo; i < hi; ++i) {
            uint32_t off, size;
            int cw, ch, meta;
            ke_webp_container(files + offsets[i], (size_t)sizes[i], off, size, cw, ch, meta);
            flags_out[i] = meta ? KE_CAVEAT_ORIENTATION : 0;
        }
    });
    return KE_OK;
}

KE_API int ke_webp_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                          uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out) {
    if (!ctx) return KE_EINVAL;
    if (n < 0 || (n > 0 && (!files || !offsets || !sizes || !pixels_out || !out_offsets || !status_out)))
        return ke_fail(ctx, KE_EINVAL, "NULL argument");
    if (n == 0) return KE_OK;
    if (ke_is_device_ptr(files)) return ke_fail(ctx, KE_EINVAL, "the files' headers are parsed on the host: pass host memory (pinned staging is fine)");
    if (!ke_is_device_ptr(pixels_out)) return ke_fail(ctx, KE_EINVAL, "pixels_out must be device memory");
    for (const void *p : {(const void *)offsets, (const void *)sizes, (const void *)out_offsets, (const void *)status_out})
        if (ke_is_device_ptr(p)) return ke_fail(ctx, KE_EINVAL, "offsets/sizes/status are host arrays");
    KE_HIP(ctx, hipSetDevice(ctx->device));
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
    void *d_files;
    KE_TRY(ke_reserve(ctx, KE_BUF_PIXELS, (size_t)(hi - lo) + 256, &d_files));
    KE_HIP(ctx, hipMemcpyAsync(d_files, files + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, ctx->stream));
    // sub-batches bounded by scratch: 1 172 B per macroblock
    size_t free_b = 0, total_b = 0;
    KE_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    const uint64_t held = (uint64_t)ctx->buf[KE_BUF_SSIM_IN].bytes;
    uint64_t budget = std::max<uint64_t>((uint64_t)2 << 30, std::min<uint64_t>((held + (uint64_t)free_b) / 2, (uint64_t)160 << 30));
    if (const char *e = getenv("KE_WEBP_SCRATCH_BYTES")) {          // a smaller budget (tests: many sub-batches); results do not depend on it
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v > 0) budget = std::min<uint64_t>(budget, v);
    }
    std::vector<KeWebpDev> devs;
    std::vector<int32_t> st;
    size_t first = 0;
    ke_time_begin(ctx, KE_T_JPEG);
    while (first < which.size()) {
        uint64_t bytes = 0;
        int max_height = 0;
        size_t last = first;
        devs.clear();
        while (last < which.size()) {
            KeWebpDev d = items[(size_t)which[last]];
            const uint64_t need = ke_webp_frame_scratch(d.h);
            if (last > first && bytes + need > budget) break;
            d.file_off -= lo;
            d.scratch_off = bytes;
            bytes += need;
            max_height = std::max(max_height, d.h.height);
            devs.push_back(d);
            ++last;
        }
        const int64_t m = (int64_t)devs.size();
        void *d_imgs, *d_scratch, *d_status;
        KE_TRY(ke_reserve(ctx, KE_BUF_META, (size_t)m * sizeof(KeWebpDev), &d_imgs));
        KE_TRY(ke_reserve(ctx, KE_BUF_SSIM_IN, (size_t)bytes + 64, &d_scratch));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT0, (size_t)m * 4, &d_status));
        KE_HIP(ctx, hipMemcpyAsync(d_imgs, devs.data(), (size_t)m * sizeof(KeWebpDev), hipMemcpyHostToDevice, ctx->stream));
        KE_TRY(ke_webp_launch_frames(ctx, (const KeWebpDev *)d_imgs, m, (const uint8_t *)d_files, (uint8_t *)d_scratch, (int32_t *)d_status));
        const int rows = std::max(kRowsPerBlock, (max_height + 65534) / 65535);
        hipLaunchKernelGGL(ke_webp_colour_k, dim3((unsigned)m, (unsigned)((max_height + rows - 1) / rows)), dim3(256), 0, ctx->stream,
                           (const KeWebpDev *)d_imgs, (const uint8_t *)d_scratch, (const int32_t *)d_status, pixels_out, rows);
        KE_HIP(ctx, hipGetLastError());
        st.resize((size_t)m);
        KE_HIP(ctx, hipMemcpyAsync(st.data(), d_status, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
        KE_HIP(ctx, hipStreamSynchronize(ctx->stream));                  // devs / st are host vectors; the scratch is reused
        for (int64_t k = 0; k < m; ++k) status_out[which[first + (size_t)k]] = st[(size_t)k];
        first = last;
    }
    ke_time_end(ctx, KE_T_JPEG);
    return KE_OK;
}
