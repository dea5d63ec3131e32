// ke_webpa.hip -- lossy WebP files with an alpha plane (one VP8 key frame + one ALPH chunk, or the VP8X alpha flag alone) decoded
// on the GPU: the decode step in front of the hash path for what `cwebp` and `Image.save("x.webp")` write for a
// picture with transparency, among the WebP files the reference ranks with its keepers (src/dup/scanner.py:16-28).  Replaces
// `Image.open(path)` + pixel access of the reference's batch hasher (src/core/fastsig.py:31-34) for the files ke_webpa_parse.h
// takes; the arithmetic is ke_webp_core.h's (frame), ke_webpl_core.h's (a plane coded as a VP8L stream) and ke_webpa_core.h's
// (the plane's filters), each held against Pillow on the CPU.  The container, the frame header and the ALPH header byte are
// read on the host's threads.
//
//   frame              ke_webp.hip's token and reconstruction kernels as they are (ke_webp_launch_frames).
//   ke_webpa_entropy   ONE THREAD PER METHOD-1 PLANE walks the header-less VP8L stream, as ke_webpl_entropy does (the colour cache
//                      forbids deferring the copies); neighbours in a wave are sorted to like stream lengths.
//   ke_webpa_transform ONE WORKGROUP PER METHOD-1 PLANE undoes the VP8L transforms (ke_webpl_transform.h's scheme).
//   ke_webpa_filter    ONE WORKGROUP PER FILTERED PLANE.  Horizontal: column 0 is a prefix sum (mod 256) down the column, then every
//                      row a prefix sum from its first pixel -- a wave per row, 64 pixels a step, __shfl_up scans with a carry.
//                      Vertical: row 0 a prefix sum, then a lane per column running down it (rows read coalesced).  Gradient:
//                      clip(left + above - above-left) is not linear, so a wavefront over anti-diagonals -- (x, y) at step x + y,
//                      one lane per row of a step, the two diagonals before it kept in LDS (3 x height bytes; lanes of a step
//                      touch neighbouring bytes: same dword or the next bank, no conflicts).
//   ke_webpa_colour    one thread per pixel: fancy upsampling + YUV -> RGB as ke_webp_colour, and the plane's byte (255 without a
//                      plane) as the fourth.
// A method-1 plane stays where the stream decoder left it, in the green bytes of its ARGB words (stride 4); a raw plane is read
// from the file's bytes and, when filtered, written to W x H bytes of scratch.
#include <algorithm>
#include <vector>

#include "ke_decode_batch.h"
#include "ke_webp_launch.h"
#include "ke_webpa_launch.h"
#include "ke_webpl_transform.h"

namespace {

__global__ __launch_bounds__(64) void ke_webpa_entropy_k(const KeWebpaDev *__restrict__ planes, const int32_t *__restrict__ order, int64_t n,
                                                        const uint8_t *__restrict__ files, uint8_t *__restrict__ scratch,
                                                        KeVp8lPlan *__restrict__ plans, int32_t *__restrict__ status) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const int32_t i = order[k];
    const KeWebpaDev &a = planes[i];
    KeVp8lBits b;
    ke_vp8l_bits_init(b, files + a.alph_off, a.alph_size);
    KeVp8lPlan plan;
    status[i] = ke_vp8l_decode_body(b, a.width, a.height, (uint32_t *)(scratch + a.plane_off), a.plane_words, plan);
    plans[i] = plan;
}

constexpr int kPlaneThreads = 256;

__global__ __launch_bounds__(kPlaneThreads) void ke_webpa_transform_k(const KeWebpaDev *__restrict__ planes, const int32_t *__restrict__ order,
                                                                     uint8_t *__restrict__ scratch, const KeVp8lPlan *__restrict__ plans,
                                                                     const int32_t *__restrict__ status) {
    const int32_t i = order[blockIdx.x];
    if (status[i] != KE_WEBPL_OK) return;
    const KeWebpaDev &a = planes[i];
    ke_vp8l_undo_transforms_wg<kPlaneThreads>((uint32_t *)(scratch + a.plane_off), plans[i], a.width, a.height, (int)threadIdx.x);
}

// Inclusive prefix sum over the wave's 64 lanes.
__device__ __forceinline__ uint32_t ke_wave_scan(uint32_t v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

// dst[k * step] = (carry + src[0] + .. + src[k * step]) & 255 for k in [0, n): a prefix sum (mod 256) along a row (step 1) or a
// column (step W) by the whole workgroup, 256 values a round.  totals: 4 words of LDS.
__device__ __forceinline__ void ke_block_prefix(const uint8_t *src, uint8_t *dst, size_t stride, size_t step, int n, uint32_t *totals, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t carry = 0;
    for (int k0 = 0; k0 < n; k0 += kPlaneThreads) {
        const int k = k0 + tid;
        uint32_t v = k < n ? src[(size_t)k * step * stride] : 0u;
        v = ke_wave_scan(v, lane);
        if (lane == 63) totals[wave] = v;
        __syncthreads();
        uint32_t before = carry;
        for (int w = 0; w < wave; ++w) before += totals[w];
        if (k < n) dst[(size_t)k * step * stride] = (uint8_t)(before + v);
        carry += totals[0] + totals[1] + totals[2] + totals[3];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kPlaneThreads) void ke_webpa_filter_k(const KeWebpaDev *__restrict__ planes, const uint8_t *__restrict__ files,
                                                                  uint8_t *__restrict__ scratch, const int32_t *__restrict__ status_f,
                                                                  const int32_t *__restrict__ status_a) {
    extern __shared__ uint8_t diag[];                              // gradient: three anti-diagonals, `height` bytes each
    __shared__ uint32_t totals[4];
    const int64_t i = blockIdx.x;
    const KeWebpaDev &a = planes[i];
    if (status_f[i] != KE_WEBP_OK || status_a[i] != KE_WEBPL_OK || a.method == KE_ALPH_OPAQUE || a.filter == KE_ALPH_FILTER_NONE) return;
    const int W = a.width, H = a.height, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // stored values and finished plane: the green bytes of the decoded ARGB words, in place; or the file's bytes -> scratch
    const bool raw = a.method == KE_ALPH_RAW;
    const size_t stride = raw ? 1 : 4;
    uint8_t *dst = scratch + a.plane_off + (raw ? 0 : 1);
    const uint8_t *src = raw ? files + a.alph_off : dst;
    if (a.filter == KE_ALPH_FILTER_HORIZONTAL) {
        ke_block_prefix(src, dst, stride, (size_t)W, H, totals, tid);    // column 0: every pixel predicted by the one above
        __syncthreads();
        for (int y = wave; y < H; y += kPlaneThreads / 64) {
            const size_t row = (size_t)y * W;
            uint32_t carry = dst[row * stride];
            for (int x0 = 1; x0 < W; x0 += 64) {
                const int x = x0 + lane;
                uint32_t v = x < W ? src[(row + x) * stride] : 0u;
                v = carry + ke_wave_scan(v, lane);
                if (x < W) dst[(row + x) * stride] = (uint8_t)v;
                carry = __shfl(v, 63, 64);
            }
        }
    } else if (a.filter == KE_ALPH_FILTER_VERTICAL) {
        ke_block_prefix(src, dst, stride, 1, W, totals, tid);            // row 0: every pixel predicted by the one to its left
        __syncthreads();
        for (int x = tid; x < W; x += kPlaneThreads) {
            uint32_t acc = dst[(size_t)x * stride];
            for (int y = 1; y < H; ++y) {
                const size_t j = (size_t)y * W + x;
                acc += src[j * stride];
                dst[j * stride] = (uint8_t)acc;
            }
        }
    } else {
        uint8_t *cur = diag, *d1 = diag + H, *d2 = diag + 2 * (size_t)H;    // this step's diagonal, the one before, the one before that
        const int steps = W + H - 1;
        for (int s = 0; s < steps; ++s) {
            // pixels (s - y, y) of this step: y from max(0, s - W + 1) to min(H - 1, s)
            const int ylo = s - W + 1 > 0 ? s - W + 1 : 0, yhi = min(H - 1, s);
            for (int y = ylo + tid; y <= yhi; y += kPlaneThreads) {
                const int x = s - y;
                const size_t j = (size_t)y * W + x;
                const uint32_t left = x ? d1[y] : 0u, above = y ? d1[y - 1] : 0u, above_left = x && y ? d2[y - 1] : 0u;
                const uint32_t v = (src[j * stride] + ke_alph_predict(KE_ALPH_FILTER_GRADIENT, x, y, left, above, above_left)) & 255u;
                dst[j * stride] = (uint8_t)v;
                cur[y] = (uint8_t)v;
            }
            __syncthreads();
            uint8_t *t = d2;
            d2 = d1; d1 = cur; cur = t;
        }
    }
}

constexpr int kRowsPerBlock = 8;

__global__ __launch_bounds__(256) void ke_webpa_colour_k(const KeWebpDev *__restrict__ imgs, const KeWebpaDev *__restrict__ planes,
                                                        const uint8_t *__restrict__ files, const uint8_t *__restrict__ scratch,
                                                        const int32_t *__restrict__ status_f, const int32_t *__restrict__ status_a,
                                                        uint8_t *__restrict__ out, int rows) {
    const int64_t i = blockIdx.x;
    const KeWebpDev &d = imgs[i];
    const int y0 = blockIdx.y * rows;
    if (status_f[i] != KE_WEBP_OK || status_a[i] != KE_WEBPL_OK || y0 >= d.h.height) return;
    const KeWebpaDev &a = planes[i];
    const int W = d.h.width, H = d.h.height, mb_w = d.h.mb_w;
    const size_t nmb = (size_t)mb_w * d.h.mb_h;
    const uint8_t *Y = ke_webp_frame_planes(d, scratch), *U = Y + nmb * 256, *V = U + nmb * 64;
    // the plane: the file's own bytes (raw, unfiltered), the scratch's bytes (raw, filtered), the green bytes of the ARGB words
    const uint8_t *alpha = nullptr;
    size_t stride = 1;
    if (a.method == KE_ALPH_RAW) alpha = a.filter == KE_ALPH_FILTER_NONE ? files + a.alph_off : scratch + a.plane_off;
    else if (a.method == KE_ALPH_VP8L) { alpha = scratch + a.plane_off + 1; stride = 4; }
    const int y1 = min(y0 + rows, H);
    const bool aligned = ((uintptr_t)(out + a.out_off) & 3) == 0;    // one store per pixel where the caller's offset allows it
    for (int y = y0; y < y1; ++y)
        for (int x = threadIdx.x; x < W; x += 256) {
            uint8_t rgb[3];
            ke_webp_rgb_at(Y, U, V, mb_w, W, H, x, y, rgb);
            const size_t j = (size_t)y * W + x;
            const uint32_t al = alpha ? alpha[j * stride] : 255u;
            uint8_t *o = out + a.out_off + j * 4;
            if (aligned) {
                *(uint32_t *)o = (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16) | (al << 24);
            } else {
                o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2]; o[3] = (uint8_t)al;
            }
        }
}

}  // namespace

int ke_webpa_launch_planes(ke_ctx *ctx, const KeWebpaDev *d_planes, const int32_t *d_order, int64_t m, int64_t m1, int max_gradient_height,
                           const uint8_t *d_files, uint8_t *d_scratch, KeVp8lPlan *d_plans, const int32_t *d_status_f, int32_t *d_status_a) {
    if (m1) {
        hipLaunchKernelGGL(ke_webpa_entropy_k, dim3((unsigned)((m1 + 63) / 64)), dim3(64), 0, ctx->stream, d_planes, d_order, m1, d_files, d_scratch,
                           d_plans, d_status_a);
        hipLaunchKernelGGL(ke_webpa_transform_k, dim3((unsigned)m1), dim3(kPlaneThreads), 0, ctx->stream, d_planes, d_order, d_scratch,
                           (const KeVp8lPlan *)d_plans, (const int32_t *)d_status_a);
    }
    hipLaunchKernelGGL(ke_webpa_filter_k, dim3((unsigned)m), dim3(kPlaneThreads), (size_t)3 * max_gradient_height, ctx->stream, d_planes, d_files,
                       d_scratch, d_status_f, (const int32_t *)d_status_a);
    return KE_OK;
}

KE_API int ke_webpa_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                          int32_t *heights, int32_t *channels, int32_t *status_out) {
    return ke_probe_each(files, offsets, sizes, n, widths, heights, channels, status_out,
                         [](const uint8_t *file, size_t size, int32_t &w, int32_t &h, int32_t &c, int32_t &st) {
                             KeWebpaHeader hd;                       // container, frame tag, ALPH header byte: the decode call parses the rest
                             ke_webpa_tag(file, size, hd);
                             w = hd.f.width; h = hd.f.height; c = 4; st = hd.f.status;
                         });
}

KE_API int ke_webpa_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out) {
    // An EXIF chunk or an XMP packet may carry an orientation the reference's loader applies (flagged without reading it); every
    // file taken here is RGBA, which that loader composites over white.
    return ke_caveats_each(files, offsets, sizes, n, flags_out, [](const uint8_t *file, size_t size) {
        KeWebpaHeader h;
        ke_webpa_tag(file, size, h);
        return (h.f.meta ? KE_CAVEAT_ORIENTATION : 0) | (h.f.status == KE_WEBPA_OK ? KE_CAVEAT_TRANSPARENCY : 0);
    });
}

KE_API int ke_webpa_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                           uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out) {
    KE_TRY(ke_decode_check_args(ctx, files, offsets, sizes, n, pixels_out, out_offsets, status_out, "the files' headers are parsed"));
    if (n == 0) return KE_OK;
    std::vector<KeWebpaHeader> items((size_t)n);                    // the headers are parsed on the host's threads
    ke_parallel_ranges(n, [&](int64_t a, int64_t b, int) {
        for (int64_t i = a; i < b; ++i) ke_parse_webpa(files + offsets[i], (size_t)sizes[i], items[(size_t)i]);
    });
    std::vector<int64_t> which;
    which.reserve((size_t)n);
    uint64_t lo = ~0ull, hi = 0;
    for (int64_t i = 0; i < n; ++i) {
        status_out[i] = items[(size_t)i].f.status;
        if (status_out[i] != KE_WEBPA_OK) continue;
        lo = std::min(lo, offsets[i]);
        hi = std::max(hi, offsets[i] + sizes[i]);
        which.push_back(i);
    }
    if (which.empty()) return KE_OK;
    // lanes of one wave finish together at best: neighbours in the batch should have streams of like length
    std::stable_sort(which.begin(), which.end(), [&](int64_t a, int64_t b) { return items[(size_t)a].f.vp8_size > items[(size_t)b].f.vp8_size; });
    std::vector<KeWebpDev> devs;
    std::vector<KeWebpaDev> planes;
    std::vector<int32_t> order;
    KeStreamGuard guard;                                           // after the host vectors it waits for
    void *d_files;
    KE_TRY(ke_upload_files(ctx, guard, files, lo, hi, KE_BUF_PIXELS, 256, &d_files));
    // sub-batches bounded by scratch: 1 172 B per macroblock, and the plane's -- about 9.2 bytes per pixel and 96 KiB for a stream,
    // a byte per pixel for raw bytes
    uint64_t budget;                                                // KE_WEBP_SCRATCH_BYTES: a smaller one (tests: many sub-batches)
    KE_TRY(ke_scratch_budget(ctx, {KE_BUF_SSIM_IN}, (uint64_t)2 << 30, (uint64_t)160 << 30, "KE_WEBP_SCRATCH_BYTES", KE_BUDGET_ENV_LOWERS, &budget));
    uint64_t bytes = 0;
    int max_height = 0, max_filtered = 0;
    auto take = [&](size_t k, bool fresh) {
        if (fresh) {
            bytes = 0;
            max_height = max_filtered = 0;
            devs.clear();
            planes.clear();
            order.clear();
        }
        const int64_t i = which[k];
        const KeWebpaHeader &h = items[(size_t)i];
        const uint64_t frame = ke_webp_frame_scratch(h.f), plane = (ke_webpa_plane_words(h) * 4 + 15) & ~15ull;
        if (!fresh && bytes + frame + plane > budget) return false;
        KeWebpDev d;
        d.h = h.f;
        d.file_off = offsets[i] - lo;
        d.scratch_off = bytes;
        d.out_off = out_offsets[i];
        KeWebpaDev a;
        a.alph_off = d.file_off + h.alph_off;
        a.plane_off = bytes + frame;
        a.plane_words = ke_webpa_plane_words(h);
        a.out_off = out_offsets[i];
        a.alph_size = h.alph_size;
        a.method = h.method; a.filter = h.filter;
        a.width = h.f.width; a.height = h.f.height;
        bytes += frame + plane;
        max_height = std::max(max_height, h.f.height);
        if (h.method != KE_ALPH_OPAQUE && h.filter == KE_ALPH_FILTER_GRADIENT) max_filtered = std::max(max_filtered, h.f.height);
        if (h.method == KE_ALPH_VP8L) order.push_back((int32_t)devs.size());
        devs.push_back(d);
        planes.push_back(a);
        return true;
    };
    auto launch = [&](size_t um, const int32_t **status, size_t *words) {
        const int64_t m = (int64_t)um, m1 = (int64_t)order.size();
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return planes[(size_t)a].alph_size > planes[(size_t)b].alph_size; });
        // one record buffer: [frames | planes | order]; one status buffer: [frames | planes]
        const size_t at_planes = ((size_t)m * sizeof(KeWebpDev) + 15) & ~(size_t)15, at_order = at_planes + (((size_t)m * sizeof(KeWebpaDev) + 15) & ~(size_t)15);
        void *d_meta, *d_scratch, *d_status, *d_plans;
        KE_TRY(ke_reserve(ctx, KE_BUF_META, at_order + (size_t)m * 4 + 16, &d_meta));
        KE_TRY(ke_reserve(ctx, KE_BUF_SSIM_IN, (size_t)bytes + 64, &d_scratch));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT0, (size_t)m * 8, &d_status));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT1, (size_t)m * sizeof(KeVp8lPlan), &d_plans));
        const KeWebpDev *d_imgs = (const KeWebpDev *)d_meta;
        const KeWebpaDev *d_planes = (const KeWebpaDev *)((uint8_t *)d_meta + at_planes);
        const int32_t *d_order = (const int32_t *)((uint8_t *)d_meta + at_order);
        int32_t *d_status_f = (int32_t *)d_status, *d_status_a = d_status_f + m;
        KE_HIP(ctx, hipMemcpyAsync(d_meta, devs.data(), (size_t)m * sizeof(KeWebpDev), hipMemcpyHostToDevice, ctx->stream));
        KE_HIP(ctx, hipMemcpyAsync((uint8_t *)d_meta + at_planes, planes.data(), (size_t)m * sizeof(KeWebpaDev), hipMemcpyHostToDevice, ctx->stream));
        if (m1) KE_HIP(ctx, hipMemcpyAsync((uint8_t *)d_meta + at_order, order.data(), (size_t)m1 * 4, hipMemcpyHostToDevice, ctx->stream));
        KE_HIP(ctx, hipMemsetAsync(d_status_a, 0, (size_t)m * 4, ctx->stream));      // planes without a stream have nothing to fail
        KE_TRY(ke_webp_launch_frames(ctx, d_imgs, m, (const uint8_t *)d_files, (uint8_t *)d_scratch, d_status_f));
        KE_TRY(ke_webpa_launch_planes(ctx, d_planes, d_order, m, m1, max_filtered, (const uint8_t *)d_files, (uint8_t *)d_scratch, (KeVp8lPlan *)d_plans,
                                      (const int32_t *)d_status_f, d_status_a));
        const KeRowTiles tiles = ke_row_tiles(max_height, kRowsPerBlock);
        hipLaunchKernelGGL(ke_webpa_colour_k, dim3((unsigned)m, tiles.grid_y), dim3(256), 0, ctx->stream, d_imgs,
                           d_planes, (const uint8_t *)d_files, (const uint8_t *)d_scratch, (const int32_t *)d_status_f,
                           (const int32_t *)d_status_a, pixels_out, tiles.rows);
        *status = d_status_f;
        *words = (size_t)m * 2;
        return (int)KE_OK;
    };
    // a frame that failed keeps its status; otherwise the plane's decides
    KE_TRY(ke_decode_sub_batches(ctx, which.size(), take, launch, [&](size_t at, size_t k, size_t m, const int32_t *st) {
        status_out[which[at]] = st[k] != KE_WEBP_OK ? st[k] : st[m + k];
    }));
    guard.disarm();
    return KE_OK;
}
