// ke_webpn.hip -- the first frame of animated WebP files decoded on the GPU: the decode step in front of the hash path (SURVEY
// 8 f2) for the last class of WebP file the reference's batch hasher opens with `Image.open(path)` (src/core/fastsig.py:31-34;
// WebP ranks second among its keeper formats, src/dup/scanner.py:16-28) that stayed with Pillow.  For an animation that call
// yields frame 0 on an all-zero canvas.  ke_webpn_parse.h walks the container on the host's threads; frame 0 is a VP8 key
// frame, a VP8 key frame behind an ALPH chunk, or a VP8L image, and runs through the still decoders' kernels as they are:
//
//   lossy frames       ke_webp_launch_frames (tokens, reconstruction), then ke_webpa_launch_planes for the ones with a plane.
//   lossless frames    ke_webpl_launch_images (stream, transforms).
//   ke_webpn_canvas    ONE WORKGROUP PER (IMAGE, TILE OF ROWS) writes every pixel of the canvas exactly once: zeros outside the
//                      frame's rectangle; inside it fancy upsampling + YUV -> RGB over the frame's planes and the plane's byte
//                      (255 without one), or the ARGB word of a lossless frame.  3 or 4 bytes per pixel at the canvas stride.
//                      The kernel is write-bound: lanes of a wave write neighbouring dwords of a canvas row -- one pixel each
//                      with four channels; with three, dword q of the canvas holds bytes of pixels 4q / 3 and 4q / 3 + 1, both
//                      computed by its lane -- wherever the caller's offset is a multiple of four, and bytes otherwise
//                      (outputs lie packed back to back, so odd offsets are normal).
// A batch mixes the three codecs: records are grouped per codec (lossy frames first) and each group is sorted by stream length.
// The upload is the span of the taken files, so the later frames of an animation cross PCIe too.
#include <algorithm>
#include <vector>

#include "ke_decode_batch.h"
#include "ke_webp_launch.h"
#include "ke_webpa_launch.h"
#include "ke_webpl_launch.h"
#include "ke_webpn_parse.h"

namespace {

struct KeWebpnDev {
    uint64_t out_off;        // bytes into the caller's pixel buffer
    int32_t canvas_w, canvas_h, channels;
    int32_t x, y;            // the frame's offset inside the canvas
};

struct KeWebpnSource {       // one image's frame, as its pipeline left it
    const KeWebpDev *d;      // lossy: the frame's record and its plane's
    const KeWebpaDev *a;
    const uint8_t *Y, *U, *V;
    const uint32_t *pix;     // lossless: the ARGB words
    const uint8_t *files, *scratch;
    int x, y, W, H, canvas_w;
};

// Canvas pixel j as R | G << 8 | B << 16 | A << 24: the frame's inside its rectangle, zero outside.
__device__ __forceinline__ uint32_t ke_webpn_pixel(const KeWebpnSource &s, size_t j) {
    const int fx = (int)(j % (size_t)s.canvas_w) - s.x, fy = (int)(j / (size_t)s.canvas_w) - s.y;
    if (fx < 0 || fy < 0 || fx >= s.W || fy >= s.H) return 0u;
    const size_t k = (size_t)fy * s.W + fx;
    if (s.pix) {
        const uint32_t argb = s.pix[k];
        return ((argb >> 16) & 0xffu) | (argb & 0xff00ff00u) | ((argb & 0xffu) << 16);
    }
    uint8_t rgb[3];
    ke_webp_rgb_at(s.Y, s.U, s.V, s.d->h.mb_w, s.W, s.H, fx, fy, rgb);
    return (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16) | (ke_webpa_alpha_at(*s.a, s.files, s.scratch, k) << 24);
}

constexpr int kRowsPerBlock = 8;
constexpr int kCanvasThreads = 256;

// recs: the sub-batch's m images, the nf lossy ones first (imgs / planes / status_f / status_a by the same index), then the
// lossless ones (limgs / status_l by index - nf).
__global__ __launch_bounds__(kCanvasThreads) void ke_webpn_canvas_k(const KeWebpnDev *__restrict__ recs, const KeWebpDev *__restrict__ imgs,
                                                                   const KeWebpaDev *__restrict__ planes, const KeWebplDev *__restrict__ limgs, int64_t nf,
                                                                   const uint8_t *__restrict__ files, const uint8_t *__restrict__ scratch,
                                                                   const int32_t *__restrict__ status_f, const int32_t *__restrict__ status_a,
                                                                   const int32_t *__restrict__ status_l, uint8_t *__restrict__ out, int rows) {
    const int64_t i = blockIdx.x;
    const KeWebpnDev &c = recs[i];
    const int y0 = blockIdx.y * rows;
    if (y0 >= c.canvas_h) return;
    KeWebpnSource s;
    s.files = files; s.scratch = scratch;
    s.x = c.x; s.y = c.y; s.canvas_w = c.canvas_w;
    if (i < nf) {                                                   // a frame or a plane that failed leaves its canvas untouched
        if (status_f[i] != KE_WEBP_OK || status_a[i] != KE_WEBPL_OK) return;
        s.d = imgs + i; s.a = planes + i; s.pix = nullptr;
        s.W = s.d->h.width; s.H = s.d->h.height;
        const size_t nmb = (size_t)s.d->h.mb_w * s.d->h.mb_h;
        s.Y = ke_webp_frame_planes(*s.d, scratch); s.U = s.Y + nmb * 256; s.V = s.U + nmb * 64;
    } else {
        const KeWebplDev &l = limgs[i - nf];
        if (status_l[i - nf] != KE_WEBPL_OK) return;
        s.d = nullptr; s.a = nullptr; s.Y = s.U = s.V = nullptr;
        s.pix = (const uint32_t *)(scratch + l.scratch_off);         // the finished image lies at the front
        s.W = l.h.width; s.H = l.h.height;
    }
    const int y1 = min(y0 + rows, c.canvas_h), ch = c.channels;
    const size_t CW = (size_t)c.canvas_w, lo = (size_t)y0 * CW, hi = (size_t)y1 * CW;       // this tile's pixels
    uint8_t *o = out + c.out_off;
    const bool aligned = ((uintptr_t)o & 3) == 0;
    if (!aligned) {
        for (size_t j = lo + threadIdx.x; j < hi; j += kCanvasThreads) ke_webpn_store(ke_webpn_pixel(s, j), o + j * ch, ch);
    } else if (ch == 4) {
        for (size_t j = lo + threadIdx.x; j < hi; j += kCanvasThreads) *(uint32_t *)(o + j * 4) = ke_webpn_pixel(s, j);
    } else {
        // the dwords whose first byte lies in this tile's rows; the canvas's last bytes where they do not fill one
        const size_t total = CW * (size_t)c.canvas_h * 3;
        for (size_t q = (lo * 3 + 3) / 4 + threadIdx.x; q * 4 < hi * 3; q += kCanvasThreads) {
            const size_t b = q * 4, p0 = b / 3;
            const int r = (int)(b - p0 * 3);
            if (b + 4 <= total) {
                const uint64_t both = (uint64_t)(ke_webpn_pixel(s, p0) & 0xffffffu) | ((uint64_t)(ke_webpn_pixel(s, p0 + 1) & 0xffffffu) << 24);
                *(uint32_t *)(o + b) = (uint32_t)(both >> (8 * r));
            } else {
                for (size_t k = b; k < total; ++k) o[k] = (uint8_t)(ke_webpn_pixel(s, k / 3) >> (8 * (k % 3)));
            }
        }
    }
}

inline size_t ke_align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

KE_API int ke_webpn_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                          int32_t *heights, int32_t *channels, int32_t *status_out) {
    return ke_probe_each(files, offsets, sizes, n, widths, heights, channels, status_out,
                         [](const uint8_t *file, size_t size, int32_t &w, int32_t &h, int32_t &c, int32_t &st) {
                             KeWebpnHeader hd;                       // container, frame 0's tag / ALPH byte / stream header
                             ke_webpn_tag(file, size, hd);
                             w = hd.canvas_w; h = hd.canvas_h; c = hd.channels; st = hd.status;
                         });
}

KE_API int ke_webpn_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out) {
    // An EXIF chunk or an XMP packet may carry an orientation the reference's loader applies (flagged without reading it); an
    // RGBA canvas is composited over white by it.
    return ke_caveats_each(files, offsets, sizes, n, flags_out, [](const uint8_t *file, size_t size) {
        KeWebpnHeader h;
        ke_webpn_tag(file, size, h);
        return (h.meta ? KE_CAVEAT_ORIENTATION : 0) | (h.channels == 4 ? KE_CAVEAT_TRANSPARENCY : 0);
    });
}

KE_API int ke_webpn_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                           uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out) {
    KE_TRY(ke_decode_check_args(ctx, files, offsets, sizes, n, pixels_out, out_offsets, status_out, "the files' headers are parsed"));
    if (n == 0) return KE_OK;
    std::vector<KeWebpnHeader> items((size_t)n);                    // the headers are parsed on the host's threads
    ke_parallel_ranges(n, [&](int64_t a, int64_t b, int) {
        for (int64_t i = a; i < b; ++i) ke_parse_webpn(files + offsets[i], (size_t)sizes[i], items[(size_t)i]);
    });
    std::vector<int64_t> which;
    which.reserve((size_t)n);
    uint64_t lo = ~0ull, hi = 0;
    for (int64_t i = 0; i < n; ++i) {
        status_out[i] = items[(size_t)i].status;
        if (status_out[i] != KE_WEBPN_OK) continue;
        lo = std::min(lo, offsets[i]);
        hi = std::max(hi, offsets[i] + sizes[i]);
        which.push_back(i);
    }
    if (which.empty()) return KE_OK;
    // grouped per codec, the lossy frames first; lanes of one wave finish together at best, so neighbours in a group should have
    // streams of like length
    auto lossless = [&](int64_t i) { return items[(size_t)i].codec == KE_WEBPN_LOSSLESS; };
    auto stream = [&](int64_t i) { return lossless(i) ? items[(size_t)i].l.size : items[(size_t)i].a.f.vp8_size; };
    std::stable_sort(which.begin(), which.end(), [&](int64_t a, int64_t b) {
        return lossless(a) != lossless(b) ? lossless(b) : stream(a) > stream(b);
    });
    std::vector<KeWebpDev> devs;
    std::vector<KeWebpaDev> planes;
    std::vector<int32_t> order;
    std::vector<KeWebplDev> ldevs;
    std::vector<KeWebpnDev> recs;
    KeStreamGuard guard;                                           // after the host vectors it waits for
    void *d_files;
    KE_TRY(ke_upload_files(ctx, guard, files, lo, hi, KE_BUF_PIXELS, 256, &d_files));
    // sub-batches bounded by scratch, per codec what the still decoders' cost functions say; the canvas needs none
    uint64_t budget;                                                // KE_WEBP_SCRATCH_BYTES: a smaller one (tests: many sub-batches)
    KE_TRY(ke_scratch_budget(ctx, {KE_BUF_SSIM_IN}, (uint64_t)2 << 30, (uint64_t)160 << 30, "KE_WEBP_SCRATCH_BYTES", KE_BUDGET_ENV_LOWERS, &budget));
    uint64_t bytes = 0;
    int max_height = 0, max_filtered = 0;
    auto take = [&](size_t k, bool fresh) {
        if (fresh) {
            bytes = 0;
            max_height = max_filtered = 0;
            devs.clear(); planes.clear(); order.clear(); ldevs.clear(); recs.clear();
        }
        const int64_t i = which[k];
        const KeWebpnHeader &h = items[(size_t)i];
        const uint64_t frame = lossless(i) ? 0 : ke_webp_frame_scratch(h.a.f);
        const uint64_t rest = ((lossless(i) ? ke_vp8l_scratch_words(h.width, h.height) : ke_webpa_plane_words(h.a)) * 4 + 15) & ~15ull;
        if (!fresh && bytes + frame + rest > budget) return false;
        if (lossless(i)) {
            KeWebplDev d;
            d.h = h.l;
            d.file_off = offsets[i] - lo;
            d.scratch_off = bytes;
            d.scratch_words = ke_vp8l_scratch_words(h.width, h.height);
            d.out_off = out_offsets[i];
            ldevs.push_back(d);
        } else {
            KeWebpDev d;
            d.h = h.a.f;
            d.file_off = offsets[i] - lo;
            d.scratch_off = bytes;
            d.out_off = out_offsets[i];
            KeWebpaDev a;
            a.alph_off = d.file_off + h.a.alph_off;
            a.plane_off = bytes + frame;
            a.plane_words = ke_webpa_plane_words(h.a);
            a.out_off = out_offsets[i];
            a.alph_size = h.a.alph_size;
            a.method = h.a.method; a.filter = h.a.filter;
            a.width = h.width; a.height = h.height;
            if (h.a.method != KE_ALPH_OPAQUE && h.a.filter == KE_ALPH_FILTER_GRADIENT) max_filtered = std::max(max_filtered, h.height);
            if (h.a.method == KE_ALPH_VP8L) order.push_back((int32_t)devs.size());
            devs.push_back(d);
            planes.push_back(a);
        }
        bytes += frame + rest;
        max_height = std::max(max_height, h.canvas_h);
        recs.push_back(KeWebpnDev{out_offsets[i], h.canvas_w, h.canvas_h, h.channels, h.x, h.y});
        return true;
    };
    size_t nf = 0;                                                  // the lossy frames of the sub-batch under way
    auto launch = [&](size_t um, const int32_t **status, size_t *words) {
        nf = devs.size();
        const size_t nl = ldevs.size(), m1 = order.size();
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return planes[(size_t)a].alph_size > planes[(size_t)b].alph_size; });
        // one record buffer: [frames | planes | order | lossless images | canvases]; one status buffer: [frames | planes | images]
        const size_t at_planes = ke_align16(nf * sizeof(KeWebpDev)), at_order = at_planes + ke_align16(nf * sizeof(KeWebpaDev));
        const size_t at_images = at_order + ke_align16(nf * 4), at_recs = at_images + ke_align16(nl * sizeof(KeWebplDev));
        void *d_meta, *d_scratch, *d_status, *d_plans;
        KE_TRY(ke_reserve(ctx, KE_BUF_META, at_recs + um * sizeof(KeWebpnDev) + 16, &d_meta));
        KE_TRY(ke_reserve(ctx, KE_BUF_SSIM_IN, (size_t)bytes + 64, &d_scratch));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT0, (2 * nf + nl) * 4 + 16, &d_status));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT1, (nf + nl) * sizeof(KeVp8lPlan) + 16, &d_plans));
        uint8_t *meta = (uint8_t *)d_meta;
        const KeWebpDev *d_imgs = (const KeWebpDev *)meta;
        const KeWebpaDev *d_planes = (const KeWebpaDev *)(meta + at_planes);
        const int32_t *d_order = (const int32_t *)(meta + at_order);
        const KeWebplDev *d_limgs = (const KeWebplDev *)(meta + at_images);
        const KeWebpnDev *d_recs = (const KeWebpnDev *)(meta + at_recs);
        int32_t *d_status_f = (int32_t *)d_status, *d_status_a = d_status_f + nf, *d_status_l = d_status_a + nf;
        KeVp8lPlan *d_plans_a = (KeVp8lPlan *)d_plans, *d_plans_l = d_plans_a + nf;
        if (nf) {
            KE_HIP(ctx, hipMemcpyAsync(meta, devs.data(), nf * sizeof(KeWebpDev), hipMemcpyHostToDevice, ctx->stream));
            KE_HIP(ctx, hipMemcpyAsync(meta + at_planes, planes.data(), nf * sizeof(KeWebpaDev), hipMemcpyHostToDevice, ctx->stream));
            if (m1) KE_HIP(ctx, hipMemcpyAsync(meta + at_order, order.data(), m1 * 4, hipMemcpyHostToDevice, ctx->stream));
            KE_HIP(ctx, hipMemsetAsync(d_status_a, 0, nf * 4, ctx->stream));         // planes without a stream have nothing to fail
            KE_TRY(ke_webp_launch_frames(ctx, d_imgs, (int64_t)nf, (const uint8_t *)d_files, (uint8_t *)d_scratch, d_status_f));
            KE_TRY(ke_webpa_launch_planes(ctx, d_planes, d_order, (int64_t)nf, (int64_t)m1, max_filtered, (const uint8_t *)d_files, (uint8_t *)d_scratch,
                                          d_plans_a, (const int32_t *)d_status_f, d_status_a));
        }
        if (nl) {
            KE_HIP(ctx, hipMemcpyAsync(meta + at_images, ldevs.data(), nl * sizeof(KeWebplDev), hipMemcpyHostToDevice, ctx->stream));
            KE_TRY(ke_webpl_launch_images(ctx, d_limgs, (int64_t)nl, (const uint8_t *)d_files, (uint8_t *)d_scratch, d_plans_l, d_status_l));
        }
        KE_HIP(ctx, hipMemcpyAsync(meta + at_recs, recs.data(), um * sizeof(KeWebpnDev), hipMemcpyHostToDevice, ctx->stream));
        const KeRowTiles tiles = ke_row_tiles(max_height, kRowsPerBlock);
        hipLaunchKernelGGL(ke_webpn_canvas_k, dim3((unsigned)um, tiles.grid_y), dim3(kCanvasThreads), 0, ctx->stream, d_recs, d_imgs, d_planes, d_limgs,
                           (int64_t)nf, (const uint8_t *)d_files, (const uint8_t *)d_scratch, (const int32_t *)d_status_f, (const int32_t *)d_status_a,
                           (const int32_t *)d_status_l, pixels_out, tiles.rows);
        *status = d_status_f;
        *words = 2 * nf + nl;
        return (int)KE_OK;
    };
    // a frame that failed keeps its status; otherwise the plane's decides; a lossless image has the one
    KE_TRY(ke_decode_sub_batches(ctx, which.size(), take, launch, [&](size_t at, size_t k, size_t, const int32_t *st) {
        status_out[which[at]] = k >= nf ? st[nf + k] : st[k] != KE_WEBP_OK ? st[k] : st[nf + k];
    }));
    guard.disarm();
    return KE_OK;
}
