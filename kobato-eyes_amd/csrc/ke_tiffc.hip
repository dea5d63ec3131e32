// ke_tiffc.hip -- LZW and PackBits TIFF files decoded on the GPU: the decode step in front of the hash path for the
// compressed files of the fifth format the reference ranks as a keeper (src/dup/scanner.py:16-28).  Replaces `Image.open(path)` +
// pixel access of the reference's batch hasher (src/core/fastsig.py:31-34) for the files ke_tiffc_parse.h takes -- those Pillow
// hands to libtiff; the pixels that leave are ke_tiff_decode's for the same image stored uncompressed.  The arithmetic is
// ke_tiffc_core.h's (held against Pillow on the CPU).  The scheme is ke_gif.hip's, with one difference that matters: every
// strip of a TIFF file is a stream of its own (libtiff writes strips of at most 64 KB: a 512 x 512 RGB file has 13), so the
// sequential walk is as long as a strip, not as a file, and there are strips-per-file times as many lanes.
//
//   ke_tiffc_codes   ONE LANE PER STRIP walks the LZW codes or the PackBits headers.  A literal goes to its place in the strip's
//                    plane (its bytes before the predictor); a string or a run lies in the output already and is recorded as
//                    a copy (ke_lz_copies.h), not made: a lane that waited for its own stores would stall the other 63.  The
//                    strip's bytes come through a 16-byte register window refilled one step ahead.  The LZW dictionary (4 096
//                    x {where, how long}) is a slice of HBM per RESIDENT lane, not per strip: the waves take groups of 64
//                    strips off a list (one atomic per group) until it is empty.  The list is sorted by compression and
//                    compressed length, longest first, so the lanes of a wave walk strips of like length and the long
//                    groups start first.
//   ke_tiffc_copies  ONE WAVE PER STRIP makes the recorded copies, 64 per round (ke_lz_copies.h, the PNG path's).
//   ke_tiffc_rows    one wave per row: undoes predictor 2 (a prefix sum per sample modulo 256 over the lanes, 64 pixels a step,
//                    the carry handed on), then ke_tiff_unpack's mapping -- WhiteIsZero and palette files through the table, an
//                    unspecified fourth sample dropped -- into the caller's pixels.  Bytes in + bytes out, each once.
#include <algorithm>
#include <vector>

#include "ke_decode_batch.h"

#include "ke_lz_copies.h"
#include "ke_lz_records.h"
#include "ke_lz_window.h"
#include "ke_tiffc_parse.h"
#include "ke_tiffc_rows.h"

namespace {

struct KeTiffcStripDev {
    uint64_t file_off;     // the strip's bytes inside the uploaded bytes
    uint64_t plane_off;    // its plane inside the scratch
    uint64_t rec_off;      // its copy records (8 bytes each)
    uint32_t bytes, want;  // compressed bytes; bytes the strip yields
    uint32_t img, comp;
};

constexpr uint32_t kMaxWaves = 2048;              // resident lanes: 131 072 dictionaries of 32 KB = 4 GB at most

__global__ __launch_bounds__(64) void ke_tiffc_codes(const KeTiffcStripDev *__restrict__ strips, uint32_t n, const uint8_t *__restrict__ files,
                                                   uint8_t *__restrict__ planes, uint2 *__restrict__ records, uint2 *__restrict__ dicts,
                                                   int32_t *__restrict__ status, uint32_t *__restrict__ nrec, uint32_t *__restrict__ next_group) {
    HbmDict dict{dicts + ((size_t)blockIdx.x * 64 + threadIdx.x) * 4096};
    for (;;) {
        uint32_t g = 0;
        if (threadIdx.x == 0) g = atomicAdd(next_group, 1u);
        g = (uint32_t)__shfl((int)g, 0);
        if ((uint64_t)g * 64 >= n) break;
        const uint32_t s = g * 64 + threadIdx.x;
        if (s < n) {
            const KeTiffcStripDev &d = strips[s];
            WindowSrc src;
            src.file = files + d.file_off;
            src.limit = d.bytes;
            src.start(0);
            KeLzRecSink sink{planes + d.plane_off, records + d.rec_off, 0, 0};
            const int st = d.comp == KE_TIFFC_LZW ? ke_tiffc_lzw(src, 0u, d.bytes, d.want, dict, sink) : ke_tiffc_packbits(src, 0u, d.bytes, d.want, sink);
            if (st != KE_TIFFC_OK) status[d.img] = st;             // any strip's failure is the image's (the same value or another: not 0)
            nrec[s] = sink.nrec;
        }
    }
}

__global__ __launch_bounds__(64) void ke_tiffc_copies(const KeTiffcStripDev *__restrict__ strips, uint8_t *__restrict__ planes,
                                                    const uint2 *__restrict__ records, const int32_t *__restrict__ status,
                                                    const uint32_t *__restrict__ nrec) {
    const KeTiffcStripDev &d = strips[blockIdx.x];
    if (status[d.img] != KE_TIFFC_OK) return;
    ke_lz_make_copies(planes + d.plane_off, records + d.rec_off, nrec[blockIdx.x], 2u);
}

}  // namespace

KE_API int ke_tiffc_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                          int32_t *heights, int32_t *channels, int32_t *status_out) {
    return ke_probe_each(files, offsets, sizes, n, widths, heights, channels, status_out,
                         [](const uint8_t *file, size_t size, int32_t &w, int32_t &h, int32_t &c, int32_t &st) {
                             KeTiffcInfo info;
                             ke_parse_tiffc(file, size, nullptr, info);
                             w = info.t.width; h = info.t.height; c = info.t.channels; st = info.t.status;
                         });
}

KE_API int ke_tiffc_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out) {
    // files that carry an orientation (the tag, an EXIF directory, an XMP packet) are refused by the parser: Pillow turns them
    return ke_caveats_none(files, offsets, sizes, n, flags_out);
}

KE_API int ke_tiffc_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                           uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out) {
    KE_TRY(ke_decode_check_args(ctx, files, offsets, sizes, n, pixels_out, out_offsets, status_out, "the files' directories are parsed"));
    if (n == 0) return KE_OK;
    std::vector<KeTiffcInfo> infos((size_t)n);                   // the directories are read on the host's threads
    std::vector<std::vector<KeTiffcStrip>> found((size_t)n);
    ke_parallel_ranges(n, [&](int64_t a, int64_t b, int) {
        for (int64_t i = a; i < b; ++i) ke_parse_tiffc(files + offsets[i], (size_t)sizes[i], &found[(size_t)i], infos[(size_t)i]);
    });
    std::vector<int64_t> which;
    uint64_t lo = ~0ull, hi = 0;
    for (int64_t i = 0; i < n; ++i) {
        status_out[i] = infos[(size_t)i].t.status;
        if (status_out[i] != KE_TIFF_OK) continue;
        which.push_back(i);
        lo = std::min(lo, offsets[i]);
        hi = std::max(hi, offsets[i] + sizes[i]);
    }
    if (which.empty()) return KE_OK;
    std::vector<KeTiffcImgDev> imgs;
    std::vector<KeTiffcStripDev> strips;
    KeStreamGuard guard;                                           // after the host vectors it waits for
    void *d_files;
    KE_TRY(ke_upload_files(ctx, guard, files, lo, hi, KE_BUF_PIXELS, 256, &d_files));
    // sub-batches bounded by scratch: the strips' planes (1 B per sample) + their copy records (8 B each) + 32 KB of dictionary
    // per resident lane when the sub-batch has LZW strips
    uint64_t budget;
    KE_TRY(ke_scratch_budget(ctx, {KE_BUF_TMP, KE_BUF_SSIM_AUX, KE_BUF_SSIM_IN}, (uint64_t)1 << 30, (uint64_t)32 << 30, "KE_TIFFC_SCRATCH_BYTES",
                             KE_BUDGET_ENV_REPLACES, &budget));
    auto dict_bytes = [](uint64_t strips_so_far, bool lzw) {
        return lzw ? std::min<uint64_t>((strips_so_far + 63) / 64, kMaxWaves) * 64 * 32768 : (uint64_t)64;
    };
    uint64_t plane_bytes = 0, nrecs = 0;
    int max_height = 0;
    bool any_lzw = false;
    auto take = [&](size_t k, bool fresh) {
        if (fresh) {
            plane_bytes = nrecs = 0;
            max_height = 0;
            any_lzw = false;
            imgs.clear();
            strips.clear();
        }
        const int64_t i = which[k];
        const KeTiffcInfo &info = infos[(size_t)i];
        const KeTiffInfo &t = info.t;
        const uint64_t row = (uint64_t)t.width * t.spp;
        const uint64_t stride = (row * t.rows_per_strip + 2 + 15) & ~15ull;
        uint64_t pb = stride * t.nstrips, rc = 0;
        for (int s = 0; s < t.nstrips; ++s) {
            const uint64_t want = row * std::min(t.rows_per_strip, t.height - s * t.rows_per_strip);
            // a record per string or run -- at most one per compressed byte -- and per further 513 bytes of a long one;
            // never more than one per 2 bytes the strip yields
            rc += std::min<uint64_t>(want / 2 + 2, (uint64_t)found[(size_t)i][(size_t)s].bytes + want / 512 + 2);
        }
        const bool lzw = any_lzw || info.compression == KE_TIFFC_LZW;
        if (!fresh && plane_bytes + pb + (nrecs + rc) * 8 + dict_bytes(strips.size() + (size_t)t.nstrips, lzw) > budget) return false;
        KeTiffcImgDev d;
        d.out_off = out_offsets[i];
        d.plane_off = plane_bytes;
        d.strip_stride = (uint32_t)stride;
        d.width = t.width; d.height = t.height; d.spp = t.spp; d.channels = t.channels; d.mapped = t.mapped;
        d.rows_per_strip = t.rows_per_strip; d.predictor = info.predictor;
        std::memcpy(d.lut, t.lut, 256);
        for (int s = 0; s < t.nstrips; ++s) {
            const KeTiffcStrip &f = found[(size_t)i][(size_t)s];
            KeTiffcStripDev sd;
            sd.file_off = offsets[i] - lo + f.off;
            sd.plane_off = plane_bytes + stride * (uint64_t)s;
            sd.rec_off = nrecs;
            sd.bytes = f.bytes;
            sd.want = (uint32_t)(row * std::min(t.rows_per_strip, t.height - s * t.rows_per_strip));
            sd.img = (uint32_t)imgs.size();
            sd.comp = (uint32_t)info.compression;
            nrecs += std::min<uint64_t>((uint64_t)sd.want / 2 + 2, (uint64_t)f.bytes + sd.want / 512 + 2);
            strips.push_back(sd);
        }
        any_lzw = lzw;
        plane_bytes += pb;
        max_height = std::max(max_height, t.height);
        imgs.push_back(d);
        return true;
    };
    auto launch = [&](size_t m, const int32_t **status, size_t *words) {
        // lanes of one wave finish together at best: neighbours in the list are strips of one compression and of like length,
        // and the longest walks start first
        std::stable_sort(strips.begin(), strips.end(), [](const KeTiffcStripDev &a, const KeTiffcStripDev &b) {
            return a.comp != b.comp ? a.comp < b.comp : a.bytes > b.bytes;
        });
        const size_t ns = strips.size();
        const uint32_t waves = (uint32_t)std::min<uint64_t>((ns + 63) / 64, kMaxWaves);
        void *d_imgs, *d_strips, *d_planes, *d_rec, *d_dict, *d_status, *d_nrec;
        KE_TRY(ke_reserve(ctx, KE_BUF_META, m * sizeof(KeTiffcImgDev), &d_imgs));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT1, ns * sizeof(KeTiffcStripDev), &d_strips));
        KE_TRY(ke_reserve(ctx, KE_BUF_TMP, (size_t)plane_bytes + 128, &d_planes));
        KE_TRY(ke_reserve(ctx, KE_BUF_SSIM_AUX, (size_t)nrecs * 8 + 8, &d_rec));
        KE_TRY(ke_reserve(ctx, KE_BUF_SSIM_IN, (size_t)dict_bytes(ns, any_lzw), &d_dict));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT0, (m + 1) * 4, &d_status));                  // the statuses, then the list's counter
        KE_TRY(ke_reserve(ctx, KE_BUF_TILE32, ns * 4, &d_nrec));
        KE_HIP(ctx, hipMemcpyAsync(d_imgs, imgs.data(), m * sizeof(KeTiffcImgDev), hipMemcpyHostToDevice, ctx->stream));
        KE_HIP(ctx, hipMemcpyAsync(d_strips, strips.data(), ns * sizeof(KeTiffcStripDev), hipMemcpyHostToDevice, ctx->stream));
        KE_HIP(ctx, hipMemsetAsync(d_status, 0, (m + 1) * 4, ctx->stream));
        hipLaunchKernelGGL(ke_tiffc_codes, dim3(waves), dim3(64), 0, ctx->stream, (const KeTiffcStripDev *)d_strips, (uint32_t)ns, (const uint8_t *)d_files,
                           (uint8_t *)d_planes, (uint2 *)d_rec, (uint2 *)d_dict, (int32_t *)d_status, (uint32_t *)d_nrec, (uint32_t *)d_status + m);
        hipLaunchKernelGGL(ke_tiffc_copies, dim3((unsigned)ns), dim3(64), 0, ctx->stream, (const KeTiffcStripDev *)d_strips, (uint8_t *)d_planes,
                           (const uint2 *)d_rec, (const int32_t *)d_status, (const uint32_t *)d_nrec);
        const KeRowTiles tiles = ke_row_tiles(max_height, kRowsPerBlock);
        hipLaunchKernelGGL(ke_tiffc_rows, dim3((unsigned)m, tiles.grid_y), dim3(256), 0, ctx->stream,
                           (const KeTiffcImgDev *)d_imgs, (const uint8_t *)d_planes, (const int32_t *)d_status, pixels_out, tiles.rows);
        *status = (const int32_t *)d_status;
        *words = m;
        return (int)KE_OK;
    };
    KE_TRY(ke_decode_sub_batches(ctx, which.size(), take, launch,
                                 [&](size_t at, size_t k, size_t, const int32_t *st) { status_out[which[at]] = st[k]; }));
    guard.disarm();
    return KE_OK;
}
