// ke_tiffz.hip -- deflate-compressed TIFF files decoded on the GPU: the decode step in front of the hash path for the
// "ZIP" files of the fifth format the reference ranks as a keeper (src/dup/scanner.py:16-28).  Replaces `Image.open(path)` +
// pixel access of the reference's batch hasher (src/core/fastsig.py:31-34) for the files ke_tiffz_parse.h takes -- Compression
// 8 and 32946, which Pillow hands to libtiff; the pixels that leave are ke_tiff_decode's for the same image stored
// uncompressed.  No arithmetic of its own but the Adler sum (ke_tiffz_core.h): the inflate is the PNG path's (ke_png_core.h,
// its lane policies in ke_inflate_lanes.h), the scheme ke_tiffc.hip's.  Every strip of a TIFF file is a zlib stream of its own
// (libtiff writes strips of at most 64 KB: a 512 x 512 RGB file has 13), so where a PNG call lasts as long as its longest
// image's stream, the walk here is as long as a strip and there are strips-per-file times as many lanes.
//
//   ke_png_gather     every strip's bytes -> a 16-byte aligned stream of its own in a staging area (strips start at any byte of
//                     a file; LdsStream reads whole aligned 16-byte chunks and nothing beyond the chunk that holds the last byte)
//   ke_tiffz_inflate  ONE LANE PER STRIP runs ke_inflate_zlib with limit = the bytes of the strip's rows.  Literals go to their
//                     place in the strip's plane, a match is recorded (ke_lz_copies.h, length bias 3).  The waves take groups
//                     of 64 strips off a list (one atomic per group) until it is empty; the list is sorted by compressed
//                     length, longest first.  LDS per wave: 26 880 bytes, as ke_png_inflate.
//   ke_tiffz_copies   ONE WAVE PER STRIP makes the recorded copies, then -- the same wave -- sums the Adler-32 of the plane as it
//                     is before the predictor and holds it against the stream's trailer: a mismatch is the image's status 2.
//   ke_tiffc_rows     (ke_tiffc_rows.h) predictor 2 undone, samples mapped, into the caller's pixels.
#include <algorithm>
#include <vector>

#include "ke_decode_batch.h"

#include "ke_inflate_lanes.h"
#include "ke_lz_copies.h"
#include "ke_png_core.h"
#include "ke_tiffc_rows.h"
#include "ke_tiffz_parse.h"

namespace {

struct KeTiffzStripDev {
    uint64_t z_off;        // the strip's zlib stream inside the staging area (16-byte aligned)
    uint64_t plane_off;    // its plane inside the scratch (16-byte aligned, at least 3 bytes of slack behind `want`)
    uint64_t rec_off;      // its copy records (8 bytes each)
    uint32_t bytes, want;  // compressed bytes; bytes the strip yields
    uint32_t img, max_rec; // its image in the sub-batch; the records it has room for
};

constexpr uint32_t kMaxWaves = 4096;              // resident waves: more than the chip holds at 26 880 B of LDS each (not measured against fewer)
constexpr int kWorkBytes = 160;                   // per resident lane in HBM: the code lengths of the block header being read
constexpr uint32_t kPieceBytes = 1u << 18;        // a strip longer than this is gathered by several workgroups
// Streams that wait with a match before the wave turns to the matches (RecSink::matches_now): ke_png_decode's default, measured
// there on whole images, not here on strips (which are shorter and far more alike).  64 lanes per wave always: the list hands
// out groups of 64.
constexpr int kHold = 6;

// RecSink with the strip's share of the records as a bound.  A stream has at most one match per 2 of its bits, so a strip's
// records are sized from its compressed length where that is less than one per 3 bytes it yields -- but ke_inflate_zlib looks at
// the stream's end between blocks only.  Past the end the ring hands out what is left of the stream's last 16-byte chunk -- up
// to 15 stale bytes of whatever the staging area held before: the gather writes the strip's bytes and nothing else -- and then
// zeros; either can decode as matches.  No result depends on those bytes: a walk that has used a bit beyond the end is refused
// at the next look between blocks or at the trailer, literals stop at `limit`, and its matches beyond the bound are counted,
// not written down.
struct BoundedRecSink : RecSink {
    uint32_t max_rec;
    __device__ __forceinline__ void copy(uint32_t dist, uint32_t len) {
        if (nrec < max_rec) { RecSink::copy(dist, len); return; }
        settle();
        n += len;
        ++nrec;
    }
};

__global__ __launch_bounds__(64) void ke_tiffz_inflate(const KeTiffzStripDev *__restrict__ strips, uint32_t n, const uint8_t *__restrict__ streams,
                                                     uint8_t *__restrict__ planes, uint8_t *__restrict__ work, uint2 *__restrict__ records,
                                                     int32_t *__restrict__ status, uint32_t *__restrict__ adler, uint32_t *__restrict__ nrec,
                                                     uint32_t *__restrict__ next_group) {
    __shared__ uint8_t s_lsym[288 * 64], s_dsym[32 * 64];
    __shared__ uint32_t s_lhigh[9 * 64], s_win[16 * 64];
    for (;;) {
        uint32_t g = 0;
        if (threadIdx.x == 0) g = atomicAdd(next_group, 1u);
        g = (uint32_t)__shfl((int)g, 0);
        if ((uint64_t)g * 64 >= n) break;
        const uint32_t s = g * 64 + threadIdx.x;
        if (s < n) {
            const KeTiffzStripDev &d = strips[s];
            LdsStream src;
            src.z = reinterpret_cast<const u32x4 *>(streams + d.z_off);
            src.win = s_win + threadIdx.x;
            src.nchunk = (d.bytes + 15u) >> 4;
            src.avail = src.req = src.t = 0;
            KeBitsLsb<LdsStream> bits{&src, 0, 0, 0};
            BoundedRecSink sink{{planes + d.plane_off, 0, 0, records + d.rec_off, 0, kHold}, d.max_rec};
            LaneTab tab;
            tab.lsym_ = s_lsym + threadIdx.x;
            tab.lhigh_ = s_lhigh + threadIdx.x;
            tab.dsym_ = s_dsym + threadIdx.x;
            tab.nib_ = reinterpret_cast<uint32_t *>(work + ((size_t)blockIdx.x * 64 + threadIdx.x) * kWorkBytes);
            tab.lim0 = tab.lim1 = tab.base0 = tab.base1 = Oct{0, 0, 0, 0, 0, 0, 0, 0};
            uint32_t trailer = 0;
            int rc = ke_inflate_zlib(bits, sink, d.bytes, d.want, tab, &trailer);
            if (rc == KE_PNG_OK && (sink.n != d.want || sink.nrec > d.max_rec)) rc = KE_PNG_CORRUPT;
            if (rc != KE_PNG_OK) status[d.img] = rc;               // any strip's failure is the image's (the same value or another: not 0)
            adler[s] = trailer;
            nrec[s] = sink.nrec;
        }
    }
}

__global__ __launch_bounds__(64) void ke_tiffz_copies(const KeTiffzStripDev *__restrict__ strips, uint8_t *__restrict__ planes,
                                                    const uint2 *__restrict__ records, int32_t *__restrict__ status,
                                                    const uint32_t *__restrict__ adler, const uint32_t *__restrict__ nrec) {
    const KeTiffzStripDev &d = strips[blockIdx.x];
    if (status[d.img] != KE_TIFF_OK) return;                       // (the whole wave: the status is read once per workgroup)
    uint8_t *plane = planes + d.plane_off;
    ke_lz_make_copies(plane, records + d.rec_off, nrec[blockIdx.x], 3u);      // a deflate match is at least 3 bytes long
    __syncthreads();                                               // the copies' stores have landed before the plane is read back
    const KeTiffzAdlerLane mine = ke_tiffz_adler_lane(plane, d.want, threadIdx.x);
    uint32_t s1 = mine.s1, s2 = mine.s2;
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        s1 += (uint32_t)__shfl_xor((int)s1, sh);
        s2 += (uint32_t)__shfl_xor((int)s2, sh);
    }
    if (threadIdx.x == 0 && ke_tiffz_adler_join(d.want, s1, s2) != adler[blockIdx.x]) status[d.img] = KE_TIFF_CORRUPT;
}

}  // namespace

KE_API int ke_tiffz_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                          int32_t *heights, int32_t *channels, int32_t *status_out) {
    return ke_probe_each(files, offsets, sizes, n, widths, heights, channels, status_out,
                         [](const uint8_t *file, size_t size, int32_t &w, int32_t &h, int32_t &c, int32_t &st) {
                             KeTiffcInfo info;
                             ke_parse_tiffz(file, size, nullptr, info);
                             w = info.t.width; h = info.t.height; c = info.t.channels; st = info.t.status;
                         });
}

KE_API int ke_tiffz_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out) {
    // files that carry an orientation (the tag, an EXIF directory, an XMP packet) are refused by the parser: Pillow turns them
    return ke_caveats_none(files, offsets, sizes, n, flags_out);
}

KE_API int ke_tiffz_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                           uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out) {
    KE_TRY(ke_decode_check_args(ctx, files, offsets, sizes, n, pixels_out, out_offsets, status_out, "the files' directories are parsed"));
    if (n == 0) return KE_OK;
    std::vector<KeTiffcInfo> infos((size_t)n);                   // the directories are read on the host's threads
    std::vector<std::vector<KeTiffcStrip>> found((size_t)n);
    ke_parallel_ranges(n, [&](int64_t a, int64_t b, int) {
        for (int64_t i = a; i < b; ++i) ke_parse_tiffz(files + offsets[i], (size_t)sizes[i], &found[(size_t)i], infos[(size_t)i]);
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
    std::vector<KeTiffzStripDev> strips;
    std::vector<KePngPiece> pieces;
    KeStreamGuard guard;                                           // after the host vectors it waits for
    void *d_files;
    KE_TRY(ke_upload_files(ctx, guard, files, lo, hi, KE_BUF_PIXELS, 256, &d_files));
    // sub-batches bounded by scratch: the strips' planes (1 B per sample) + their copy records (8 B each) + the staged streams +
    // 160 B of header work per resident lane
    uint64_t budget;
    KE_TRY(ke_scratch_budget(ctx, {KE_BUF_TMP, KE_BUF_SSIM_AUX, KE_BUF_SSIM_IN}, (uint64_t)1 << 30, (uint64_t)32 << 30, "KE_TIFFZ_SCRATCH_BYTES",
                             KE_BUDGET_ENV_REPLACES, &budget));
    auto work_bytes = [](uint64_t strips_so_far) { return std::min<uint64_t>((strips_so_far + 63) / 64, kMaxWaves) * 64 * kWorkBytes; };
    // a match per 3 bytes the strip yields at most, and none shorter in the stream than 2 bits: whichever is less
    auto records_of = [](uint64_t want, uint64_t bytes) { return std::min<uint64_t>(want / 3 + 2, bytes * 4 + 2); };
    uint64_t plane_bytes = 0, nrecs = 0, zbytes = 0;
    int max_height = 0;
    auto take = [&](size_t k, bool fresh) {
        if (fresh) {
            plane_bytes = nrecs = zbytes = 0;
            max_height = 0;
            imgs.clear();
            strips.clear();
            pieces.clear();
        }
        const int64_t i = which[k];
        const KeTiffcInfo &info = infos[(size_t)i];
        const KeTiffInfo &t = info.t;
        const uint64_t row = (uint64_t)t.width * t.spp;
        // RecSink writes whole dwords: a plane starts 4-byte aligned and has 3 bytes of slack; 16: the Adler sum's chunks
        const uint64_t stride = (row * t.rows_per_strip + 3 + 15) & ~15ull;
        uint64_t pb = stride * t.nstrips, rc = 0, zb = 0;
        for (int s = 0; s < t.nstrips; ++s) {
            const uint64_t want = row * std::min(t.rows_per_strip, t.height - s * t.rows_per_strip);
            rc += records_of(want, found[(size_t)i][(size_t)s].bytes);
            zb += ((uint64_t)found[(size_t)i][(size_t)s].bytes + 15) & ~15ull;
        }
        if (!fresh && plane_bytes + pb + (nrecs + rc) * 8 + zbytes + zb + work_bytes(strips.size() + (size_t)t.nstrips) > budget) return false;
        KeTiffcImgDev d;
        d.out_off = out_offsets[i];
        d.plane_off = plane_bytes;
        d.strip_stride = (uint32_t)stride;
        d.width = t.width; d.height = t.height; d.spp = t.spp; d.channels = t.channels; d.mapped = t.mapped;
        d.rows_per_strip = t.rows_per_strip; d.predictor = info.predictor;
        std::memcpy(d.lut, t.lut, 256);
        for (int s = 0; s < t.nstrips; ++s) {
            const KeTiffcStrip &f = found[(size_t)i][(size_t)s];
            KeTiffzStripDev sd;
            sd.z_off = zbytes;
            sd.plane_off = plane_bytes + stride * (uint64_t)s;
            sd.rec_off = nrecs;
            sd.bytes = f.bytes;
            sd.want = (uint32_t)(row * std::min(t.rows_per_strip, t.height - s * t.rows_per_strip));
            sd.img = (uint32_t)imgs.size();
            sd.max_rec = (uint32_t)records_of(sd.want, f.bytes);
            for (uint32_t o = 0; o < f.bytes; o += kPieceBytes)
                pieces.push_back(KePngPiece{offsets[i] - lo + f.off + o, zbytes + o, std::min(kPieceBytes, f.bytes - o), 0});
            nrecs += records_of(sd.want, f.bytes);
            zbytes += ((uint64_t)f.bytes + 15) & ~15ull;
            strips.push_back(sd);
        }
        plane_bytes += pb;
        max_height = std::max(max_height, t.height);
        imgs.push_back(d);
        return true;
    };
    auto launch = [&](size_t m, const int32_t **status, size_t *words) {
        // lanes of one wave finish together at best: neighbours in the list are strips of like length, the longest walks start first
        std::stable_sort(strips.begin(), strips.end(), [](const KeTiffzStripDev &a, const KeTiffzStripDev &b) { return a.bytes > b.bytes; });
        const size_t ns = strips.size();
        const uint32_t waves = (uint32_t)std::min<uint64_t>((ns + 63) / 64, kMaxWaves);
        void *d_imgs, *d_strips, *d_pieces, *d_streams, *d_planes, *d_rec, *d_work, *d_status, *d_words;
        KE_TRY(ke_reserve(ctx, KE_BUF_META, m * sizeof(KeTiffcImgDev), &d_imgs));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT1, ns * sizeof(KeTiffzStripDev), &d_strips));
        KE_TRY(ke_reserve(ctx, KE_BUF_JPEG_TABLES, pieces.size() * sizeof(KePngPiece), &d_pieces));
        KE_TRY(ke_reserve(ctx, KE_BUF_SSIM_IN, (size_t)zbytes + 16, &d_streams));
        KE_TRY(ke_reserve(ctx, KE_BUF_TMP, (size_t)plane_bytes + 128, &d_planes));
        KE_TRY(ke_reserve(ctx, KE_BUF_SSIM_AUX, (size_t)nrecs * 8 + 8, &d_rec));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT2, (size_t)work_bytes(ns), &d_work));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT0, (m + 1) * 4, &d_status));                  // the statuses, then the list's counter
        KE_TRY(ke_reserve(ctx, KE_BUF_TILE32, ns * 8, &d_words));                      // per strip: the trailer, then the record count
        uint32_t *d_adler = (uint32_t *)d_words, *d_nrec = (uint32_t *)d_words + ns;
        KE_HIP(ctx, hipMemcpyAsync(d_imgs, imgs.data(), m * sizeof(KeTiffcImgDev), hipMemcpyHostToDevice, ctx->stream));
        KE_HIP(ctx, hipMemcpyAsync(d_strips, strips.data(), ns * sizeof(KeTiffzStripDev), hipMemcpyHostToDevice, ctx->stream));
        KE_HIP(ctx, hipMemcpyAsync(d_pieces, pieces.data(), pieces.size() * sizeof(KePngPiece), hipMemcpyHostToDevice, ctx->stream));
        KE_HIP(ctx, hipMemsetAsync(d_status, 0, (m + 1) * 4, ctx->stream));
        hipLaunchKernelGGL(ke_png_gather, dim3((unsigned)pieces.size()), dim3(256), 0, ctx->stream, (const KePngPiece *)d_pieces,
                           (const uint8_t *)d_files, (uint8_t *)d_streams);
        hipLaunchKernelGGL(ke_tiffz_inflate, dim3(waves), dim3(64), 0, ctx->stream, (const KeTiffzStripDev *)d_strips, (uint32_t)ns,
                           (const uint8_t *)d_streams, (uint8_t *)d_planes, (uint8_t *)d_work, (uint2 *)d_rec, (int32_t *)d_status, d_adler, d_nrec,
                           (uint32_t *)d_status + m);
        hipLaunchKernelGGL(ke_tiffz_copies, dim3((unsigned)ns), dim3(64), 0, ctx->stream, (const KeTiffzStripDev *)d_strips, (uint8_t *)d_planes,
                           (const uint2 *)d_rec, (int32_t *)d_status, (const uint32_t *)d_adler, (const uint32_t *)d_nrec);
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
