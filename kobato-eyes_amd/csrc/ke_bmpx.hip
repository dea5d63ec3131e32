// ke_bmpx.hip -- RLE, 1 / 4-bit and 16-bit BMP files decoded on the GPU: the decode step in front of the hash path for
// the files of the third format the reference ranks as a keeper (src/dup/scanner.py:16-28) that ke_bmp.hip leaves out.  Replaces
// `Image.open(path)` + pixel access of the reference's batch hasher (src/core/fastsig.py:31-34) for the files ke_bmpx_parse.h
// takes -- for RLE files a Python loop in Pillow (BmpRleDecoder: two read(1) per code).  The arithmetic is ke_bmpx_core.h's (held
// against Pillow on the CPU).  The files travel to the device as they are; a palette file leaves as the luma the reference's
// hashes see (src/sig/phash.py:25), a 16-bit file as RGB.
//
//   ke_bmpx_unpack  blockIdx.x = image, blockIdx.y = a band of rows, in the manner of ke_bmp_unpack.  1-bit and 4-bit rows: a
//                   thread takes eight pixels (one / four stored bytes) through the table; 16-bit rows: four pixels (8 bytes in,
//                   12 out).  HBM-bound: bytes in + bytes out, each once.  An RLE file's band is cleared to the luma of index 0
//                   -- what end-of-line padding and deltas leave behind -- with 16-byte stores.
//   ke_bmpx_codes   ONE LANE PER RLE FILE walks the codes (ke_bmpx_walk) through ke_tiffc_codes' reader, a 16-byte register window
//                   refilled one step ahead and restarted where a literal's bytes are stepped over.  The lane writes no pixel: a
//                   run or a literal is written down as a record that carries its place in the walk's buffer, cut to W * H.  The
//                   waves take groups of 64 files off a list (one atomic per group) until it is empty; the list is sorted by
//                   stream length, longest first, so that the lanes of a wave walk streams of like length.
//   ke_bmpx_expand  parallel over the records, which are independent once they carry their place: blockIdx.x = RLE file,
//                   blockIdx.y = a chunk of 256 records, one per thread.  A record of up to 8 pixels is written by its own
//                   lane; the longer ones are taken up by the whole wave one after the other, a pixel per lane.  Every pixel
//                   goes through the table to its place in the caller's plane -- entry i of the buffer is column i % W of row
//                   H - 1 - i / W (row i / W in a top-down file), so a literal that spills over a row's end needs nothing
//                   special.  Nothing is written beyond the plane: the walker cuts every record to W * H.
#include <algorithm>
#include <vector>

#include "ke_decode_batch.h"

#include "ke_bmpx_parse.h"
#include "ke_lz_window.h"

namespace {

struct KeBmpxDev {
    uint64_t src;          // the image's pixel data (an RLE file's stream) inside the uploaded files
    uint64_t out_off;      // bytes into the caller's pixel buffer
    uint64_t rec_off;      // RLE: its records inside the scratch
    int32_t width, height, kind, topdown;
    uint32_t stride;       // bytes per stored row (not RLE)
    uint32_t bytes;        // RLE: the stream's bytes, up to the file's end
    uint32_t data_off;     // RLE: the stream's place in its file (its parity decides the skip behind a literal)
    uint32_t max_rec;      // RLE: the records it has room for
    uint8_t lut[256];
};

constexpr int kRowsPerBlock = 8;        // at least; more for images taller than 65 535 bands of them
constexpr uint32_t kMaxWaves = 4096;    // of ke_bmpx_codes: more than the chip holds (not measured against fewer)
constexpr uint32_t kChunk = 256;        // records per workgroup of ke_bmpx_expand
constexpr uint32_t kShort = 8;          // pixels up to which a record is its own lane's

__device__ __forceinline__ uint32_t ld4(const uint8_t *p) {       // any alignment
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

__global__ __launch_bounds__(256) void ke_bmpx_unpack(const KeBmpxDev *__restrict__ imgs, const uint8_t *__restrict__ files,
                                                      uint8_t *__restrict__ out, int rows) {
    __shared__ uint8_t s_lut[256];
    const KeBmpxDev &d = imgs[blockIdx.x];
    const int y0 = blockIdx.y * rows;
    if (y0 >= d.height) return;
    const int W = d.width, kind = d.kind;
    const int y1 = min(y0 + rows, d.height);
    if (kind == KE_BMPX_RLE8 || kind == KE_BMPX_RLE4) {
        // the band is one stretch of the plane: bytes up to the first aligned 16, whole 16s, the rest
        uint8_t *dst = out + d.out_off + (size_t)y0 * W;
        const size_t len = (size_t)(y1 - y0) * W;
        const uint32_t b = d.lut[0] * 0x01010101u;
        const size_t to16 = (size_t)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15), head = to16 < len ? to16 : len;
        if (threadIdx.x < head) dst[threadIdx.x] = (uint8_t)b;
        const size_t body = (len - head) >> 4, tail0 = head + (body << 4);
        for (size_t k = threadIdx.x; k < body; k += 256) *reinterpret_cast<u32x4 *>(dst + head + 16 * k) = u32x4{b, b, b, b};
        if (tail0 + threadIdx.x < len) dst[tail0 + threadIdx.x] = (uint8_t)b;
        return;
    }
    if (kind == KE_BMPX_P1 || kind == KE_BMPX_P4) {
        s_lut[threadIdx.x] = d.lut[threadIdx.x];
        __syncthreads();
    }
    const bool is565 = kind == KE_BMPX_RGB565;
    for (int y = y0; y < y1; ++y) {
        const uint8_t *row = files + d.src + (size_t)(d.topdown ? y : d.height - 1 - y) * d.stride;
        if (kind == KE_BMPX_P1 || kind == KE_BMPX_P4) {
            uint8_t *dst = out + d.out_off + (size_t)y * W;
            const int octets = (W + 7) >> 3;
            for (int q = threadIdx.x; q < octets; q += 256) {
                const int x = 8 * q, n = min(8, W - x);
                uint32_t o0 = 0, o1 = 0;
                if (kind == KE_BMPX_P1) {
                    const uint32_t v = row[q];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        o0 |= (uint32_t)s_lut[(v >> (7 - k)) & 1u] << (8 * k);
                        o1 |= (uint32_t)s_lut[(v >> (3 - k)) & 1u] << (8 * k);
                    }
                } else {
                    // eight pixels are four stored bytes; fewer at the row's end, where only the pixels' bytes are read
                    uint32_t v = 0;
                    if (n == 8) v = ld4(row + 4 * q);
                    else for (int k = 0; k < (n + 1) >> 1; ++k) v |= (uint32_t)row[4 * q + k] << (8 * k);
                    o0 = (uint32_t)s_lut[(v >> 4) & 15u] | (uint32_t)s_lut[v & 15u] << 8 | (uint32_t)s_lut[(v >> 12) & 15u] << 16 |
                         (uint32_t)s_lut[(v >> 8) & 15u] << 24;
                    o1 = (uint32_t)s_lut[(v >> 20) & 15u] | (uint32_t)s_lut[(v >> 16) & 15u] << 8 | (uint32_t)s_lut[(v >> 28) & 15u] << 16 |
                         (uint32_t)s_lut[(v >> 24) & 15u] << 24;
                }
                if (n == 8) {
                    __builtin_memcpy(dst + x, &o0, 4);
                    __builtin_memcpy(dst + x + 4, &o1, 4);
                } else {
                    for (int k = 0; k < n; ++k) dst[x + k] = (uint8_t)((k < 4 ? o0 >> (8 * k) : o1 >> (8 * (k - 4))));
                }
            }
        } else {
            uint8_t *dst = out + d.out_off + (size_t)y * W * 3;
            const int quads = (W + 3) >> 2;
            for (int q = threadIdx.x; q < quads; q += 256) {
                const int x = 4 * q, n = min(4, W - x);
                if (n == 4) {
                    const uint32_t a = ld4(row + 8 * (size_t)q), b = ld4(row + 8 * (size_t)q + 4);
                    const uint32_t p0 = ke_bmpx_rgb16(a & 0xFFFFu, is565), p1 = ke_bmpx_rgb16(a >> 16, is565);
                    const uint32_t p2 = ke_bmpx_rgb16(b & 0xFFFFu, is565), p3 = ke_bmpx_rgb16(b >> 16, is565);
                    // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
                    const uint32_t o0 = p0 | (p1 << 24), o1 = (p1 >> 8) | (p2 << 16), o2 = (p2 >> 16) | (p3 << 8);
                    uint8_t *w = dst + 3 * (size_t)x;
                    __builtin_memcpy(w, &o0, 4);
                    __builtin_memcpy(w + 4, &o1, 4);
                    __builtin_memcpy(w + 8, &o2, 4);
                } else {
                    for (int k = 0; k < n; ++k) {
                        const uint8_t *s = row + 2 * (size_t)(x + k);
                        const uint32_t p = ke_bmpx_rgb16((uint32_t)s[0] | ((uint32_t)s[1] << 8), is565);
                        uint8_t *w = dst + 3 * (size_t)(x + k);
                        w[0] = (uint8_t)p; w[1] = (uint8_t)(p >> 8); w[2] = (uint8_t)(p >> 16);
                    }
                }
            }
        }
    }
}

// ke_tiffc_codes' reader for a walk that steps over bytes (a literal's payload, up to 255 of them): within the window and the
// one on its way it goes on as it is, beyond them it starts again where the walk stands.
struct SkipSrc : WindowSrc {
    __device__ __forceinline__ uint32_t byte(uint32_t pos) {
        if (pos >= base + 32) start(pos);
        return WindowSrc::byte(pos);
    }
};

__global__ __launch_bounds__(64) void ke_bmpx_codes(const KeBmpxDev *__restrict__ imgs, const uint32_t *__restrict__ list, uint32_t n,
                                                  const uint8_t *__restrict__ files, KeBmpxRec *__restrict__ records,
                                                  int32_t *__restrict__ status, uint32_t *__restrict__ nrec, uint32_t *__restrict__ next_group) {
    for (;;) {
        uint32_t g = 0;
        if (threadIdx.x == 0) g = atomicAdd(next_group, 1u);
        g = (uint32_t)__shfl((int)g, 0);
        if ((uint64_t)g * 64 >= n) break;
        const uint32_t s = g * 64 + threadIdx.x;
        if (s < n) {
            const uint32_t i = list[s];
            const KeBmpxDev &d = imgs[i];
            SkipSrc src;
            src.file = files + d.src;
            src.limit = d.bytes;
            src.start(0);
            KeBmpxRecSink sink{records + d.rec_off, 0, d.max_rec};
            int st = ke_bmpx_walk(src, d.bytes, d.data_off, (uint32_t)d.width, (uint32_t)d.width * (uint32_t)d.height, d.kind == KE_BMPX_RLE4, sink);
            if (sink.nrec > d.max_rec) st = KE_BMPX_CORRUPT;       // (cannot be: a record per code, a code of two bytes at least)
            status[i] = st;
            nrec[i] = min(sink.nrec, d.max_rec);
        }
    }
}

__global__ __launch_bounds__(256) void ke_bmpx_expand(const KeBmpxDev *__restrict__ imgs, const uint32_t *__restrict__ list,
                                                      const uint8_t *__restrict__ files, const KeBmpxRec *__restrict__ records,
                                                      const int32_t *__restrict__ status, const uint32_t *__restrict__ nrec,
                                                      uint8_t *__restrict__ out) {
    __shared__ uint8_t s_lut[256];
    const uint32_t i = list[blockIdx.x];
    const KeBmpxDev &d = imgs[i];
    const uint32_t m = nrec[i];
    if (status[i] != KE_BMPX_OK || blockIdx.y * kChunk >= m) return;            // (the whole workgroup)
    s_lut[threadIdx.x] = d.lut[threadIdx.x];
    __syncthreads();
    const uint32_t W = (uint32_t)d.width, H = (uint32_t)d.height;
    const bool rle4 = d.kind == KE_BMPX_RLE4, topdown = d.topdown != 0;
    const uint8_t *stream = files + d.src;
    const KeBmpxRec *rec = records + d.rec_off;
    uint8_t *plane = out + d.out_off;
    const uint32_t lane = threadIdx.x & 63u;
    auto pixel = [&](uint32_t pos, uint32_t literal, uint32_t arg, uint32_t k) {
        const uint32_t idx = literal ? ke_bmpx_literal_index(stream + arg, k, rle4) : ke_bmpx_run_index(arg, k, rle4);
        plane[ke_bmpx_place(pos + k, W, H, topdown)] = s_lut[idx & 255u];
    };
    for (uint32_t first = blockIdx.y * kChunk; first < m; first += gridDim.y * kChunk) {
        const uint32_t j = first + threadIdx.x;
        uint32_t pos = 0, len = 0, literal = 0, arg = 0;
        if (j < m) {
            const KeBmpxRec r = rec[j];
            pos = r.pos; len = r.len; literal = r.literal; arg = r.arg;
        }
        if (len <= kShort)
            for (uint32_t k = 0; k < len; ++k) pixel(pos, literal, arg, k);
        uint64_t longer = __ballot(len > kShort);
        while (longer) {
            const int from = __ffsll((long long)longer) - 1;
            longer &= longer - 1;
            const uint32_t bpos = (uint32_t)__shfl((int)pos, from), blen = (uint32_t)__shfl((int)len, from);
            const uint32_t bliteral = (uint32_t)__shfl((int)literal, from), barg = (uint32_t)__shfl((int)arg, from);
            for (uint32_t k = lane; k < blen; k += 64) pixel(bpos, bliteral, barg, k);
        }
    }
}

}  // namespace

KE_API int ke_bmpx_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                         int32_t *heights, int32_t *channels, int32_t *status_out) {
    return ke_probe_each(files, offsets, sizes, n, widths, heights, channels, status_out,
                         [](const uint8_t *file, size_t size, int32_t &w, int32_t &h, int32_t &c, int32_t &st) {
                             KeBmpxInfo info;
                             ke_parse_bmpx(file, size, info);
                             w = info.width; h = info.height; c = info.channels; st = info.status;
                         });
}

KE_API int ke_bmpx_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out) {
    // the format carries no orientation tag, and none of the files taken here has an alpha channel
    return ke_caveats_none(files, offsets, sizes, n, flags_out);
}

KE_API int ke_bmpx_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                          uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out) {
    KE_TRY(ke_decode_check_args(ctx, files, offsets, sizes, n, pixels_out, out_offsets, status_out, "the files' headers are parsed"));
    if (n == 0) return KE_OK;
    std::vector<KeBmpxInfo> infos((size_t)n);                    // the headers are read on the host's threads
    ke_parallel_ranges(n, [&](int64_t a, int64_t b, int) {
        for (int64_t i = a; i < b; ++i) ke_parse_bmpx(files + offsets[i], (size_t)sizes[i], infos[(size_t)i]);
    });
    std::vector<int64_t> which;
    uint64_t lo = ~0ull, hi = 0;
    for (int64_t i = 0; i < n; ++i) {
        status_out[i] = infos[(size_t)i].status;
        if (status_out[i] != KE_BMPX_OK) continue;
        which.push_back(i);
        lo = std::min(lo, offsets[i]);
        hi = std::max(hi, offsets[i] + sizes[i]);
    }
    if (which.empty()) return KE_OK;
    std::vector<KeBmpxDev> imgs;
    std::vector<uint32_t> list;                                    // the sub-batch's RLE files
    KeStreamGuard guard;                                           // after the host vectors it waits for
    void *d_files;
    KE_TRY(ke_upload_files(ctx, guard, files, lo, hi, KE_BUF_PIXELS, 256, &d_files));
    // sub-batches bounded by scratch: the records of the RLE files, 16 B each, one per two bytes of stream at most
    uint64_t budget;
    KE_TRY(ke_scratch_budget(ctx, {KE_BUF_SSIM_AUX}, (uint64_t)1 << 30, (uint64_t)32 << 30, "KE_BMPX_SCRATCH_BYTES", KE_BUDGET_ENV_REPLACES, &budget));
    uint64_t nrecs = 0;
    uint32_t most_rec = 0;
    int max_height = 0;
    auto take = [&](size_t k, bool fresh) {
        if (fresh) {
            nrecs = 0;
            most_rec = 0;
            max_height = 0;
            imgs.clear();
            list.clear();
        }
        const int64_t i = which[k];
        const KeBmpxInfo &info = infos[(size_t)i];
        const bool rle = info.kind == KE_BMPX_RLE8 || info.kind == KE_BMPX_RLE4;
        const uint32_t bytes = rle ? (uint32_t)(sizes[i] - info.data_off) : 0, rc = bytes / 2;
        if (!fresh && (nrecs + rc) * sizeof(KeBmpxRec) > budget) return false;
        KeBmpxDev d;
        d.src = offsets[i] - lo + info.data_off;
        d.out_off = out_offsets[i];
        d.rec_off = nrecs;
        d.width = info.width; d.height = info.height; d.kind = info.kind; d.topdown = info.topdown;
        d.stride = info.stride;
        d.bytes = bytes;
        d.data_off = info.data_off;
        d.max_rec = rc;
        std::memcpy(d.lut, info.lut, 256);
        if (rle) list.push_back((uint32_t)imgs.size());
        nrecs += rc;
        most_rec = std::max(most_rec, rc);
        max_height = std::max(max_height, info.height);
        imgs.push_back(d);
        return true;
    };
    auto launch = [&](size_t m, const int32_t **status, size_t *words) {
        // lanes of one wave finish together at best: neighbours in the list are streams of like length, the longest walks start first
        std::stable_sort(list.begin(), list.end(), [&](uint32_t a, uint32_t b) { return imgs[a].bytes > imgs[b].bytes; });
        const size_t nl = list.size();
        void *d_imgs, *d_list, *d_rec, *d_status, *d_nrec;
        KE_TRY(ke_reserve(ctx, KE_BUF_META, m * sizeof(KeBmpxDev), &d_imgs));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT1, (nl + 1) * 4, &d_list));
        KE_TRY(ke_reserve(ctx, KE_BUF_SSIM_AUX, ((size_t)nrecs + 1) * sizeof(KeBmpxRec), &d_rec));
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT0, (m + 1) * 4, &d_status));                  // the statuses, then the list's counter
        KE_TRY(ke_reserve(ctx, KE_BUF_TILE32, m * 4, &d_nrec));
        KE_HIP(ctx, hipMemcpyAsync(d_imgs, imgs.data(), m * sizeof(KeBmpxDev), hipMemcpyHostToDevice, ctx->stream));
        KE_HIP(ctx, hipMemsetAsync(d_status, 0, (m + 1) * 4, ctx->stream));
        const KeRowTiles tiles = ke_row_tiles(max_height, kRowsPerBlock);
        hipLaunchKernelGGL(ke_bmpx_unpack, dim3((unsigned)m, tiles.grid_y), dim3(256), 0, ctx->stream, (const KeBmpxDev *)d_imgs,
                           (const uint8_t *)d_files, pixels_out, tiles.rows);
        if (nl) {
            KE_HIP(ctx, hipMemcpyAsync(d_list, list.data(), nl * 4, hipMemcpyHostToDevice, ctx->stream));
            const uint32_t waves = (uint32_t)std::min<uint64_t>((nl + 63) / 64, kMaxWaves);
            hipLaunchKernelGGL(ke_bmpx_codes, dim3(waves), dim3(64), 0, ctx->stream, (const KeBmpxDev *)d_imgs, (const uint32_t *)d_list, (uint32_t)nl,
                               (const uint8_t *)d_files, (KeBmpxRec *)d_rec, (int32_t *)d_status, (uint32_t *)d_nrec, (uint32_t *)d_status + m);
            const unsigned chunks = (unsigned)std::min<uint64_t>(((uint64_t)most_rec + kChunk - 1) / kChunk, 65535);
            if (chunks)
                hipLaunchKernelGGL(ke_bmpx_expand, dim3((unsigned)nl, chunks), dim3(256), 0, ctx->stream, (const KeBmpxDev *)d_imgs,
                                   (const uint32_t *)d_list, (const uint8_t *)d_files, (const KeBmpxRec *)d_rec, (const int32_t *)d_status,
                                   (const uint32_t *)d_nrec, pixels_out);
        }
        *status = (const int32_t *)d_status;
        *words = m;
        return (int)KE_OK;
    };
    KE_TRY(ke_decode_sub_batches(ctx, which.size(), take, launch,
                                 [&](size_t at, size_t k, size_t, const int32_t *st) { status_out[which[at]] = st[k]; }));
    guard.disarm();
    return KE_OK;
}
