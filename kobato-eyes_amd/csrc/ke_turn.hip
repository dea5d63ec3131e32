// ke_turn.hip -- the luma plane of a view of a picture: one of the eight orientations (turned.ORIENTATIONS) of a box of it, in one
// pass over the box's pixels.  ke_crop_turn_luma exports it; ke_turn_luma is the same with the box (0, 0, w, h).  It serves the
// SSIM re-check of turned pairs and of pairs that are bordered and turned (ke_api.hip, the pair calls): image a is scored against
// orientation k of a box of image b, and that view's luma is all the fit step needs.  Luma is a per-pixel function, so it commutes
// with the crop and with the permutation: the plane written here is byte for byte the luma of the cropped and turned picture.
//
// One view per blockIdx.y, 64 x 64 tiles of the destination over blockIdx.x (a workgroup strides over the view's tiles), 256
// threads.  The destination is the box's size, swapped for k & 4; a tile's source rectangle lies at the box's origin inside the
// image (ke_turn_core.h has the turn's coordinate arithmetic, ke_view_core.h the box's).  A tile goes through LDS twice:
//   A  the tile's source rectangle, source row by source row: a wave takes a row and reads its bytes as aligned dwords --
//      64 / 192 / 256 contiguous bytes for 1 / 3 / 4 channels -- into `raw`, one row per kRawPitch bytes.  The rows are the IMAGE's
//      pitch of w * ch bytes apart, so a row starts on any byte whatever the box's width: the row's first dword is the aligned one
//      below it and `raw` keeps the 0..3 bytes of lead.  This may read the margin pixels beside the box that share a dword with
//      it, never a byte outside the image: only a dword that reaches outside the image's own bytes (the first and the last of an
//      image) is put together from byte loads.
//   B  a thread per source pixel takes luma from `raw` and writes the byte where the pixel lies in the DESTINATION tile:
//      `tile`, one destination row per kTilePitch = 68 bytes.  For the transposing orientations the 32 lanes of a half wave
//      write a column: bytes (68 r + c), banks ((68 r + c) / 4) % 32 = (17 r + c / 4) % 32, all distinct since 17 is odd.
//   C  the tile goes out destination row by destination row: 16 lanes a row, a dword each, stored at aligned addresses.
//      Destination rows are packed and start on any byte, so the dword a lane stores is cut from two neighbouring LDS dwords
//      (banks 17 r + j and 17 r + j + 1 over the 16 lanes of a row: distinct), and the row's first and last <= 3 bytes are byte
//      stores.
// No byte-wide global access inside a tile.
#include "ke_internal.h"
#include "ke_view_core.h"

namespace {

constexpr int kT = KE_TURN_TILE;
constexpr int kRawPitch = 4 * kT + 4;     // a source row of the tile at 4 channels, and its lead
constexpr int kTilePitch = kT + 4;        // 68: see B and C above

__global__ __launch_bounds__(256) void ke_view_luma_kernel(const uint8_t *__restrict__ src, const KeViewJob *__restrict__ items, int64_t first,
                                                           uint8_t *__restrict__ dst) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[kT * kRawPitch];
    __shared__ __attribute__((aligned(16))) uint8_t tile[kT * kTilePitch + 4];
    const KeViewJob it = items[first + blockIdx.y];
    const int k = it.orientation, w = it.w, ch = it.channels;
    const KeViewBox box{it.x0, it.y0, it.bw, it.bh};
    int dw, dh;
    ke_view_dst_size(k, box, &dw, &dh);
    const int ntx = ke_turn_tiles_x(dw), tiles = ntx * ke_turn_tiles_y(dh);
    const uint8_t *s = src + it.src_off;
    const uint8_t *s_end = s + (size_t)w * it.h * ch;
    const int base_mod4 = (int)((uintptr_t)s & 3);
    uint8_t *d = dst + it.dst_off;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const KeTurnRect dr = ke_turn_tile_dst_rect(dw, dh, t % ntx, t / ntx);
        const KeTurnRect sr = ke_view_src_rect(k, box, dw, dh, dr);
        // A: source rows -> raw, walked with the image's pitch
        for (int ly = wave; ly < sr.h; ly += 4) {
            const size_t at = ke_view_px_byte(w, ch, sr.x0, sr.y0 + ly);
            int lead;
            const int ndw = ke_view_row_dwords(at, base_mod4, sr.w, ch, &lead);
            const uint8_t *a0 = s + at - lead;
            uint32_t *out = (uint32_t *)(raw + ly * kRawPitch);
            for (int j = lane; j < ndw; j += 64) {
                const uint8_t *p = a0 + 4 * j;
                uint32_t v;
                if (p >= s && p + 4 <= s_end) {
                    v = *(const uint32_t *)p;
                } else {
                    v = 0;
                    for (int b = 0; b < 4; ++b)
                        if (p + b >= s && p + b < s_end) v |= (uint32_t)p[b] << (8 * b);
                }
                out[j] = v;
            }
        }
        __syncthreads();
        // B: luma, placed where the pixel lies in the destination tile
        for (int ly = wave; ly < sr.h; ly += 4) {
            if (lane < sr.w) {
                int lead, x, y;
                ke_view_row_dwords(ke_view_px_byte(w, ch, sr.x0, sr.y0 + ly), base_mod4, sr.w, ch, &lead);
                ke_view_dst_xy(k, box, dw, dh, sr.x0 + lane, sr.y0 + ly, &x, &y);
                tile[(y - dr.y0) * kTilePitch + (x - dr.x0)] = (uint8_t)ke_turn_luma_px(raw + ly * kRawPitch + lead + lane * ch, ch);
            }
        }
        __syncthreads();
        // C: destination rows out of the tile
        for (int slot = threadIdx.x; slot < dr.h * 16; slot += 256) {
            const int r = slot >> 4, j = slot & 15;
            uint8_t *g = d + (size_t)(dr.y0 + r) * dw + dr.x0;
            const uint8_t *trow = tile + r * kTilePitch;
            int head = (int)((4 - ((uintptr_t)g & 3)) & 3);
            if (head > dr.w) head = dr.w;
            const int nd = (dr.w - head) >> 2, done = head + 4 * nd;
            if (j < nd) {
                const uint32_t *q = (const uint32_t *)trow + j + (head ? 1 : 0);
                // bytes head + 4 j .. + 3 of the row: head = 0 is the dword itself, else the upper bytes of one dword and the lower of the next
                const uint32_t v = head ? __funnelshift_r(q[-1], q[0], 8 * head) : q[0];
                *(uint32_t *)(g + head + 4 * j) = v;
            }
            if (j == 0)
                for (int b = 0; b < head; ++b) g[b] = trow[b];
            if (j == 15)
                for (int b = done; b < dr.w; ++b) g[b] = trow[b];
        }
        // the next tile's A writes `raw`, which nobody reads after the second barrier; its B writes `tile` behind A's barrier
    }
}

}  // namespace

int ke_launch_view_luma(ke_ctx *ctx, const uint8_t *d_src, const KeViewJob *jobs, int64_t n, uint8_t *d_dst, int timer) {
    if (n == 0) return KE_OK;
    int64_t most = 1;
    for (int64_t i = 0; i < n; ++i) {
        int dw, dh;
        ke_view_dst_size(jobs[i].orientation, KeViewBox{jobs[i].x0, jobs[i].y0, jobs[i].bw, jobs[i].bh}, &dw, &dh);
        most = std::max<int64_t>(most, (int64_t)ke_turn_tiles_x(dw) * ke_turn_tiles_y(dh));
    }
    void *d_items;                                         // the kernel reads the jobs as they are
    KE_TRY(ke_reserve(ctx, KE_BUF_META, (size_t)n * sizeof(KeViewJob), &d_items));
    KE_HIP(ctx, hipMemcpyAsync(d_items, jobs, (size_t)n * sizeof(KeViewJob), hipMemcpyHostToDevice, ctx->stream));
    const unsigned gx = (unsigned)std::min<int64_t>(most, 4096);
    if (timer >= 0) ke_time_begin(ctx, timer);
    for (int64_t first = 0; first < n; first += 65535) {
        const unsigned gy = (unsigned)std::min<int64_t>(65535, n - first);
        hipLaunchKernelGGL(ke_view_luma_kernel, dim3(gx, gy), dim3(256), 0, ctx->stream, d_src, (const KeViewJob *)d_items, first, d_dst);
    }
    if (timer >= 0) ke_time_end(ctx, timer);
    KE_HIP(ctx, hipGetLastError());
    KE_HIP(ctx, hipStreamSynchronize(ctx->stream));       // `jobs` is the caller's host array
    return KE_OK;
}

KE_API int ke_turn_luma(ke_ctx *ctx, const uint8_t *src, const uint64_t *src_offsets, const int32_t *widths, const int32_t *heights,
                        const int32_t *channels, const int32_t *orientations, int64_t n, uint8_t *dst, const uint64_t *dst_offsets) {
    if (!ctx) return KE_EINVAL;
    if (n < 0 || (n > 0 && (!src || !src_offsets || !widths || !heights || !channels || !orientations || !dst || !dst_offsets)))
        return ke_fail(ctx, KE_EINVAL, "NULL argument");
    if (n == 0) return KE_OK;
    if (!ke_is_device_ptr(src) || !ke_is_device_ptr(dst)) return ke_fail(ctx, KE_EINVAL, "src and dst are device memory");
    KE_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<KeViewJob> jobs((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (widths[i] <= 0 || heights[i] <= 0 || (channels[i] != 1 && channels[i] != 3 && channels[i] != 4) || orientations[i] < 0 ||
            orientations[i] > 7)
            return ke_fail(ctx, KE_EINVAL, "image %lld: %dx%d, %d channels, orientation %d", (long long)i, widths[i], heights[i], channels[i],
                           orientations[i]);
        jobs[(size_t)i] = KeViewJob{src_offsets[i], dst_offsets[i], widths[i], heights[i], channels[i], orientations[i], 0, 0, widths[i], heights[i]};
    }
    return ke_launch_view_luma(ctx, src, jobs.data(), n, dst, -1);
}

KE_API int ke_crop_turn_luma(ke_ctx *ctx, const uint8_t *src, const uint64_t *src_offsets, const int32_t *widths, const int32_t *heights,
                             const int32_t *channels, const int32_t *boxes, const int32_t *orientations, int64_t n, uint8_t *dst,
                             const uint64_t *dst_offsets) {
    if (!ctx) return KE_EINVAL;
    if (n < 0 || (n > 0 && (!src || !src_offsets || !widths || !heights || !channels || !boxes || !orientations || !dst || !dst_offsets)))
        return ke_fail(ctx, KE_EINVAL, "NULL argument");
    if (n == 0) return KE_OK;
    if (!ke_is_device_ptr(src) || !ke_is_device_ptr(dst)) return ke_fail(ctx, KE_EINVAL, "src and dst are device memory");
    KE_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<KeViewJob> jobs((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t *b = boxes + 4 * i;
        const int ch = channels[i], w = widths[i], h = heights[i], o = orientations[i];
        const bool shape = w > 0 && h > 0 && (ch == 1 || ch == 3 || ch == 4) && (int64_t)w * ch <= INT32_MAX - 64;
        if (!shape || o < 0 || o > 7 || b[0] < 0 || b[1] < 0 || b[2] <= b[0] || b[3] <= b[1] || b[2] > w || b[3] > h)
            return ke_fail(ctx, KE_EINVAL, "image %lld: %dx%d, %d channels, box (%d, %d, %d, %d), orientation %d", (long long)i, w, h, ch, b[0],
                           b[1], b[2], b[3], o);
        jobs[(size_t)i] = KeViewJob{src_offsets[i], dst_offsets[i], w, h, ch, o, b[0], b[1], b[2] - b[0], b[3] - b[1]};
    }
    return ke_launch_view_luma(ctx, src, jobs.data(), n, dst, KE_T_VIEW_LUMA);
}
