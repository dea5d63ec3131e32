// ke_trim.hip -- bordered copies: the content box of every image of a batch (ke_content_boxes), the boxes' rows copied out
// packed (ke_crop_pack), the pHash of the qualifying crops through the existing hash dispatch (ke_hash_images_trimmed), and the
// luma plane of a box (ke_crop_luma, the crop of ke_ssim_pairs_boxed in ke_api.hip).
// The definition is in include/keyes.h, the arithmetic in ke_trim_core.h, the luma in ke_turn_core.h.
//
// ke_content_boxes_kernel: one read of every pixel.  A work item is (image, band of KE_TRIM_BAND_ROWS rows); a workgroup of
// 256 threads takes a run of the item list.  A wave takes a row, its lanes the row's aligned 16-byte vectors: the row starts on
// any byte, so its first vector is the aligned one below it and the bytes in front of the row, like those behind it in the
// last vector, are masked off.  Only a vector that reaches outside the image's own bytes -- the first and the last of an
// image -- is put together from byte loads.  The four bytes of a dword are tested in registers against bounds spread into
// 16-bit fields (KeTrimPat); the pattern of a dword depends on the channel of its first byte only, the patterns of an image
// are made once per run (four threads, LDS) and a lane picks its three per row and turns them round from vector to vector.  A lane
// keeps min and max of the byte-in-row index and of the row of the differing bytes it saw, across the items of one image;
// when the run moves on to another image, and at its end: one wave reduction, one LDS step and at most four atomics on the
// image's box in global memory, which ke_trim_init_boxes_kernel set to (INT_MAX, INT_MAX, 0, 0) on the same stream.
// Atomics, not partial boxes and a second kernel: a flush is four atomics on 16 bytes against the 48 KiB or more read for
// it, the workgroups that share an image are few, and the second kernel would need the same table again.
//
// ke_crop_pack_kernel: a wave per box row, a lane per aligned dword of the DESTINATION; the source bytes of that dword lie
// at any alignment, so they are cut from two aligned source dwords with a funnel shift (ke_turn.hip's step C), and a row's
// first and last <= 3 bytes are byte stores.  A source dword that reaches outside the image's bytes is put together from
// byte loads.
//
// ke_crop_luma_kernel: the same, for the luma plane of the box (ke_ssim_pairs_boxed's crops): a destination dword is four pixels,
// so 4, 12 or 16 source bytes, and what is written is 1 byte per pixel instead of the box's rows as they are.
#include <algorithm>

#include "ke_internal.h"
#include "ke_trim_core.h"
#include "ke_turn_core.h"

namespace {

struct TrimImage {
    uint64_t off;        // bytes from the pixel base
    int32_t w, h;
};
struct TrimItem {
    int32_t image, y0;   // band [y0, min(y0 + KE_TRIM_BAND_ROWS, h))
};
struct CropJob {
    uint64_t src_off, dst_off;
    int32_t w, h;              // source size
    int32_t x0, y0, bw, bh;    // the box
};

constexpr size_t kStageBytes = (size_t)1 << 30;   // host pixels go through the staging buffer in chunks of at most this
constexpr size_t kCropBytes = (size_t)1 << 30;    // crops of one chunk of ke_hash_images_trimmed (or one crop, if larger)
constexpr int64_t kRunItems = 64;                 // items a workgroup of the box kernel takes at most, once the chip is full

__global__ void ke_trim_init_boxes_kernel(int32_t *boxes, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * 4) boxes[i] = (i & 3) < 2 ? INT32_MAX : 0;
}

// one wave reduction, one LDS step, at most four atomics: the bounds a workgroup gathered for the image whose box is b
__device__ __forceinline__ void trim_flush(KeTrimAcc acc, KeTrimAcc *part, int lane, int wave, int ch, int32_t *b) {
    for (int d = 32; d >= 1; d >>= 1) {
        KeTrimAcc o;
        o.bmin = __shfl_xor(acc.bmin, d);
        o.bmax = __shfl_xor(acc.bmax, d);
        o.ymin = __shfl_xor(acc.ymin, d);
        o.ymax = __shfl_xor(acc.ymax, d);
        ke_trim_acc_merge(&acc, o);
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) ke_trim_acc_merge(&acc, part[k]);
        if (acc.ymax >= 0) {
            int32_t box[4];
            ke_trim_box(acc, ch, box);
            atomicMin(b + 0, box[0]);
            atomicMin(b + 1, box[1]);
            atomicMax(b + 2, box[2]);
            atomicMax(b + 3, box[3]);
        }
    }
    __syncthreads();   // `part`, and the patterns beside it, are written again for the next image
}

__global__ __launch_bounds__(256) void ke_content_boxes_kernel(const uint8_t *__restrict__ px, const TrimImage *__restrict__ images,
                                                               const TrimItem *__restrict__ items, int64_t n_items, int ch, int tol,
                                                               int32_t *__restrict__ boxes) {
    __shared__ KeTrimPat pats[4];
    __shared__ KeTrimAcc part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // this workgroup's items: a run of the list, so that the bands of one image mostly meet in one workgroup
    const int64_t per = (n_items + gridDim.x - 1) / gridDim.x;
    int64_t it = (int64_t)blockIdx.x * per;
    const int64_t end = it + per < n_items ? it + per : n_items;
    if (it >= end) return;
    TrimItem item = items[it];
    int32_t cur = -1;                      // the image `acc`, `pats` and the pointers below belong to
    KeTrimAcc acc = ke_trim_acc_empty();
    const uint8_t *s = nullptr, *s_end = nullptr;
    int32_t row_bytes = 0, h = 0;

    for (; it < end; ++it) {
        int32_t next_image = item.image, next_y0 = item.y0;              // asked for before this item's rows, used after them
        if (it + 1 < end) {
            next_image = items[it + 1].image;
            next_y0 = items[it + 1].y0;
        }
        if (item.image != cur) {                                         // the same in every thread
            if (cur >= 0) {
                trim_flush(acc, part, lane, wave, ch, boxes + (size_t)cur * 4);
                acc = ke_trim_acc_empty();
            }
            cur = item.image;
            const TrimImage im = images[cur];
            s = px + im.off;
            row_bytes = im.w * ch;
            h = im.h;
            s_end = s + (size_t)row_bytes * h;
            if (threadIdx.x < 4) {
                const uint8_t ref[4] = {s[0], ch > 1 ? s[1] : (uint8_t)0, ch > 1 ? s[2] : (uint8_t)0, 0};   // pixel (0, 0): inside the image
                pats[threadIdx.x] = ke_trim_pat(ref, tol, ch, (int)threadIdx.x % ch);
            }
            __syncthreads();
        }
        const int y1 = min(item.y0 + KE_TRIM_BAND_ROWS, h);
        for (int y = item.y0 + wave; y < y1; y += 4) {
            const uint8_t *row = s + (size_t)y * row_bytes;
            const int lead = (int)((uintptr_t)row & (KE_TRIM_VEC - 1));
            const int nv = (lead + row_bytes + KE_TRIM_VEC - 1) / KE_TRIM_VEC;
            if (lane >= nv) continue;
            const int f0 = ke_trim_phase(KE_TRIM_VEC * lane - lead, ch);
            // dword k of this lane's vector has phase (f0 + 4 k) % ch, and the lane's next vector, 64 * 16 bytes on, (f0 + 1024) % ch:
            // for 3 channels both go up by one, for 1 and 4 they stay
            KeTrimPat p0 = pats[f0], p1 = pats[(f0 + 4) % ch], p2 = pats[(f0 + 8) % ch];
            for (int j = lane; j < nv; j += 64) {
                const int32_t at = KE_TRIM_VEC * j - lead;
                uint32_t v[4];
                ke_trim_load_vec(row + at, s, s_end, v);
                ke_trim_vec(&acc, v, p0, p1, p2, p0, at, row_bytes, y);
                if (ch == 3) {
                    const KeTrimPat t = p0;
                    p0 = p1; p1 = p2; p2 = t;
                }
            }
        }
        item.image = next_image;
        item.y0 = next_y0;
    }
    trim_flush(acc, part, lane, wave, ch, boxes + (size_t)cur * 4);
}

// the dword at the aligned address p, bytes outside [s, s_end) as 0
__device__ __forceinline__ uint32_t load_dword_inside(const uint8_t *p, const uint8_t *s, const uint8_t *s_end) {
    if (p >= s && p + 4 <= s_end) return *(const uint32_t *)p;
    uint32_t v = 0;
    for (int b = 0; b < 4; ++b)
        if (p + b >= s && p + b < s_end) v |= (uint32_t)p[b] << (8 * b);
    return v;
}

__global__ __launch_bounds__(256) void ke_crop_pack_kernel(const uint8_t *__restrict__ src, const CropJob *__restrict__ jobs, int64_t first,
                                                           int ch, uint8_t *__restrict__ dst) {
    const CropJob job = jobs[first + blockIdx.y];
    const uint8_t *s = src + job.src_off;
    const uint8_t *s_end = s + (size_t)job.w * job.h * ch;
    uint8_t *d = dst + job.dst_off;
    const int len = job.bw * ch;                 // bytes of a box row
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = blockIdx.x * 4 + wave; r < job.bh; r += gridDim.x * 4) {
        const uint8_t *srow = s + ((size_t)(job.y0 + r) * job.w + job.x0) * ch;
        uint8_t *g = d + (size_t)r * len;
        int head = (int)((4 - ((uintptr_t)g & 3)) & 3);
        if (head > len) head = len;
        const int nd = (len - head) >> 2, done = head + 4 * nd;
        for (int j = lane; j < nd; j += 64) {
            const uint8_t *a = srow + head + 4 * j;          // the four source bytes of this destination dword
            const int sh = (int)((uintptr_t)a & 3);
            const uint8_t *a0 = a - sh;
            uint32_t v = load_dword_inside(a0, s, s_end);
            if (sh) v = __funnelshift_r(v, load_dword_inside(a0 + 4, s, s_end), 8 * sh);
            *(uint32_t *)(g + head + 4 * j) = v;
        }
        if (lane == 0)
            for (int b = 0; b < head; ++b) g[b] = srow[b];
        if (lane == 63)
            for (int b = done; b < len; ++b) g[b] = srow[b];
    }
}

// ke_crop_luma_kernel: ke_crop_pack_kernel's shape with the luma between the load and the store.  A destination dword is four
// pixels, so its source is 4 * CH bytes at any alignment: CH aligned dwords and, unless the bytes start on one, one more, cut
// with funnel shifts into CH dwords that start at the first pixel.  The alignment is the same for every dword of a row.
template <int CH>
__device__ __forceinline__ void crop_luma_rows(const uint8_t *__restrict__ s, const uint8_t *s_end, uint8_t *__restrict__ d,
                                               const KeCropLumaJob &job, int lane, int wave) {
    for (int r = blockIdx.x * 4 + wave; r < job.bh; r += gridDim.x * 4) {
        const uint8_t *srow = s + ((size_t)(job.y0 + r) * job.w + job.x0) * CH;
        uint8_t *g = d + (size_t)r * job.bw;
        int head = (int)((4 - ((uintptr_t)g & 3)) & 3);
        if (head > job.bw) head = job.bw;
        const int nd = (job.bw - head) >> 2, done = head + 4 * nd;
        const int sh = (int)((uintptr_t)(srow + head * CH) & 3);
        const uint8_t *a0 = srow + head * CH - sh;
        for (int j = lane; j < nd; j += 64) {
            const uint8_t *a = a0 + (size_t)j * (4 * CH);
            uint32_t t[CH + 1];
#pragma unroll
            for (int k = 0; k < CH; ++k) t[k] = load_dword_inside(a + 4 * k, s, s_end);
            if (sh) {
                t[CH] = load_dword_inside(a + 4 * CH, s, s_end);
#pragma unroll
                for (int k = 0; k < CH; ++k) t[k] = __funnelshift_r(t[k], t[k + 1], 8 * sh);
            }
            uint32_t v = 0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                uint8_t px[CH];
#pragma unroll
                for (int c = 0; c < CH; ++c) px[c] = (uint8_t)(t[(p * CH + c) >> 2] >> (8 * ((p * CH + c) & 3)));
                v |= (uint32_t)ke_turn_luma_px(px, CH) << (8 * p);
            }
            *(uint32_t *)(g + head + 4 * j) = v;
        }
        if (lane == 0)
            for (int b = 0; b < head; ++b) g[b] = (uint8_t)ke_turn_luma_px(srow + b * CH, CH);
        if (lane == 63)
            for (int b = done; b < job.bw; ++b) g[b] = (uint8_t)ke_turn_luma_px(srow + b * CH, CH);
    }
}

__global__ __launch_bounds__(256) void ke_crop_luma_kernel(const uint8_t *__restrict__ src, const KeCropLumaJob *__restrict__ jobs,
                                                           int64_t first, uint8_t *__restrict__ dst) {
    const KeCropLumaJob job = jobs[first + blockIdx.y];
    const uint8_t *s = src + job.src_off;
    const uint8_t *s_end = s + (size_t)job.w * job.h * job.channels;
    uint8_t *d = dst + job.dst_off;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (job.channels == 1) crop_luma_rows<1>(s, s_end, d, job, lane, wave);
    else if (job.channels == 3) crop_luma_rows<3>(s, s_end, d, job, lane, wave);
    else crop_luma_rows<4>(s, s_end, d, job, lane, wave);
}

bool shape_ok(int32_t w, int32_t h, int ch) { return w > 0 && h > 0 && (int64_t)w * ch <= INT32_MAX - 64; }

// Boxes of n images in device memory, into a host array; images with take[i] == 0 get four zeros.  Drains the stream.
int boxes_on_device(ke_ctx *ctx, const uint8_t *d_px, const uint64_t *off, const int32_t *w, const int32_t *h, const uint8_t *take, int ch,
                    int64_t n, int tol, int32_t *boxes) {
    std::vector<TrimImage> images((size_t)n);
    std::vector<TrimItem> items;
    for (int64_t i = 0; i < n; ++i) {
        images[(size_t)i] = TrimImage{off[i], w[i], h[i]};
        if (!take[i]) continue;
        for (int b = 0; b < ke_trim_bands(h[i]); ++b) items.push_back(TrimItem{(int32_t)i, b * KE_TRIM_BAND_ROWS});
    }
    const size_t img_bytes = ((size_t)n * sizeof(TrimImage) + 15) & ~(size_t)15, item_bytes = items.size() * sizeof(TrimItem);
    void *meta, *d_boxes;
    KE_TRY(ke_reserve(ctx, KE_BUF_META, img_bytes + item_bytes, &meta));
    KE_TRY(ke_reserve(ctx, KE_BUF_TRIM_BOXES, (size_t)n * 16, &d_boxes));
    KE_HIP(ctx, hipMemcpyAsync(meta, images.data(), (size_t)n * sizeof(TrimImage), hipMemcpyHostToDevice, ctx->stream));
    if (item_bytes) KE_HIP(ctx, hipMemcpyAsync((uint8_t *)meta + img_bytes, items.data(), item_bytes, hipMemcpyHostToDevice, ctx->stream));
    ke_time_begin(ctx, KE_T_TRIM_BOX);
    hipLaunchKernelGGL(ke_trim_init_boxes_kernel, dim3((unsigned)((n * 4 + 255) / 256)), dim3(256), 0, ctx->stream, (int32_t *)d_boxes, n);
    if (!items.empty()) {
        // runs of at most kRunItems items, and at least 32 workgroups per compute unit while the items last: a workgroup that
        // stays with an image flushes once for it, and the last round of workgroups is a small share of the launch
        const int64_t n_items = (int64_t)items.size();
        const unsigned grid = (unsigned)std::min<int64_t>(n_items, std::max<int64_t>((int64_t)std::max(ctx->cu_count, 1) * 32, (n_items + kRunItems - 1) / kRunItems));
        hipLaunchKernelGGL(ke_content_boxes_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_px, (const TrimImage *)meta,
                           (const TrimItem *)((uint8_t *)meta + img_bytes), (int64_t)items.size(), ch, tol, (int32_t *)d_boxes);
    }
    ke_time_end(ctx, KE_T_TRIM_BOX);
    KE_HIP(ctx, hipGetLastError());
    KE_HIP(ctx, hipMemcpyAsync(boxes, d_boxes, (size_t)n * 16, hipMemcpyDeviceToHost, ctx->stream));
    KE_HIP(ctx, hipStreamSynchronize(ctx->stream));       // `images` and `items` are host vectors
    for (int64_t i = 0; i < n; ++i)
        if (boxes[4 * i + 2] == 0) boxes[4 * i] = boxes[4 * i + 1] = 0;   // nothing differed: x1 was never raised
    return KE_OK;
}

// Box rows of m jobs, packed; drains the stream (the job table is a host vector).
int launch_crop_pack(ke_ctx *ctx, const uint8_t *d_src, const std::vector<CropJob> &jobs, int ch, uint8_t *d_dst) {
    const int64_t m = (int64_t)jobs.size();
    if (m == 0) return KE_OK;
    int most = 1;
    for (const CropJob &j : jobs) most = std::max(most, j.bh);
    void *d_jobs;
    KE_TRY(ke_reserve(ctx, KE_BUF_META, (size_t)m * sizeof(CropJob), &d_jobs));
    KE_HIP(ctx, hipMemcpyAsync(d_jobs, jobs.data(), (size_t)m * sizeof(CropJob), hipMemcpyHostToDevice, ctx->stream));
    const unsigned gx = (unsigned)std::min(std::max((most + 15) / 16, 1), 256);   // a wave copies four rows or more
    ke_time_begin(ctx, KE_T_TRIM_CROP);
    for (int64_t first = 0; first < m; first += 65535) {
        const unsigned gy = (unsigned)std::min<int64_t>(65535, m - first);
        hipLaunchKernelGGL(ke_crop_pack_kernel, dim3(gx, gy), dim3(256), 0, ctx->stream, d_src, (const CropJob *)d_jobs, first, ch, d_dst);
    }
    ke_time_end(ctx, KE_T_TRIM_CROP);
    KE_HIP(ctx, hipGetLastError());
    KE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KE_OK;
}

bool box_inside(const int32_t *b, int32_t w, int32_t h) { return b[0] >= 0 && b[1] >= 0 && b[2] > b[0] && b[3] > b[1] && b[2] <= w && b[3] <= h; }

// Host pixels reach the device in chunks of whole images, packed, of at most kStageBytes (or one image): [lo, hi) and the
// packed offsets of its images.
int64_t stage_chunk(ke_ctx *ctx, const uint8_t *pixels, const std::vector<uint64_t> &off, const int32_t *w, const int32_t *h,
                    const std::vector<uint8_t> &take, int ch, int64_t lo, int64_t n, std::vector<uint64_t> &packed, const uint8_t **d_px, int *rc) {
    size_t bytes = 0;
    int64_t hi = lo;
    packed.clear();
    for (; hi < n; ++hi) {
        const size_t b = take[(size_t)hi] ? (size_t)w[hi] * h[hi] * ch : 0;
        if (hi > lo && bytes + b > kStageBytes) break;
        packed.push_back(bytes);
        bytes += b;
    }
    void *tmp = nullptr;
    *rc = ke_reserve(ctx, KE_BUF_PIXELS, bytes, &tmp);
    if (*rc != KE_OK) return hi;
    for (int64_t i = lo; i < hi; ++i) {
        if (!take[(size_t)i]) continue;
        const hipError_t e = hipMemcpyAsync((uint8_t *)tmp + packed[(size_t)(i - lo)], pixels + off[(size_t)i], (size_t)w[i] * h[i] * ch,
                                            hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            *rc = ke_fail(ctx, KE_EHIP, "hipMemcpyAsync failed: %s", hipGetErrorString(e));
            return hi;
        }
    }
    *d_px = (const uint8_t *)tmp;
    return hi;
}

struct TrimCall {
    std::vector<uint64_t> off;
    std::vector<uint8_t> take;
};

int check_images(ke_ctx *ctx, const uint8_t *pixels, const uint64_t *offsets, const int32_t *widths, const int32_t *heights, int32_t channels,
                 int64_t n, int32_t tolerance, int32_t *status_out, TrimCall &c) {
    if (n < 0 || n > INT32_MAX || (n > 0 && (!pixels || !widths || !heights))) return ke_fail(ctx, KE_EINVAL, "pixels/widths/heights must be non-NULL");
    if (channels != 1 && channels != 3 && channels != 4) return ke_fail(ctx, KE_EINVAL, "channels must be 1, 3 or 4 (got %d)", channels);
    if (tolerance < 0 || tolerance > 255) return ke_fail(ctx, KE_EINVAL, "tolerance must be in 0..255 (got %d)", tolerance);
    if (n > 0 && (ke_is_device_ptr(widths) || ke_is_device_ptr(heights) || ke_is_device_ptr(offsets) || ke_is_device_ptr(status_out)))
        return ke_fail(ctx, KE_EINVAL, "offsets/widths/heights/status are metadata and must be host arrays");
    c.off.resize((size_t)n);
    c.take.resize((size_t)n);
    uint64_t run = 0;
    for (int64_t i = 0; i < n; ++i) {
        c.off[(size_t)i] = offsets ? offsets[i] : run;
        c.take[(size_t)i] = shape_ok(widths[i], heights[i], channels);
        if (c.take[(size_t)i]) run += (uint64_t)widths[i] * heights[i] * channels;
        if (status_out) status_out[i] = c.take[(size_t)i] ? KE_IMG_OK : KE_IMG_BAD_SHAPE;
    }
    return KE_OK;
}

// boxes, the qualifying rule, crops in chunks, the hash dispatch on the crops: n images in device memory, host outputs
int trimmed_on_device(ke_ctx *ctx, const uint8_t *d_px, const uint64_t *off, const int32_t *w, const int32_t *h, const uint8_t *take, int ch,
                      int64_t n, int tol, uint64_t *phash, int32_t *boxes, uint8_t *has, int32_t *status, uint64_t *turned8 = nullptr) {
    // turned8 (ke_hash_images_turned_trimmed; phash is NULL then): the crops go to ke_hash_images_turned instead, eight hashes each
    KE_TRY(boxes_on_device(ctx, d_px, off, w, h, take, ch, n, tol, boxes));
    std::vector<int64_t> q;
    for (int64_t i = 0; i < n; ++i) {
        if (turned8) std::memset(turned8 + 8 * i, 0, 64);
        else phash[i] = 0;
        has[i] = 0;
        if (take[i] && ke_trim_qualifies(w[i], h[i], boxes + 4 * i)) q.push_back(i);
    }
    std::vector<CropJob> jobs;
    std::vector<uint64_t> c_off, c_hash;
    std::vector<int32_t> c_w, c_h, c_st;
    for (size_t lo = 0; lo < q.size();) {
        jobs.clear(); c_off.clear(); c_w.clear(); c_h.clear();
        size_t bytes = 0, hi = lo;
        for (; hi < q.size(); ++hi) {
            const int32_t *b = boxes + 4 * q[hi];
            const size_t cb = (size_t)(b[2] - b[0]) * (b[3] - b[1]) * ch;
            if (hi > lo && bytes + cb > kCropBytes) break;
            jobs.push_back(CropJob{off[q[hi]], bytes, w[q[hi]], h[q[hi]], b[0], b[1], b[2] - b[0], b[3] - b[1]});
            c_off.push_back(bytes);
            c_w.push_back(b[2] - b[0]);
            c_h.push_back(b[3] - b[1]);
            bytes += cb;
        }
        const int64_t m = (int64_t)(hi - lo);
        void *d_crops;
        KE_TRY(ke_reserve(ctx, KE_BUF_TRIM_CROPS, bytes, &d_crops));
        KE_TRY(launch_crop_pack(ctx, d_px, jobs, ch, (uint8_t *)d_crops));
        c_st.assign((size_t)m, 0);
        c_hash.assign((size_t)m * (turned8 ? 8 : 1), 0);
        if (turned8) KE_TRY(ke_hash_images_turned(ctx, (const uint8_t *)d_crops, c_off.data(), c_w.data(), c_h.data(), ch, m, c_hash.data(), c_st.data()));
        else KE_TRY(ke_hash_images(ctx, (const uint8_t *)d_crops, c_off.data(), c_w.data(), c_h.data(), ch, m, c_hash.data(), nullptr, c_st.data()));
        for (int64_t k = 0; k < m; ++k) {
            const int64_t i = q[lo + (size_t)k];
            if (c_st[(size_t)k] == KE_IMG_OK) {
                if (turned8) std::memcpy(turned8 + 8 * i, c_hash.data() + 8 * (size_t)k, 64);
                else phash[i] = c_hash[(size_t)k];
                has[i] = 1;
            } else {
                status[i] = c_st[(size_t)k];
            }
        }
        lo = hi;
    }
    return KE_OK;
}

}  // namespace

KE_API int ke_content_boxes(ke_ctx *ctx, const uint8_t *pixels, const uint64_t *offsets, const int32_t *widths, const int32_t *heights,
                            int32_t channels, int64_t n, int32_t tolerance, int32_t *boxes_out, int32_t *status_out) {
    if (!ctx) return KE_EINVAL;
    if (n > 0 && (!boxes_out || ke_is_device_ptr(boxes_out))) return ke_fail(ctx, KE_EINVAL, "boxes_out must be a host array");
    TrimCall c;
    KE_TRY(check_images(ctx, pixels, offsets, widths, heights, channels, n, tolerance, status_out, c));
    if (n == 0) return KE_OK;
    KE_HIP(ctx, hipSetDevice(ctx->device));
    if (ke_is_device_ptr(pixels)) return boxes_on_device(ctx, pixels, c.off.data(), widths, heights, c.take.data(), channels, n, tolerance, boxes_out);
    std::vector<uint64_t> packed;
    for (int64_t lo = 0; lo < n;) {
        const uint8_t *d_px = nullptr;
        int rc = KE_OK;
        const int64_t hi = stage_chunk(ctx, pixels, c.off, widths, heights, c.take, channels, lo, n, packed, &d_px, &rc);
        KE_TRY(rc);
        KE_TRY(boxes_on_device(ctx, d_px, packed.data(), widths + lo, heights + lo, c.take.data() + lo, channels, hi - lo, tolerance, boxes_out + 4 * lo));
        lo = hi;
    }
    return KE_OK;
}

KE_API int ke_crop_pack(ke_ctx *ctx, const uint8_t *src, const uint64_t *src_offsets, const int32_t *widths, const int32_t *heights,
                        int32_t channels, const int32_t *boxes, int64_t n, uint8_t *dst, const uint64_t *dst_offsets) {
    if (!ctx) return KE_EINVAL;
    if (n < 0 || (n > 0 && (!src || !src_offsets || !widths || !heights || !boxes || !dst || !dst_offsets))) return ke_fail(ctx, KE_EINVAL, "NULL argument");
    if (channels != 1 && channels != 3 && channels != 4) return ke_fail(ctx, KE_EINVAL, "channels must be 1, 3 or 4 (got %d)", channels);
    if (n == 0) return KE_OK;
    if (!ke_is_device_ptr(src) || !ke_is_device_ptr(dst)) return ke_fail(ctx, KE_EINVAL, "src and dst are device memory");
    KE_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<CropJob> jobs((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t *b = boxes + 4 * i;
        if (!shape_ok(widths[i], heights[i], channels) || b[0] < 0 || b[1] < 0 || b[2] <= b[0] || b[3] <= b[1] || b[2] > widths[i] || b[3] > heights[i])
            return ke_fail(ctx, KE_EINVAL, "image %lld: %dx%d, box (%d, %d, %d, %d)", (long long)i, widths[i], heights[i], b[0], b[1], b[2], b[3]);
        jobs[(size_t)i] = CropJob{src_offsets[i], dst_offsets[i], widths[i], heights[i], b[0], b[1], b[2] - b[0], b[3] - b[1]};
    }
    return launch_crop_pack(ctx, src, jobs, channels, dst);
}

int ke_launch_crop_luma(ke_ctx *ctx, const uint8_t *d_src, const KeCropLumaJob *jobs, int64_t n, uint8_t *d_dst) {
    if (n == 0) return KE_OK;
    int most = 1;
    for (int64_t i = 0; i < n; ++i) most = std::max(most, jobs[i].bh);
    void *d_jobs;
    KE_TRY(ke_reserve(ctx, KE_BUF_META, (size_t)n * sizeof(KeCropLumaJob), &d_jobs));
    KE_HIP(ctx, hipMemcpyAsync(d_jobs, jobs, (size_t)n * sizeof(KeCropLumaJob), hipMemcpyHostToDevice, ctx->stream));
    // a wave takes eight rows or more of the tallest box: a row costs it CH dwords in for one out, and the job record and the
    // row set-up are paid once per wave
    const unsigned gx = (unsigned)std::min(std::max((most + 31) / 32, 1), 256);
    ke_time_begin(ctx, KE_T_TRIM_LUMA);
    for (int64_t first = 0; first < n; first += 65535) {
        const unsigned gy = (unsigned)std::min<int64_t>(65535, n - first);
        hipLaunchKernelGGL(ke_crop_luma_kernel, dim3(gx, gy), dim3(256), 0, ctx->stream, d_src, (const KeCropLumaJob *)d_jobs, first, d_dst);
    }
    ke_time_end(ctx, KE_T_TRIM_LUMA);
    KE_HIP(ctx, hipGetLastError());
    KE_HIP(ctx, hipStreamSynchronize(ctx->stream));       // `jobs` is the caller's host array
    return KE_OK;
}

KE_API int ke_crop_luma(ke_ctx *ctx, const uint8_t *src, const uint64_t *src_offsets, const int32_t *widths, const int32_t *heights,
                        const int32_t *channels, const int32_t *boxes, int64_t n, uint8_t *dst, const uint64_t *dst_offsets) {
    if (!ctx) return KE_EINVAL;
    if (n < 0 || (n > 0 && (!src || !src_offsets || !widths || !heights || !channels || !boxes || !dst || !dst_offsets)))
        return ke_fail(ctx, KE_EINVAL, "NULL argument");
    if (n == 0) return KE_OK;
    if (!ke_is_device_ptr(src) || !ke_is_device_ptr(dst)) return ke_fail(ctx, KE_EINVAL, "src and dst are device memory");
    KE_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<KeCropLumaJob> jobs((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t *b = boxes + 4 * i;
        const int ch = channels[i];
        if ((ch != 1 && ch != 3 && ch != 4) || !shape_ok(widths[i], heights[i], ch) || !box_inside(b, widths[i], heights[i]))
            return ke_fail(ctx, KE_EINVAL, "image %lld: %dx%d, %d channels, box (%d, %d, %d, %d)", (long long)i, widths[i], heights[i], ch, b[0],
                           b[1], b[2], b[3]);
        jobs[(size_t)i] = KeCropLumaJob{src_offsets[i], dst_offsets[i], widths[i], heights[i], ch, b[0], b[1], b[2] - b[0], b[3] - b[1]};
    }
    return ke_launch_crop_luma(ctx, src, jobs.data(), n, dst);
}

KE_API int ke_hash_images_trimmed(ke_ctx *ctx, const uint8_t *pixels, const uint64_t *offsets, const int32_t *widths, const int32_t *heights,
                                  int32_t channels, int64_t n, int32_t tolerance, uint64_t *phash_out, int32_t *boxes_out, uint8_t *has_out,
                                  int32_t *status_out) {
    if (!ctx) return KE_EINVAL;
    if (n > 0 && (!phash_out || !boxes_out || !has_out || !status_out || ke_is_device_ptr(phash_out) || ke_is_device_ptr(boxes_out) ||
                  ke_is_device_ptr(has_out)))
        return ke_fail(ctx, KE_EINVAL, "phash_out/boxes_out/has_out/status_out must be host arrays");
    TrimCall c;
    KE_TRY(check_images(ctx, pixels, offsets, widths, heights, channels, n, tolerance, status_out, c));
    if (n == 0) return KE_OK;
    KE_HIP(ctx, hipSetDevice(ctx->device));
    if (ke_is_device_ptr(pixels))
        return trimmed_on_device(ctx, pixels, c.off.data(), widths, heights, c.take.data(), channels, n, tolerance, phash_out, boxes_out, has_out,
                                 status_out);
    std::vector<uint64_t> packed;
    for (int64_t lo = 0; lo < n;) {
        const uint8_t *d_px = nullptr;
        int rc = KE_OK;
        const int64_t hi = stage_chunk(ctx, pixels, c.off, widths, heights, c.take, channels, lo, n, packed, &d_px, &rc);
        KE_TRY(rc);
        KE_TRY(trimmed_on_device(ctx, d_px, packed.data(), widths + lo, heights + lo, c.take.data() + lo, channels, hi - lo, tolerance,
                                 phash_out + lo, boxes_out + 4 * lo, has_out + lo, status_out + lo));
        lo = hi;
    }
    return KE_OK;
}

// One resident chunk of ke_hash_images_turned_trimmed: the turned hashes of the pictures as they lie, then boxes and the turned
// hashes of the qualifying crops.  `w` and `h` hold zeros for the images the box pass does not take, so neither pass reads them.
static int turned_trimmed_on_device(ke_ctx *ctx, const uint8_t *d_px, const uint64_t *off, const int32_t *w, const int32_t *h, const uint8_t *take,
                                    int ch, int64_t n, int tol, uint64_t *turned, uint64_t *trimmed_turned, int32_t *boxes, uint8_t *has,
                                    int32_t *status) {
    std::vector<int32_t> st((size_t)n);
    KE_TRY(ke_hash_images_turned(ctx, d_px, off, w, h, ch, n, turned, st.data()));
    for (int64_t i = 0; i < n; ++i)
        if (take[i] && st[(size_t)i] != KE_IMG_OK) status[i] = st[(size_t)i];
    return trimmed_on_device(ctx, d_px, off, w, h, take, ch, n, tol, nullptr, boxes, has, status, trimmed_turned);
}

KE_API int ke_hash_images_turned_trimmed(ke_ctx *ctx, const uint8_t *pixels, const uint64_t *offsets, const int32_t *widths, const int32_t *heights,
                                         int32_t channels, int64_t n, int32_t tolerance, uint64_t *turned_out, uint64_t *trimmed_turned_out,
                                         int32_t *boxes_out, uint8_t *has_out, int32_t *status_out) {
    if (!ctx) return KE_EINVAL;
    if (n > 0 && (!turned_out || !trimmed_turned_out || !boxes_out || !has_out || !status_out || ke_is_device_ptr(turned_out) ||
                  ke_is_device_ptr(trimmed_turned_out) || ke_is_device_ptr(boxes_out) || ke_is_device_ptr(has_out)))
        return ke_fail(ctx, KE_EINVAL, "turned_out/trimmed_turned_out/boxes_out/has_out/status_out must be host arrays");
    TrimCall c;
    KE_TRY(check_images(ctx, pixels, offsets, widths, heights, channels, n, tolerance, status_out, c));
    if (n == 0) return KE_OK;
    KE_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> w(widths, widths + n), h(heights, heights + n);
    for (int64_t i = 0; i < n; ++i)
        if (!c.take[(size_t)i]) w[(size_t)i] = h[(size_t)i] = 0;
    if (ke_is_device_ptr(pixels))
        return turned_trimmed_on_device(ctx, pixels, c.off.data(), w.data(), h.data(), c.take.data(), channels, n, tolerance, turned_out,
                                        trimmed_turned_out, boxes_out, has_out, status_out);
    // host pixels: a chunk is staged once and both passes walk it where it lies
    std::vector<uint64_t> packed;
    for (int64_t lo = 0; lo < n;) {
        const uint8_t *d_px = nullptr;
        int rc = KE_OK;
        const int64_t hi = stage_chunk(ctx, pixels, c.off, widths, heights, c.take, channels, lo, n, packed, &d_px, &rc);
        KE_TRY(rc);
        KE_TRY(turned_trimmed_on_device(ctx, d_px, packed.data(), w.data() + lo, h.data() + lo, c.take.data() + lo, channels, hi - lo, tolerance,
                                        turned_out + 8 * lo, trimmed_turned_out + 8 * lo, boxes_out + 4 * lo, has_out + lo, status_out + lo));
        lo = hi;
    }
    return KE_OK;
}
