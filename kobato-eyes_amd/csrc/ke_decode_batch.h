// ke_decode_batch.h -- the host side that the twelve ke_<kind>_{probe,caveats,decode} entry points share (keyes.h, "arguments and
// conventions" at ke_jpeg_decode): the argument checks, the per-file loops of probe and caveats, the upload of the files, the
// scratch budget, the row-tile geometry and the loop over sub-batches (ten of them run it: uncompressed BMP and TIFF have no
// scratch).  No kernels; a format supplies its parser, its records, what an image costs and what is launched for a sub-batch.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "ke_internal.h"

// The arguments of ke_<kind>_decode.  KE_OK: go on, unless n == 0 (nothing to do: the caller returns KE_OK).  `parsed_how` is the
// message's subject, e.g. "the files' headers are parsed".  Selects the context's device.
inline int ke_decode_check_args(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                                const uint8_t *pixels_out, const uint64_t *out_offsets, const int32_t *status_out, const char *parsed_how) {
    if (!ctx) return KE_EINVAL;
    if (n < 0 || (n > 0 && (!files || !offsets || !sizes || !pixels_out || !out_offsets || !status_out)))
        return ke_fail(ctx, KE_EINVAL, "NULL argument");
    if (n == 0) return KE_OK;
    if (ke_is_device_ptr(files)) return ke_fail(ctx, KE_EINVAL, "%s on the host: pass host memory (pinned staging is fine)", parsed_how);
    if (!ke_is_device_ptr(pixels_out)) return ke_fail(ctx, KE_EINVAL, "pixels_out must be device memory");
    for (const void *p : {(const void *)offsets, (const void *)sizes, (const void *)out_offsets, (const void *)status_out})
        if (ke_is_device_ptr(p)) return ke_fail(ctx, KE_EINVAL, "offsets/sizes/status are host arrays");
    KE_HIP(ctx, hipSetDevice(ctx->device));
    return KE_OK;
}

// ke_<kind>_probe: parse_one(file, size, width &, height &, channels &, status &) for every file, on the host's threads.
template <typename ParseOne>
int ke_probe_each(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths, int32_t *heights,
                  int32_t *channels, int32_t *status_out, ParseOne parse_one) {
    if (n < 0 || (n > 0 && (!files || !offsets || !sizes || !widths || !heights || !channels || !status_out))) return KE_EINVAL;
    ke_parallel_ranges(n, [=](int64_t lo, int64_t hi, int) {
        for (int64_t i = lo; i < hi; ++i) parse_one(files + offsets[i], (size_t)sizes[i], widths[i], heights[i], channels[i], status_out[i]);
    });
    return KE_OK;
}

// ke_<kind>_caveats: flags_out[i] = flags_of_one(file, size), on the host's threads.
template <typename FlagsOfOne>
int ke_caveats_each(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out, FlagsOfOne flags_of_one) {
    if (n < 0 || (n > 0 && (!files || !offsets || !sizes || !flags_out))) return KE_EINVAL;
    ke_parallel_ranges(n, [=](int64_t lo, int64_t hi, int) {
        for (int64_t i = lo; i < hi; ++i) flags_out[i] = flags_of_one(files + offsets[i], (size_t)sizes[i]);
    });
    return KE_OK;
}

// ke_<kind>_caveats of a format whose accepted files carry nothing the reference's loader would act on.
inline int ke_caveats_none(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out) {
    if (n < 0 || (n > 0 && (!files || !offsets || !sizes || !flags_out))) return KE_EINVAL;
    for (int64_t i = 0; i < n; ++i) flags_out[i] = 0;
    return KE_OK;
}

// keyes.h: host memory handed to a decode call is free again when the call returns -- also when it returns an error after the
// first asynchronous copy, from the caller's files or from a host vector of records, has been queued.  ke_upload_files arms the
// guard; the decoder disarms it on its way out behind the last synchronise, so that success pays for no second one.  Locals go
// in reverse order of declaration: the guard is declared after the host vectors that copies are queued from.
struct KeStreamGuard {
    hipStream_t stream = nullptr;
    bool armed = false;
    KeStreamGuard() = default;
    KeStreamGuard(const KeStreamGuard &) = delete;
    KeStreamGuard &operator=(const KeStreamGuard &) = delete;
    ~KeStreamGuard() {
        if (armed) (void)hipStreamSynchronize(stream);
    }
    void arm(ke_ctx *ctx) { stream = ctx->stream; armed = true; }
    void disarm() { armed = false; }
};

// files[lo, hi) -> buffer `which` (`pad` bytes of slack behind them for the kernels' wide loads), asynchronously.
inline int ke_upload_files(ke_ctx *ctx, KeStreamGuard &guard, const uint8_t *files, uint64_t lo, uint64_t hi, int which, size_t pad,
                           void **d_files) {
    KE_TRY(ke_reserve(ctx, which, (size_t)(hi - lo) + pad, d_files));
    guard.arm(ctx);
    KE_HIP(ctx, hipMemcpyAsync(*d_files, files + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, ctx->stream));
    return KE_OK;
}

// What a sub-batch's scratch may take: half of what the buffers in `held` (the ones the sub-batches regrow) and the free HBM come
// to together -- a sum that does not move when the scratch is regrown, so that consecutive calls cut their batches alike and keep
// their buffers -- within [floor, ceiling].  `env_name` (nullable): a variable for the tests, which want many sub-batches; it can
// only lower the budget (0 = ignored), or it replaces it (at least 1).  Results do not depend on the budget.
enum KeBudgetEnv { KE_BUDGET_ENV_LOWERS, KE_BUDGET_ENV_REPLACES };
inline int ke_scratch_budget(ke_ctx *ctx, std::initializer_list<int> held, uint64_t floor, uint64_t ceiling, const char *env_name,
                             KeBudgetEnv mode, uint64_t *budget) {
    size_t free_b = 0, total_b = 0;
    KE_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    uint64_t have = free_b;
    for (int which : held) have += ctx->buf[which].bytes;
    *budget = std::max<uint64_t>(floor, std::min<uint64_t>(have / 2, ceiling));
    if (const char *e = env_name ? std::getenv(env_name) : nullptr) {
        const uint64_t v = std::strtoull(e, nullptr, 10);
        if (mode == KE_BUDGET_ENV_REPLACES) *budget = std::max<uint64_t>(1, v);
        else if (v > 0) *budget = std::min<uint64_t>(*budget, v);
    }
    return KE_OK;
}

// Row kernels run blockIdx.x = image, blockIdx.y = a band of `rows` rows: at least rows_per_block, more for an image taller than
// 65 535 bands of them.  grid_y covers the tallest image; the blocks beyond a shorter one's rows return at once.
struct KeRowTiles {
    int rows;
    unsigned grid_y;
};
inline KeRowTiles ke_row_tiles(int max_height, int rows_per_block) {
    const int rows = std::max(rows_per_block, (max_height + 65534) / 65535);
    return {rows, (unsigned)((max_height + rows - 1) / rows)};
}

// The accepted images [0, count), in the decoder's order, worked off in sub-batches bounded by its scratch budget:
//   take(k, fresh)            adds image k's records to the sub-batch being packed and returns true, or returns false when
//                             it would exceed the budget.  fresh: k opens a sub-batch -- start from empty, and take it
//                             whatever it costs.
//   launch(m, &d_status, &words)  reserves, uploads the records and enqueues the kernels of the m images packed; names the
//                             device array of `words` status words to bring back.
//   scatter(at, k, m, st)     image `at` was the sub-batch's k-th of m: its status from the words brought back.
// Each sub-batch ends in a synchronise: the records are host vectors and the scratch is reused.  Kernel time: KE_T_JPEG.
template <typename Take, typename Launch, typename Scatter>
int ke_decode_sub_batches(ke_ctx *ctx, size_t count, Take take, Launch launch, Scatter scatter) {
    std::vector<int32_t> st;
    KeStreamGuard guard;                                           // st is written by a queued copy
    guard.arm(ctx);
    ke_time_begin(ctx, KE_T_JPEG);
    ctx->decode_sub_batches = 0;
    for (size_t first = 0, last; first < count; first = last) {
        ++ctx->decode_sub_batches;
        for (last = first; last < count && take(last, last == first); ++last) {}
        const size_t m = last - first;
        const int32_t *d_status = nullptr;
        size_t words = 0;
        KE_TRY(launch(m, &d_status, &words));
        KE_HIP(ctx, hipGetLastError());
        st.resize(words);
        KE_HIP(ctx, hipMemcpyAsync(st.data(), d_status, words * 4, hipMemcpyDeviceToHost, ctx->stream));
        KE_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t k = 0; k < m; ++k) scatter(first + k, k, m, st.data());
    }
    ke_time_end(ctx, KE_T_JPEG);
    guard.disarm();
    return KE_OK;
}
