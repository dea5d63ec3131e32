// ke_webpa_launch.h -- the alpha plane's per-image record and the launch of its stream, transform and filter kernels
// (ke_webpa.hip), for the translation units that decode an ALPH chunk beside a VP8 key frame: ke_webpa.hip itself and
// ke_webpn.hip (the same pair as the first frame of an animation).  The kernels stay where they are; what goes out is the
// plane where ke_webpa_alpha_at finds it.
#pragma once

#include "ke_internal.h"
#include "ke_webpa_parse.h"

struct KeWebpaDev {
    uint64_t alph_off;       // what follows the ALPH header byte, inside the uploaded bytes
    uint64_t plane_off;      // bytes into the scratch (16-aligned): the stream decoder's memory, or a raw plane's bytes
    uint64_t plane_words;    // ke_webpa_plane_words
    uint64_t out_off;        // bytes into the caller's pixel buffer
    uint32_t alph_size;
    int32_t method, filter;  // KE_ALPH_*, KE_ALPH_FILTER_*
    int32_t width, height;
};

// Where pixel j's alpha byte of a finished plane lies: the file's own bytes (raw, unfiltered), the scratch's bytes (raw,
// filtered), the green bytes of the ARGB words (a method-1 stream); 255 without a plane.
KE_HD uint32_t ke_webpa_alpha_at(const KeWebpaDev &a, const uint8_t *files, const uint8_t *scratch, size_t j) {
    if (a.method == KE_ALPH_RAW) return (a.filter == KE_ALPH_FILTER_NONE ? files + a.alph_off : scratch + a.plane_off)[j];
    if (a.method == KE_ALPH_VP8L) return scratch[a.plane_off + 1 + j * 4];
    return 255u;
}

// ke_webpa_entropy_k (one lane per method-1 plane), ke_webpa_transform_k (one workgroup per method-1 plane) and
// ke_webpa_filter_k (one workgroup per plane; it looks at the frames' statuses too) on ctx->stream over the m records at
// d_planes, of which the m1 named by d_order carry a stream.  max_gradient_height: the tallest gradient-filtered plane's
// height (0: none).  d_status_a: zeroed by the caller.  Returns KE_OK; launch errors are the caller's to collect.
int ke_webpa_launch_planes(ke_ctx *ctx, const KeWebpaDev *d_planes, const int32_t *d_order, int64_t m, int64_t m1, int max_gradient_height,
                           const uint8_t *d_files, uint8_t *d_scratch, KeVp8lPlan *d_plans, const int32_t *d_status_f, int32_t *d_status_a);
