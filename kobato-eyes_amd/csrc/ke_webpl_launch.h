// ke_webpl_launch.h -- the lossless WebP decoder's per-image record and the launch of its stream and transform kernels
// (ke_webpl.hip), for the translation units that decode a VP8L image: ke_webpl.hip itself and ke_webpn.hip (the same image as
// the first frame of an animation).  The kernels stay where they are; what goes out is the ARGB words at the front of the
// image's scratch.
#pragma once

#include "ke_internal.h"
#include "ke_webpl_parse.h"

struct KeWebplDev {
    KeWebplHeader h;
    uint64_t file_off;       // the file inside the uploaded bytes
    uint64_t scratch_off;    // bytes into the scratch (16-aligned)
    uint64_t scratch_words;  // ke_vp8l_scratch_words(width, height)
    uint64_t out_off;        // bytes into the caller's pixel buffer
};

// ke_webpl_entropy_k (one lane per image, status and plan per image) and ke_webpl_transform_k (one workgroup per image) on
// ctx->stream over the m records at d_imgs.  Returns KE_OK; launch errors are the caller's to collect (hipGetLastError).
int ke_webpl_launch_images(ke_ctx *ctx, const KeWebplDev *d_imgs, int64_t m, const uint8_t *d_files, uint8_t *d_scratch, KeVp8lPlan *d_plans,
                           int32_t *d_status);
