// ke_webp_launch.h -- the lossy WebP decoder's per-image record and the launch of its token and reconstruction kernels
// (ke_webp.hip), for the translation units that decode a VP8 key frame: ke_webp.hip itself and ke_webpa.hip (the same frame
// beside an alpha plane).  The kernels stay where they are; what goes out is the planes in the scratch.
#pragma once

#include "ke_internal.h"
#include "ke_webp_parse.h"

struct KeWebpDev {
    KeWebpHeader h;
    uint64_t file_off;     // the file inside the uploaded bytes
    uint64_t scratch_off;  // coefficients (768 B per macroblock) | planes (384 B) | mode records (20 B), inside the scratch
    uint64_t out_off;      // bytes into the caller's pixel buffer
};

// Scratch of one frame, 16-aligned: 1 172 B per macroblock.
static inline uint64_t ke_webp_frame_scratch(const KeWebpHeader &h) {
    return ((uint64_t)h.mb_w * h.mb_h * (768 + 384 + sizeof(KeWebpMb)) + 15) & ~15ull;
}

// Where the finished Y / U / V planes of a frame lie inside its scratch: Y at nmb * 768, U behind its nmb * 256 bytes, V
// behind U's nmb * 64.
KE_HD const uint8_t *ke_webp_frame_planes(const KeWebpDev &d, const uint8_t *scratch) {
    return scratch + d.scratch_off + (size_t)d.h.mb_w * d.h.mb_h * 768;
}

// ke_webp_tokens_k (one lane per image, status per image) and ke_webp_recon_k (one wave per image) on ctx->stream over the
// m records at d_imgs.  Returns KE_OK; launch errors are the caller's to collect (hipGetLastError).
int ke_webp_launch_frames(ke_ctx *ctx, const KeWebpDev *d_imgs, int64_t m, const uint8_t *d_files, uint8_t *d_scratch, int32_t *d_status);
