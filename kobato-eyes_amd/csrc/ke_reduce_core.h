// ke_reduce_core.h -- Pillow's Image.reduce((fx, fy)) for 8-bit pixels (libImaging/Reduce.c), shared by the HIP kernel
// (ke_normalise.hip, ke_reduce_rgb) and by the CPU build the tests hold against Pillow.  The reference's loader reaches it
// through Image.thumbnail's reducing_gap (src/utils/image_io.py:122-124): an image more than four times the target is first
// averaged over fx x fy cells, then resampled.
//
// Every output sample is the mean of its cell in Pillow's fixed point: (sum + n / 2) * floor(2^24 / n) >> 24, n = the pixels
// the cell holds -- fx * fy inside the image, fewer in the partial last column and row (ImagingReduceCorners), which are
// averaged over what they have.  Reduce.c's special cases (1x2, 2x2, 4x4: a shift) give the same values: 2^24 / n is exact
// for a power of two.  The product stays below 2^32 for any n (255.5 * 2^24).
#pragma once

#include <stdint.h>

#include "ke_jpeg_core.h"      // KE_HD

KE_HD int ke_reduced_side(int side, int f) { return (side + f - 1) / f; }

// output pixel (ox, oy) of a width x height image of packed RGB bytes: the cell is walked once for the three channels
KE_HD void ke_reduce_rgb_pixel(const uint8_t *src, int width, int height, int fx, int fy, int ox, int oy, uint8_t *rgb) {
    const int x0 = ox * fx, y0 = oy * fy;
    const int x1 = x0 + fx < width ? x0 + fx : width, y1 = y0 + fy < height ? y0 + fy : height;
    uint32_t r = 0, g = 0, b = 0;
    for (int y = y0; y < y1; ++y) {
        const uint8_t *p = src + ((int64_t)y * width + x0) * 3;
        for (int x = x0; x < x1; ++x, p += 3) { r += p[0]; g += p[1]; b += p[2]; }
    }
    const uint32_t n = (uint32_t)(x1 - x0) * (uint32_t)(y1 - y0), mult = (1u << 24) / n, amend = n / 2;
    rgb[0] = (uint8_t)(((r + amend) * mult) >> 24);
    rgb[1] = (uint8_t)(((g + amend) * mult) >> 24);
    rgb[2] = (uint8_t)(((b + amend) * mult) >> 24);
}
