// ke_tiffc_rows.h -- the last kernel of the decoders of compressed TIFF files (ke_tiffc.hip: LZW and PackBits; ke_tiffz.hip:
// deflate), one for both: from the strips' planes -- a strip's bytes as its stream yields them -- to the caller's pixels.
//
//   ke_tiffc_rows    one wave per row: undoes predictor 2 (a prefix sum per sample modulo 256 over the lanes, 64 pixels a step,
//                    the carry handed on), then ke_tiff_unpack's mapping -- WhiteIsZero and palette files through the table, an
//                    unspecified fourth sample dropped.  Images whose status is not 0 are skipped.
#pragma once

#include "ke_tiffc_core.h"

namespace {

struct KeTiffcImgDev {
    uint64_t out_off;      // bytes into the caller's pixel buffer
    uint64_t plane_off;    // the image's strip planes inside the scratch: strip s at plane_off + s * strip_stride
    uint32_t strip_stride;
    int32_t width, height, spp, channels, mapped, rows_per_strip, predictor;
    uint8_t lut[256];
};

constexpr int kRowsPerBlock = 8;      // at least; more for images taller than 65 535 bands of them

__global__ __launch_bounds__(256) void ke_tiffc_rows(const KeTiffcImgDev *__restrict__ imgs, const uint8_t *__restrict__ planes,
                                                   const int32_t *__restrict__ status, uint8_t *__restrict__ out, int rows) {
    __shared__ uint8_t s_lut[256];
    const KeTiffcImgDev &d = imgs[blockIdx.x];
    const int y0 = blockIdx.y * rows;
    if (status[blockIdx.x] != KE_TIFFC_OK || y0 >= d.height) return;
    s_lut[threadIdx.x] = d.lut[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = d.width, spp = d.spp, ch = d.channels, y1 = min(y0 + rows, d.height);
    const bool mapped = d.mapped != 0;
    for (int y = y0 + wave; y < y1; y += 4) {
        const uint8_t *row = planes + d.plane_off + (size_t)(y / d.rows_per_strip) * d.strip_stride + (size_t)(y % d.rows_per_strip) * W * spp;
        uint8_t *dst = out + d.out_off + (size_t)y * W * ch;
        if (d.predictor != 2) {
            if (spp == ch) {
                const int n = W * ch;
                for (int k = lane; k < n; k += 64) dst[k] = mapped ? s_lut[row[k]] : row[k];
            } else {                                           // four samples stored, three leave
                for (int x = lane; x < W; x += 64) {
                    uint32_t v;
                    __builtin_memcpy(&v, row + 4 * (size_t)x, 4);
                    uint8_t *w = dst + 3 * (size_t)x;
                    w[0] = (uint8_t)v; w[1] = (uint8_t)(v >> 8); w[2] = (uint8_t)(v >> 16);
                }
            }
            continue;
        }
        uint32_t carry = 0;                                    // the pixel in front of this step's first, its samples in the bytes
        for (int x0 = 0; x0 < W; x0 += 64) {
            const int x = x0 + lane;
            uint32_t v = 0;
            if (x < W) {
                const uint8_t *r = row + (size_t)x * spp;
                if (spp == 1) v = r[0];
                else if (spp == 3) v = (uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16);
                else __builtin_memcpy(&v, r, 4);
            }
#pragma unroll
            for (int step = 1; step < 64; step <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)v, step);
                if (lane >= step) v = ke_tiffc_add4(v, t);
            }
            v = ke_tiffc_add4(v, carry);
            carry = (uint32_t)__shfl((int)v, 63);
            if (x < W) {
                if (ch == 1) {
                    dst[x] = mapped ? s_lut[v & 255u] : (uint8_t)v;
                } else if (ch == 3) {
                    uint8_t *w = dst + 3 * (size_t)x;
                    w[0] = (uint8_t)v; w[1] = (uint8_t)(v >> 8); w[2] = (uint8_t)(v >> 16);
                } else {
                    __builtin_memcpy(dst + 4 * (size_t)x, &v, 4);
                }
            }
        }
    }
}

}  // namespace
