// ke_webpl_transform.h -- the inverse VP8L transforms as one workgroup undoes them, for the kernels that run them: the lossless
// decoder's (ke_webpl.hip, an image's ARGB) and the alpha decoder's (ke_webpa.hip, the plane of a lossy file coded as a VP8L
// stream).  Last transform first.  Predictor: rows as a skewed wavefront, (x, y) at step x + 2y -- after (x - 1, y) and
// (x + 1, y - 1) --, one lane per row of a step.  Cross-colour and subtract-green: a lane per pixel.  Colour indexing with packed
// pixels: row by row towards the front of the buffer, the packed rows lying behind where their pixels go.
#pragma once

#include "ke_webpl_core.h"

// mem: the stream's decoder memory as ke_vp8l_decode_stream / ke_vp8l_decode_body left it; the finished W x H image ends up at
// its front.  Every thread of the workgroup (kThreads of them) calls this with its index.
template <int kThreads>
__device__ __forceinline__ void ke_vp8l_undo_transforms_wg(uint32_t *mem, const KeVp8lPlan &plan, int W, int H, int tid) {
    uint32_t *pix = mem + plan.pix;
    for (int k = plan.ntrans - 1; k >= 0; --k) {
        const KeVp8lXform t = plan.t[k];
        const int w = t.xsize;
        const uint32_t *data = mem + t.data;
        const size_t count = (size_t)w * H;
        if (t.type == KE_VP8L_PREDICTOR) {
            const int steps = w + 2 * (H - 1);
            for (int s = 0; s < steps; ++s) {
                // pixels (s - 2y, y) of this step: y from max(0, ceil((s - w + 1) / 2)) to min(H - 1, s / 2)
                const int ylo = s - w + 1 > 0 ? (s - w + 2) >> 1 : 0, yhi = min(H - 1, s >> 1);
                for (int y = ylo + tid; y <= yhi; y += kThreads) {
                    const int x = s - 2 * y;
                    uint32_t *p = pix + (size_t)y * w + x;
                    *p = ke_vp8l_add(*p, ke_vp8l_predict(pix, w, x, y, data, t.bits));
                }
                __syncthreads();
            }
        } else if (t.type == KE_VP8L_CROSS_COLOUR) {
            const int sw = ke_vp8l_subsample(w, t.bits);
            for (size_t j = tid; j < count; j += kThreads) {
                const int y = (int)(j / w), x = (int)(j - (size_t)y * w);
                pix[j] = ke_vp8l_cross_colour(pix[j], data[(size_t)(y >> t.bits) * sw + (x >> t.bits)]);
            }
        } else if (t.type == KE_VP8L_SUBTRACT_GREEN) {
            for (size_t j = tid; j < count; j += kThreads) pix[j] = ke_vp8l_add_green(pix[j]);
        } else if (t.bits == 0) {
            for (size_t j = tid; j < count; j += kThreads) pix[j] = data[(pix[j] >> 8) & 255u];
        } else {
            // Pixel x of row y goes to y * w + x and comes from the packed word (W * H - sw * H) + y * sw + (x >> bits), which
            // never lies in front of it: in ascending order, every chunk read before it is written, no word is lost.
            const int sw = ke_vp8l_subsample(w, t.bits);
            uint32_t *wide = mem + ((size_t)W * H - count);
            for (int y = 0; y < H; ++y)
                for (int x0 = 0; x0 < w; x0 += kThreads) {
                    const int x = x0 + tid;
                    uint32_t v = 0;
                    if (x < w) v = ke_vp8l_colour_index(pix + (size_t)y * sw, x, t.bits, data);
                    __syncthreads();
                    if (x < w) wide[(size_t)y * w + x] = v;
                    __syncthreads();
                }
            pix = wide;
        }
        __syncthreads();
    }
}
