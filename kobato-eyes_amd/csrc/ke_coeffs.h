// ke_coeffs.h -- tap tables of the resampler kernels, built on the host by ke_coeffs.cpp.  Plain C++, no HIP: the host tests
// build ke_coeffs.cpp against this header alone.
#pragma once

#include <cstdint>
#include <map>
#include <vector>

#include "../../include/keyes.h"

// ---------------------------------------------------------------------------------------
// Coefficient tables of one axis.
// plain  : Pillow's own layout, bounds[o] = (first tap, tap count), kk[o][ksize] 22-bit ints.
// packed : the layout the fused kernel eats.  For output o the window starts at byte
//          start[o] (multiple of 8) and spans 4*ndw bytes; tap weight k is split into three
//          balanced signed bytes k = b0 + 256*b1 + 65536*b2, stored per window dword as three
//          packed i8x4 words (one per byte plane) so a v_dot4_i32_i8 against four signed luma
//          bytes (L-128) accumulates each plane; bias[o] = 128*sum(k) + 2^21.
// ---------------------------------------------------------------------------------------
struct KeAxisCoeffs {
    int in_size = 0, out_size = 0;
    int ksize = 0;
    std::vector<int32_t> bounds;  // 2*out
    std::vector<int32_t> kk;      // out*ksize
    int ndw = 0;                  // window dwords (multiple of 4)
    int span = 0;                 // max(start[o] + 4*ndw)
    std::vector<int32_t> start;   // out
    std::vector<int32_t> bias;    // out
    std::vector<int32_t> packed;  // out*ndw*3
    // device copies
    int32_t *d_bounds = nullptr, *d_kk = nullptr, *d_start = nullptr, *d_bias = nullptr, *d_packed = nullptr;
    // chunked byte-plane layouts, by chunks-per-output (see KeChunkTable)
    std::map<int, struct KeChunkTable *> chunked;
    // matrix-core operand layouts of the same byte planes (see KeMxTable), built on first use, by (min_ks, align64)
    std::map<int, struct KeMxTable *> mx;
};

// The tap matrix as B operands of v_mfma_i32_16x16x64_i8: the resample of one axis is the banded product
// out[row][o] = sum_x luma[row][x] * k[o][x]; outputs are taken 16 at a time (tile j = o / 16), the taps of a tile
// live in x in [base[j], base[j] + 64*ks), and step s of tile j, byte plane p is one 64x16 operand whose lane l
// holds the 16 bytes k_p[o = 16j + (l & 15)][x = base[j] + 64s + 16(l >> 4) + 0..15] (zero outside the window
// and for o >= out_size).  frag index: (((j*ks + s)*3 + p)*64 + l)*4 dwords.
struct KeMxTable {
    int tiles = 0, ks = 0;
    std::vector<int32_t> base;   // tiles, multiples of 16
    std::vector<int32_t> frag;
    int32_t *d_frag = nullptr;
};

// Chunked byte-plane layout for long windows: every output's packed window is cut into `cpo` chunks of
// `ndwc` dwords; virtual column v = o*cpo + c starts at cstart[v] and owns cpacked[v][ndwc][3]; the
// chunks' plane sums are added before bias[o] and the clip.
struct KeChunkTable {
    int cpo = 0, ndwc = 0, cspan = 0;
    std::vector<int32_t> cstart, cpacked;
    // cxor[v] in 0..3: lane v visits window dword pair p at physical pair p ^ cxor[v], chosen on the host so
    // that the 32 lanes of a half-wave hit distinct LDS banks with ds_read_b64 (needs ndwc % 8 == 0)
    std::vector<int32_t> cxor;
    int32_t *d_cstart = nullptr, *d_cpacked = nullptr, *d_cxor = nullptr;
};

void ke_build_axis_coeffs(int in_size, int out_size, KeAxisCoeffs &out, int filter, float in0, float in1);
void ke_build_chunked(const KeAxisCoeffs &c, int cpo, KeChunkTable &out, int ndwc_multiple = 4);
void ke_build_mx(const KeAxisCoeffs &c, KeMxTable &out, int min_ks = 0, bool align64 = false);
