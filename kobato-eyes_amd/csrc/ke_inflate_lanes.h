// ke_inflate_lanes.h -- ke_inflate_zlib (ke_png_core.h) on the GPU, one stream per lane: the three policies it is written against
// and the gather in front of them, shared by the two decoders whose files hold zlib streams -- PNG (ke_png.hip: one stream per
// image, its IDAT payloads) and deflate TIFF (ke_tiffz.hip: one stream per strip).
//
//   ke_png_gather    pieces of the uploaded files -> contiguous, 16-byte aligned streams (LdsStream reads whole 16-byte chunks)
//   LdsStream        Src: the compressed bytes through a 64-byte ring per lane in LDS, topped up at wave-uniform moments
//   RecSink          Sink: literals to their final place, four at a time; a copy only recorded for ke_lz_make_copies
//   Oct, LaneTab     Tab: limits and bases in registers, the symbols in per-lane slices of LDS, a header's code lengths in HBM
// LDS per wave of 64 streams: 288 + 32 bytes of symbols, 9 + 16 dwords of high bits and ring per lane = 26 880 bytes.
#pragma once

#include "ke_lz_copies.h"

namespace {

struct KePngPiece {        // part of one IDAT payload: bytes [src, src + len) of the uploaded files -> [dst, dst + len) of the streams
    uint64_t src, dst;
    uint32_t len, pad;
};

__global__ __launch_bounds__(256) void ke_png_gather(const KePngPiece *__restrict__ pieces, const uint8_t *__restrict__ files,
                                                     uint8_t *__restrict__ streams) {
    const KePngPiece pc = pieces[blockIdx.x];
    const uint8_t *src = files + pc.src;
    uint8_t *dst = streams + pc.dst;
    const uint32_t head = (uint32_t)((16 - (pc.dst & 15)) & 15);      // bytes up to the first aligned 16 of the destination
    if (threadIdx.x < head && threadIdx.x < pc.len) dst[threadIdx.x] = src[threadIdx.x];
    if (pc.len <= head) return;
    const uint32_t body = (pc.len - head) >> 4, tail0 = head + (body << 4);
    for (uint32_t k = threadIdx.x; k < body; k += 256) *reinterpret_cast<u32x4 *>(dst + head + 16 * k) = ld16(src + head + 16 * k);
    if (tail0 + threadIdx.x < pc.len) dst[tail0 + threadIdx.x] = src[tail0 + threadIdx.x];
}

// ---- inflate: the three policies of ke_inflate_zlib on the GPU

// The compressed bytes through a 64-byte ring per lane in LDS.  Waiting for a load stalls all 64 lanes, so inside the symbol
// loop the ring is topped up at wave-uniform moments (every 16th symbol): what was asked for 16 symbols ago is written to the
// ring, what has been consumed since is asked for, and nobody waits for memory that is still on its way.  Outside that loop
// (headers) and for a lane that outruns its ring the same two steps run back to back.
struct LdsStream {
    const u32x4 *z;        // global: this image's zlib stream (16-byte aligned)
    uint32_t *win;         // dword j of the ring at win[64 * (j & 15)]
    uint32_t nchunk;       // 16-byte chunks that hold stream data
    uint32_t avail, req;   // dwords landed in the ring / asked for (multiples of 4, avail <= req <= avail + 16)
    uint32_t t;
    u32x4 nx0, nx1, nx2, nx3;
    __device__ __forceinline__ void land1(int c, u32x4 v) {
        if (avail + 4 * c < req) {
            uint32_t *slot = win + 64 * ((avail + 4 * c) & 15);
            slot[0] = v.x; slot[64] = v.y; slot[128] = v.z; slot[192] = v.w;
        }
    }
    __device__ __forceinline__ void land() {
        land1(0, nx0); land1(1, nx1); land1(2, nx2); land1(3, nx3);
        avail = req;
    }
    __device__ __forceinline__ void ask1(uint32_t limit, u32x4 &v) {
        if (req + 4 <= limit) {
            const uint32_t chunk = req >> 2;
            v = chunk < nchunk ? z[chunk] : u32x4{0, 0, 0, 0};
            req += 4;
        }
    }
    __device__ __forceinline__ void ask(uint32_t next) {       // `next`: the reader's next dword; everything before its chunk is free
        const uint32_t limit = (next & ~3u) + 16;
        ask1(limit, nx0); ask1(limit, nx1); ask1(limit, nx2); ask1(limit, nx3);
    }
    __device__ __forceinline__ uint32_t word(uint32_t k) {
        if (k >= avail) {
            land();
            if (k >= avail) { ask(k); land(); }
        }
        return win[64 * (k & 15)];
    }
    __device__ __forceinline__ void tick(uint32_t next) {
        ++t;
        if ((__builtin_amdgcn_readfirstlane(t) & 15) == 0) { land(); ask(next); }
    }
};

// Literals go to their final place in HBM, four at a time; an LZ77 copy is only written down -- (destination, distance,
// length) -- and its bytes are left open: reading the source back here would stall the wave once per match, so ke_png_matches
// fills the copies in afterwards with a whole wave per image.  A dword that straddles the edge of a copy is written with
// zeros on the copy's side; the copy overwrites them later.
struct RecSink {
    uint8_t *p;
    uint32_t n, w;
    uint2 *rec;
    uint32_t nrec;
    int hold;           // streams that must wait with a match before the wave turns to the matches (matches_now)
    __device__ __forceinline__ uint32_t size() const { return n; }
    __device__ __forceinline__ void put(uint8_t b) {
        w |= (uint32_t)b << (8 * (n & 3));
        ++n;
        if ((n & 3) == 0) { *reinterpret_cast<uint32_t *>(p + n - 4) = w; w = 0; }
    }
    __device__ __forceinline__ void settle() {
        if (n & 3) *reinterpret_cast<uint32_t *>(p + (n & ~3u)) = w;
        w = 0;
    }
    __device__ __forceinline__ void finish() { settle(); }
    // ke_inflate_zlib's question once per turn: finish the held matches now?  Yes when `hold` streams wait with one, or all
    // that are still inside the symbol loop (the others would only watch).
    __device__ __forceinline__ bool matches_now(bool waiting) const {
        const int waiters = __popcll(__ballot(waiting)), inside = __popcll(__ballot(true));
        return waiters >= min(hold, inside);
    }
    __device__ __forceinline__ void copy(uint32_t dist, uint32_t len) {
        settle();
        rec[nrec++] = make_uint2(n, (dist << 9) | (len - 3));
        n += len;
    }
};

// eight table words held as named values (arrays indexed in loops end up in scratch memory before they are unrolled)
struct Oct {
    uint32_t a0, a1, a2, a3, a4, a5, a6, a7;
    __device__ __forceinline__ uint32_t get(int k) const {
        // each value through an empty asm: otherwise the selects below are folded into one load at a selected address and
        // the table stays in scratch memory for good
        uint32_t b0 = a0, b1 = a1, b2 = a2, b3 = a3, b4 = a4, b5 = a5, b6 = a6, b7 = a7;
        asm("" : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7));
        uint32_t r = b0;
        r = k == 1 ? b1 : r; r = k == 2 ? b2 : r; r = k == 3 ? b3 : r; r = k == 4 ? b4 : r;
        r = k == 5 ? b5 : r; r = k == 6 ? b6 : r; r = k == 7 ? b7 : r;
        return r;
    }
    __device__ __forceinline__ void set(int k, uint32_t v) {
        a0 = k == 0 ? v : a0; a1 = k == 1 ? v : a1; a2 = k == 2 ? v : a2; a3 = k == 3 ? v : a3;
        a4 = k == 4 ? v : a4; a5 = k == 5 ? v : a5; a6 = k == 6 ? v : a6; a7 = k == 7 ? v : a7;
    }
};

struct LaneTab {           // limits and bases in registers, the symbols in this lane's slices of LDS, a header's code lengths in HBM
    Oct lim0, lim1, base0, base1;
    uint8_t *lsym_;        // low 8 bits of literal/length symbol i at lsym_[64 * i]
    uint32_t *lhigh_;      // bit 8 of symbol i: bit (i & 31) of lhigh_[64 * (i >> 5)]
    uint8_t *dsym_;        // distance symbol i at dsym_[64 * i]
    uint32_t *nib_;
    __device__ __forceinline__ uint32_t lim2(int which, int k) const { return which ? lim1.get(k) : lim0.get(k); }
    __device__ __forceinline__ void set_lim2(int which, int k, uint32_t v) { if (which) lim1.set(k, v); else lim0.set(k, v); }
    __device__ __forceinline__ uint32_t base2(int which, int k) const { return which ? base1.get(k) : base0.get(k); }
    __device__ __forceinline__ void set_base2(int which, int k, uint32_t v) { if (which) base1.set(k, v); else base0.set(k, v); }
    __device__ __forceinline__ uint32_t sym(int which, uint32_t i) const {
        if (which) return dsym_[64 * (i & 31)];
        i = i < 288 ? i : 0;
        return (uint32_t)lsym_[64 * i] | (((lhigh_[64 * (i >> 5)] >> (i & 31)) & 1u) << 8);
    }
    __device__ __forceinline__ void clear_syms(int which) {
        if (!which)
            for (int k = 0; k < 9; ++k) lhigh_[64 * k] = 0;
    }
    __device__ __forceinline__ void set_sym(int which, uint32_t i, uint32_t s) {
        if (which) { dsym_[64 * (i & 31)] = (uint8_t)s; return; }
        i = i < 288 ? i : 0;
        lsym_[64 * i] = (uint8_t)s;
        if (s & 256u) lhigh_[64 * (i >> 5)] |= 1u << (i & 31);
    }
    __device__ __forceinline__ uint32_t nibword(int k) const { return nib_[k]; }
    __device__ __forceinline__ void set_nibword(int k, uint32_t v) { nib_[k] = v; }
};

}  // namespace
