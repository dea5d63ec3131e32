// ke_lz_window.h -- what a lane that walks an LZW stream on its own needs besides the arithmetic (ke_gif.hip, ke_tiffc.hip): the
// stream's bytes through a 16-byte register window that is refilled one step ahead, and the dictionary -- 4 096 x {where the
// string was last written, how long it is} -- as a slice of HBM per lane.
#pragma once

#include <stdint.h>

#include "ke_lz_copies.h"

struct WindowSrc {                                // the file's bytes at ascending positions, 16 at a time, the next 16 on their way
    const uint8_t *file;
    uint32_t base, limit;                         // window = [base, base + 16); nothing is read at or beyond `limit`
    uint64_t lo, hi, nlo, nhi;
    __device__ __forceinline__ void load(uint32_t at, uint64_t &a, uint64_t &b) const {
        a = b = 0;
        if (at < limit) {                         // the uploaded files end with slack: 16 bytes from a position inside are there
            const u32x4 v = ld16(file + at);
            a = (uint64_t)v.x | ((uint64_t)v.y << 32);
            b = (uint64_t)v.z | ((uint64_t)v.w << 32);
        }
    }
    __device__ __forceinline__ void start(uint32_t at) {
        base = at;
        load(at, lo, hi);
        load(at + 16, nlo, nhi);
    }
    __device__ __forceinline__ uint32_t byte(uint32_t pos) {
        if (pos >= base + 16) {                   // positions ascend by one: the next window, and the one after it requested
            base += 16;
            lo = nlo; hi = nhi;
            load(base + 16, nlo, nhi);
        }
        const uint32_t k = pos - base;
        return (uint32_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 255ull);
    }
};

struct HbmDict {
    uint2 *e;
    __device__ __forceinline__ void set(uint32_t code, uint32_t pos, uint32_t len) { e[code] = make_uint2(pos, len); }
    __device__ __forceinline__ void get(uint32_t code, uint32_t &pos, uint32_t &len) const {
        const uint2 v = e[code];
        pos = v.x; len = v.y;
    }
};
