// ke_turn_core.h -- the eight orientations of a picture as coordinate arithmetic, shared by the HIP kernel (ke_turn.hip,
// ke_turn_luma) and by the host build the tests hold against turned.turn (tests/_turn_core_cpu.cpp).
//
// Orientation k in 0..7 of a picture a is turned.ORIENTATIONS':  t = a.T if k & 4;  mirror (left <-> right) if k & 1;
// flip (top <-> bottom) if k & 2.  A pure permutation of the pixels, so a per-pixel function such as luma commutes with it.
//
// The kernel works on tiles of the DESTINATION, KE_TURN_TILE on a side.  Since the map is a permutation that sends
// rectangles to rectangles, the source rectangles of the destination's tiles cover every source pixel exactly once.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define KE_TURN_HD __host__ __device__ static inline
#else
#define KE_TURN_HD static inline
#endif

// Side of a destination tile.  64 x 64: the transposing orientations read 64 source rows of 64 pixels for every tile, so
// the source side moves 64 / 192 / 256 contiguous bytes per row and the destination side 64, whichever way the tile lies.
#define KE_TURN_TILE 64

// luma of one pixel: Pillow's convert("L") (ke_hash.hip's luma_of); the fourth channel is ignored
KE_TURN_HD int ke_turn_luma_px(const uint8_t *p, int ch) {
    if (ch == 1) return p[0];
    return (int)((19595u * p[0] + 38470u * p[1] + 7471u * p[2] + 0x8000u) >> 16);
}

// size of orientation k of a w x h picture
KE_TURN_HD void ke_turn_dst_size(int k, int w, int h, int *dw, int *dh) {
    *dw = (k & 4) ? h : w;
    *dh = (k & 4) ? w : h;
}

// destination pixel (x, y) of a dw x dh turned picture <- source pixel (*sx, *sy)
KE_TURN_HD void ke_turn_src_xy(int k, int dw, int dh, int x, int y, int *sx, int *sy) {
    const int mx = (k & 1) ? dw - 1 - x : x, my = (k & 2) ? dh - 1 - y : y;
    *sx = (k & 4) ? my : mx;
    *sy = (k & 4) ? mx : my;
}

// the other way: source pixel (sx, sy) -> destination pixel (*x, *y)
KE_TURN_HD void ke_turn_dst_xy(int k, int dw, int dh, int sx, int sy, int *x, int *y) {
    const int mx = (k & 4) ? sy : sx, my = (k & 4) ? sx : sy;
    *x = (k & 1) ? dw - 1 - mx : mx;
    *y = (k & 2) ? dh - 1 - my : my;
}

KE_TURN_HD int ke_turn_tiles_x(int dw) { return (dw + KE_TURN_TILE - 1) / KE_TURN_TILE; }
KE_TURN_HD int ke_turn_tiles_y(int dh) { return (dh + KE_TURN_TILE - 1) / KE_TURN_TILE; }

struct KeTurnRect {
    int x0, y0, w, h;
};

// tile (tx, ty) of the destination, cut at the picture's edge
KE_TURN_HD KeTurnRect ke_turn_tile_dst_rect(int dw, int dh, int tx, int ty) {
    KeTurnRect r;
    r.x0 = tx * KE_TURN_TILE;
    r.y0 = ty * KE_TURN_TILE;
    r.w = dw - r.x0 < KE_TURN_TILE ? dw - r.x0 : KE_TURN_TILE;
    r.h = dh - r.y0 < KE_TURN_TILE ? dh - r.y0 : KE_TURN_TILE;
    return r;
}

// the source pixels a destination rectangle is made of: a rectangle too
KE_TURN_HD KeTurnRect ke_turn_src_rect(int k, int dw, int dh, KeTurnRect d) {
    const int mx0 = (k & 1) ? dw - d.x0 - d.w : d.x0, my0 = (k & 2) ? dh - d.y0 - d.h : d.y0;
    KeTurnRect s;
    s.x0 = (k & 4) ? my0 : mx0;
    s.y0 = (k & 4) ? mx0 : my0;
    s.w = (k & 4) ? d.h : d.w;
    s.h = (k & 4) ? d.w : d.h;
    return s;
}
