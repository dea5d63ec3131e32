// ke_view_core.h -- a view of a picture: box (x0, y0, x0 + bw, y0 + bh) of it, then orientation k of that crop
// (turned.turn(k, image[y0:y1, x0:x1])), as coordinate arithmetic.  Shared by the HIP kernel (ke_turn.hip, ke_crop_turn_luma)
// and by the host build the tests hold against NumPy (tests/_view_core_cpu.cpp).
//
// Everything about the turn is ke_turn_core.h's, applied to the bw x bh crop; what this header adds is the addressing: a
// destination tile's source rectangle is moved by the box's origin, and the bytes of its rows are found with the IMAGE's
// pitch w * ch, not the box's.  The order is crop, then turn: the destination is bw x bh, sides swapped for k & 4.
#pragma once

#include <stddef.h>

#include "ke_turn_core.h"

struct KeViewBox {
    int x0, y0, bw, bh;   // inside its image, bw and bh > 0
};

// size of orientation k of the box
KE_TURN_HD void ke_view_dst_size(int k, KeViewBox b, int *dw, int *dh) { ke_turn_dst_size(k, b.bw, b.bh, dw, dh); }

// destination pixel (x, y) of the dw x dh view <- pixel (*sx, *sy) of the IMAGE
KE_TURN_HD void ke_view_src_xy(int k, KeViewBox b, int dw, int dh, int x, int y, int *sx, int *sy) {
    ke_turn_src_xy(k, dw, dh, x, y, sx, sy);
    *sx += b.x0;
    *sy += b.y0;
}

// the other way: pixel (sx, sy) of the image, inside the box -> destination pixel (*x, *y)
KE_TURN_HD void ke_view_dst_xy(int k, KeViewBox b, int dw, int dh, int sx, int sy, int *x, int *y) {
    ke_turn_dst_xy(k, dw, dh, sx - b.x0, sy - b.y0, x, y);
}

// the pixels of the IMAGE a destination rectangle is made of: ke_turn_src_rect's rectangle of the crop, moved by the box's
// origin.  The destination's tiles cover the box exactly once and nothing beside it.
KE_TURN_HD KeTurnRect ke_view_src_rect(int k, KeViewBox b, int dw, int dh, KeTurnRect d) {
    KeTurnRect s = ke_turn_src_rect(k, dw, dh, d);
    s.x0 += b.x0;
    s.y0 += b.y0;
    return s;
}

// byte of pixel (sx, sy) of a w-wide image of ch channels, from the image's first byte
KE_TURN_HD size_t ke_view_px_byte(int w, int ch, int sx, int sy) { return ((size_t)sy * (size_t)w + (size_t)sx) * (size_t)ch; }

// The dwords phase A of the kernel reads for one source row of a tile: `row` is the byte (from the image's first byte) of the
// row's first pixel, `base_mod4` the image's own address mod 4.  *lead: bytes between the aligned dword below the row's first
// byte and that byte; the return value counts the dwords from there that hold the row's pixels * ch bytes.
KE_TURN_HD int ke_view_row_dwords(size_t row, int base_mod4, int pixels, int ch, int *lead) {
    *lead = (int)((row + (size_t)base_mod4) & 3);
    return (*lead + pixels * ch + 3) >> 2;
}
