// csrc/ke_view_core.h without a GPU: the coordinate map of a view (a box of an image, then one of the eight orientations of that
// crop), driven by host loops.  tests/test_view_core_cpu.py builds this file as a shared object (the vc_* functions, held against
// turned.turn of the oracle's cropped luma) and, with -fsanitize=address,undefined, as a program: `main` runs the same sweep
// against a crop and a turn spelled out here from the definition, with every buffer exactly as large as its picture.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ke_view_core.h"

namespace {
constexpr int kRawPitch = 4 * KE_TURN_TILE + 4;   // ke_turn.hip's: a source row of a tile at 4 channels, and its lead
}

extern "C" {

int vc_tile() { return KE_TURN_TILE; }

void vc_dst_size(int k, int bw, int bh, int *dw, int *dh) { ke_view_dst_size(k, KeViewBox{0, 0, bw, bh}, dw, dh); }

// destination pixel by destination pixel, as a gather: dst[y][x] = luma(src[sy][sx]), (sx, sy) in the image
void vc_view_luma(const uint8_t *src, int w, int h, int ch, int x0, int y0, int bw, int bh, int k, uint8_t *dst) {
    (void)h;
    const KeViewBox box{x0, y0, bw, bh};
    int dw, dh;
    ke_view_dst_size(k, box, &dw, &dh);
    for (int y = 0; y < dh; ++y)
        for (int x = 0; x < dw; ++x) {
            int sx, sy;
            ke_view_src_xy(k, box, dw, dh, x, y, &sx, &sy);
            dst[(size_t)y * dw + x] = (uint8_t)ke_turn_luma_px(src + ke_view_px_byte(w, ch, sx, sy), ch);
        }
}

// Tile by tile as the kernel walks.  Phase A: a tile's source rectangle row by row with the image's pitch, every row read as
// the dwords ke_view_row_dwords counts from the aligned address below its first byte (`base_mod4`: the image's address mod 4,
// which the caller is free to choose), a byte of a dword taken only where it lies inside the image's w * h * ch bytes.  Phase B:
// luma from that row buffer, scattered to where the pixel lies in the destination.  cover[sy][sx] counts the visits of an image
// pixel.  Returns the number of faults: a source rectangle outside the box, a row that does not fit the kernel's row buffer, a
// pixel that lands outside its tile, a disagreement between the two directions of the map.
int64_t vc_view_luma_tiles(const uint8_t *src, int w, int h, int ch, int x0, int y0, int bw, int bh, int k, int base_mod4, uint8_t *dst,
                           int32_t *cover) {
    const KeViewBox box{x0, y0, bw, bh};
    const int64_t bytes = (int64_t)w * h * ch;
    int dw, dh;
    ke_view_dst_size(k, box, &dw, &dh);
    int64_t faults = 0;
    uint8_t raw[kRawPitch];
    for (int ty = 0; ty < ke_turn_tiles_y(dh); ++ty)
        for (int tx = 0; tx < ke_turn_tiles_x(dw); ++tx) {
            const KeTurnRect d = ke_turn_tile_dst_rect(dw, dh, tx, ty);
            const KeTurnRect s = ke_view_src_rect(k, box, dw, dh, d);
            if (s.x0 < x0 || s.y0 < y0 || s.w < 1 || s.h < 1 || s.x0 + s.w > x0 + bw || s.y0 + s.h > y0 + bh || s.w > KE_TURN_TILE ||
                s.h > KE_TURN_TILE || (int64_t)s.w * s.h != (int64_t)d.w * d.h) {
                ++faults;
                continue;
            }
            for (int ly = 0; ly < s.h; ++ly) {
                const size_t at = ke_view_px_byte(w, ch, s.x0, s.y0 + ly);
                int lead;
                const int ndw = ke_view_row_dwords(at, base_mod4, s.w, ch, &lead);
                if (ndw * 4 > kRawPitch) { ++faults; continue; }
                std::memset(raw, 0, sizeof raw);
                for (int j = 0; j < ndw; ++j)
                    for (int b = 0; b < 4; ++b) {
                        const int64_t p = (int64_t)at - lead + 4 * j + b;
                        if (p >= 0 && p < bytes) raw[4 * j + b] = src[p];
                    }
                for (int lx = 0; lx < s.w; ++lx) {
                    const int sx = s.x0 + lx, sy = s.y0 + ly;
                    int x, y, bx, by;
                    ke_view_dst_xy(k, box, dw, dh, sx, sy, &x, &y);
                    if (x < d.x0 || y < d.y0 || x >= d.x0 + d.w || y >= d.y0 + d.h) { ++faults; continue; }
                    ke_view_src_xy(k, box, dw, dh, x, y, &bx, &by);
                    if (bx != sx || by != sy) ++faults;
                    cover[(size_t)sy * w + sx] += 1;
                    dst[(size_t)y * dw + x] = (uint8_t)ke_turn_luma_px(raw + lead + lx * ch, ch);
                }
            }
        }
    return faults;
}

}  // extern "C"

#ifdef VIEW_CORE_MAIN
// turned.turn from its definition: t = a.T if k & 4; mirror if k & 1; flip if k & 2 -- one step after the other on whole planes
static std::vector<uint8_t> turn_by_definition(const std::vector<uint8_t> &a, int w, int h, int k) {
    std::vector<uint8_t> t = a;
    int tw = w, th = h;
    if (k & 4) {
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) t[(size_t)x * h + y] = a[(size_t)y * w + x];
        tw = h;
        th = w;
    }
    std::vector<uint8_t> u = t;
    if (k & 1)
        for (int y = 0; y < th; ++y)
            for (int x = 0; x < tw; ++x) u[(size_t)y * tw + x] = t[(size_t)y * tw + (tw - 1 - x)];
    t = u;
    if (k & 2)
        for (int y = 0; y < th; ++y)
            for (int x = 0; x < tw; ++x) u[(size_t)y * tw + x] = t[(size_t)(th - 1 - y) * tw + x];
    return u;
}

int main() {
    std::vector<int> sides;
    for (int s = 1; s <= 9; ++s) sides.push_back(s);
    for (int s : {KE_TURN_TILE - 1, KE_TURN_TILE, KE_TURN_TILE + 1, 2 * KE_TURN_TILE + 3}) sides.push_back(s);
    uint32_t state = 12345u;
    int64_t cases = 0;
    for (int bw : sides)
        for (int bh : sides)
            for (int x0 = 0; x0 < 4; ++x0)
                for (int y0 = 0; y0 < 4; ++y0)
                    for (int ch : {1, 3, 4}) {
                        // one to three pixels of margin on the far sides, every count taken in turn
                        const int w = x0 + bw + 1 + (int)(cases / 8 % 3), h = y0 + bh + 1 + (int)(cases / 24 % 3);
                        std::vector<uint8_t> src((size_t)w * h * ch), crop((size_t)bw * bh);
                        for (auto &b : src) { state = state * 1664525u + 1013904223u; b = (uint8_t)(state >> 24); }
                        for (int y = 0; y < bh; ++y)
                            for (int x = 0; x < bw; ++x)
                                crop[(size_t)y * bw + x] = (uint8_t)ke_turn_luma_px(src.data() + ((size_t)(y0 + y) * w + x0 + x) * ch, ch);
                        for (int k = 0; k < 8; ++k) {
                            const std::vector<uint8_t> want = turn_by_definition(crop, bw, bh, k);
                            std::vector<uint8_t> gathered((size_t)bw * bh, 0xAA), scattered((size_t)bw * bh, 0x55);
                            std::vector<int32_t> cover((size_t)w * h, 0);
                            vc_view_luma(src.data(), w, h, ch, x0, y0, bw, bh, k, gathered.data());
                            const int64_t faults = vc_view_luma_tiles(src.data(), w, h, ch, x0, y0, bw, bh, k, (int)(cases % 4), scattered.data(), cover.data());
                            bool once = true;
                            for (int y = 0; y < h; ++y)
                                for (int x = 0; x < w; ++x) {
                                    const bool inside = x >= x0 && x < x0 + bw && y >= y0 && y < y0 + bh;
                                    once = once && cover[(size_t)y * w + x] == (inside ? 1 : 0);
                                }
                            if (faults || !once || gathered != want || scattered != want) {
                                std::printf("FAIL box %dx%d at (%d, %d) of %dx%d ch %d k %d: faults %lld, covered once %d, gather %d, scatter %d\n", bw,
                                            bh, x0, y0, w, h, ch, k, (long long)faults, (int)once, (int)(gathered == want), (int)(scattered == want));
                                return 1;
                            }
                            ++cases;
                        }
                    }
    std::printf("ok %lld\n", (long long)cases);
    return 0;
}
#endif
