// csrc/ke_turn_core.h without a GPU: the coordinate map of the eight orientations, the luma and the tiles' source
// rectangles, driven by host loops.  tests/test_turn_core_cpu.py builds this file as a shared object (the tc_* functions,
// held against turned.turn and the oracle's luma) and, with -fsanitize=address,undefined, as a program: `main` runs the same
// sweep against a turn spelled out here from the definition, with every buffer exactly as large as its picture.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ke_turn_core.h"

extern "C" {

int tc_tile() { return KE_TURN_TILE; }

void tc_dst_size(int k, int w, int h, int *dw, int *dh) { ke_turn_dst_size(k, w, h, dw, dh); }

// destination pixel by destination pixel, as a gather: dst[y][x] = luma(src[sy][sx])
void tc_turn_luma(const uint8_t *src, int w, int h, int ch, int k, uint8_t *dst) {
    int dw, dh;
    ke_turn_dst_size(k, w, h, &dw, &dh);
    for (int y = 0; y < dh; ++y)
        for (int x = 0; x < dw; ++x) {
            int sx, sy;
            ke_turn_src_xy(k, dw, dh, x, y, &sx, &sy);
            dst[(size_t)y * dw + x] = (uint8_t)ke_turn_luma_px(src + ((size_t)sy * w + sx) * ch, ch);
        }
}

// tile by tile as the kernel walks: a tile's source rectangle row by row, every source pixel scattered to where it lies in
// the destination.  cover[sy][sx] counts the visits of a source pixel.  Returns the number of faults: a source rectangle
// outside the picture, a source pixel that lands outside its tile, a disagreement between the two directions of the map.
int64_t tc_turn_luma_tiles(const uint8_t *src, int w, int h, int ch, int k, uint8_t *dst, int32_t *cover) {
    int dw, dh;
    ke_turn_dst_size(k, w, h, &dw, &dh);
    int64_t faults = 0;
    for (int ty = 0; ty < ke_turn_tiles_y(dh); ++ty)
        for (int tx = 0; tx < ke_turn_tiles_x(dw); ++tx) {
            const KeTurnRect d = ke_turn_tile_dst_rect(dw, dh, tx, ty);
            const KeTurnRect s = ke_turn_src_rect(k, dw, dh, d);
            if (s.x0 < 0 || s.y0 < 0 || s.w < 1 || s.h < 1 || s.x0 + s.w > w || s.y0 + s.h > h || s.w > KE_TURN_TILE || s.h > KE_TURN_TILE ||
                (int64_t)s.w * s.h != (int64_t)d.w * d.h) {
                ++faults;
                continue;
            }
            for (int ly = 0; ly < s.h; ++ly)
                for (int lx = 0; lx < s.w; ++lx) {
                    const int sx = s.x0 + lx, sy = s.y0 + ly;
                    int x, y, bx, by;
                    ke_turn_dst_xy(k, dw, dh, sx, sy, &x, &y);
                    if (x < d.x0 || y < d.y0 || x >= d.x0 + d.w || y >= d.y0 + d.h) { ++faults; continue; }
                    ke_turn_src_xy(k, dw, dh, x, y, &bx, &by);
                    if (bx != sx || by != sy) ++faults;
                    cover[(size_t)sy * w + sx] += 1;
                    dst[(size_t)y * dw + x] = (uint8_t)ke_turn_luma_px(src + ((size_t)sy * w + sx) * ch, ch);
                }
        }
    return faults;
}

}  // extern "C"

#ifdef TURN_CORE_MAIN
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
    for (int w : sides)
        for (int h : sides)
            for (int ch : {1, 3, 4}) {
                std::vector<uint8_t> src((size_t)w * h * ch), luma((size_t)w * h);
                for (auto &b : src) { state = state * 1664525u + 1013904223u; b = (uint8_t)(state >> 24); }
                for (size_t p = 0; p < luma.size(); ++p) luma[p] = (uint8_t)ke_turn_luma_px(src.data() + p * ch, ch);
                for (int k = 0; k < 8; ++k) {
                    const std::vector<uint8_t> want = turn_by_definition(luma, w, h, k);
                    std::vector<uint8_t> gathered((size_t)w * h, 0xAA), scattered((size_t)w * h, 0x55);
                    std::vector<int32_t> cover((size_t)w * h, 0);
                    tc_turn_luma(src.data(), w, h, ch, k, gathered.data());
                    const int64_t faults = tc_turn_luma_tiles(src.data(), w, h, ch, k, scattered.data(), cover.data());
                    bool once = true;
                    for (int32_t c : cover) once = once && c == 1;
                    if (faults || !once || gathered != want || scattered != want) {
                        std::printf("FAIL %dx%d ch %d k %d: faults %lld, covered once %d, gather %d, scatter %d\n", w, h, ch, k, (long long)faults,
                                    (int)once, (int)(gathered == want), (int)(scattered == want));
                        return 1;
                    }
                    ++cases;
                }
            }
    std::printf("ok %lld\n", (long long)cases);
    return 0;
}
#endif
