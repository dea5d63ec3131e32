// _jpeg_scaled_cpu.cpp -- TEST INFRASTRUCTURE: the reduced-size JPEG decode (ke_jpeg_core.h: ke_jpeg_scaled_geometry, the
// reduced transforms, ke_upsample_scaled_at) and Image.reduce (ke_reduce_core.h) -- the very headers the HIP kernels compile --
// driven sequentially on the CPU, so that tests/test_jpeg_scaled_cpu.py can hold them against the installed Pillow without a
// GPU.  With -DJSC_MAIN the file is a program of its own: it reads the cases the test wrote (files with Pillow's pixels) and
// compares -- the form the sanitised run takes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ke_jpeg_parse.h"
#include "ke_reduce_core.h"

namespace {

struct TableReader {       // the reader of ke_prog_*: Huffman symbols through the parsed look-up tables
    KeBits &b;
    const KeJpegTables &tables;
    const int32_t *ids;
    int sym(int slot) { return ke_huff_decode(b, tables.pool[(size_t)ids[slot]]); }
    uint32_t bits(int k) {
        ke_bits_fill(b);
        const uint32_t v = ke_bits_peek(b, k);
        ke_bits_skip(b, k);
        return v;
    }
    int bit() { return (int)bits(1); }
};

// every block's coefficients (int16, natural order, not dequantised) into coef[c]: blocks of the padded planes
int entropy(const uint8_t *file, const KeJpegTables &tables, const KeJpegInfo &info, const std::vector<KeJpegScan> &scans,
            std::vector<int16_t> *coef) {
    if (!info.progressive) {
        KeBits bits;
        ke_bits_init(bits, file, info.scan_offset, info.scan_end);
        int pred[3] = {0, 0, 0};
        int32_t blk[64];
        const uint16_t ones[64] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                   1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
        int restart_left = info.restart_interval;
        for (int my = 0; my < info.mcus_y; ++my)
            for (int mx = 0; mx < info.mcus_x; ++mx) {
                if (info.restart_interval && restart_left == 0) {
                    if (ke_bits_restart(bits) != KE_JPEG_OK) return KE_JPEG_CORRUPT;
                    pred[0] = pred[1] = pred[2] = 0;
                    restart_left = info.restart_interval;
                }
                for (int c = 0; c < info.ncomp; ++c)
                    for (int by = 0; by < info.vs[c]; ++by)
                        for (int bx = 0; bx < info.hs[c]; ++bx) {
                            if (ke_decode_block(bits, tables.pool[(size_t)info.huff_dc[c]], tables.pool[(size_t)info.huff_ac[c]], ones, kKeZigzag,
                                                pred[c], blk) != KE_JPEG_OK)
                                return KE_JPEG_CORRUPT;
                            int16_t *dst = coef[c].data() + ((size_t)(my * info.vs[c] + by) * (info.plane_w[c] >> 3) + (mx * info.hs[c] + bx)) * 64;
                            for (int k = 0; k < 64; ++k) dst[k] = (int16_t)blk[k];
                        }
                --restart_left;
            }
        return ke_bits_ran_dry(bits) ? KE_JPEG_CORRUPT : KE_JPEG_OK;
    }
    for (int si = 0; si < info.nscans; ++si) {
        const KeJpegScan &sc = scans[info.first_scan + (size_t)si];
        KeBits bits;
        ke_bits_init(bits, file, sc.offset, sc.end);
        TableReader rd{bits, tables, sc.ss == 0 ? sc.dc_tab : sc.ac_tab};
        int pred[3] = {0, 0, 0};
        uint32_t eobrun = 0;
        int restart_left = sc.restart_interval;
        auto block = [&](int k, int c, int brow, int bcol) -> int {
            int16_t *blk = coef[c].data() + ((size_t)brow * (info.plane_w[c] >> 3) + bcol) * 64;
            if (sc.ss == 0) {
                if (sc.ah == 0) {
                    int v;
                    if (ke_prog_dc_first(rd, k, pred[k], sc.al, &v) != KE_JPEG_OK) return KE_JPEG_CORRUPT;
                    blk[0] = (int16_t)v;
                } else if (rd.bit()) {
                    blk[0] = (int16_t)(blk[0] | (1 << sc.al));
                }
                return KE_JPEG_OK;
            }
            return sc.ah == 0 ? ke_prog_ac_first(rd, k, blk, kKeZigzag, sc.ss, sc.se, sc.al, eobrun)
                              : ke_prog_ac_refine(rd, k, blk, kKeZigzag, sc.ss, sc.se, sc.al, eobrun);
        };
        auto restart = [&]() -> int {
            if (sc.restart_interval && restart_left == 0) {
                if (ke_bits_restart(bits) != KE_JPEG_OK) return KE_JPEG_CORRUPT;
                pred[0] = pred[1] = pred[2] = 0;
                eobrun = 0;
                restart_left = sc.restart_interval;
            }
            return KE_JPEG_OK;
        };
        if (sc.ncomp > 1) {
            for (int my = 0; my < info.mcus_y; ++my)
                for (int mx = 0; mx < info.mcus_x; ++mx) {
                    if (restart() != KE_JPEG_OK) return KE_JPEG_CORRUPT;
                    for (int k = 0; k < sc.ncomp; ++k) {
                        const int c = sc.comp[k];
                        for (int by = 0; by < info.vs[c]; ++by)
                            for (int bx = 0; bx < info.hs[c]; ++bx)
                                if (block(k, c, my * info.vs[c] + by, mx * info.hs[c] + bx) != KE_JPEG_OK) return KE_JPEG_CORRUPT;
                    }
                    --restart_left;
                }
        } else {
            const int c = sc.comp[0], bw = (info.comp_w[c] + 7) >> 3, bh = (info.comp_h[c] + 7) >> 3;
            for (int brow = 0; brow < bh; ++brow)
                for (int bcol = 0; bcol < bw; ++bcol) {
                    if (restart() != KE_JPEG_OK) return KE_JPEG_CORRUPT;
                    if (block(0, c, brow, bcol) != KE_JPEG_OK) return KE_JPEG_CORRUPT;
                    --restart_left;
                }
        }
        if (ke_bits_ran_dry(bits)) return KE_JPEG_CORRUPT;
    }
    return KE_JPEG_OK;
}

}  // namespace

extern "C" {

// info: status, width, height, components
void jsc_probe(const uint8_t *file, uint64_t size, int32_t *info4) {
    KeJpegTables tables;
    KeJpegInfo info;
    ke_parse_jpeg(file, (size_t)size, tables, info, false);
    info4[0] = info.status; info4[1] = info.width; info4[2] = info.height; info4[3] = info.ncomp;
}

// the file at 1 / denom into out (ceil(h / denom) x ceil(w / denom) x components bytes, packed); returns KE_JPEG_*
int jsc_decode(const uint8_t *file, uint64_t size, int denom, uint8_t *out) {
    if (denom != 1 && denom != 2 && denom != 4 && denom != 8) return -1;
    KeJpegTables tables;
    KeJpegInfo info;
    std::vector<KeJpegScan> scans;
    ke_parse_jpeg(file, (size_t)size, tables, info, true, &scans);
    if (info.status != KE_JPEG_OK) return info.status;
    std::vector<int16_t> coef[3];
    for (int c = 0; c < info.ncomp; ++c) coef[c].assign((size_t)info.plane_w[c] * info.plane_h[c], 0);
    if (entropy(file, tables, info, scans, coef) != KE_JPEG_OK) return KE_JPEG_CORRUPT;
    KeJpegScaled g;
    ke_jpeg_scaled_geometry(info, denom, g);
    bool narrow = true;
    std::vector<uint8_t> planes[3];
    for (int c = 0; c < info.ncomp; ++c) {
        const int bpr = info.plane_w[c] >> 3, rows = info.plane_h[c] >> 3, ss = g.ss[c];
        planes[c].assign((size_t)g.plane_w[c] * rows * ss, 0);
        for (int brow = 0; brow < rows; ++brow)
            for (int bcol = 0; bcol < bpr; ++bcol) {
                int32_t blk[64];
                const int16_t *src = coef[c].data() + ((size_t)brow * bpr + bcol) * 64;
                for (int k = 0; k < 64; ++k) blk[k] = (int32_t)src[k] * (int32_t)info.quant[c][k];
                narrow &= ke_idct_scaled(blk, ss, planes[c].data() + (size_t)brow * ss * g.plane_w[c] + (size_t)bcol * ss, g.plane_w[c]);
            }
    }
    if (!narrow) return KE_JPEG_UNSUPPORTED;
    for (int y = 0; y < g.out_h; ++y)
        for (int x = 0; x < g.out_w; ++x) {
            const int Y = planes[0][(size_t)y * g.plane_w[0] + x];
            if (info.ncomp == 1) { out[(size_t)y * g.out_w + x] = (uint8_t)Y; continue; }
            const int cb = ke_upsample_scaled_at(planes[1].data(), g.plane_w[1], g.comp_w[1], g.comp_h[1], g.hfac[1], g.vfac[1], g.fancy, x, y);
            const int cr = ke_upsample_scaled_at(planes[2].data(), g.plane_w[2], g.comp_w[2], g.comp_h[2], g.hfac[2], g.vfac[2], g.fancy, x, y);
            ke_ycc_to_rgb(Y, cb, cr, out + ((size_t)y * g.out_w + x) * 3);
        }
    return KE_JPEG_OK;
}

// Image.reduce((fx, fy)) of width x height packed RGB bytes into dst (ceil(height / fy) x ceil(width / fx) x 3)
void jsc_reduce(const uint8_t *src, int width, int height, int fx, int fy, uint8_t *dst) {
    const int ow = ke_reduced_side(width, fx), oh = ke_reduced_side(height, fy);
    for (int y = 0; y < oh; ++y)
        for (int x = 0; x < ow; ++x) ke_reduce_rgb_pixel(src, width, height, fx, fy, x, y, dst + ((size_t)y * ow + x) * 3);
}

}  // extern "C"

#ifdef JSC_MAIN
// The cases file: records of seven little-endian u32 (kind, a, b, c, d, input bytes, expected bytes) followed by the input
// and the expected bytes.  kind 1: a JPEG file decoded at 1 / a (expected = Pillow's pixels, or none where b, the expected
// status, is not 0); kind 2: a x b RGB bytes reduced by (c, d).  Exit status 0 = every case as expected.
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t head[7];
    long cases = 0, bad = 0;
    while (std::fread(head, 4, 7, f) == 7) {
        // exactly the bytes a case has, so that a read or write beyond them is one the sanitiser sees
        std::vector<uint8_t> in(head[5]), want(head[6]);
        if ((head[5] && std::fread(in.data(), 1, head[5], f) != head[5]) || (head[6] && std::fread(want.data(), 1, head[6], f) != head[6])) return 2;
        ++cases;
        if (head[0] == 1) {
            int32_t info[4];
            jsc_probe(in.data(), in.size(), info);
            if (info[0] != KE_JPEG_OK) { bad += head[2] == 0; continue; }
            const size_t bytes = (size_t)ke_jpeg_scaled_side(info[1], (int)head[1]) * ke_jpeg_scaled_side(info[2], (int)head[1]) * info[3];
            std::vector<uint8_t> got(bytes);
            const int st = jsc_decode(in.data(), in.size(), (int)head[1], got.data());
            if (st != (int)head[2] || (st == 0 && (bytes != want.size() || std::memcmp(got.data(), want.data(), bytes) != 0))) {
                std::fprintf(stderr, "case %ld: decode at 1/%u differs (status %d)\n", cases, head[1], st);
                ++bad;
            }
        } else if (head[0] == 2) {
            const size_t bytes = (size_t)ke_reduced_side((int)head[1], (int)head[3]) * ke_reduced_side((int)head[2], (int)head[4]) * 3;
            std::vector<uint8_t> got(bytes);
            jsc_reduce(in.data(), (int)head[1], (int)head[2], (int)head[3], (int)head[4], got.data());
            if (bytes != want.size() || std::memcmp(got.data(), want.data(), bytes) != 0) {
                std::fprintf(stderr, "case %ld: reduce %ux%u by (%u, %u) differs\n", cases, head[1], head[2], head[3], head[4]);
                ++bad;
            }
        } else {
            return 2;
        }
    }
    std::fclose(f);
    std::printf("%ld cases, %ld differ\n", cases, bad);
    return bad ? 1 : (cases ? 0 : 2);
}
#endif
