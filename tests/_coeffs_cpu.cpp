// csrc/ke_coeffs.cpp compiled for the CPU with the sanitizers on: what tests/test_coeffs_cpu.py builds and runs.
//   check                       every layout of the tap tables against the plain taps it is built from (see below)
//   dump in out filter in0 in1  the plain taps of one axis: "ksize K", then per output "lo cnt k[0] .. k[cnt-1]"
// check walks filter 0, 1, 2, the (in, out) pairs of kSizes and, per pair, the whole axis and (for in >= 20) two fractional
// source intervals.  Per case: the windows and the packed byte planes of ke_build_axis_coeffs, the chunked layout of
// ke_build_chunked for 1..32 chunks per output, and (out <= 128) the matrix-core operands of ke_build_mx in three settings.
// The planes are read back as signed bytes b0 + 256 b1 + 65536 b2 -- what the kernels' dot products and combine step
// assume -- and compared with kk; nothing here repeats the splitting arithmetic of the file under test.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ke_coeffs.h"

static int failures = 0;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++failures <= 20) {                       \
                std::printf("FAIL %s: ", #cond);          \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

static const int kSizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 5}, {64, 100}, {100, 64}, {640, 128}, {641, 129}, {2340, 130},
                                {4096, 16}, {4000, 300}, {8192, 12}, {8192, 8}, {33, 128}, {257, 256}, {1000, 999},
                                {999, 1000}, {8, 3000}};

static inline int sbyte(int32_t word, int e) { return (int)(int8_t)(((uint32_t)word >> (8 * e)) & 255u); }

// tap weight of output o at input position x, 0 outside the window
static inline int32_t tap_at(const KeAxisCoeffs &c, int o, int x) {
    const int t = x - c.bounds[2 * o];
    return (t >= 0 && t < c.bounds[2 * o + 1]) ? c.kk[(size_t)o * c.ksize + t] : 0;
}

static void check_axis(const KeAxisCoeffs &c, int in, int out, const char *tag) {
    CHECK(c.in_size == in && c.out_size == out, "%s", tag);
    CHECK(c.ksize >= 1 && c.bounds.size() == 2 * (size_t)out && c.kk.size() == (size_t)out * c.ksize, "%s", tag);
    CHECK(c.ndw > 0 && c.ndw % 4 == 0, "%s ndw=%d", tag, c.ndw);
    CHECK(c.start.size() == (size_t)out && c.bias.size() == (size_t)out && c.packed.size() == (size_t)out * c.ndw * 3, "%s", tag);
    if (failures) return;
    int span = 0;
    for (int o = 0; o < out; ++o) {
        const int lo = c.bounds[2 * o], cnt = c.bounds[2 * o + 1], st = c.start[o];
        CHECK(lo >= 0 && cnt >= 1 && cnt <= c.ksize && lo + cnt <= in, "%s o=%d window [%d,+%d)", tag, o, lo, cnt);
        CHECK(st >= 0 && st % 8 == 0 && st <= lo && lo + cnt <= st + 4 * c.ndw, "%s o=%d start=%d lo=%d cnt=%d ndw=%d", tag, o, st, lo, cnt, c.ndw);
        if (st + 4 * c.ndw > span) span = st + 4 * c.ndw;
        int64_t ksum = 0;
        for (int t = 0; t < cnt; ++t) ksum += c.kk[(size_t)o * c.ksize + t];
        CHECK((int64_t)c.bias[o] == 128 * ksum + (1 << 21), "%s o=%d bias=%d ksum=%lld", tag, o, c.bias[o], (long long)ksum);
        for (int j = 0; j < c.ndw; ++j)
            for (int e = 0; e < 4; ++e) {
                const int x = st + 4 * j + e;
                const int32_t *w = &c.packed[((size_t)o * c.ndw + j) * 3];
                const int b0 = sbyte(w[0], e), b1 = sbyte(w[1], e), b2 = sbyte(w[2], e);
                const bool inside = x >= lo && x < lo + cnt;
                CHECK(b0 + 256 * b1 + 65536 * b2 == tap_at(c, o, x), "%s o=%d x=%d planes %d %d %d tap %d", tag, o, x, b0, b1, b2, tap_at(c, o, x));
                CHECK(inside || (b0 == 0 && b1 == 0 && b2 == 0), "%s o=%d x=%d outside the window: %d %d %d", tag, o, x, b0, b1, b2);
            }
    }
    CHECK(c.span == span, "%s span=%d max=%d", tag, c.span, span);
}

static void check_chunked(const KeAxisCoeffs &c, int cpo, const char *tag) {
    KeChunkTable t;
    ke_build_chunked(c, cpo, t, 8);
    const int nv = c.out_size * cpo;
    CHECK(t.cpo == cpo && t.ndwc > 0 && t.ndwc % 8 == 0 && cpo * t.ndwc >= c.ndw, "%s cpo=%d ndwc=%d ndw=%d", tag, cpo, t.ndwc, c.ndw);
    CHECK(t.cstart.size() == (size_t)nv && t.cxor.size() == (size_t)nv && t.cpacked.size() == (size_t)nv * t.ndwc * 3, "%s cpo=%d", tag, cpo);
    if (failures) return;
    int cspan = 0;
    for (int o = 0; o < c.out_size; ++o)
        for (int k = 0; k < cpo; ++k) {
            const int v = o * cpo + k;
            CHECK(t.cstart[v] == c.start[o] + 4 * t.ndwc * k, "%s cpo=%d v=%d cstart=%d", tag, cpo, v, t.cstart[v]);
            CHECK(t.cxor[v] >= 0 && t.cxor[v] <= 3, "%s cpo=%d v=%d cxor=%d", tag, cpo, v, t.cxor[v]);
            if (t.cstart[v] + 4 * t.ndwc > cspan) cspan = t.cstart[v] + 4 * t.ndwc;
            for (int j = 0; j < t.ndwc; ++j) {
                const int src = k * t.ndwc + j;      // the chunks laid end to end are the packed window
                for (int p = 0; p < 3; ++p) {
                    const int32_t want = src < c.ndw ? c.packed[((size_t)o * c.ndw + src) * 3 + p] : 0;
                    CHECK(t.cpacked[((size_t)v * t.ndwc + j) * 3 + p] == want, "%s cpo=%d v=%d j=%d p=%d", tag, cpo, v, j, p);
                }
            }
        }
    CHECK(t.cspan == cspan, "%s cpo=%d cspan=%d max=%d", tag, cpo, t.cspan, cspan);
}

static void check_mx(const KeAxisCoeffs &c, int min_ks, bool align64, const char *tag) {
    KeMxTable t;
    ke_build_mx(c, t, min_ks, align64);
    const int out = c.out_size;
    CHECK(t.tiles == (out + 15) / 16 && t.ks >= 1 && t.ks >= min_ks, "%s mx(%d,%d) tiles=%d ks=%d", tag, min_ks, (int)align64, t.tiles, t.ks);
    CHECK(t.base.size() == (size_t)t.tiles && t.frag.size() == (size_t)t.tiles * t.ks * 3 * 64 * 4, "%s mx(%d,%d)", tag, min_ks, (int)align64);
    if (failures) return;
    for (int j = 0; j < t.tiles; ++j) {
        const int base = t.base[j];
        CHECK(base >= 0 && base % (align64 ? 64 : 16) == 0, "%s mx(%d,%d) tile %d base=%d", tag, min_ks, (int)align64, j, base);
        for (int o = 16 * j; o < 16 * j + 16 && o < out; ++o) {
            const int lo = c.bounds[2 * o], cnt = c.bounds[2 * o + 1];
            CHECK(lo >= base && lo + cnt <= base + 64 * t.ks, "%s mx(%d,%d) o=%d window [%d,+%d) base=%d ks=%d", tag, min_ks, (int)align64, o, lo, cnt, base, t.ks);
        }
        for (int s = 0; s < t.ks; ++s)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 16; ++e) {
                    const int o = 16 * j + (l & 15), x = base + 64 * s + 16 * (l >> 4) + e;
                    int b[3];
                    for (int p = 0; p < 3; ++p) b[p] = sbyte(t.frag[((((size_t)j * t.ks + s) * 3 + p) * 64 + l) * 4 + e / 4], e % 4);
                    const bool inside = o < out && x >= c.bounds[2 * o] && x < c.bounds[2 * o] + c.bounds[2 * o + 1];
                    const int32_t want = inside ? tap_at(c, o, x) : 0;
                    CHECK(b[0] + 256 * b[1] + 65536 * b[2] == want, "%s mx(%d,%d) j=%d s=%d l=%d e=%d planes %d %d %d tap %d", tag, min_ks, (int)align64, j, s, l, e, b[0], b[1], b[2], want);
                    CHECK(inside || (b[0] == 0 && b[1] == 0 && b[2] == 0), "%s mx(%d,%d) j=%d s=%d l=%d e=%d outside", tag, min_ks, (int)align64, j, s, l, e);
                }
    }
}

static int run_check() {
    int cases = 0;
    for (int filter = 0; filter < 3; ++filter)
        for (const auto &sz : kSizes) {
            const int in = sz[0], out = sz[1];
            const float boxes[3][2] = {{0.0f, (float)in}, {1.25f, (float)in - 3.75f}, {0.5f, (float)in / 2 + 0.25f}};
            for (int b = 0; b < (in >= 20 ? 3 : 1); ++b) {
                char tag[96];
                std::snprintf(tag, sizeof tag, "f%d %d->%d box(%g,%g)", filter, in, out, (double)boxes[b][0], (double)boxes[b][1]);
                KeAxisCoeffs c;
                ke_build_axis_coeffs(in, out, c, filter, boxes[b][0], boxes[b][1]);
                check_axis(c, in, out, tag);
                if (!failures)
                    for (int cpo = 1; cpo <= 32; cpo *= 2) check_chunked(c, cpo, tag);
                if (!failures && out <= 128) {
                    check_mx(c, 0, false, tag);
                    check_mx(c, 0, true, tag);
                    check_mx(c, 3, false, tag);
                }
                ++cases;
                if (failures) {
                    std::printf("failed at %s\n", tag);
                    return 1;
                }
            }
        }
    std::printf("ok cases=%d\n", cases);
    return 0;
}

static int run_dump(char **v) {
    const int in = std::atoi(v[0]), out = std::atoi(v[1]), filter = std::atoi(v[2]);
    const float in0 = (float)std::atof(v[3]), in1 = (float)std::atof(v[4]);
    KeAxisCoeffs c;
    ke_build_axis_coeffs(in, out, c, filter, in0, in1);
    std::printf("ksize %d\n", c.ksize);
    for (int o = 0; o < out; ++o) {
        std::printf("%d %d", c.bounds[2 * o], c.bounds[2 * o + 1]);
        for (int t = 0; t < c.bounds[2 * o + 1]; ++t) std::printf(" %d", c.kk[(size_t)o * c.ksize + t]);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "check")) return run_check();
    if (argc == 7 && !std::strcmp(argv[1], "dump")) return run_dump(argv + 2);
    std::fprintf(stderr, "usage: %s check | dump in out filter in0 in1\n", argv[0]);
    return 2;
}
