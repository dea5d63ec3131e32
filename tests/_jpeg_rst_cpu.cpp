// The restart-interval split (csrc/ke_jpeg_restarts.h) without a GPU: for every file of a manifest -- lines of
// "<path> <min MCUs per lane> <expected verdict>" -- the program parses the file (ke_jpeg_parse.h), walks the whole
// entropy-coded segment with ke_decode_block as ke_jpeg_entropy does, builds the marker index and the plan, walks the segment
// again lane by lane as ke_jpeg_entropy_rst does, and compares every coefficient and the status.  Verdicts: split, numbers,
// few, many (ke_rst_index's reasons), one_lane (the plan does not split), refused (the parser's).  Then the plan arithmetic,
// exhaustively.  Built with -fsanitize=address,undefined by tests/test_jpeg_restarts_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ke_jpeg_parse.h"
#include "ke_jpeg_restarts.h"

static int g_failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            if (++g_failures > 20) std::exit(1);          \
        }                                                 \
    } while (0)

// MCUs [mcu_first, mcu_last) from `start` with the reader ending at `end`: the loop of the kernels.  Blocks go to
// coefs[(block index) * 64 ..], component after component, rows of plane_w / 8 blocks.
static int walk(const uint8_t *p, const KeJpegInfo &in, const KeJpegTables &tables, uint32_t mcu_first, uint32_t mcu_last, uint32_t start,
                uint32_t end, uint32_t next_rst, std::vector<int32_t> &coefs) {
    KeBits bits;
    ke_bits_init(bits, p, start, end);
    bits.next_rst = (int32_t)next_rst;
    size_t block_base[3] = {0, 0, 0};
    for (int c = 1; c < in.ncomp; ++c) block_base[c] = block_base[c - 1] + (size_t)(in.plane_w[c - 1] >> 3) * (in.plane_h[c - 1] >> 3);
    int pred[3] = {0, 0, 0};
    int restart_left = in.restart_interval;
    for (uint32_t m = mcu_first; m < mcu_last; ++m) {
        const int my = (int)(m / (uint32_t)in.mcus_x), mx = (int)(m % (uint32_t)in.mcus_x);
        if (in.restart_interval && restart_left == 0) {
            if (ke_bits_restart(bits) != KE_JPEG_OK) return KE_JPEG_CORRUPT;
            pred[0] = pred[1] = pred[2] = 0;
            restart_left = in.restart_interval;
        }
        for (int c = 0; c < in.ncomp; ++c)
            for (int by = 0; by < in.vs[c]; ++by)
                for (int bx = 0; bx < in.hs[c]; ++bx) {
                    const size_t b = block_base[c] + (size_t)(my * in.vs[c] + by) * (size_t)(in.plane_w[c] >> 3) + (size_t)(mx * in.hs[c] + bx);
                    int32_t *blk = coefs.data() + b * 64;
                    if (ke_decode_block(bits, tables.pool[(size_t)in.huff_dc[c]], tables.pool[(size_t)in.huff_ac[c]], in.quant[c], kKeZigzag, pred[c], blk) !=
                        KE_JPEG_OK)
                        return KE_JPEG_CORRUPT;
                }
        --restart_left;
    }
    return ke_bits_ran_dry(bits) ? KE_JPEG_CORRUPT : KE_JPEG_OK;
}

static const char *kWhy[4] = {"split", "numbers", "few", "many"};

static void one_file(const std::string &path, uint32_t min_mcus, const std::string &expected) {
    std::ifstream f(path, std::ios::binary);
    std::vector<uint8_t> data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    CHECK(!data.empty(), "%s: cannot read", path.c_str());
    const size_t size = data.size();
    data.resize(size + 256, 0xA5);                               // the slack the device buffer has (nothing here may depend on it)
    KeJpegTables tables;
    KeJpegInfo in;
    ke_parse_jpeg(data.data(), size, tables, in);
    if (in.status != KE_JPEG_OK || in.progressive) {
        CHECK(expected == "refused", "%s: refused by the parser (status %d), expected %s", path.c_str(), in.status, expected.c_str());
        std::printf("%s refused\n", path.c_str());
        return;
    }
    const uint32_t mcus = (uint32_t)in.mcus_x * (uint32_t)in.mcus_y, ri = (uint32_t)in.restart_interval;
    size_t blocks = 0;
    for (int c = 0; c < in.ncomp; ++c) blocks += (size_t)(in.plane_w[c] >> 3) * (in.plane_h[c] >> 3);
    std::vector<int32_t> whole(blocks * 64, 0x7FFFFFFF), lanes(blocks * 64, 0x7FFFFFFE);
    const int st_whole = walk(data.data(), in, tables, 0, mcus, in.scan_offset, in.scan_end, 0, whole);
    const KeRstPlan plan = ke_rst_plan(mcus, ri, min_mcus, KE_RST_LANE_CAP);
    CHECK(plan.n_int == (ri ? (mcus + ri - 1) / ri : 1), "%s: n_int", path.c_str());
    if (!ke_rst_plan_splits(plan)) {
        CHECK(expected == "one_lane", "%s: the plan has one lane, expected %s", path.c_str(), expected.c_str());
        std::printf("%s one_lane status=%d\n", path.c_str(), st_whole);
        return;
    }
    std::vector<uint32_t> lane_start(plan.n_lanes, 0xFFFFFFFFu);
    int why = -1;
    const bool split = ke_rst_index(data.data(), in.scan_offset, in.scan_end, plan, lane_start.data(), &why);
    CHECK(why >= 0 && why <= 3 && split == (why == 0), "%s: why %d", path.c_str(), why);
    CHECK(expected == kWhy[why & 3], "%s: verdict %s, expected %s", path.c_str(), kWhy[why & 3], expected.c_str());
    if (!split) {
        std::printf("%s %s status=%d\n", path.c_str(), kWhy[why & 3], st_whole);
        return;
    }
    int st_lanes = KE_JPEG_OK;
    uint32_t covered = 0;
    for (uint32_t j = 0; j < plan.n_lanes; ++j) {
        const KeRstLane ln = ke_rst_lane(plan, mcus, ri, j);
        CHECK(ln.mcu_first == covered && ln.mcu_last > ln.mcu_first, "%s: lane %u covers [%u, %u) behind %u", path.c_str(), j, ln.mcu_first, ln.mcu_last, covered);
        covered = ln.mcu_last;
        if (j > 0) CHECK(lane_start[j] != 0xFFFFFFFFu && data[lane_start[j]] == 0xFF && data[lane_start[j] + 1] == 0xD0 + ((ln.int_first - 1) & 7),
                         "%s: lane %u starts behind no marker", path.c_str(), j);
        const uint32_t start = j == 0 ? in.scan_offset : lane_start[j] + 2;
        const uint32_t end = j + 1 == plan.n_lanes ? in.scan_end : lane_start[j + 1];
        CHECK(start <= end && end <= in.scan_end, "%s: lane %u bytes [%u, %u)", path.c_str(), j, start, end);
        if (walk(data.data(), in, tables, ln.mcu_first, ln.mcu_last, start, end, ln.next_rst, lanes) != KE_JPEG_OK) st_lanes = KE_JPEG_CORRUPT;
    }
    CHECK(covered == mcus, "%s: lanes cover %u of %u MCUs", path.c_str(), covered, mcus);
    CHECK(st_lanes == st_whole, "%s: status %d lane by lane, %d in one walk", path.c_str(), st_lanes, st_whole);
    if (st_whole == KE_JPEG_OK && st_lanes == KE_JPEG_OK) {
        size_t differ = 0;
        for (size_t k = 0; k < whole.size(); ++k) differ += whole[k] != lanes[k];
        CHECK(differ == 0, "%s: %zu coefficients differ", path.c_str(), differ);
    }
    std::printf("%s split lanes=%u status=%d\n", path.c_str(), plan.n_lanes, st_whole);
}

static long plan_arithmetic() {
    long plans = 0;
    const uint32_t cap = 5;
    std::vector<int> seen;
    for (uint32_t mcus = 1; mcus <= 300; ++mcus)
        for (uint32_t ri = 1; ri <= mcus + 1; ++ri)
            for (uint32_t min_mcus : {1u, 2u, 7u, 64u}) {
                const KeRstPlan p = ke_rst_plan(mcus, ri, min_mcus, cap);
                ++plans;
                const uint32_t n_int = (mcus + ri - 1) / ri;
                CHECK(p.n_int == n_int && p.g >= 1 && p.g <= n_int && p.n_lanes == (n_int + p.g - 1) / p.g && p.n_lanes >= 1 && p.n_lanes <= cap,
                      "plan mcus=%u ri=%u min=%u: n_int %u g %u lanes %u", mcus, ri, min_mcus, p.n_int, p.g, p.n_lanes);
                // g is the smallest: every smaller count gives a lane too few MCUs or the file too many lanes
                for (uint32_t s = 1; s < p.g; ++s)
                    CHECK((uint64_t)s * ri < min_mcus || (n_int + s - 1) / s > cap, "plan mcus=%u ri=%u min=%u: g %u, but %u would do", mcus, ri, min_mcus, p.g, s);
                // unless one lane has everything, every lane but the last has the minimum
                if (p.n_lanes > 1) CHECK((uint64_t)p.g * ri >= min_mcus || p.g == n_int, "plan mcus=%u ri=%u min=%u: lanes of %u MCUs", mcus, ri, min_mcus, p.g * ri);
                seen.assign(mcus, 0);
                for (uint32_t j = 0; j < p.n_lanes; ++j) {
                    const KeRstLane ln = ke_rst_lane(p, mcus, ri, j);
                    CHECK(ln.int_first == j * p.g && ln.int_last == (ln.int_first + p.g < n_int ? ln.int_first + p.g : n_int) && ln.int_first < ln.int_last,
                          "lane mcus=%u ri=%u min=%u j=%u: intervals [%u, %u)", mcus, ri, min_mcus, j, ln.int_first, ln.int_last);
                    CHECK(ln.next_rst == (ln.int_first & 7), "lane mcus=%u ri=%u min=%u j=%u: next_rst %u", mcus, ri, min_mcus, j, ln.next_rst);
                    CHECK(ln.mcu_first == ln.int_first * ri && ln.mcu_last <= mcus && ln.mcu_first < ln.mcu_last, "lane mcus=%u ri=%u min=%u j=%u: MCUs [%u, %u)", mcus,
                          ri, min_mcus, j, ln.mcu_first, ln.mcu_last);
                    if (j > 0) CHECK(ln.start_marker == ln.int_first - 1, "lane j=%u: start marker %u", j, ln.start_marker);
                    if (j + 1 < p.n_lanes) CHECK(ln.end_marker == ln.int_last - 1 && ln.end_marker < n_int - 1, "lane j=%u: end marker %u", j, ln.end_marker);
                    for (uint32_t m = ln.mcu_first; m < ln.mcu_last && m < mcus; ++m) ++seen[m];
                }
                bool once = true;
                for (uint32_t m = 0; m < mcus; ++m) once = once && seen[m] == 1;
                CHECK(once, "plan mcus=%u ri=%u min=%u: the lanes do not tile [0, mcus)", mcus, ri, min_mcus);
            }
    // no DRI, and the sizes of a 65 500 x 65 500 file with an interval of 1: no overflow, the cap holds
    const KeRstPlan none = ke_rst_plan(1000, 0, 64, KE_RST_LANE_CAP);
    CHECK(none.n_lanes == 1 && !ke_rst_plan_splits(none), "no DRI: %u lanes", none.n_lanes);
    const uint32_t huge = 8188u * 8188u;
    const KeRstPlan big = ke_rst_plan(huge, 1, 64, KE_RST_LANE_CAP);
    CHECK(big.n_int == huge && big.n_lanes <= KE_RST_LANE_CAP && (uint64_t)big.g * big.n_lanes >= huge, "huge: g %u lanes %u", big.g, big.n_lanes);
    const KeRstLane last = ke_rst_lane(big, huge, 1, big.n_lanes - 1);
    CHECK(last.mcu_last == huge && last.mcu_first < huge, "huge: last lane [%u, %u)", last.mcu_first, last.mcu_last);
    const KeRstPlan wide = ke_rst_plan(huge, 65535, 64, KE_RST_LANE_CAP);
    CHECK(wide.g == 1 && wide.n_lanes == wide.n_int && ke_rst_lane(wide, huge, 65535, wide.n_lanes - 1).mcu_last == huge, "wide: g %u", wide.g);
    return plans;
}

int main(int argc, char **argv) {
    long files = 0;
    if (argc > 1) {
        std::ifstream manifest(argv[1]);
        std::string line;
        while (std::getline(manifest, line)) {
            std::istringstream ls(line);
            std::string path, expected;
            uint32_t min_mcus = 0;
            if (!(ls >> path >> min_mcus >> expected)) continue;
            one_file(path, min_mcus, expected);
            ++files;
        }
    }
    const long plans = plan_arithmetic();
    if (g_failures) return 1;
    std::printf("ok files=%ld plans=%ld\n", files, plans);
    return 0;
}
