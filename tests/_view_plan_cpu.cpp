// csrc/ke_view_plan.h without a GPU: the pair plan of the four SSIM pair calls, from a table of tiny calls.
// tests/test_view_plan_cpu.py builds this file as a shared object (vp_case_* hand the table's calls over, vp_plan runs the header
// on whatever it is given and writes the plan out as a stream of int64 words; the test holds that against a model of the rules
// written in Python) and, with -fsanitize=address,undefined, as a program: `main` plans every call of the table on arrays exactly
// as large as the call says and checks what every plan must satisfy, whatever the rules make of it.
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "ke_view_plan.h"

namespace {

using Box = std::array<int32_t, 4>;
constexpr Box Z{0, 0, 0, 0};

struct Case {
    const char *name;
    std::vector<int32_t> w, h;
    std::vector<uint64_t> off;           // empty: NULL, as the arrays below
    int32_t channels;
    std::vector<int64_t> pa, pb;
    std::vector<Box> ba, bb;
    std::vector<int32_t> ob;
    int64_t bad_pair;                    // -1: the call is planned
    const char *bad_what;                // "box_a", "box_b" or "orientation"
};

// images of most calls: 0 40x30, 1 30x40, 2 0x10 (no image), 3 6x6, 4 and 5 20x7, 6 300x40, 7 64x64
const std::vector<int32_t> W{40, 30, 0, 6, 20, 20, 300, 64}, H{30, 40, 10, 6, 7, 7, 40, 64};

const std::vector<Case> kCases = {
    // all three pointer arrays NULL, images packed back to back: a bad image, a 6x6, indices -1 and n_images, a repeated pair
    {"plain", W, H, {}, 3, {0, 0, 0, -1, 0, 4, 0, 6, 1}, {1, 2, 3, 0, 8, 5, 1, 7, 0}, {}, {}, {}, -1, ""},
    // offsets given, out of order and with gaps; "as it lies" spelt as zeros and as (0, 0, w, h) on side a, as NULL on side b
    {"as it lies on a", W, H, {5000, 100, 7, 9000, 9200, 9400, 20000, 60000}, 1, {0, 0, 1, 4}, {1, 1, 0, 5},
     {Z, {0, 0, 40, 30}, {0, 0, 30, 40}, Z}, {}, {0, 0, 0, 0}, -1, ""},
    // ... and the other way round, no orientations
    {"as it lies on b", W, H, {}, 4, {0, 0, 1, 4}, {1, 1, 0, 5}, {}, {Z, {0, 0, 30, 40}, {0, 0, 40, 30}, Z}, {}, -1, ""},
    // every kind of view
    {"views", W, H, {}, 3,
     {0, 0, 0, 0, 0, 4, 0, 7, 7, 7, 7, 7, 2, 1},
     {1, 1, 1, 1, 1, 5, 1, 6, 6, 6, 6, 6, 0, 0},
     {Z, Z, Z, Z, Z, Z, {0, 0, 6, 30}, Z, Z, Z, Z, Z, {5, 5, 1, 1}, {2, 3, 22, 33}},
     {{2, 3, 22, 33},      // a box at orientation 0: a crop job
      Z,                   // a whole picture at orientation 3: a turn job
      {2, 3, 22, 33},      // a box at orientation 5: a view job, 30 x 20
      {2, 3, 22, 33},      // the same (image, box, orientation) again: no new source
      Z,                   // the image whole and as it lies: a source of its own, not made
      Z,                   // 20x7 against orientation 4 of a 20x7: 7x7, scored
      Z,                   // a's box is 6 wide: too small only after the crop
      {0, 0, 1, 1}, {0, 0, 257, 1}, {0, 0, 15, 17}, {0, 0, 16, 16}, {0, 0, 7, 37},   // areas 1, 257 (too small: no plane), 255, 256, 259 (turned)
      Z,                   // a has no image: its box is not looked at
      {0, 0, 40, 30}},     // image 1 boxed on side a, image 0 whole by its (0, 0, w, h) and turned on side b
     {0, 3, 5, 5, 0, 4, 0, 0, 0, 0, 0, 6, 7, 1}, -1, ""},
    {"empty box", W, H, {}, 3, {0, 0}, {1, 1}, {Z, {4, 0, 4, 30}}, {Z, Z}, {}, 1, "box_a"},
    {"box beyond the image", W, H, {}, 3, {0, 0, 0}, {1, 1, 1}, {}, {Z, Z, {0, 0, 31, 40}}, {0, 1, 4}, 2, "box_b"},
    {"negative origin", W, H, {}, 3, {0}, {1}, {{-1, 0, 40, 30}}, {}, {}, 0, "box_a"},
    {"orientation -1", W, H, {}, 3, {0, 0}, {1, 1}, {}, {}, {7, -1}, 1, "orientation"},
    // validated for every pair, also where an image is missing
    {"orientation 8", W, H, {}, 3, {2, 0}, {1, 1}, {}, {}, {8, 0}, 0, "orientation"},
};

}  // namespace

extern "C" {

int64_t vp_cases() { return (int64_t)kCases.size(); }
const char *vp_case_name(int64_t i) { return kCases[(size_t)i].name; }
const char *vp_case_bad_what(int64_t i) { return kCases[(size_t)i].bad_what; }

// [n_images, offsets given, channels, n_pairs, box_a given, box_b given, orient_b given, bad_pair]
void vp_case_dims(int64_t i, int64_t *out) {
    const Case &c = kCases[(size_t)i];
    const int64_t dims[8] = {(int64_t)c.w.size(), !c.off.empty(), c.channels, (int64_t)c.pa.size(), !c.ba.empty(), !c.bb.empty(), !c.ob.empty(), c.bad_pair};
    std::memcpy(out, dims, sizeof dims);
}

// the arrays of call i, each where it is given
void vp_case_data(int64_t i, int32_t *w, int32_t *h, uint64_t *off, int64_t *pa, int64_t *pb, int32_t *ba, int32_t *bb, int32_t *ob) {
    const Case &c = kCases[(size_t)i];
    std::memcpy(w, c.w.data(), c.w.size() * 4);
    std::memcpy(h, c.h.data(), c.h.size() * 4);
    std::memcpy(pa, c.pa.data(), c.pa.size() * 8);
    std::memcpy(pb, c.pb.data(), c.pb.size() * 8);
    if (!c.off.empty()) std::memcpy(off, c.off.data(), c.off.size() * 8);
    if (!c.ba.empty()) std::memcpy(ba, c.ba.data(), c.ba.size() * 16);
    if (!c.bb.empty()) std::memcpy(bb, c.bb.data(), c.bb.size() * 16);
    if (!c.ob.empty()) std::memcpy(ob, c.ob.data(), c.ob.size() * 4);
}

// The plan of a call as words: [bad_pair, total_bytes, made_bytes | n_srcs, (made, off, w, h) each | a, b of every pair |
// n_crops, 9 fields each | n_turns, 10 each | n_views, 10 each | n_sizes, each: w, h, np, its pairs, n_groups, each group: w, h, made,
// base, m, its sources; then planes and the 2 * np plane indices].  Returns the words written, -1 where `cap` is too small.
int64_t vp_plan(const uint64_t *offsets, const int32_t *widths, const int32_t *heights, int32_t channels, int64_t n_images, const int64_t *pair_a,
                const int64_t *pair_b, int64_t n_pairs, const int32_t *box_a, const int32_t *box_b, const int32_t *orient_b, double *ssim_out,
                int32_t *status_out, int64_t *out, int64_t cap, char *error, int64_t error_cap) {
    const KeViewPlan p = ke_plan_view_pairs(offsets, widths, heights, channels, n_images, pair_a, pair_b, n_pairs, box_a, box_b, orient_b, ssim_out,
                                            status_out);
    std::snprintf(error, (size_t)error_cap, "%s", p.error.c_str());
    std::vector<int64_t> v{p.bad_pair, (int64_t)p.total_bytes, (int64_t)p.made_bytes, (int64_t)p.srcs.size()};
    for (const KePlaneSrc &s : p.srcs) v.insert(v.end(), {s.made, (int64_t)s.off, s.w, s.h});
    for (size_t k = 0; k < p.a.size(); ++k) v.insert(v.end(), {p.a[k], p.b[k]});
    v.push_back((int64_t)p.crops.size());
    for (const KeCropLumaJob &j : p.crops) v.insert(v.end(), {(int64_t)j.src_off, (int64_t)j.dst_off, j.w, j.h, j.channels, j.x0, j.y0, j.bw, j.bh});
    for (const std::vector<KeViewJob> *jobs : {&p.turns, &p.views}) {
        v.push_back((int64_t)jobs->size());
        for (const KeViewJob &j : *jobs)
            v.insert(v.end(), {(int64_t)j.src_off, (int64_t)j.dst_off, j.w, j.h, j.channels, j.orientation, j.x0, j.y0, j.bw, j.bh});
    }
    v.push_back((int64_t)p.sizes.size());
    for (const KeSizePlan &sp : p.sizes) {
        v.insert(v.end(), {sp.w, sp.h, (int64_t)sp.pairs.size()});
        v.insert(v.end(), sp.pairs.begin(), sp.pairs.end());
        v.push_back((int64_t)sp.groups.size());
        for (const KeFitGroup &g : sp.groups) {
            v.insert(v.end(), {g.w, g.h, g.made, g.base, (int64_t)g.srcs.size()});
            v.insert(v.end(), g.srcs.begin(), g.srcs.end());
        }
        v.push_back(sp.planes);
        v.insert(v.end(), sp.idx.begin(), sp.idx.end());
    }
    if ((int64_t)v.size() > cap) return -1;
    std::memcpy(out, v.data(), v.size() * 8);
    return (int64_t)v.size();
}

}  // extern "C"

#ifdef VIEW_PLAN_MAIN
template <class T> static const T *ptr(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }
static const int32_t *ptr(const std::vector<Box> &v) { return v.empty() ? nullptr : v.data()->data(); }

#define CHECK(cond)                                                                         \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            std::printf("FAIL %s: %s (line %d)\n", c.name, #cond, __LINE__);                 \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

int main() {
    int64_t cases = 0;
    for (const Case &c : kCases) {
        const size_t np = c.pa.size();
        std::vector<double> ssim(np, -2.0);
        std::vector<int32_t> status(np, -2);
        const KeViewPlan p = ke_plan_view_pairs(ptr(c.off), c.w.data(), c.h.data(), c.channels, (int64_t)c.w.size(), c.pa.data(), c.pb.data(), (int64_t)np,
                                                ptr(c.ba), ptr(c.bb), ptr(c.ob), ssim.data(), status.data());
        const size_t made = p.crops.size() + p.turns.size() + p.views.size();
        CHECK(p.bad_pair == c.bad_pair);
        if (c.bad_pair >= 0) {               // the error names the pair and what is wrong with it; nothing is planned or written
            CHECK(p.error.find("pair " + std::to_string(c.bad_pair) + ":") != std::string::npos && p.error.find(c.bad_what) != std::string::npos);
            CHECK(p.srcs.empty() && p.sizes.empty() && made == 0 && p.made_bytes == 0);
            for (size_t k = 0; k < np; ++k) CHECK(ssim[k] == -2.0 && status[k] == -2);
            ++cases;
            continue;
        }
        // every pair has a status; the scored ones have two sources and lie in exactly one common size
        std::set<int64_t> scored;
        for (const KeSizePlan &sp : p.sizes)
            for (int64_t k : sp.pairs) CHECK(scored.insert(k).second);
        for (size_t k = 0; k < np; ++k) {
            CHECK(std::isnan(ssim[k]) && status[k] >= KE_PAIR_OK && status[k] <= KE_PAIR_BAD_IMAGE);
            const bool ok = status[k] == KE_PAIR_OK;
            CHECK(ok == (scored.count((int64_t)k) == 1));
            for (int64_t s : {p.a[k], p.b[k]}) CHECK(ok ? (s >= 0 && s < (int64_t)p.srcs.size()) : s == -1);
        }
        // the made planes lie back to back in first-use order, each on a multiple of 256, one job each
        uint64_t at = 0;
        size_t n_made = 0;
        std::set<uint64_t> job_dst;
        for (const KeCropLumaJob &j : p.crops) job_dst.insert(j.dst_off);
        for (const std::vector<KeViewJob> *jobs : {&p.turns, &p.views})
            for (const KeViewJob &j : *jobs) {
                job_dst.insert(j.dst_off);
                CHECK(j.orientation >= 1 && j.orientation <= 7 && j.x0 >= 0 && j.y0 >= 0 && j.bw > 0 && j.bh > 0 && j.x0 + j.bw <= j.w && j.y0 + j.bh <= j.h);
                CHECK((jobs == &p.turns) == (j.x0 == 0 && j.y0 == 0 && j.bw == j.w && j.bh == j.h));
            }
        for (const KePlaneSrc &s : p.srcs) {
            if (!s.made) continue;
            CHECK(s.off == at && s.off % 256 == 0 && job_dst.count(s.off) == 1);
            at += ((uint64_t)s.w * s.h + 255) / 256 * 256;
            ++n_made;
        }
        CHECK(at == p.made_bytes && n_made == made && job_dst.size() == made);
        // a common size's plane stack holds every source of its pairs once, and every pair's planes are its sources'
        for (const KeSizePlan &sp : p.sizes) {
            int64_t base = 0;
            std::vector<int64_t> at_plane;
            for (const KeFitGroup &g : sp.groups) {
                CHECK(g.base == base && !g.srcs.empty());
                base += (int64_t)g.srcs.size();
                for (int64_t s : g.srcs) {
                    const KePlaneSrc &src = p.srcs[(size_t)s];
                    CHECK(src.w == g.w && src.h == g.h && src.made == g.made && src.w >= sp.w && src.h >= sp.h);
                    at_plane.push_back(s);
                }
            }
            CHECK(sp.planes == base && sp.idx.size() == 2 * sp.pairs.size());
            CHECK(std::set<int64_t>(at_plane.begin(), at_plane.end()).size() == at_plane.size());
            for (size_t j = 0; j < sp.pairs.size(); ++j) {
                const int64_t ia = sp.idx[j], ib = sp.idx[sp.pairs.size() + j];
                CHECK(ia >= 0 && ia < sp.planes && ib >= 0 && ib < sp.planes);
                CHECK(at_plane[(size_t)ia] == p.a[(size_t)sp.pairs[j]] && at_plane[(size_t)ib] == p.b[(size_t)sp.pairs[j]]);
            }
        }
        if (std::string(c.name) == "views") CHECK(p.crops.size() == 3 && p.turns.size() == 3 && p.views.size() == 2);
        if (p.sizes.empty() || std::string(c.name) == "plain" || std::string(c.name).find("as it lies") == 0) CHECK(made == 0);
        ++cases;
    }
    std::printf("ok %lld\n", (long long)cases);
    return 0;
}
#endif
