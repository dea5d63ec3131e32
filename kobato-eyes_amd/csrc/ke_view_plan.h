// The pair plan of the four SSIM pair calls (ke_ssim_pairs, _turned, _boxed, _viewed): from the host arrays of a call to what
// is made, fitted and scored, as pure functions.  No HIP, no context: ke_api.hip calls the plan, uploads, launches the job
// lists and walks the common sizes; a host-only program can include this file (tests/test_view_plan_cpu.py).
//
// Pair k is view a against view b.  A view is (image, box, orientation): box_a[k] of image pair_a[k] as it lies, orientation
// orient_b[k] of box_b[k] of image pair_b[k] -- crop, then turn.  A NULL box array, four zeros and (0, 0, w, h) all mean the
// image as it lies; a NULL orient_b means 0.  Every distinct view is a plane source, made once, in first-use order: the image
// itself where nothing is cut or turned, else a one-channel plane in the call's scratch, each starting on a multiple of 256.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/keyes.h"

// the luma plane of box (x0, y0, x0 + bw, y0 + bh) of an image, rows packed (ke_trim.hip)
struct KeCropLumaJob {
    uint64_t src_off, dst_off;   // bytes from d_src / d_dst
    int32_t w, h, channels;      // the source image
    int32_t x0, y0, bw, bh;      // the box
};

// the luma plane of orientation `orientation` (0..7, turned.ORIENTATIONS) of box (x0, y0, x0 + bw, y0 + bh) of an image, rows
// packed, bw x bh swapped for orientation & 4 (ke_turn.hip); a whole picture turned is the box (0, 0, w, h)
struct KeViewJob {
    uint64_t src_off, dst_off;   // bytes from d_src / d_dst
    int32_t w, h, channels, orientation;
    int32_t x0, y0, bw, bh;
};

// what the fit step reads
struct KePlaneSrc {
    int made;            // 0: in the call's pixels, at the call's channel count; 1: in the call's scratch, one channel
    uint64_t off;        // bytes into that buffer
    int32_t w, h;
};

// The sources of one common size that share a fit launch.  A launch reads one buffer at one channel count, so a group is
// (source w, source h, made or not).
struct KeFitGroup {
    int w, h, made;
    int64_t base;                     // the group's first plane in the stack of its common size
    std::vector<int64_t> srcs;        // in first-use order
};

// One common size: its pairs, the plane stack their sources are fitted into (the groups in ascending (w, h, made) order) and
// the planes of every pair in it.
struct KeSizePlan {
    int w, h;
    std::vector<int64_t> pairs;       // that are scored at this size, ascending
    std::vector<KeFitGroup> groups;
    int64_t planes = 0;               // in the stack
    std::vector<int64_t> idx;         // [plane of a | plane of b] for `pairs`, in their order
};

struct KeViewPlan {
    std::vector<KePlaneSrc> srcs;
    std::vector<int64_t> a, b;                                          // per pair: its two sources, -1 where it is not scored
    std::vector<KeSizePlan> sizes;                                      // ascending (w, h)
    std::vector<KeCropLumaJob> crops;                                   // a box as it lies
    std::vector<KeViewJob> turns, views;                                // a whole picture turned; a box turned
    uint64_t made_bytes = 0, total_bytes = 0;                           // of the scratch; of the pixels the images span
    int64_t bad_pair = -1;                                              // >= 0: nothing is planned and `error` says why
    std::string error;
};

// offsets (packed back to back where NULL, an invalid image taking no bytes) and the bytes the images span
inline uint64_t ke_image_offsets(const uint64_t *offsets, const int32_t *widths, const int32_t *heights, int channels, int64_t n_images,
                                 std::vector<uint64_t> &off) {
    off.resize((size_t)n_images);
    uint64_t run = 0, total = 0;
    for (int64_t i = 0; i < n_images; ++i) {
        off[i] = offsets ? offsets[i] : run;
        if (widths[i] > 0 && heights[i] > 0) {
            run += (uint64_t)widths[i] * heights[i] * channels;
            total = std::max<uint64_t>(total, off[i] + (uint64_t)widths[i] * heights[i] * channels);
        }
    }
    return total;
}

// The status of pair k of views wa x ha and wb x hb (`ok`: both images exist), NaN as its score for now.  Returns the common
// size where the pair is scored, (0, 0) where it is not.
inline std::pair<int, int> ke_classify_pair(int64_t k, bool ok, int wa, int ha, int wb, int hb, double *ssim_out, int32_t *status_out) {
    ssim_out[k] = std::nan("");
    if (!ok) { if (status_out) status_out[k] = KE_PAIR_BAD_IMAGE; return {0, 0}; }
    const int w = std::min(wa, wb), h = std::min(ha, hb);               // src/dup/refine.py:45-47
    if (w < 7 || h < 7) { if (status_out) status_out[k] = KE_PAIR_TOO_SMALL; return {0, 0}; }
    if (status_out) status_out[k] = KE_PAIR_OK;
    return {w, h};
}

// One common size of a plan whose sources are known.  plane_of: one entry per source, all -1 before and after.
inline void ke_plan_common_size(const KeViewPlan &plan, KeSizePlan &sp, std::vector<int64_t> &plane_of) {
    std::map<std::tuple<int, int, int>, std::vector<int64_t>> groups;   // few: one per shape of source
    for (int64_t k : sp.pairs)
        for (int64_t s : {plan.a[(size_t)k], plan.b[(size_t)k]})
            if (plane_of[(size_t)s] < 0) {
                const KePlaneSrc &src = plan.srcs[(size_t)s];
                groups[{src.w, src.h, src.made}].push_back(s);
                plane_of[(size_t)s] = 0;
            }
    for (auto &g : groups) {
        for (int64_t s : g.second) plane_of[(size_t)s] = sp.planes++;
        sp.groups.push_back(KeFitGroup{std::get<0>(g.first), std::get<1>(g.first), std::get<2>(g.first), sp.planes - (int64_t)g.second.size(),
                                       std::move(g.second)});
    }
    const size_t np = sp.pairs.size();
    sp.idx.resize(2 * np);
    for (size_t j = 0; j < np; ++j) {
        sp.idx[j] = plane_of[(size_t)plan.a[(size_t)sp.pairs[j]]];
        sp.idx[np + j] = plane_of[(size_t)plan.b[(size_t)sp.pairs[j]]];
    }
    for (const KeFitGroup &g : sp.groups)
        for (int64_t s : g.srcs) plane_of[(size_t)s] = -1;
}

// A box is validated only where its image is valid (the pair is KE_PAIR_BAD_IMAGE otherwise), an orientation for every pair.
// ssim_out (NaN) and status_out (nullable) are filled for the pairs that are not scored, status_out for the others too.
inline KeViewPlan ke_plan_view_pairs(const uint64_t *offsets, const int32_t *widths, const int32_t *heights, int32_t channels, int64_t n_images,
                                     const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs, const int32_t *box_a, const int32_t *box_b,
                                     const int32_t *orient_b, double *ssim_out, int32_t *status_out) {
    KeViewPlan plan;
    auto image_ok = [&](int64_t i) { return i >= 0 && i < n_images && widths[i] > 0 && heights[i] > 0; };
    // the view of pair k's side: the box (four zeros for the image as it lies) and the orientation
    struct View { int32_t x0, y0, x1, y1, o; };
    auto view_of = [&](const int32_t *boxes, int64_t k, int64_t i, int o) {
        if (!boxes) return View{0, 0, 0, 0, o};
        const int32_t *b = boxes + 4 * k;
        if (b[0] == 0 && b[1] == 0 && ((b[2] == 0 && b[3] == 0) || (b[2] == widths[i] && b[3] == heights[i]))) return View{0, 0, 0, 0, o};
        return View{b[0], b[1], b[2], b[3], o};
    };
    auto cut = [](View v) { return v.x1 != 0 || v.y1 != 0 || v.x0 != 0 || v.y0 != 0; };
    char text[192];
    for (int64_t k = 0; k < n_pairs; ++k) {
        if (orient_b && (orient_b[k] < 0 || orient_b[k] > 7)) {
            std::snprintf(text, sizeof text, "pair %lld: orientation %d outside 0..7", (long long)k, orient_b[k]);
            plan.bad_pair = k;
            plan.error = text;
            return plan;
        }
        for (int side = 0; side < 2; ++side) {
            const int64_t i = side ? pair_b[k] : pair_a[k];
            if (!image_ok(i)) continue;
            const View v = view_of(side ? box_b : box_a, k, i, 0);
            if (cut(v) && (v.x0 < 0 || v.y0 < 0 || v.x1 <= v.x0 || v.y1 <= v.y0 || v.x1 > widths[i] || v.y1 > heights[i])) {
                std::snprintf(text, sizeof text, "pair %lld: box_%c (%d, %d, %d, %d) is empty or outside image %lld (%dx%d)", (long long)k,
                              side ? 'b' : 'a', v.x0, v.y0, v.x1, v.y1, (long long)i, widths[i], heights[i]);
                plan.bad_pair = k;
                plan.error = text;
                return plan;
            }
        }
    }
    std::vector<uint64_t> off;
    plan.total_bytes = ke_image_offsets(offsets, widths, heights, channels, n_images, off);
    plan.a.assign((size_t)n_pairs, -1);
    plan.b.assign((size_t)n_pairs, -1);
    std::vector<int64_t> as_it_lies((size_t)n_images, -1);                                         // image -> its source, uncut and unturned
    std::map<std::tuple<int64_t, int32_t, int32_t, int32_t, int32_t, int32_t>, int64_t> made_of;   // (image, view) -> its source
    // size of a view as the fit sees it
    auto size_of = [&](int64_t i, View v, int *w, int *h) {
        const int bw = cut(v) ? v.x1 - v.x0 : widths[i], bh = cut(v) ? v.y1 - v.y0 : heights[i];
        *w = (v.o & 4) ? bh : bw;
        *h = (v.o & 4) ? bw : bh;
    };
    auto source = [&](int64_t i, View v) {
        const int32_t w = widths[i], h = heights[i];
        if (!cut(v) && v.o == 0) {
            if (as_it_lies[(size_t)i] < 0) {
                as_it_lies[(size_t)i] = (int64_t)plan.srcs.size();
                plan.srcs.push_back(KePlaneSrc{0, off[i], w, h});
            }
            return as_it_lies[(size_t)i];
        }
        const auto found = made_of.try_emplace({i, v.x0, v.y0, v.x1, v.y1, v.o}, (int64_t)plan.srcs.size());
        if (found.second) {
            int vw, vh;
            size_of(i, v, &vw, &vh);
            plan.srcs.push_back(KePlaneSrc{1, plan.made_bytes, vw, vh});
            if (v.o == 0) plan.crops.push_back(KeCropLumaJob{off[i], plan.made_bytes, w, h, channels, v.x0, v.y0, v.x1 - v.x0, v.y1 - v.y0});
            else if (!cut(v)) plan.turns.push_back(KeViewJob{off[i], plan.made_bytes, w, h, channels, v.o, 0, 0, w, h});
            else plan.views.push_back(KeViewJob{off[i], plan.made_bytes, w, h, channels, v.o, v.x0, v.y0, v.x1 - v.x0, v.y1 - v.y0});
            plan.made_bytes += ((uint64_t)vw * vh + 255) & ~(uint64_t)255;                    // every plane starts on a dword
        }
        return found.first->second;
    };
    std::map<std::pair<int, int>, std::vector<int64_t>> by_size;        // common (w, h) -> the pairs that are scored
    for (int64_t k = 0; k < n_pairs; ++k) {
        const int64_t ia = pair_a[k], ib = pair_b[k];
        const bool ok = image_ok(ia) && image_ok(ib);
        View va{0, 0, 0, 0, 0}, vb{0, 0, 0, 0, 0};
        int wa = 0, ha = 0, wb = 0, hb = 0;
        if (ok) {
            va = view_of(box_a, k, ia, 0);
            vb = view_of(box_b, k, ib, orient_b ? orient_b[k] : 0);
            size_of(ia, va, &wa, &ha);
            size_of(ib, vb, &wb, &hb);
        }
        const std::pair<int, int> common = ke_classify_pair(k, ok, wa, ha, wb, hb, ssim_out, status_out);
        if (!common.first) continue;
        by_size[common].push_back(k);
        plan.a[(size_t)k] = source(ia, va);
        plan.b[(size_t)k] = source(ib, vb);
    }
    std::vector<int64_t> plane_of(plan.srcs.size(), -1);
    for (auto &kv : by_size) {
        plan.sizes.push_back(KeSizePlan{kv.first.first, kv.first.second, std::move(kv.second), {}, 0, {}});
        ke_plan_common_size(plan, plan.sizes.back(), plane_of);
    }
    return plan;
}
