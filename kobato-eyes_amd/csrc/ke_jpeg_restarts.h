// ke_jpeg_restarts.h -- a sequential JPEG's restart intervals as independent pieces of work (KE_JPEG_SPLIT_RESTARTS): the plan
// that deals a file's intervals to lanes, a lane's range, and the rule that says which files may be split.  Shared by the
// kernels (ke_jpeg.hip: ke_jpeg_find_restarts, ke_jpeg_entropy_rst) and by the CPU program the tests run
// (tests/_jpeg_rst_cpu.cpp); plain C++ without allocation.
//
// Why a split file decodes to what the walk (ke_jpeg_entropy: one bit reader from scan_offset to scan_end) gives -- the same
// coefficients and the same status -- by construction, not by luck:
//   * A marker is a position e in [scan_offset, scan_end - 1) with p[e] == 0xFF and p[e + 1] != 0.  By ke_jpeg_segment_end's
//     definition of scan_end every marker inside the segment is an RSTn.  A file is split only if it has exactly n_int - 1
//     of them and the k-th (from 0) carries 0xD0 + (k & 7) (ke_rst_index).  Any other file -- a wrong number, a missing
//     marker, one too many behind the last interval, 0xFF fill bytes in front of a marker (a "marker" numbered 0xFF) -- is
//     the walk's, untouched, and keeps the verdict it gets there.
//   * The walk's filler (ke_bits_fill and its device twin) stops at the first marker it meets: it sets `marker`, feeds zero
//     bytes and counts them in `overrun`.  So between two restarts the walk never reads past the next marker.
//   * ke_bits_restart checks ke_bits_ran_dry, skips whatever bytes the interval left unread in front of the marker, checks the
//     marker's number and goes on two bytes behind it with an empty buffer, no pending marker, overrun 0; the caller zeroes
//     the DC predictors.  In a file the rule admits, the marker the k-th restart arrives at is marker k - 1 (the filler cannot
//     pass one, and the skip stops at the first) and its number is right, so the restart fails only by ran_dry.
//   * A lane therefore starts interval s = j * g in exactly the state the walk is in there: position marker[s - 1] + 2,
//     empty buffer, predictors 0, next_rst = s & 7.  Its reader ends at the position of the marker that closes its last
//     interval; where the walk's filler would see that marker (0xFF, non-zero) the lane's sees `pos == end`: both feed a
//     zero byte and add one to `overrun`, so the bits and ke_bits_ran_dry agree.  The lane checks ke_bits_ran_dry at its end --
//     the check the walk's next ke_bits_restart (or its own end) makes -- and never looks at the leftover bytes, which the
//     walk only skips.
//   * Hence interval k fails in a lane if and only if the walk, having got that far, fails in it; the file is
//     KE_JPEG_CORRUPT if any lane fails (the walk: at the first such interval), and otherwise every block is the walk's.
#pragma once

#include "ke_jpeg_core.h"

constexpr uint32_t KE_RST_LANE_CAP = 16384;     // lanes per file: several waves for every SIMD of the chip from one file, and a
                                                // small marker table for a 65 500 x 65 500 file with a restart interval of 1
constexpr uint32_t KE_RST_MIN_MCUS = 64;        // MCUs a lane should at least have (KE_JPEG_SPLIT_MIN_MCUS overrides)

struct KeRstPlan {
    uint32_t n_int;        // restart intervals of the file: ceil(mcus / ri)
    uint32_t g;            // intervals per lane
    uint32_t n_lanes;      // ceil(n_int / g)
};

// g is the smallest count that gives every lane (but the last) at least min_mcus MCUs and keeps n_lanes at or below cap.
// ri == 0 (no DRI): one interval, one lane.
KE_HD KeRstPlan ke_rst_plan(uint32_t mcus, uint32_t ri, uint32_t min_mcus, uint32_t cap) {
    KeRstPlan p;
    if (ri == 0 || mcus == 0) { p.n_int = 1; p.g = 1; p.n_lanes = 1; return p; }
    if (min_mcus < 1) min_mcus = 1;
    if (cap < 1) cap = 1;
    p.n_int = (uint32_t)(((uint64_t)mcus + ri - 1) / ri);
    const uint32_t by_work = (uint32_t)(((uint64_t)min_mcus + ri - 1) / ri), by_cap = (p.n_int + cap - 1) / cap;
    uint32_t g = by_work > by_cap ? by_work : by_cap;
    if (g > p.n_int) g = p.n_int;
    p.g = g;
    p.n_lanes = (p.n_int + g - 1) / g;
    return p;
}

// A file is worth splitting when its plan has at least two lanes (a DRI that covers the whole image, or too few MCUs for two
// lanes of min_mcus, leaves it on the walk).
KE_HD bool ke_rst_plan_splits(const KeRstPlan &p) { return p.n_lanes >= 2; }

struct KeRstLane {
    uint32_t int_first, int_last;     // intervals [int_first, int_last)
    uint32_t mcu_first, mcu_last;     // MCUs [mcu_first, mcu_last)
    uint32_t next_rst;                // number the first restart marker INSIDE the lane must carry: int_first & 7
    uint32_t start_marker;            // ordinal of the marker the lane starts 2 bytes behind (lane 0: none, scan_offset)
    uint32_t end_marker;              // ordinal of the marker the lane ends at (the last lane: none, scan_end)
};

KE_HD KeRstLane ke_rst_lane(const KeRstPlan &p, uint32_t mcus, uint32_t ri, uint32_t j) {
    KeRstLane l;
    const uint64_t i0 = (uint64_t)j * p.g, i1 = i0 + p.g < p.n_int ? i0 + p.g : p.n_int;
    l.int_first = (uint32_t)i0;
    l.int_last = (uint32_t)i1;
    l.mcu_first = (uint32_t)(i0 * ri);
    l.mcu_last = (uint32_t)(i1 * ri < mcus ? i1 * ri : mcus);
    l.next_rst = (uint32_t)(i0 & 7);
    l.start_marker = (uint32_t)i0 - 1;            // (meaningless for j == 0)
    l.end_marker = (uint32_t)i1 - 1;              // (meaningless for the last lane)
    return l;
}

// The marker index of one file, the sequential way (the kernel does the same a wave wide): counts the markers of
// [scan_offset, scan_end - 1), checks every number, and stores the positions that lane boundaries need -- ordinal j * g - 1 at
// lane_start[j], j = 1 .. n_lanes - 1 (lane_start[0] is not written).  Returns whether the file may be split; *why (nullable):
// 0 split, 1 a marker's number is wrong, 2 too few markers, 3 too many.
KE_HD bool ke_rst_index(const uint8_t *p, uint32_t scan_offset, uint32_t scan_end, const KeRstPlan &plan, uint32_t *lane_start, int *why) {
    uint32_t count = 0;
    bool numbers_ok = true;
    for (uint32_t e = scan_offset; e + 1 < scan_end; ++e) {
        if (p[e] != 0xFF || p[e + 1] == 0) continue;
        if (p[e + 1] != 0xD0u + (count & 7u)) numbers_ok = false;
        const uint32_t j = (count + 1) / plan.g;
        if ((count + 1) % plan.g == 0 && j >= 1 && j < plan.n_lanes) lane_start[j] = e;
        ++count;
    }
    const int reason = !numbers_ok ? 1 : count < plan.n_int - 1 ? 2 : count > plan.n_int - 1 ? 3 : 0;
    if (why) *why = reason;
    return reason == 0;
}
