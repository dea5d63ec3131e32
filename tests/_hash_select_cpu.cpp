// ke_hash_select.h and ke_group_plan.h compiled for the CPU: what tests/test_hash_select_cpu.py calls.
#include "ke_hash_select.h"
#include "ke_group_plan.h"

extern "C" {

int hsel_row_count() { return kKeSpRowCount; }

// family, the six template arguments, first and last width
void hsel_row(int r, int32_t out[9]) {
    const KeSpRow &row = kKeSpRows[r];
    out[0] = row.family;
    for (int k = 0; k < 6; ++k) out[1 + k] = row.t[k];
    out[7] = row.w_lo;
    out[8] = row.w_hi;
}

int hsel_candidates(int w, int h, int c, int misaligned, int base_mod4, int has_offsets, uint64_t stride, int want_d, int plan, int32_t out[4]) {
    const KeSpShape s{w, h, c, misaligned != 0, base_mod4 == 0, has_offsets || stride % 4 == 0, want_d != 0, plan != 0};
    int rows[kKeSpMaxCandidates];
    const int n = ke_single_pass_candidates(s, rows);
    for (int k = 0; k < n; ++k) out[k] = rows[k];
    return n;
}

// a group of packed images (no offsets, stride = one image) on an aligned base, widths w_first..w_last: 5 ints per width
void hsel_sweep(int c, int want_d, int plan, int h, int w_first, int w_last, int32_t *out) {
    for (int w = w_first; w <= w_last; ++w, out += 5) {
        for (int k = 1; k < 5; ++k) out[k] = -1;
        out[0] = hsel_candidates(w, h, c, 0, 0, 0, (uint64_t)w * h * c, want_d, plan, out + 1);
    }
}

// groups_out: (w, h, channels, meta_at, n, misaligned) per group; returns the number of groups
int64_t hsel_plan(const uint64_t *offsets, const int32_t *widths, const int32_t *heights, const int32_t *channels, int32_t channels_all,
                  const uint8_t *take, int64_t n, uint64_t base, uint64_t *meta, int64_t *groups_out, uint64_t *meta_words) {
    size_t words = 0;
    const std::vector<KeShapeGroup> groups = ke_plan_shape_groups(offsets, widths, heights, channels, channels_all, take, n, (uintptr_t)base, meta, &words);
    *meta_words = words;
    for (size_t k = 0; k < groups.size(); ++k) {
        const KeShapeGroup &g = groups[k];
        const int64_t row[6] = {g.w, g.h, g.channels, (int64_t)g.meta_at, g.n, g.misaligned};
        for (int j = 0; j < 6; ++j) groups_out[6 * k + j] = row[j];
    }
    return (int64_t)groups.size();
}

}  // extern "C"
