// Shape groups of a ragged batch: one launch group per distinct (width, height, channels), and the metadata block the
// hash kernels read.  Host code without HIP types, so a host-only program can include it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <tuple>
#include <unordered_map>
#include <vector>

struct KeShapeGroup {
    int w, h, channels;
    size_t meta_at;    // the group's block in the metadata, in 8-byte words: n byte offsets, then n output slots
    int64_t n;
    bool misaligned;   // some image of the group starts at an address that is not a multiple of 4
};

// The dword loaders of the single-pass and aligned banded kernels want every image of a group on a dword boundary; a
// packed stream loses that after the first image whose byte size is not a multiple of 4.
inline bool ke_any_misaligned(uintptr_t base, const uint64_t *offsets, int64_t n) {
    for (int64_t k = 0; k < n; ++k)
        if ((base + offsets[k]) % 4 != 0) return true;
    return false;
}

// Groups the images i with take[i] != 0 by shape (channels == NULL: channels_all for every image; 1..4 either way) and
// returns the groups in ascending (w, h, channels) order, each group's images in input order.  meta (2 * n words) gets
// the groups' [offsets | output slots] blocks back to back, the slot being the image's index; *meta_words what was used.
// An image's group id comes from a one-entry cache or a hash lookup (the shape list of a library is short), the members
// are then laid out by a counting sort -- linear in n with small constants (a million-image call spends its host time here).
inline std::vector<KeShapeGroup> ke_plan_shape_groups(const uint64_t *offsets, const int32_t *widths, const int32_t *heights, const int32_t *channels,
                                                      int32_t channels_all, const uint8_t *take, int64_t n, uintptr_t base, uint64_t *meta, size_t *meta_words) {
    std::vector<KeShapeGroup> groups;
    std::unordered_map<uint64_t, int32_t> ids;
    std::vector<int32_t> gid((size_t)n, -1);       // group ids in order of first use
    uint64_t last_key = 0;
    int32_t last_id = -1;
    for (int64_t i = 0; i < n; ++i) {
        if (!take[i]) continue;
        const int c = channels ? channels[i] : channels_all;
        const uint64_t key = ((uint64_t)(uint32_t)widths[i] << 33) | ((uint64_t)(uint32_t)heights[i] << 2) | (uint64_t)(c - 1);
        if (last_id < 0 || key != last_key) {
            auto it = ids.find(key);
            if (it == ids.end()) {
                it = ids.emplace(key, (int32_t)groups.size()).first;
                groups.push_back(KeShapeGroup{widths[i], heights[i], c, 0, 0, false});
            }
            last_key = key;
            last_id = it->second;
        }
        gid[i] = last_id;
        ++groups[last_id].n;
    }
    std::vector<int32_t> order(groups.size());      // the ids in ascending (w, h, channels): the blocks' order in meta
    for (size_t k = 0; k < order.size(); ++k) order[k] = (int32_t)k;
    auto shape = [&](int32_t k) { return std::make_tuple(groups[k].w, groups[k].h, groups[k].channels); };
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return shape(a) < shape(b); });
    size_t cursor = 0;
    for (int32_t k : order) { groups[k].meta_at = cursor; cursor += 2 * (size_t)groups[k].n; }
    std::vector<size_t> placed(groups.size());
    for (int64_t i = 0; i < n; ++i) {
        if (gid[i] < 0) continue;
        const KeShapeGroup &g = groups[gid[i]];
        const size_t at = g.meta_at + placed[gid[i]]++;
        meta[at] = offsets[i];
        meta[at + (size_t)g.n] = (uint64_t)i;
    }
    for (KeShapeGroup &g : groups) g.misaligned = ke_any_misaligned(base, meta + g.meta_at, g.n);
    std::sort(groups.begin(), groups.end(), [](const KeShapeGroup &a, const KeShapeGroup &b) { return a.meta_at < b.meta_at; });
    *meta_words = cursor;
    return groups;
}
