// ke_resample_plan.h compiled for the CPU, with the real tables of ke_coeffs.cpp: what tests/test_resample_plan_cpu.py calls.
// A record is what every path of the header answers for one case, each answer preceded by its length; a key is the
// decisions among them (accepted or why not, chunks, launches, step counts), which stay the same over runs of widths.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <tuple>
#include <vector>

#include "ke_resample_plan.h"

namespace {

using Sw = KeHashSwitches;
using Rec = std::vector<int64_t>;

struct Case {
    int w, h, c;
    int64_t n;
    int misaligned, base_dword, stride_dword, has_offsets;
    int ow, oh, filter;
};

// the tables as ke_get_coeffs / ke_get_chunks / ke_get_mx hand them out, without a device
struct Tables {
    std::map<std::tuple<int, int, int>, std::unique_ptr<KeAxisCoeffs>> axes;
    ~Tables() { clear(); }
    void clear() {
        for (auto &kv : axes) {
            for (auto &c : kv.second->chunked) delete c.second;
            for (auto &m : kv.second->mx) delete m.second;
        }
        axes.clear();
    }
    const KeAxisCoeffs *coeffs(int in_size, int out_size, int filter = KE_FILTER_LANCZOS) {
        auto &slot = axes[std::make_tuple(in_size, out_size, filter)];
        if (!slot) {
            slot.reset(new KeAxisCoeffs());
            ke_build_axis_coeffs(in_size, out_size, *slot, filter, 0.0f, (float)in_size);
        }
        return slot.get();
    }
    const KeChunkTable *chunks(const KeAxisCoeffs *cc, int cpo, int ndwc_multiple = 4) {
        auto *c = const_cast<KeAxisCoeffs *>(cc);
        auto &slot = c->chunked[cpo * 64 + ndwc_multiple];
        if (!slot) {
            slot = new KeChunkTable();
            ke_build_chunked(*c, cpo, *slot, ndwc_multiple);
        }
        return slot;
    }
    const KeMxTable *mx(const KeAxisCoeffs *cc, int min_ks = 0, bool align64 = false) {
        auto *c = const_cast<KeAxisCoeffs *>(cc);
        auto &slot = c->mx[min_ks * 2 + (align64 ? 1 : 0)];
        if (!slot) {
            slot = new KeMxTable();
            ke_build_mx(*c, *slot, min_ks, align64);
        }
        return slot;
    }
};

enum { P_HBAND = 0, P_VTILE, P_STRIPS, P_SPB, P_FUSED, P_GENERIC, P_COUNT };
constexpr int kEntries = 17;
struct Stats {
    int64_t seen[P_COUNT][32];      // [path][answer]: how often each path gave each answer
    int64_t entry[kEntries];        // calls per function of the header
};
thread_local Tables t_horizontal, t_vertical;      // by row length (dropped when a sweep moves to the next width) and by height
thread_local Stats t_stats;
Stats g_stats;
std::mutex g_stats_lock;

void flush_stats() {
    std::lock_guard<std::mutex> hold(g_stats_lock);
    for (int p = 0; p < P_COUNT; ++p)
        for (int k = 0; k < 32; ++k) g_stats.seen[p][k] += t_stats.seen[p][k];
    for (int k = 0; k < kEntries; ++k) g_stats.entry[k] += t_stats.entry[k];
    std::memset(&t_stats, 0, sizeof t_stats);
}

constexpr int kHbandHp = 14;        // where probe_hband's answer holds the column pitch
const int kCu[2] = {8, 256};
const Sw kFm[3] = {{false, 0, false}, {true, 1, false}, {true, 1000, false}};

// ---- the plans: one probe per path, answer[0] (fused: [1]) = KeDecline ----------------------------------------------
const char *const kEntryNames[kEntries] = {"ke_column_pitch", "ke_fits_one_launch", "ke_chunk_images", "ke_hash_scratch_per_image",
                                           "ke_resize_scratch_per_image", "ke_fused_min_images", "ke_plan_hband_chunks", "ke_plan_hband",
                                           "ke_hband_launch", "ke_vtile_on_mx", "ke_plan_vtile", "ke_plan_strips_steps", "ke_plan_strips",
                                           "ke_plan_sp_bands", "ke_plan_fused_steps", "ke_plan_fused", "ke_plan_generic"};
#define CALLED(k) (++t_stats.entry[k])

KePlanShape shape_of(const Case &c) { return {c.w, c.h, c.c, c.n, c.misaligned != 0, c.base_dword != 0, c.stride_dword != 0, c.has_offsets != 0}; }

Rec probe_hband(const Case &c) {
    const KePlanShape g = shape_of(c);
    const KeAxisCoeffs *chz = t_horizontal.coeffs(c.w, c.ow, c.filter), *cvt = t_vertical.coeffs(c.h, c.oh, c.filter);
    CALLED(6);
    const KeHbandChunks ch = ke_plan_hband_chunks(g, c.ow, c.oh, chz->ndw);
    if (ch.why) return {ch.why};
    const KeChunkTable *tc = t_horizontal.chunks(chz, 1 << ch.best_log2, 8);
    CALLED(7);
    const KeHbandPlan p = ke_plan_hband(g, c.ow, ch.best_log2, tc->cspan, cvt->span);
    if (p.why) return {p.why, p.best_log2, tc->ndwc};
    Rec r{0, p.best_log2, tc->ndwc, p.launches, p.aligned, p.qr, p.lp, p.rt, p.band_rows, p.bands, p.bp, p.per_launch, p.lt_half, (int64_t)p.lds, p.hp,
          (int64_t)p.scratch_bytes, tc->cspan};
    for (int i = 0; i < p.launches; ++i) {
        CALLED(8);
        const KeHbandLaunch l = ke_hband_launch(p, c.ow, i);
        r.push_back(l.out_first); r.push_back(l.nout); r.push_back(l.vcp_log2);
    }
    return r;
}

Rec probe_vtile(const Case &c, int hp, const Sw &sw) {
    CALLED(9);
    const int tiles = ke_vtile_on_mx(c.oh, sw) ? t_vertical.mx(t_vertical.coeffs(c.h, c.oh, c.filter))->tiles : 0;
    CALLED(10);
    const KeVtilePlan p = ke_plan_vtile(c.ow, c.oh, hp, c.n, sw, tiles);
    return {p.why, p.on_mx, p.nt, p.items, p.blocks, p.cg, (int64_t)p.lds};
}

Rec probe_strips(const Case &c, int cu_count, const Sw &sw) {
    const KePlanShape g = shape_of(c);
    const KeAxisCoeffs *chz = t_horizontal.coeffs(c.w, c.ow), *cvt = t_vertical.coeffs(c.h, c.oh);
    CALLED(11);
    const KeStripSteps s = ke_plan_strips_steps(g, c.ow, c.oh, chz->bounds.data());
    if (s.why) return s.why == KE_DECLINE_ST_STEPS ? Rec{s.why, s.ksh} : Rec{s.why};
    const KeMxTable *mx = t_horizontal.mx(chz, s.parts * s.ksh, true);
    CALLED(12);
    const KeStripPlan p = ke_plan_strips(g, c.ow, s, *mx, cvt->span, cu_count, sw);
    if (p.why) return {p.why, s.ksh};
    return {0, s.ksh, s.nt, s.parts, p.nstrips, p.band_rows, p.bands, p.bp, p.base0, p.base1, p.x_off, p.hb_off, (int64_t)p.lds, p.hp, (int64_t)p.scratch_bytes};
}

KeSpBandPlan sp_bands(const Case &c, bool want_d, int cu_count) {
    const KeAxisCoeffs *cvt = t_vertical.coeffs(c.h, 32), *cvd = want_d ? t_vertical.coeffs(c.h, 8) : nullptr;
    CALLED(13);
    return ke_plan_sp_bands(shape_of(c), want_d, cvt->span, cvd ? cvd->span : 0, cu_count);
}

Rec probe_spb(const Case &c, bool want_d, int cu_count) {
    const KeSpBandPlan p = sp_bands(c, want_d, cu_count);
    if (p.why) return {p.why};
    return {0, p.bands, p.band_rows, p.hs_hp, p.hsd_hp, (int64_t)p.scratch_bytes};
}

// plan (nullable): probe_spb's answer for the bands the kernel runs on
Rec probe_fused(const Case &c, int r, const Rec *plan) {
    KeSpBandPlan bands{};
    if (plan) { bands.bands = (int)(*plan)[1]; bands.band_rows = (int)(*plan)[2]; bands.hs_hp = (int)(*plan)[3]; bands.hsd_hp = (int)(*plan)[4]; }
    CALLED(14);
    const KeFusedSteps s = ke_plan_fused_steps(r, c.w);
    if (s.why) return {r, s.why};
    const KeMxTable *mx = t_horizontal.mx(t_horizontal.coeffs(c.w, 32), s.ks);
    const KeMxTable *mxd = kKeSpRows[r].dh() ? t_horizontal.mx(t_horizontal.coeffs(c.w, 9), s.ksd) : nullptr;
    const KeChunkTable *vd = mxd ? t_vertical.chunks(t_vertical.coeffs(c.h, 8), 3) : nullptr;
    CALLED(15);
    const KeFusedPlan p = ke_plan_fused(r, c.w, c.h, c.n, s, *mx, t_vertical.coeffs(c.h, 32)->span, mxd, vd, plan ? &bands : nullptr);
    if (p.why) return {r, p.why};
    return {r, 0, s.ks, s.ksd, p.qw, p.qw_inv, p.lp, p.lt_half, p.hp, p.hpd, p.x_off, p.row_bytes, p.threads, p.workgroups, (int64_t)p.lds, p.raise_lds_limit};
}

Rec probe_generic(const Case &c) {
    CALLED(16);
    const KeGenericPlan p = ke_plan_generic(c.w, c.h, c.ow, c.oh);
    return {p.vertical_first, p.mid_w, p.mid_h, (int64_t)p.mid_bytes, p.max_n, p.b0, p.b1};
}

// the crossover under the three states of KE_FUSED_MIN_IMAGES, the chunk sizes of the two entry points, the shared rules
Rec probe_misc(const Case &c) {
    Rec r;
    for (int fm = 0; fm < 3; ++fm) { CALLED(5); r.push_back(ke_fused_min_images((int64_t)c.w * c.h * c.c, kFm[fm])); }
    CALLED(3); CALLED(2);
    r.push_back((int64_t)ke_hash_scratch_per_image(c.h)); r.push_back(ke_chunk_images(ke_hash_scratch_per_image(c.h)));
    CALLED(4); CALLED(2);
    r.push_back((int64_t)ke_resize_scratch_per_image(c.ow, c.oh, c.h)); r.push_back(ke_chunk_images(ke_resize_scratch_per_image(c.ow, c.oh, c.h)));
    CALLED(0); CALLED(1);
    r.push_back(ke_column_pitch(t_vertical.coeffs(c.h, c.oh, c.filter)->span, c.h)); r.push_back(ke_fits_one_launch(c.n * c.h));
    return r;
}

// ---- the sweep: one record per case, runs of equal keys over consecutive widths ---------------------------------------
constexpr int kKeyInts = 61;

struct Out {
    Rec rec;
    int32_t key[kKeyInts];
    int at = 0;
    Out() { for (int32_t &k : key) k = -1; }
    // a probe's answer: all of it into the record, its first nkey values (the decisions) into `slots` key slots
    void add(int path, const Rec &r, int nkey, int slots) {
        if (path >= 0) ++t_stats.seen[path][path == P_GENERIC ? 0 : r[path == P_FUSED ? 1 : 0]];
        rec.push_back((int64_t)r.size());
        rec.insert(rec.end(), r.begin(), r.end());
        for (int k = 0; k < slots; ++k) key[at + k] = k < nkey && k < (int)r.size() ? (int32_t)r[k] : -1;
        at += slots;
    }
    void skip(int slots) { at += slots; }
};

void record(const Case &c, Out &o) {
    const Rec hb = probe_hband(c);
    o.add(P_HBAND, hb, 5, 5);
    for (int valu = 0; valu < 2; ++valu) {
        if (hb[0] == 0) o.add(P_VTILE, probe_vtile(c, (int)hb[kHbandHp], Sw{false, 0, valu != 0}), 2, 2);
        else o.skip(2);
    }
    const bool hash32 = c.ow == 32 && c.oh == 32 && c.filter == KE_FILTER_LANCZOS, hash98 = c.ow == 9 && c.oh == 8 && c.filter == KE_FILTER_LANCZOS;
    for (int cu = 0; cu < 2; ++cu)
        for (int fm = 0; fm < 3; ++fm) {
            // the strip kernel is the hashes' alone: another target asks it once, to be declined
            if (hash32 || hash98 || (cu == 1 && fm == 0 && c.filter == KE_FILTER_LANCZOS)) o.add(P_STRIPS, probe_strips(c, kCu[cu], kFm[fm]), 2, 2);
            else o.skip(2);
        }
    for (int want_d = 0; want_d < 2; ++want_d)
        for (int cu = 0; cu < 2; ++cu) {
            if (hash32) o.add(P_SPB, probe_spb(c, want_d != 0, kCu[cu]), 1, 1);
            else o.skip(1);
        }
    // the single-pass kernels: every row the shape is offered, for one hash or both, one workgroup per image or per band
    // (the bands of 256 CUs); and, where the list leaves room, one row the shape was not offered
    for (int want_d = 0; want_d < 2; ++want_d)
        for (int banded = 0; banded < 2; ++banded) {
            int filled = 0;
            if (hash32) {
                const Rec plan = banded ? probe_spb(c, want_d != 0, 256) : Rec{0};
                if (plan[0] == 0) {
                    const KeSpShape shape{c.w, c.h, c.c, c.misaligned != 0, c.base_dword != 0, c.has_offsets || c.stride_dword, want_d != 0, banded != 0};
                    int rows[kKeSpMaxCandidates];
                    const int nc = ke_single_pass_candidates(shape, rows);
                    for (int k = 0; k < nc; ++k, ++filled) o.add(P_FUSED, probe_fused(c, rows[k], banded ? &plan : nullptr), 2, 2);
                    if (filled < kKeSpMaxCandidates) { o.add(P_FUSED, probe_fused(c, c.h % kKeSpRowCount, banded ? &plan : nullptr), 2, 2); ++filled; }
                }
            }
            o.skip(2 * (kKeSpMaxCandidates - filled));
        }
    o.add(P_GENERIC, probe_generic(c), 1, 1);
    o.add(-1, probe_misc(c), 3, 3);
}

// of one record; a sequence's digest is the sum over its widths, so that it does not depend on how the widths are shared out
uint64_t digest_of(const Case &c, const Rec &r) {
    uint64_t d = 0xcbf29ce484222325ull ^ ((uint64_t)c.w * 0x9E3779B97F4A7C15ull);
    for (int64_t v : r)
        for (int b = 0; b < 8; ++b) { d ^= (uint64_t)(v >> (8 * b)) & 255; d *= 0x100000001b3ull; }
    return d;
}

struct Seq {
    uint64_t digest = 0;
    std::vector<int64_t> runs;      // first width, last width, key
    int64_t nruns = 0;
    // the widths of a sequence come in order and without a gap: a run ends where the key changes
    template <typename K>
    void add(int64_t first, int64_t last, const K *key) {
        if (nruns && std::equal(key, key + kKeyInts, runs.end() - kKeyInts)) { runs[runs.size() - kKeyInts - 1] = last; return; }
        runs.push_back(first); runs.push_back(last);
        runs.insert(runs.end(), key, key + kKeyInts);
        ++nruns;
    }
};

std::vector<int64_t> g_result;

}  // namespace

extern "C" {

int rp_key_ints() { return kKeyInts; }
int rp_why_count() { return KE_DECLINE_COUNT; }
int rp_entry_count() { return kEntries; }
const char *rp_entry_name(int k) { return kEntryNames[k]; }
int64_t rp_entry_calls(int k) { return g_stats.entry[k]; }
void rp_seen(int64_t *out) { std::memcpy(out, g_stats.seen, sizeof g_stats.seen); }

const char *rp_why_name(int k) {
    static const char *const names[KE_DECLINE_COUNT] = {"OK", "ONE_LAUNCH", "HB_VERTICAL_FIRST", "HB_SHAPE", "HB_WINDOW", "HB_ROW", "HB_LDS", "VT_LDS",
                                                        "ST_TARGET", "ST_SHAPE", "ST_ADDRESS", "ST_STEPS", "ST_TABLE", "ST_LAST_STRIP", "ST_SWITCH", "ST_FILL",
                                                        "SPB_SHAPE", "FU_WIDTH", "FU_TABLE", "FU_DH_TABLE", "FU_LDS", "FU_BANDS_FIT"};
    static_assert(KE_DECLINE_FU_BANDS_FIT == 21 && KE_DECLINE_ST_TARGET == 8 && KE_DECLINE_SPB_SHAPE == 16, "the names follow the enum");
    return names[k];
}

// One case: v = w, h, channels, n, misaligned, base on a dword, stride a multiple of 4, offset array, ow, oh, filter.
// Returns the record's length (the first `cap` values are written), its key and its digest.
int64_t rp_case(const int64_t *v, int64_t *out, int64_t cap, int32_t *key, uint64_t *digest) {
    const Case c{(int)v[0], (int)v[1], (int)v[2], v[3], (int)v[4], (int)v[5], (int)v[6], (int)v[7], (int)v[8], (int)v[9], (int)v[10]};
    Out o;
    record(c, o);
    for (size_t k = 0; k < o.rec.size() && (int64_t)k < cap; ++k) out[k] = o.rec[k];
    std::memcpy(key, o.key, sizeof o.key);
    *digest = digest_of(c, o.rec);
    t_horizontal.clear();
    flush_stats();
    return (int64_t)o.rec.size();
}

// Widths w_first..w_last x heights x targets (ow, oh pairs) x channels x group sizes: packed images on an aligned base, LANCZOS.
// A sequence is one (height, target, channels, n, w % 4 == 0 or not) over the widths; its result is
//   h, ow, oh, c, n, aligned, digest, number of runs, then per run: first width, last width, the key.
// The widths are shared out over the threads in blocks.  Returns the int64 count of rp_result.
int64_t rp_sweep(int w_first, int w_last, const int32_t *heights, int nh, const int32_t *targets, int nt, const int32_t *channels, int nc,
                 const int64_t *ns, int nn) {
    const size_t nseq = (size_t)nh * nt * nc * nn * 2;
    const int nthreads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    constexpr int kBlock = 40;      // widths a thread takes at a time
    const int nblocks = (w_last - w_first + kBlock) / kBlock;
    std::vector<std::vector<Seq>> part((size_t)nblocks, std::vector<Seq>(nseq));
    std::atomic<int> next{0};
    auto work = [&]() {
        for (int b = next++; b < nblocks; b = next++) {
            for (int w = w_first + b * kBlock; w < std::min(w_first + (b + 1) * kBlock, w_last + 1); ++w) {
                size_t s = 0;
                for (int ih = 0; ih < nh; ++ih)
                    for (int it = 0; it < nt; ++it)
                        for (int ic = 0; ic < nc; ++ic)
                            for (int in = 0; in < nn; ++in, s += 2) {
                                const Case c{w, heights[ih], channels[ic], ns[in], 0, 1, 1, 0, targets[2 * it], targets[2 * it + 1], KE_FILTER_LANCZOS};
                                Out o;
                                record(c, o);
                                Seq &q = part[(size_t)b][s + (w % 4 == 0 ? 1 : 0)];
                                q.digest += digest_of(c, o.rec);
                                q.add(w, w, o.key);
                            }
                t_horizontal.clear();
            }
        }
        t_vertical.clear();
        flush_stats();
    };
    std::vector<std::thread> threads;
    for (int t = 1; t < nthreads; ++t) threads.emplace_back(work);
    work();
    for (auto &t : threads) t.join();
    g_result.clear();
    size_t s = 0;
    for (int ih = 0; ih < nh; ++ih)
        for (int it = 0; it < nt; ++it)
            for (int ic = 0; ic < nc; ++ic)
                for (int in = 0; in < nn; ++in)
                    for (int al = 0; al < 2; ++al, ++s) {
                        Seq all;
                        for (int b = 0; b < nblocks; ++b) {
                            const Seq &q = part[(size_t)b][s];
                            all.digest += q.digest;
                            for (int64_t k = 0; k < q.nruns; ++k) {     // runs that meet at a block edge join again
                                const int64_t *run = &q.runs[(size_t)k * (kKeyInts + 2)];
                                all.add(run[0], run[1], run + 2);
                            }
                        }
                        const int64_t head[8] = {heights[ih], targets[2 * it], targets[2 * it + 1], channels[ic], ns[in], al, (int64_t)all.digest, all.nruns};
                        g_result.insert(g_result.end(), head, head + 8);
                        g_result.insert(g_result.end(), all.runs.begin(), all.runs.end());
                    }
    return (int64_t)g_result.size();
}

void rp_result(int64_t *out) { std::memcpy(out, g_result.data(), g_result.size() * sizeof(int64_t)); }

}  // extern "C"
