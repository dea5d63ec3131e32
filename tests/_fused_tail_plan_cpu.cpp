// ke_plan_fused_tail of ke_resample_plan.h compiled for the CPU, with the real tables of ke_coeffs.cpp: what
// tests/test_fused_tail_plan_cpu.py calls.  One call answers, for packed RGB images of w x h in one workgroup per image,
// every row of the kernel table the shape is offered: the plan of ke_plan_fused, the tail's plan with KE_VTILE_VALU unset
// and set, and the numbers of the vertical tables the properties are stated in.
#include <cstdint>
#include <memory>

#include "ke_resample_plan.h"

namespace {

struct Axis {
    KeAxisCoeffs c;
    KeMxTable mx;
    KeChunkTable chunks;
    Axis(int in_size, int out_size, int min_ks, int cpo = 0) {
        ke_build_axis_coeffs(in_size, out_size, c, KE_FILTER_LANCZOS, 0.0f, (float)in_size);
        ke_build_mx(c, mx, min_ks);
        if (cpo) ke_build_chunked(c, cpo, chunks);
    }
};

}  // namespace

extern "C" {

int ft_fields() { return 24; }

// out: ft_fields() values per row; returns the number of rows.
//   0 row, 1 why, 2 wide, 3 dh, 4 lt_half, 5 p.hp, 6 p.hpd, 7 p.x_off, 8 p.lds, 9 p.raise_lds_limit,
//   10 natural steps of the 32-output vertical axis, 11 its window bases' maximum, 12 natural steps of the 8-output axis,
//   13 on_mx, 14 hp, 15 hpd, 16 x_off, 17 lds, 18 raise_lds_limit, 19 ks, 20 kdq,
//   21 on_mx under KE_VTILE_VALU, 22 whether that plan equals ke_plan_fused's fields, 23 steps of the table the tail got
int ft_case(int w, int h, int want_d, int64_t *out) {
    const KeSpShape shape{w, h, 3, false, true, true, want_d != 0, false};
    int rows[kKeSpMaxCandidates];
    const int n = ke_single_pass_candidates(shape, rows);
    for (int k = 0; k < n; ++k) {
        int64_t *o = out + (size_t)k * ft_fields();
        for (int i = 0; i < ft_fields(); ++i) o[i] = -1;
        const int r = rows[k];
        const bool DH = kKeSpRows[r].dh();
        o[0] = r; o[2] = kKeSpRows[r].family == KE_SP_WIDE; o[3] = DH;
        const KeFusedSteps s = ke_plan_fused_steps(r, w);
        o[1] = s.why;
        if (s.why) continue;
        Axis hz(w, 32, s.ks), vt(h, 32, 0);
        std::unique_ptr<Axis> hzd, vtd, vtd_tail;
        if (DH) { hzd.reset(new Axis(w, 9, s.ksd)); vtd.reset(new Axis(h, 8, 0, 3)); }
        const KeFusedPlan p = ke_plan_fused(r, w, h, 4, s, hz.mx, vt.c.span, DH ? &hzd->mx : nullptr, DH ? &vtd->chunks : nullptr, nullptr);
        o[1] = p.why;
        if (p.why) continue;
        o[4] = p.lt_half; o[5] = p.hp; o[6] = p.hpd; o[7] = p.x_off; o[8] = (int64_t)p.lds; o[9] = p.raise_lds_limit;
        Axis vt_tail(h, 32, ke_fused_tail_steps(vt.mx.ks));
        if (DH) vtd_tail.reset(new Axis(h, 8, ke_fused_tail_dsteps(vtd->mx.ks)));
        o[10] = vt.mx.ks; o[11] = std::max(vt.mx.base[0], vt.mx.base[1]); o[12] = DH ? vtd->mx.ks : 0;
        const KeFusedTailPlan t = ke_plan_fused_tail(r, p, vt_tail.mx, DH ? &vtd_tail->mx : nullptr, KeHashSwitches{});
        o[13] = t.on_mx; o[14] = t.hp; o[15] = t.hpd; o[16] = t.x_off; o[17] = (int64_t)t.lds; o[18] = t.raise_lds_limit; o[19] = t.ks; o[20] = t.kdq;
        const KeFusedTailPlan v = ke_plan_fused_tail(r, p, vt_tail.mx, DH ? &vtd_tail->mx : nullptr, KeHashSwitches{false, 0, true});
        o[21] = v.on_mx;
        o[22] = v.hp == p.hp && v.hpd == p.hpd && v.x_off == p.x_off && v.lds == p.lds && v.raise_lds_limit == p.raise_lds_limit;
        o[23] = vt_tail.mx.ks;
    }
    return n;
}

}  // extern "C"
