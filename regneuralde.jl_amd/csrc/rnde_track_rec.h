// rnde_track_rec.h -- the scalar reverse of the step-size controller and of the initial-step rule as the tracked sweeps on the tile layout use
// it (rnde_tile_driver.h: rnde_tile_reverse_kernel<Dyn, KIN, true>), beside the records of a sweep's walk.  No kernel lives here: both
// translation units of the tile layout include it, and a stand-alone host program checks it against finite differences
// (tests/track_host/track_host_check.cpp).
#pragma once
#include "rnde_device.h"       // StepMeta, InitRec, the controller's constants and flags
#include <cmath>

namespace rnde {

struct FfStepRec { float t, dt, eest, svb; };     // one accepted step, in forward order; svb = cotangent of its saved value EEst * dt

// One attempt of the tracked sweep, in forward order: (t, dt, EEst) and the flags of the step log, the tape record that holds the attempt's
// uprev, and the scalar reverse of the controller branch the forward took (rnde_bchain.h's prologue with track_ctrl = 1, t0-bar and t1-bar
// dropped).  That reverse is linear in the running cotangents (t-bar, dtp-bar, qold-bar) behind the attempt, with coefficients that depend
// on the step log alone, so the host forms them once, in double (ff_att_rec):
//     EEst-bar  = e0 + e_dtp dtp-bar + e_q qold-bar                 (e0 = svb dt: the saved value EEst * dt)
//     dt-bar    = d0 + d_t t-bar + d_dtp dtp-bar + (the three sums)   (d0 = svb EEst; d_t = 1 on an accepted attempt: t' = t + dt)
//     qold-bar' = c_dtp dtp-bar + c_q qold-bar                        (in front of the attempt)
struct FfAttRec {
    float t, dt, eest;
    int flags, rec, pad;
    double e0, e_dtp, e_q, d0, d_t, d_dtp, c_dtp, c_q;
};
// Accepted: dtp' = dt / q, q = clip(q11 / qold^beta2 / gamma), qold' = max(EEst, qoldinit).  Rejected: dtp' = dt / rej_m, rej_m =
// min(1 / qmin, q11 / gamma).  F_QCLAMP, F_DTMAXCLAMP and F_EZERO cut the path, F_REJQ11 selects it; q11 = EEst^beta1.
inline FfAttRec ff_att_rec(const StepMeta& m, float svb, int rec) {
    FfAttRec a{};
    a.t = m.t; a.dt = m.dt; a.eest = m.eest; a.flags = m.flags; a.rec = rec;
    const double dt = m.dt;
    double qb = 0.0, q11b = 0.0;         // per unit of dtp-bar
    if (m.flags & F_ACCEPT) {
        a.e0 = (double)svb * dt; a.d0 = (double)svb * (double)m.eest;
        a.d_t = 1.0;
        if (!(m.flags & F_DTMAXCLAMP)) { a.d_dtp = 1.0 / (double)m.q; qb = -dt / ((double)m.q * (double)m.q); }
        if (m.eest > kQoldInit) a.e_q = 1.0;
    } else {
        a.d_dtp = 1.0 / (double)m.rej_m;
        if (m.flags & F_REJQ11) q11b = -dt / ((double)m.rej_m * (double)m.rej_m) / (double)kGamma;
        a.c_q = 1.0;
    }
    if (!(m.flags & F_QCLAMP) && !(m.flags & F_EZERO)) {
        q11b += qb / (pow((double)m.qold_in, (double)kBeta2) * (double)kGamma);
        a.c_dtp = -(double)kBeta2 * qb * (double)m.q / (double)m.qold_in;
    }
    if (!(m.flags & F_EZERO) && m.eest > 0.f) a.e_dtp = q11b * (double)kBeta1 * (double)m.q11 / (double)m.eest;
    return a;
}

// ---- the initial-step rule, scalar part of its reverse: the arithmetic of rnde_bchain_init_kernel's two phases ----
//     d0 = rms(x / sk), d1 = rms(f0 / sk), dt0 = (d0 / d1) / 100 (1e-6 when dt0_const; t1 - t0 when dt0_clamped)
//     u1 = x + dt0 f0, f1 = f(u1, t0 + dt0), d2 = rms((f1 - f0) / sk) / dt0
//     dt1 = 10^(-(2 + log10 max(d1, d2)) / 5)  (max(1e-6, 1e-3 dt0) when dt1_const),  dt = min(100 dt0, dt1, t1 - t0): sel 0 / 1 / 2
// Phase 1 maps the cotangent of dt (dtp-bar in front of attempt 0) to the cotangents of dt0, d1, d2 and of the span, and to coef_w, the
// factor of f1-bar = coef_w (f1 - f0) / sk^2; the VJP at (u1, t0 + dt0) then yields u1-bar and the two sums <u1-bar, f0>, tau.
struct InitBar1 { double dt0b, d1b, d2b, coef_w, t0b, t1b; };
__host__ __device__ inline InitBar1 init_rev_phase1(const InitRec& ir, double dtpb, double N) {
    InitBar1 b{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double dt0 = (double)ir.dt0;
    if (ir.sel == 2) { b.t1b += dtpb; b.t0b -= dtpb; }
    else if (ir.sel == 0) b.dt0b += 100.0 * dtpb;
    else if (!ir.dt1_const) {
        const double mm = ir.max_is_d2 ? (double)ir.d2 : (double)ir.d1;
        const double mb = dtpb * (-0.2) * (double)ir.dt1 / mm;
        if (ir.max_is_d2) b.d2b += mb; else b.d1b += mb;
    } else if (ir.dt0 * 1e-3f > 1e-6f) b.dt0b += 1e-3 * dtpb;
    const double n2 = (double)ir.d2 * dt0, n2b = b.d2b / dt0;
    b.dt0b += -b.d2b * (double)ir.d2 / dt0;
    b.coef_w = n2 > 0 ? n2b / (N * n2) : 0.0;
    return b;
}
// Phase 2 takes the two sums of phase 1's VJP (dot = <u1-bar, f0>: u1 = x + dt0 f0; tau: the time t0 + dt0) and closes dt0: the cotangents
// of d0 and d1 (the x-bar and f0-bar terms of the three norms follow from them and coef_w) and of the span.
struct InitBar2 { double d0b, d1b, t0b, t1b; };
__host__ __device__ inline InitBar2 init_rev_phase2(const InitRec& ir, const InitBar1& b, double dot, double tau) {
    InitBar2 c{0.0, b.d1b, b.t0b + tau, b.t1b};
    const double dt0b = b.dt0b + tau + dot;
    if (ir.dt0_clamped) { c.t1b += dt0b; c.t0b -= dt0b; }
    else if (!ir.dt0_const) { c.d0b = dt0b / (100.0 * (double)ir.d1); c.d1b += -dt0b * (double)ir.dt0 / (double)ir.d1; }
    return c;
}

}  // namespace rnde
