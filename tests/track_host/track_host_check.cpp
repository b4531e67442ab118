// The scalar reverses of csrc/rnde_track_rec.h, checked by a program of its own (tests/test_node_tiled_track_host.py compiles and runs it; no
// GPU is touched): init_rev_phase1 / init_rev_phase2 against central finite differences of the initial-step rule, and ff_att_rec's eight
// coefficients against finite differences of the PI controller, both forward rules written here in double beside them; and the two record
// builders of csrc/rnde_tile_host.h (the accepted steps and the attempts a reverse sweep walks) on written-down step logs, against records
// written out by hand.  Prints one line per failed check; exit status 0 when there is none.
#include "rnde_tile_host.h"
#include "rnde_track_rec.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

using namespace rnde;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static bool close_to(const char* what, const char* name, double got, double want, double scale) {
    const bool ok = std::fabs(got - want) <= 1e-4 * std::max(std::fabs(want), scale);      // (the records hold floats: 6e-8 relative on every field)
    if (!ok) { std::printf("FAILED %s / %s: reverse %.9g, finite difference %.9g\n", what, name, got, want); ++failures; }
    return ok;
}

// ---- the initial-step rule (rnde_tile_solve_kernel and advance_state_t, n == 0) over its scalars ----
// n2 = rms((f1 - f0) / sk) depends on dt0 through u1 = x + dt0 f0 and through the time t0 + dt0: modelled as n2 = n2b + kd dt0 + kt (t0 + dt0),
// so that the two sums of phase 1's VJP are dot = kd n2-bar and tau = kt n2-bar.
struct InitIn { double d0, d1, n2b, kd, kt, t0, t1; };
static double init_fwd(const InitIn& in, InitRec* rec, double* n2_out) {
    const double dtmax = in.t1 - in.t0;
    double dt0; int c0 = 0, cl = 0;
    if (in.d0 < 1e-5 || in.d1 < 1e-5) { dt0 = 1e-6; c0 = 1; }
    else dt0 = (in.d0 / in.d1) / 100.0;
    if (dtmax < dt0) { dt0 = dtmax; cl = 1; }
    const double n2 = in.n2b + in.kd * dt0 + in.kt * (in.t0 + dt0);
    const double d2 = n2 / dt0, m = in.d1 > d2 ? in.d1 : d2;
    double dt1; int c1 = 0;
    if (m <= 1e-15) { dt1 = std::max(1e-6, dt0 * 1e-3); c1 = 1; }
    else dt1 = std::pow(10.0, -(2.0 + std::log10(m)) / 5.0);
    double dt = 100.0 * dt0; int sel = 0;
    if (dt1 < dt) { dt = dt1; sel = 1; }
    if (dtmax < dt) { dt = dtmax; sel = 2; }
    if (rec) {
        rec->d0 = (float)in.d0; rec->d1 = (float)in.d1; rec->d2 = (float)d2; rec->dt0 = (float)dt0; rec->dt1 = (float)dt1; rec->dt = (float)dt;
        rec->dt0_const = c0; rec->dt0_clamped = cl; rec->sel = sel; rec->dt1_const = c1; rec->max_is_d2 = d2 >= in.d1; rec->pad = 0;
    }
    if (n2_out) *n2_out = n2;
    return dt;
}
static double init_fd(InitIn in, double InitIn::*field) {
    const bool time = field == &InitIn::t0 || field == &InitIn::t1;
    const double x = in.*field, h = 1e-6 * (time ? std::max(std::fabs(x), 1e-3) : std::fabs(x));      // (norms: a relative step, so that no branch flips)
    in.*field = x + h; const double a = init_fwd(in, nullptr, nullptr);
    in.*field = x - h; const double b = init_fwd(in, nullptr, nullptr);
    return (a - b) / (2 * h);
}
static void check_init(const char* what, const InitIn& in, int sel, int dt1_const, int max_is_d2, int dt0_const, int dt0_clamped) {
    InitRec ir;
    double n2;
    const double dt = init_fwd(in, &ir, &n2);
    CHECK(ir.sel == sel && ir.dt1_const == dt1_const && ir.dt0_const == dt0_const && ir.dt0_clamped == dt0_clamped);
    if (sel == 1 && !dt1_const) CHECK(ir.max_is_d2 == max_is_d2);
    const double N = 12.0, dtb = 1.7;      // (N divides out: coef_w N n2 is n2-bar)
    const InitBar1 b1 = init_rev_phase1(ir, dtb, N);
    const double n2bar = b1.coef_w * N * n2;
    const InitBar2 b2 = init_rev_phase2(ir, b1, in.kd * n2bar, in.kt * n2bar);
    close_to(what, "d0", b2.d0b, dtb * init_fd(in, &InitIn::d0), 1e-9 * dt);
    close_to(what, "d1", b2.d1b, dtb * init_fd(in, &InitIn::d1), 1e-9 * dt);
    close_to(what, "n2", n2bar, dtb * init_fd(in, &InitIn::n2b), 1e-9 * dt);
    close_to(what, "t0", b2.t0b, dtb * init_fd(in, &InitIn::t0), 1e-9);
    close_to(what, "t1", b2.t1b, dtb * init_fd(in, &InitIn::t1), 1e-9);
}

// ---- the PI controller (advance_state_t, n > 0) over its scalars ----
struct CtlIn { double eest, dt, t, qold; };
struct CtlOut { double t, dtp, qold; };
static CtlOut ctl_fwd(const CtlIn& in, bool accept, double dtmax, StepMeta* m) {
    const double b1 = (double)kBeta1, b2 = (double)kBeta2, g = (double)kGamma, lo = 1.0 / (double)kQmax, hi = 1.0 / (double)kQmin;
    int flags = 0;
    const double q11 = std::pow(in.eest, b1);
    double q = q11 / std::pow(in.qold, b2);
    const double qg = q / g;
    if (qg < lo) { q = lo; flags |= F_QCLAMP; }
    else if (qg > hi) { q = hi; flags |= F_QCLAMP; }
    else q = qg;
    CtlOut o{in.t, 0.0, in.qold};
    double rej_m = 0.0;
    if (accept) {
        flags |= F_ACCEPT;
        o.qold = in.eest > (double)kQoldInit ? in.eest : (double)kQoldInit;
        o.dtp = in.dt / q;
        if (dtmax < o.dtp) { o.dtp = dtmax; flags |= F_DTMAXCLAMP; }
        o.t = in.t + in.dt;
    } else {
        rej_m = hi;
        const double m2 = q11 / g;
        if (m2 < rej_m) { rej_m = m2; flags |= F_REJQ11; }
        o.dtp = in.dt / rej_m;
    }
    if (m) {
        *m = StepMeta{};
        m->t = (float)in.t; m->dt = (float)in.dt; m->dtp_in = (float)in.dt; m->eest = (float)in.eest; m->q11 = (float)q11; m->q = (float)q;
        m->qold_in = (float)in.qold; m->rej_m = (float)rej_m; m->flags = flags;
    }
    return o;
}
static CtlOut ctl_fd(CtlIn in, double CtlIn::*field, bool accept, double dtmax) {
    const double x = in.*field, h = 1e-6 * std::fabs(x);
    in.*field = x + h; const CtlOut a = ctl_fwd(in, accept, dtmax, nullptr);
    in.*field = x - h; const CtlOut b = ctl_fwd(in, accept, dtmax, nullptr);
    return CtlOut{(a.t - b.t) / (2 * h), (a.dtp - b.dtp) / (2 * h), (a.qold - b.qold) / (2 * h)};
}
static void check_ctl(const char* what, const CtlIn& in, bool accept, double dtmax, int want_flags) {
    StepMeta m;
    ctl_fwd(in, accept, dtmax, &m);
    CHECK(m.flags == want_flags);
    const float svb = 0.75f;
    const FfAttRec a = ff_att_rec(m, svb, 3);
    CHECK(a.rec == 3 && a.flags == m.flags && a.t == m.t && a.dt == m.dt && a.eest == m.eest);
    const CtlOut de = ctl_fd(in, &CtlIn::eest, accept, dtmax), dd = ctl_fd(in, &CtlIn::dt, accept, dtmax), dq = ctl_fd(in, &CtlIn::qold, accept, dtmax);
    close_to(what, "e_dtp", a.e_dtp, de.dtp, 1e-9);
    close_to(what, "e_q", a.e_q, de.qold, 1e-9);
    close_to(what, "d_t", a.d_t, dd.t, 1e-9);
    close_to(what, "d_dtp", a.d_dtp, dd.dtp, 1e-9);
    close_to(what, "c_dtp", a.c_dtp, dq.dtp, 1e-9);
    close_to(what, "c_q", a.c_q, dq.qold, 1e-9);
    // the saved value EEst * dt of an accepted attempt, cotangent svb
    close_to(what, "e0", a.e0, accept ? (double)svb * in.dt : 0.0, 1e-12);
    close_to(what, "d0", a.d0, accept ? (double)svb * in.eest : 0.0, 1e-12);
}

// ---- the record builders (tile_step_recs, tile_att_recs) on written-down step logs; every number is a dyadic fraction, so == is exact ----
static StepMeta log_entry(float t, float dt, float eest, int flags) {
    StepMeta m{};
    m.t = t; m.dt = dt; m.dtp_in = dt; m.eest = eest; m.q11 = 1.f; m.q = 1.f; m.qold_in = 1.f; m.rej_m = 2.f; m.flags = flags;
    return m;
}
struct StepWant { float t, dt, eest, svb; };
struct AttWant { float t, dt, eest; int flags, rec; double e0, d0; };
template <int NS, int NA>
static void check_records(const char* what, const std::vector<StepMeta>& log, const float* bar, bool skip_first, const StepWant (&sw)[NS], const AttWant (&aw)[NA]) {
    std::vector<FfStepRec> rec{FfStepRec{9.f, 9.f, 9.f, 9.f}};      // (the builders clear what they are given)
    std::vector<FfAttRec> att(7);
    tile_step_recs(log.data(), (int)log.size(), bar, skip_first, rec);
    tile_att_recs(log.data(), (int)log.size(), rec, att);
    if (rec.size() != (size_t)NS || att.size() != (size_t)NA) { std::printf("FAILED %s: %zu step and %zu attempt records\n", what, rec.size(), att.size()); ++failures; return; }
    for (int i = 0; i < NS; ++i)
        if (!(rec[i].t == sw[i].t && rec[i].dt == sw[i].dt && rec[i].eest == sw[i].eest && rec[i].svb == sw[i].svb)) { std::printf("FAILED %s: step record %d\n", what, i); ++failures; }
    for (int i = 0; i < NA; ++i) {
        const FfAttRec& a = att[i];
        const FfAttRec c = ff_att_rec(log[i], 0.f, 0);        // (the controller's coefficients do not depend on svb: checked above)
        if (!(a.t == aw[i].t && a.dt == aw[i].dt && a.eest == aw[i].eest && a.flags == aw[i].flags && a.rec == aw[i].rec && a.e0 == aw[i].e0 && a.d0 == aw[i].d0 &&
              a.e_dtp == c.e_dtp && a.e_q == c.e_q && a.d_t == c.d_t && a.d_dtp == c.d_dtp && a.c_dtp == c.c_dtp && a.c_q == c.c_q)) {
            std::printf("FAILED %s: attempt record %d\n", what, i); ++failures;
        }
    }
}
static void check_builders() {
    const int A = F_ACCEPT, J = F_REJQ11;
    // a rejected first attempt, a rejection between accepted steps, the last step clamped to t1
    const std::vector<StepMeta> first{log_entry(0.f, 0.5f, 2.5f, J), log_entry(0.f, 0.25f, 0.5f, A), log_entry(0.25f, 0.25f, 0.25f, A), log_entry(0.5f, 1.f, 3.f, 0),
                                      log_entry(0.5f, 0.5f, 0.125f, A | F_CLAMP)};
    const float bar_on[4] = {9.f, 0.5f, 0.25f, 0.75f}, bar_off[3] = {0.5f, 0.25f, 0.75f};
    const StepWant sw[3] = {{0.f, 0.25f, 0.5f, 0.5f}, {0.25f, 0.25f, 0.25f, 0.25f}, {0.5f, 0.5f, 0.125f, 0.75f}};
    const AttWant aw[5] = {{0.f, 0.5f, 2.5f, J, 0, 0.0, 0.0}, {0.f, 0.25f, 0.5f, A, 0, 0.125, 0.25}, {0.25f, 0.25f, 0.25f, A, 1, 0.0625, 0.0625},
                           {0.5f, 1.f, 3.f, 0, 2, 0.0, 0.0}, {0.5f, 0.5f, 0.125f, A | F_CLAMP, 2, 0.375, 0.09375}};
    check_records("rejected first attempt, cb_save_start on", first, bar_on, true, sw, aw);
    check_records("rejected first attempt, cb_save_start off", first, bar_off, false, sw, aw);
    const StepWant sw0[3] = {{0.f, 0.25f, 0.5f, 0.f}, {0.25f, 0.25f, 0.25f, 0.f}, {0.5f, 0.5f, 0.125f, 0.f}};
    const AttWant aw0[5] = {{0.f, 0.5f, 2.5f, J, 0, 0.0, 0.0}, {0.f, 0.25f, 0.5f, A, 0, 0.0, 0.0}, {0.25f, 0.25f, 0.25f, A, 1, 0.0, 0.0}, {0.5f, 1.f, 3.f, 0, 2, 0.0, 0.0},
                            {0.5f, 0.5f, 0.125f, A | F_CLAMP, 2, 0.0, 0.0}};
    check_records("null saveval_bar", first, nullptr, false, sw0, aw0);
    check_records("null saveval_bar, cb_save_start on", first, nullptr, true, sw0, aw0);
    // rejected attempts behind the last accepted one (a solve that ran into max_attempts): trimmed from the attempt records
    const std::vector<StepMeta> tail{log_entry(0.f, 0.25f, 0.5f, A), log_entry(0.25f, 0.5f, 0.25f, A), log_entry(0.75f, 0.5f, 4.f, J), log_entry(0.75f, 0.25f, 2.f, J)};
    const StepWant tw[2] = {{0.f, 0.25f, 0.5f, 0.25f}, {0.25f, 0.5f, 0.25f, 0.75f}};
    const AttWant ta[2] = {{0.f, 0.25f, 0.5f, A, 0, 0.0625, 0.125}, {0.25f, 0.5f, 0.25f, A, 1, 0.375, 0.1875}};
    check_records("rejections behind the last accepted step", tail, bar_on + 2, false, tw, ta);
    check_records("rejections behind the last accepted step, cb_save_start on", tail, bar_on + 1, true, tw, ta);
    // a log with no accepted step: no record of either kind
    std::vector<FfStepRec> rec;
    std::vector<FfAttRec> att;
    const std::vector<StepMeta> none{log_entry(0.f, 0.5f, 2.5f, J)};
    tile_step_recs(none.data(), 1, nullptr, false, rec);
    tile_att_recs(none.data(), 1, rec, att);
    CHECK(rec.empty() && att.empty());
}

int main() {
    // ---- the initial step: every branch of the rule ----
    //                                   d0    d1   n2b    kd     kt    t0   t1     sel c1 mx c0 cl
    check_init("sel 0", InitIn{0.01, 1.0, 1e-5, 0.0, 0.0, 0.0, 1.0}, 0, 0, 0, 0, 0);
    check_init("sel 0, u1 and time terms", InitIn{0.01, 1.0, 1e-5, 2e-2, 1e-5, 0.1, 1.0}, 0, 0, 0, 0, 0);
    check_init("sel 1, max is d1", InitIn{1.0, 1.0, 0.005, 0.0, 0.0, 0.0, 1.0}, 1, 0, 0, 0, 0);
    check_init("sel 1, max is d2", InitIn{1.0, 1.0, 0.04, 0.5, 0.3, 0.2, 1.2}, 1, 0, 1, 0, 0);
    check_init("sel 2", InitIn{1.0, 1.0, 0.04, 0.5, 0.3, 0.0, 0.2}, 2, 0, 1, 0, 0);
    check_init("dt0 constant, sel 0", InitIn{1e-6, 1.0, 1e-6, 0.0, 0.0, 0.0, 1.0}, 0, 0, 0, 1, 0);
    check_init("dt0 constant, sel 1", InitIn{1e-6, 1.0, 1e13, 3.0, 2.0, 0.0, 1.0}, 1, 0, 1, 1, 0);
    check_init("dt1 constant", InitIn{1e-6, 1e-16, 1e-24, 0.0, 0.0, 0.0, 1.0}, 1, 1, 0, 1, 0);
    check_init("dt0 clamped, sel 2", InitIn{1.0, 1.0, 0.005, 0.1, 0.1, 0.0, 0.005}, 2, 0, 1, 0, 1);
    check_init("dt0 clamped, sel 1", InitIn{1.0, 1.0, 5e7, 3.0, 2.0, 0.1, 0.105}, 1, 0, 1, 0, 1);
    // ---- the controller: accepted, rejected (rej_m = q11 / gamma, rej_m = 1 / qmin), q at its clamp, dtp' = t1 - t0 ----
    check_ctl("accepted", CtlIn{0.3, 0.05, 0.2, 0.2}, true, 1.0, F_ACCEPT);
    check_ctl("accepted, qold' = qoldinit", CtlIn{5e-5, 0.05, 0.2, 0.2}, true, 1.0, F_ACCEPT);
    check_ctl("rejected, rej_m = q11 / gamma", CtlIn{1.7, 0.05, 0.2, 0.2}, false, 1.0, F_REJQ11);
    check_ctl("rejected, rej_m = 1 / qmin", CtlIn{1e5, 0.05, 0.2, 10.0}, false, 1.0, 0);
    check_ctl("accepted, F_QCLAMP", CtlIn{1e-12, 0.05, 0.2, 1e-4}, true, 1.0, F_ACCEPT | F_QCLAMP);
    check_ctl("rejected, F_QCLAMP", CtlIn{1e6, 0.05, 0.2, 1e-4}, false, 1.0, F_QCLAMP);
    check_ctl("accepted, F_DTMAXCLAMP", CtlIn{2e-4, 0.5, 0.2, 0.2}, true, 1.0, F_ACCEPT | F_DTMAXCLAMP);
    check_builders();
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("track host checks passed\n");
    return 0;
}
