// The scalar reverses of csrc/rnde_track_rec.h, checked by a program of its own (tests/test_node_tiled_track_host.py compiles and runs it; no
// GPU is touched): init_rev_phase1 / init_rev_phase2 against central finite differences of the initial-step rule, and ff_att_rec's eight
// coefficients against finite differences of the PI controller, both forward rules written here in double beside them; and the two record
// builders of csrc/rnde_tile_host.h (the accepted steps and the attempts a reverse sweep walks) on written-down step logs, against records
// written out by hand; the map from the controller's final status to the call's, the saved values and the two exports of written-down step
// logs; and tile_step_params against the StepParams of its three users, written out by hand.  Prints one line per failed check; exit
// status 0 when there is none.
#include "rnde_group_plan.h"
#include "rnde_tile_host.h"
#include "rnde_track_rec.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

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

// ---- behind a solve: the status map, the saved values and the two exports of a step log (rnde_fwd_plan.h, rnde_tile_host.h) ----
static void check_status_map() {
    // what advance_state (rnde_fwd.h) can write: 0, 2, 3, 4; and values it cannot
    const struct { int ctl; rnde_status st; const char* msg; } want[] = {
        {0, RNDE_OK, ""}, {2, RNDE_ERR_MAX_ATTEMPTS, "max_attempts reached"}, {3, RNDE_ERR_DT_UNDERFLOW, "dt underflow"},
        {4, RNDE_ERR_NONFINITE, "non-finite error estimate or dt"}, {1, RNDE_ERR_NONFINITE, "non-finite error estimate or dt"},
        {7, RNDE_ERR_NONFINITE, "non-finite error estimate or dt"}, {-1, RNDE_ERR_NONFINITE, "non-finite error estimate or dt"}};
    for (const auto& w : want) {
        const SolveVerdict v = solve_verdict(w.ctl);
        CHECK(v.st == w.st && std::string(v.msg) == w.msg);
    }
    CHECK(group_failure(3, 2) == "TrackedFFJORD groups: group 3: max_attempts reached");
    CHECK(group_failure(0, 3) == "TrackedFFJORD groups: group 0: dt underflow");
    CHECK(group_failure(15, 4) == "TrackedFFJORD groups: group 15: non-finite error estimate or dt");
}

template <int NV>
static void check_log(const char* what, const std::vector<StepMeta>& log, const float (&sv_on)[NV + 1], const float* steps, const float* wide) {
    const int n = (int)log.size();
    // the saved values: with the value at init in front (cb_save_start), without it, without a regulariser; each also count-only
    float got[NV + 2];
    for (int start = 0; start < 2; ++start) {
        for (float& g : got) g = 77.f;
        const int cnt = gather_saved_values(log.data(), n, F_ACCEPT, RNDE_REG_ERR, start != 0, nullptr, got);
        bool ok = cnt == NV + start && gather_saved_values(log.data(), n, F_ACCEPT, RNDE_REG_ERR, start != 0, nullptr, (float*)nullptr) == cnt && got[cnt] == 77.f;
        for (int i = 0; ok && i < cnt; ++i) ok = got[i] == sv_on[i + 1 - start];
        if (!ok) { std::printf("FAILED %s: saved values, cb_save_start %d\n", what, start); ++failures; }
        for (float& g : got) g = 77.f;
        if (gather_saved_values(log.data(), n, F_ACCEPT, RNDE_REG_NONE, start != 0, nullptr, got) != 0 || gather_saved_values(log.data(), n, F_ACCEPT, RNDE_REG_NONE, start != 0, nullptr, (float*)nullptr) != 0 || got[0] != 77.f) {
            std::printf("FAILED %s: saved values without a regulariser\n", what); ++failures;
        }
    }
    std::vector<float> a(2 * n + 1, 77.f), b(4 * n + 1, 77.f);
    export_steps(log.data(), n, F_ACCEPT, a.data());
    export_step_log(log.data(), n, F_ACCEPT, b.data());
    if (!std::equal(steps, steps + 2 * n, a.begin()) || a[2 * n] != 77.f) { std::printf("FAILED %s: the (dt, accepted) export\n", what); ++failures; }
    if (!std::equal(wide, wide + 4 * n, b.begin()) || b[4 * n] != 77.f) { std::printf("FAILED %s: the (t, dt, eest, accepted) export\n", what); ++failures; }
}
static void check_logs() {
    const int A = F_ACCEPT, J = F_REJQ11;
    const float none_f[1] = {0.f};
    check_log<0>("no attempt", {}, {0.f}, none_f, none_f);
    {
        const float s[2] = {0.25f, 1.f}, w[4] = {0.f, 0.25f, 0.5f, 1.f};
        check_log<1>("one accepted attempt", {log_entry(0.f, 0.25f, 0.5f, A | F_CLAMP)}, {0.f, 0.125f}, s, w);
    }
    {
        const float s[2] = {0.5f, 0.f}, w[4] = {0.f, 0.5f, 2.5f, 0.f};
        check_log<0>("one rejected attempt", {log_entry(0.f, 0.5f, 2.5f, J)}, {0.f}, s, w);
    }
    {
        const float s[8] = {0.25f, 1.f, 0.25f, 1.f, 0.25f, 1.f, 0.25f, 1.f};
        const float w[16] = {0.f, 0.25f, 0.5f, 1.f, 0.25f, 0.25f, 0.25f, 1.f, 0.5f, 0.25f, 2.f, 1.f, 0.75f, 0.25f, 0.125f, 1.f};
        check_log<4>("four accepted attempts", {log_entry(0.f, 0.25f, 0.5f, A), log_entry(0.25f, 0.25f, 0.25f, A), log_entry(0.5f, 0.25f, 2.f, A),
                                                 log_entry(0.75f, 0.25f, 0.125f, A | F_CLAMP)},
                     {0.f, 0.125f, 0.0625f, 0.5f, 0.03125f}, s, w);
    }
    {
        const float s[8] = {0.5f, 0.f, 0.25f, 1.f, 1.f, 0.f, 0.75f, 1.f};
        const float w[16] = {0.f, 0.5f, 2.5f, 0.f, 0.f, 0.25f, 0.5f, 1.f, 0.25f, 1.f, 3.f, 0.f, 0.25f, 0.75f, 0.125f, 1.f};
        check_log<2>("four attempts, two rejected", {log_entry(0.f, 0.5f, 2.5f, J), log_entry(0.f, 0.25f, 0.5f, A), log_entry(0.25f, 1.f, 3.f, 0),
                                                      log_entry(0.25f, 0.75f, 0.125f, A | F_CLAMP)},
                     {0.f, 0.125f, 0.09375f}, s, w);
    }
}

// ---- tile_step_params against the StepParams of its three users, written out by hand ----
static bool same_params(const StepParams& a, const StepParams& b) {
    return a.x == b.x && a.f0 == b.f0 && a.h0 == b.h0 && a.u1 == b.u1 && a.f1 == b.f1 && a.h1 == b.h1 && a.arena == b.arena && a.rec_stride == b.rec_stride &&
           a.ctl == b.ctl && a.ctl_final == b.ctl_final && a.meta == b.meta && a.initrec == b.initrec && a.errpart == b.errpart && a.initpart == b.initpart &&
           a.dbg_out == b.dbg_out && a.D == b.D && a.H == b.H && a.B == b.B && a.Bpad == b.Bpad && a.nwg == b.nwg && a.Bn == b.Bn && a.reltol == b.reltol &&
           a.abstol == b.abstol && a.t0 == b.t0 && a.t1 == b.t1 && a.tape == b.tape && a.max_attempts == b.max_attempts && a.forced == b.forced &&
           a.forced_t == b.forced_t && a.forced_dt == b.forced_dt && a.rec_shift == b.rec_shift && a.xvec == b.xvec && a.reg_kind == b.reg_kind && a.sv_t == b.sv_t &&
           a.nsave == b.nsave && a.sv_out == b.sv_out && a.replay == b.replay && a.n_replay == b.n_replay && a.beta1 == b.beta1 && a.beta2 == b.beta2 &&
           a.rk_order == b.rk_order && a.esum == b.esum;
}
// (host memory behind the workspace's owners; the members are allocated by hand, as the one-workgroup engine does: alloc() itself zeroes
// norm on the device and creates the meeting place)
struct HostAlloc {
    static hipError_t get(void** p, size_t bytes) { *p = std::calloc(1, bytes ? bytes : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
    static void put(void* p) { std::free(p); }
};
using HostWs = TileSolveWsT<HostAlloc, HostAlloc>;
static void host_ws(HostWs& W, int tiles, int n_solves, bool fin_apart) {
    W.Bp = 16 * tiles; W.n_live = 2 * n_solves;
    bool ok = W.norm.alloc(8 * tiles + 512) == hipSuccess && W.ctl.alloc(fin_apart ? 2 * n_solves : 3 * n_solves) == hipSuccess &&
              W.meta.alloc(4 * n_solves) == hipSuccess && W.initrec_t.alloc(tiles) == hipSuccess;
    if (fin_apart) ok = ok && W.fin_n.alloc(n_solves) == hipSuccess;
    CHECK(ok);
}
static void check_step_params() {
    static float x[8], replay[8], sv_t[4], sv_out[4];
    const float b1 = (float)(7.0 / 50.0), b2 = (float)(2.0 / 25.0);
    HostWs F, E, G, N;
    host_ws(F, 3, 1, false);      // the tiled TrackedFFJORD handle, max_batch 40: three tiles, the final state behind the two live ones
    host_ws(G, 7, 4, true);       // a reservation of 7 tiles for 4 groups: final states of their own
    host_ws(N, 2, 1, false);      // the tiled TrackedNeuralODE, max_batch 32
    E.Bp = 64;                    // the one-workgroup FFJORD engine: ctl [3] and one record by hand, n_live as it stands
    CHECK(E.norm.alloc(512) == hipSuccess && E.ctl.alloc(3) == hipSuccess && E.meta.alloc(4) == hipSuccess && E.initrec_t.alloc(1) == hipSuccess);
    for (const int B : {1, 16, 17}) {
        // a forward along a replay, D = 2 and the kinetic rows
        StepParams w{};
        w.x = x; w.D = 5; w.B = B; w.Bn = B; w.Bpad = 48; w.nwg = 1; w.ctl = F.ctl.get(); w.ctl_final = F.ctl.get() + 2; w.meta = F.meta.get();
        w.initrec = F.initrec_t.get(); w.initpart = F.norm.get();
        w.reltol = 1e-5f; w.abstol = 1e-6f; w.t0 = 0.25f; w.t1 = 1.5f; w.tape = 1; w.max_attempts = 128; w.replay = replay; w.n_replay = 4;
        w.beta1 = b1; w.beta2 = b2; w.rk_order = 5.f;
        CHECK(same_params(tile_step_params(F, x, 5, B, 1e-5f, 1e-6f, 0.25f, 1.5f, 128, replay, 4), w));
        // ... and sampling on the one-workgroup engine: tau runs from 0 to t1 - t0, no replay (its count is dropped)
        w.D = 3; w.Bpad = 64; w.ctl = E.ctl.get(); w.ctl_final = E.ctl.get() + 2; w.meta = E.meta.get(); w.initrec = E.initrec_t.get(); w.initpart = E.norm.get();
        w.t0 = 0.f; w.t1 = 1.25f; w.replay = nullptr; w.n_replay = 0;
        CHECK(same_params(tile_step_params(E, x, 3, B, 1e-5f, 1e-6f, 0.f, 1.25f, 128, nullptr, 4), w));
        // a group call: the call's row stride (three of the seven tiles) set by the caller, B the first group's
        StepParams g = tile_step_params(G, x, 3, B, 1e-5f, 1e-5f, 0.f, 1.f, 64, nullptr, 0);
        CHECK(g.Bpad == 16 * 7);
        g.Bpad = 16 * 3;
        StepParams wg{};
        wg.x = x; wg.D = 3; wg.B = B; wg.Bn = B; wg.Bpad = 48; wg.nwg = 1; wg.ctl = G.ctl.get(); wg.ctl_final = G.fin_n.get(); wg.meta = G.meta.get();
        wg.initrec = G.initrec_t.get(); wg.initpart = G.norm.get();
        wg.reltol = 1e-5f; wg.abstol = 1e-5f; wg.t0 = 0.f; wg.t1 = 1.f; wg.tape = 1; wg.max_attempts = 64; wg.beta1 = b1; wg.beta2 = b2; wg.rk_order = 5.f;
        CHECK(same_params(g, wg));
        // the tiled TrackedNeuralODE: D rows, the saveat fields set afterwards
        StepParams n = tile_step_params(N, x, 70, B, 1e-3f, 1e-4f, -1.f, 2.f, 8000, nullptr, 0);
        n.sv_t = sv_t; n.nsave = 4; n.sv_out = sv_out;
        StepParams wn{};
        wn.x = x; wn.D = 70; wn.B = B; wn.Bn = B; wn.Bpad = 32; wn.nwg = 1; wn.ctl = N.ctl.get(); wn.ctl_final = N.ctl.get() + 2; wn.meta = N.meta.get();
        wn.initrec = N.initrec_t.get(); wn.initpart = N.norm.get();
        wn.reltol = 1e-3f; wn.abstol = 1e-4f; wn.t0 = -1.f; wn.t1 = 2.f; wn.tape = 1; wn.max_attempts = 8000; wn.sv_t = sv_t; wn.nsave = 4; wn.sv_out = sv_out;
        wn.beta1 = b1; wn.beta2 = b2; wn.rk_order = 5.f;
        CHECK(same_params(n, wn));
    }
}

int main() {
    check_status_map();
    check_logs();
    check_step_params();
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
