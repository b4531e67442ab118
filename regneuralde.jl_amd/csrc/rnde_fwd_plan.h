// rnde_fwd_plan.h -- what the host decides around a forward solve and derives from its attempt log, each rule stated once: the value the saving
// callback records (callback_value) beside its derivative (eig_cotangent, used by the reverse passes), which attempts saved a value
// (gather_saved_values), where the accepted steps ended (step_end_times), what the controller's final status means to the caller (solve_verdict),
// the two exports of an attempt log (export_steps, export_step_log), and the sizing rules of the solve forms.  Kernel-free in the manner of
// rnde_rev_plan.h (which includes this header): plain C++, templates over the record type (StepMeta, or any record with the fields named), so
// a host program can include it alone (tests/save_host/fwd_plan_check.cpp).
#pragma once
#include "../../include/rnde.h"      // rnde_reg
#include <algorithm>
#include <cmath>
#include <vector>

namespace rnde {

// ---- the saving callback: func(u, t, integrator) of the reference -- EEst*dt (mnist_node.jl:67), stab*|eigen_est| (:74-79), their blend (:88-97)
constexpr double kStabilitySize = 3.5068;      // alg_stability_size(Tsit5()), as recalled in SURVEY.md 8a row a9
static_assert((float)kStabilitySize == 3.5068f && (float)0.1 == 0.1f, "the fp32 rule's constants are the float literals");
template <class T>
inline bool estimate_counts(T v) { return !(v == T(0) || v != v); }      // an estimate (eigen_est, EEst * dt) counts unless it is zero or NaN

// The value saved for one step.  T = float (what the solve's epilogue calls): the fp32 expressions it has always formed -- stab = 1.0f / 3.5068f is
// multiplied, not divided by; the blend's weight is 0.1f.  T = double: the same rule for a host check to differentiate (eig_cotangent below).
template <class T>
inline T callback_value(int reg_kind, T eest, T dt, T eigen) {
    const T stab = T(1) / T(kStabilitySize);
    const bool eg_ok = estimate_counts(eigen);
    switch (reg_kind) {
        case RNDE_REG_ERR: return eest * dt;
        case RNDE_REG_STIFF: return eg_ok ? stab * std::fabs(eigen) : T(0);
        case RNDE_REG_ERR_STIFF: { const T e = eest * dt; return (estimate_counts(e) ? e : T(0)) + T(0.1) * (eg_ok ? stab * eigen : T(0)); }
        case RNDE_REG_STIFF_DT: return std::fabs(eigen * dt);      // test/test_node.jl:75: abs(integrator.eigen_est * integrator.dt)
        default: return T(0);
    }
}

// Cotangent coefficients of eigen_est = n1 / n2 for one attempt: the kernels add c1 * (k7 - k6) and c2 * (unew - g6) (n1, n2: the norms of the
// two differences), so c1 n1 and c2 n2 are the derivatives of callback_value in n1 and n2.  svb: the cotangent of the value the callback
// saved for this attempt; mm.eigen, mm.n1, mm.n2, mm.dt: the attempt's record.  svb |eigen| / S (RNDE_REG_STIFF), 0.1 svb eigen / S (the
// stiffness term of RNDE_REG_ERR_STIFF), svb |eigen dt| (RNDE_REG_STIFF_DT); (0, 0) for every other kind, for an estimate that does not count
// and for a zero norm.  Arithmetic in double, rounded to fp32 at the end: the results are kernel arguments.
template <class Rec>
inline void eig_cotangent(int reg_kind, float svb, const Rec& mm, float* c1, float* c2) {
    *c1 = 0.f; *c2 = 0.f;
    const bool eg_ok = estimate_counts(mm.eigen);
    const double S = kStabilitySize;
    double eigb = 0.0;
    if (reg_kind == RNDE_REG_STIFF && eg_ok) eigb = (double)svb * (mm.eigen > 0 ? 1.0 : -1.0) / S;
    if (reg_kind == RNDE_REG_ERR_STIFF && eg_ok) eigb = 0.1 * (double)svb / S;
    if (reg_kind == RNDE_REG_STIFF_DT && eg_ok) eigb = (double)svb * ((double)mm.eigen * (double)mm.dt > 0 ? 1.0 : -1.0) * (double)mm.dt;
    if (eigb != 0.0 && mm.n1 > 0.f && mm.n2 > 0.f) {
        *c1 = (float)(eigb / ((double)mm.n2 * (double)mm.n1));
        *c2 = (float)(-eigb * ((double)mm.n1 / (double)mm.n2) / ((double)mm.n2 * (double)mm.n2));
    }
}

// Saving callback values (reference neural_ode.jl:116, :126-127): one per ACCEPTED attempt (att[n].flags & accept_flag; .eest, .dt, .eigen), in
// front of them the value at init when cb_save_start (EEst = 1, dt = 0, eigen_est = 1: SURVEY B.5); none under RNDE_REG_NONE.  sv_index[n]: where
// attempt n's value sits, or -1 (may be null); values (may be null: the count alone): the values themselves.  Returns their number.
template <class Rec>
inline int gather_saved_values(const Rec* att, int n_att, int accept_flag, int reg_kind, bool cb_save_start, int* sv_index, float* values) {
    int nsv = 0;
    if (sv_index) for (int n = 0; n < n_att; ++n) sv_index[n] = -1;
    if (reg_kind == RNDE_REG_NONE) return 0;
    if (cb_save_start) { if (values) values[nsv] = callback_value(reg_kind, 1.f, 0.f, 1.f); ++nsv; }
    for (int n = 0; n < n_att; ++n)
        if (att[n].flags & accept_flag) {
            if (values) values[nsv] = callback_value(reg_kind, att[n].eest, att[n].dt, att[n].eigen);
            if (sv_index) sv_index[n] = nsv;
            ++nsv;
        }
    return nsv;
}

// What the controller's final status (StepState.status, written by advance_state in rnde_fwd.h: 0 the span is done, 2 max_attempts, 3 dt at
// or below kDtMin, 4 a non-finite dt or error estimate) means to the caller.  Any other nonzero value reads as non-finite, as it always has.
struct SolveVerdict { rnde_status st; const char* msg; };
inline SolveVerdict solve_verdict(int ctl_status) {
    switch (ctl_status) {
        case 0: return {RNDE_OK, ""};
        case 2: return {RNDE_ERR_MAX_ATTEMPTS, "max_attempts reached"};
        case 3: return {RNDE_ERR_DT_UNDERFLOW, "dt underflow"};
        default: return {RNDE_ERR_NONFINITE, "non-finite error estimate or dt"};
    }
}

// The exports of an attempt log: (dt, accepted) per attempt, what a replay takes back (out: 2 n floats), and (t, dt, EEst, accepted) (4 n).
template <class Rec>
inline void export_steps(const Rec* att, int n, int accept_flag, float* out) {
    for (int i = 0; i < n; ++i) { out[2 * i] = att[i].dt; out[2 * i + 1] = (att[i].flags & accept_flag) ? 1.f : 0.f; }
}
template <class Rec>
inline void export_step_log(const Rec* att, int n, int accept_flag, float* out) {
    for (int i = 0; i < n; ++i) {
        out[4 * i] = att[i].t; out[4 * i + 1] = att[i].dt; out[4 * i + 2] = att[i].eest; out[4 * i + 3] = (att[i].flags & accept_flag) ? 1.f : 0.f;
    }
}

// Where the accepted steps of a solve ended: t + dt in fp32, as the controller forms it, clamped to t1 (the last step ends at t1 exactly whenever
// t >= t1 / 2); t0 in front when save_start.  A rejected attempt ends nowhere.
template <class Rec>
inline std::vector<float> step_end_times(const Rec* att, int n_att, int accept_flag, float t0, float t1, bool save_start) {
    std::vector<float> times;
    if (save_start) times.push_back(t0);
    for (int n = 0; n < n_att; ++n)
        if (att[n].flags & accept_flag) { float tn = att[n].t + att[n].dt; if (tn > t1) tn = t1; times.push_back(tn); }
    return times;
}

// ---- sizing rules (cap: max_attempts; predicted: one more than the last solve's attempts) ----
// A taped one-launch multi-wave solve writes every layer input of every evaluation: its slab is sized for twice the last solve's attempts (at
// least 48); a solve that needs more ends at that limit and is redone with room for max_attempts.
inline int mw_taped_attempt_limit(int cap, int predicted) { return std::min(cap, std::max(48, 2 * predicted)); }
// Step records the one-launch stage solve copies speculatively; a longer solve fetches the rest afterwards.
inline int stage_speculative_records(int cap, int predicted) { return std::min(cap, std::max(64, 2 * predicted)); }
// Attempts enqueued between two looks at the controller state: the first chunk is normally the whole solve.  Coupled: the same launch count on
// every rank, whatever its history.
inline int first_chunk(bool coupled, int predicted) { return coupled ? 16 : std::max(4, predicted); }
inline int later_chunk(bool coupled) { return coupled ? 16 : 4; }
// A one-launch kernel that gave up gets another chance after `window` clean solves; each new failure doubles the wait.
inline int next_retry_window(int window) { return std::min(1024, 2 * window); }
// 2 (initial dt) + 1 (fsalfirst) + 6 per attempt (S - 1 for an S-stage table), SURVEY.md B.1-B.2
inline int64_t solve_nfe(int rk_S, int n_att) { return 3 + (int64_t)(rk_S - 1) * n_att; }
// saveat must be increasing and inside [t0, t1] (a NaN is neither)
inline bool saveat_valid(const float* sv, int n, float t0, float t1) {
    for (int i = 0; i < n; ++i)
        if (!(sv[i] >= t0 && sv[i] <= t1) || (i > 0 && !(sv[i] > sv[i - 1]))) return false;
    return true;
}

}  // namespace rnde
