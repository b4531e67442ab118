// rnde_rev_plan.h -- what the host derives from the attempt log of a recorded solve for the reverse sweeps, each rule stated once: which saveat
// indices an attempt covers (save_plan), the evaluation times of the chain engines' slabs (eval_times) and the saved-value cotangent per attempt
// (gather_svb); the eigen_est cotangent coefficients of an attempt (eig_cotangent) sit beside the callback's value in rnde_fwd_plan.h.  Kernel-free: plain C++, no device symbol, templates over
// the record type, so a host program can include it alone (tests/save_host/save_plan_check.cpp).
//
// The save rule, in the controller's own float comparisons (rnde_fwd.h, advance_state_t: next_save): index 0 belongs to the start when
// sv[0] == t0 (save_start: it is x itself, no attempt covers it); an ACCEPTED attempt from t to tnew = t + dt (fp32, as the controller forms it)
// covers every index not yet covered whose time is <= tnew -- so a time exactly at a step's end belongs to that step (a copy of unew, no
// interpolation) and not to the next one; a rejected attempt covers nothing.  The ranges [lo[n], hi[n]) are consecutive: together with the start
// they partition 0 .. the value returned, which is n_save whenever the solve reached the last save time.
#pragma once
#include "rnde_fwd_plan.h"           // callback_value and its derivative, eig_cotangent

namespace rnde {

struct SaveRange { int lo, hi; };      // save indices [lo, hi) of one attempt

// att[n].t, att[n].dt, att[n].flags (StepMeta, or any record with these fields); accept_flag: F_ACCEPT.  out: n_att ranges.
// Returns the number of indices covered (the start's included).
template <class Rec>
inline int save_plan(const float* sv, int n_save, float t0, const Rec* att, int n_att, int accept_flag, SaveRange* out) {
    int ns = (n_save > 0 && sv[0] == t0) ? 1 : 0;
    for (int n = 0; n < n_att; ++n) {
        out[n].lo = ns;
        if (att[n].flags & accept_flag) {
            const float tnew = att[n].t + att[n].dt;
            while (ns < n_save && sv[ns] <= tnew) ++ns;
        }
        out[n].hi = ns;
    }
    return ns;
}

// Evaluation times of a chain engine's slab (the time column of TDChain layers in the weight-gradient kernel): E per attempt, stage s = 2 .. E + 1
// of attempt n at att[n].t + c[s - 1] * att[n].dt (c: the nodes of the pair, c[0] = 0), and the two evaluations of the initial-step rule, f(u0, t0)
// and f(u1, t0 + dt0) -- in front of the attempts (init_first: the multi-wave slab) or behind them (the one-wave slab).  out: E * n_att + 2 times.
template <class Rec>
inline void eval_times(const Rec* att, int n_att, int E, const float* c, float t0, float dt0, bool init_first, float* out) {
    float* const init = init_first ? out : out + (long long)E * n_att;
    float* const ev = init_first ? out + 2 : out;
    init[0] = t0; init[1] = t0 + dt0;
    for (int n = 0; n < n_att; ++n)
        for (int s = 1; s <= E; ++s) ev[(long long)E * n + s - 1] = att[n].t + c[s] * att[n].dt;
}

// Saved-value cotangent per attempt: scale * saveval_bar[sv_index[n]] where the callback fired for attempt n (sv_index[n] >= 0), else 0; all
// zeros without a cotangent (saveval_bar == nullptr).  scale: the world size under a coupled controller (rnde_node_set_coupling), else 1.
inline void gather_svb(const int* sv_index, int n_att, float scale, const float* saveval_bar, float* out) {
    for (int n = 0; n < n_att; ++n) out[n] = (saveval_bar && sv_index[n] >= 0) ? scale * saveval_bar[sv_index[n]] : 0.f;
}

}  // namespace rnde
