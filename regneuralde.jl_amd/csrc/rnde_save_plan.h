// rnde_save_plan.h -- which saveat indices each attempt of a recorded solve covers: the host's restatement of the controller's rule
// (rnde_fwd.h, advance_state_t: next_save), for the reverse sweeps.  Kernel-free: plain C++, no device symbol, so a host program can
// include it alone (tests/save_host/save_plan_check.cpp).
//
// The rule, in the controller's own float comparisons: index 0 belongs to the start when sv[0] == t0 (save_start: it is x itself, no
// attempt covers it); an ACCEPTED attempt from t to tnew = t + dt (fp32, as the controller forms it) covers every index not yet covered
// whose time is <= tnew -- so a time exactly at a step's end belongs to that step (a copy of unew, no interpolation) and not to the next
// one; a rejected attempt covers nothing.  The ranges [lo[n], hi[n]) are consecutive: together with the start they partition 0 .. the
// value returned, which is n_save whenever the solve reached the last save time.
#pragma once

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

}  // namespace rnde
