// What the host decides around a forward solve and derives from its attempt log, checked by a program of its own (tests/test_fwd_plan_host.py
// compiles and runs it; no GPU is touched): csrc/rnde_fwd_plan.h -- the saving callback's value for every kind, the eigen_est cotangent
// coefficients against central differences of that same rule, the saved values and the step ends of written-down attempt logs, and the sizing
// rules at their corners.
// Prints one line per failed check; exit status 0 when there is none.
#include "rnde_fwd_plan.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace rnde;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static const int kAccept = 1;      // (any bit: the functions take the flag)
struct Att { float t, dt, eest, eigen; int flags; };
static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// ---- callback_value: every kind, what counts as an estimate, the values at init ------------------------------------------------------------
static void callback_value_checks() {
    const float stab = 1.0f / 3.5068f, nan = std::nanf("");
    const int kinds[5] = {RNDE_REG_NONE, RNDE_REG_ERR, RNDE_REG_STIFF, RNDE_REG_ERR_STIFF, RNDE_REG_STIFF_DT};
    // at init: EEst = 1, dt = 0, eigen_est = 1
    const float init[5] = {0.f, 0.f, stab, 0.1f * stab, 0.f};
    for (int k = 0; k < 5; ++k) CHECK(same_bits(callback_value(kinds[k], 1.f, 0.f, 1.f), init[k]));
    // an ordinary step: the fp32 expressions, written out
    const float eest = 0.37f, dt = 0.0625f, eig = -2.75f;
    CHECK(same_bits(callback_value((int)RNDE_REG_NONE, eest, dt, eig), 0.f));
    CHECK(same_bits(callback_value((int)RNDE_REG_ERR, eest, dt, eig), eest * dt));
    CHECK(same_bits(callback_value((int)RNDE_REG_STIFF, eest, dt, eig), stab * 2.75f));
    CHECK(same_bits(callback_value((int)RNDE_REG_ERR_STIFF, eest, dt, eig), eest * dt + 0.1f * (stab * eig)));
    CHECK(same_bits(callback_value((int)RNDE_REG_STIFF_DT, eest, dt, eig), 2.75f * 0.0625f));
    CHECK(stab * 2.75f != 2.75f / 3.5068f);      // (this value tells the multiplication by 1 / S from a division by S: the rule is the former)
    // estimates that do not count: a zero or NaN eigen_est gives no stiffness term; the error-estimate kind passes its product on as it is
    for (float bad : {0.f, -0.f, nan}) {
        CHECK(same_bits(callback_value((int)RNDE_REG_STIFF, eest, dt, bad), 0.f));
        CHECK(same_bits(callback_value((int)RNDE_REG_ERR_STIFF, eest, dt, bad), eest * dt + 0.1f * 0.f));
    }
    CHECK(same_bits(callback_value((int)RNDE_REG_STIFF_DT, eest, dt, 0.f), 0.f));
    CHECK(std::isnan(callback_value((int)RNDE_REG_STIFF_DT, eest, dt, nan)));      // (|eigen dt| has no such test: test/test_node.jl:75)
    CHECK(same_bits(callback_value((int)RNDE_REG_ERR, 0.f, dt, eig), 0.f));
    CHECK(std::isnan(callback_value((int)RNDE_REG_ERR, nan, dt, eig)));
    // the mixed kind: a zero or NaN EEst * dt leaves the stiffness term alone (NaN * dt, and inf * 0)
    CHECK(same_bits(callback_value((int)RNDE_REG_ERR_STIFF, 0.f, dt, eig), 0.f + 0.1f * (stab * eig)));
    CHECK(same_bits(callback_value((int)RNDE_REG_ERR_STIFF, nan, dt, eig), 0.f + 0.1f * (stab * eig)));
    CHECK(same_bits(callback_value((int)RNDE_REG_ERR_STIFF, std::numeric_limits<float>::infinity(), 0.f, eig), 0.f + 0.1f * (stab * eig)));
    CHECK(same_bits(callback_value((int)RNDE_REG_ERR_STIFF, nan, dt, nan), 0.f));
    CHECK(estimate_counts(1e-30f) && estimate_counts(-3.f) && !estimate_counts(0.f) && !estimate_counts(nan));
}

// ---- eig_cotangent: the coefficients against central differences of callback_value itself (its fp64 instance) -----------------------------
struct Eig { float eigen, n1, n2, dt; };

// the value the callback saves, times its cotangent, as a function of the two norms
static double saved(int kind, double svb, double n1, double n2, double dt) { return svb * callback_value(kind, 0.0, dt, n1 / n2); }      // (EEst = 0: the mixed kind's stiffness term alone)

static void eig_cotangent_checks() {
    const int kinds[3] = {RNDE_REG_STIFF, RNDE_REG_ERR_STIFF, RNDE_REG_STIFF_DT};
    // c1 n1 = d/dn1, c2 n2 = d/dn2.  The coefficients are fp32 roundings of fp64 expressions (2^-24 relative), the products here are exact in
    // fp64 up to 2^-53, and a central difference with a relative step of 1e-5 of these rational functions is good to 1e-10 relative
    // (truncation h^2 f'''/6 ~ 1e-10, rounding 1e-16 / 1e-5): 2^-23 covers all of it with a factor of two to spare.
    const double tol = 1.1920929e-7;
    for (int kind : kinds)
        for (const Eig& r : {Eig{0.75f / 0.31f, 0.75f, 0.31f, 0.0625f}, Eig{3.0e-3f / 41.5f, 3.0e-3f, 41.5f, 0.4f}, Eig{17.f / 0.002f, 17.f, 0.002f, 1e-3f},
                             Eig{0.75f / 0.31f, 0.75f, 0.31f, -0.0625f}})      // (the last: a solve that runs backwards in time, eigen * dt < 0)
            for (float svb : {1.f, -0.37f, 250.f}) {
                float c1 = 7.f, c2 = 7.f;
                eig_cotangent(kind, svb, r, &c1, &c2);
                const double n1 = r.n1, n2 = r.n2, h1 = 1e-5 * n1, h2 = 1e-5 * n2;
                const double d1 = (saved(kind, svb, n1 + h1, n2, r.dt) - saved(kind, svb, n1 - h1, n2, r.dt)) / (2 * h1);
                const double d2 = (saved(kind, svb, n1, n2 + h2, r.dt) - saved(kind, svb, n1, n2 - h2, r.dt)) / (2 * h2);
                const bool ok1 = std::fabs((double)c1 * n1 - d1) <= tol * std::fabs(d1), ok2 = std::fabs((double)c2 * n2 - d2) <= tol * std::fabs(d2);
                if (!ok1 || !ok2 || d1 == 0.0 || d2 == 0.0) {
                    std::printf("FAILED eig_cotangent kind %d svb %g (n1 %g n2 %g dt %g): c1 n1 %.12g against %.12g, c2 n2 %.12g against %.12g\n", kind, (double)svb,
                                n1, n2, (double)r.dt, (double)c1 * n1, d1, (double)c2 * n2, d2);
                    ++failures;
                }
            }
    // zero cases: no estimate (0 or NaN) and a zero norm give (0, 0) under every stiffness kind
    const Eig good{2.f, 1.f, 0.5f, 0.1f};
    for (int kind : kinds) {
        for (const Eig& r : {Eig{0.f, 1.f, 0.5f, 0.1f}, Eig{std::nanf(""), 1.f, 0.5f, 0.1f}, Eig{2.f, 0.f, 0.5f, 0.1f}, Eig{2.f, 1.f, 0.f, 0.1f}}) {
            float c1 = 7.f, c2 = 7.f;
            eig_cotangent(kind, 1.5f, r, &c1, &c2);
            CHECK(c1 == 0.f && c2 == 0.f);
        }
        float c1 = 7.f, c2 = 7.f;
        eig_cotangent(kind, 0.f, good, &c1, &c2);      // (and a zero cotangent)
        CHECK(c1 == 0.f && c2 == 0.f);
        eig_cotangent(kind, 1.5f, good, &c1, &c2);
        CHECK(c1 > 0.f && c2 < 0.f);                    // the value grows with n1 and falls with n2
    }
    // sign cases: |eigen| and |eigen dt| turn the coefficients round with the sign of what is inside; the mixed callback's term has no
    // absolute value and does not
    {
        float p1, p2, m1, m2;
        eig_cotangent(RNDE_REG_STIFF, 1.5f, good, &p1, &p2);
        eig_cotangent(RNDE_REG_STIFF, 1.5f, Eig{-2.f, 1.f, 0.5f, 0.1f}, &m1, &m2);
        CHECK(m1 == -p1 && m2 == -p2 && p1 != 0.f);
        eig_cotangent(RNDE_REG_ERR_STIFF, 1.5f, good, &p1, &p2);
        eig_cotangent(RNDE_REG_ERR_STIFF, 1.5f, Eig{-2.f, 1.f, 0.5f, 0.1f}, &m1, &m2);
        CHECK(m1 == p1 && m2 == p2 && p1 != 0.f);
        eig_cotangent(RNDE_REG_STIFF_DT, 1.5f, good, &p1, &p2);
        eig_cotangent(RNDE_REG_STIFF_DT, 1.5f, Eig{-2.f, 1.f, 0.5f, 0.1f}, &m1, &m2);      // eigen * dt < 0 through eigen: sign -1, times dt > 0
        CHECK(m1 == -p1 && m2 == -p2 && p1 > 0.f);
        eig_cotangent(RNDE_REG_STIFF_DT, 1.5f, Eig{2.f, 1.f, 0.5f, -0.1f}, &m1, &m2);      // eigen * dt < 0 through dt: sign -1, times dt < 0
        CHECK(m1 == p1 && m2 == p2);
        eig_cotangent(RNDE_REG_STIFF_DT, 1.5f, Eig{-2.f, 1.f, 0.5f, -0.1f}, &m1, &m2);     // both negative: sign +1, times dt < 0
        CHECK(m1 == -p1 && m2 == -p2);
    }
    // the callbacks without a stiffness estimate
    for (int kind : {(int)RNDE_REG_NONE, (int)RNDE_REG_ERR}) {
        float c1 = 7.f, c2 = 7.f;
        eig_cotangent(kind, 1.5f, good, &c1, &c2);
        CHECK(c1 == 0.f && c2 == 0.f);
    }
}

// ---- gather_saved_values: a written-down five-attempt log with one rejection ---------------------------------------------------------------
static void gather_checks() {
    const std::vector<Att> att = {{0.f, 0.25f, 0.5f, 2.f, kAccept}, {0.25f, 0.5f, 3.f, 9.f, 0}, {0.25f, 0.125f, 0.25f, -4.f, kAccept},
                                  {0.375f, 0.5f, 0.75f, 0.f, kAccept}, {0.875f, 0.125f, 1.f, 8.f, kAccept | 4}};
    const float stab = 1.0f / 3.5068f;
    const float want[5][4] = {{0, 0, 0, 0},                                                                            // none: no values at all
                              {0.5f * 0.25f, 0.25f * 0.125f, 0.75f * 0.5f, 1.f * 0.125f},
                              {stab * 2.f, stab * 4.f, 0.f, stab * 8.f},
                              {0.5f * 0.25f + 0.1f * (stab * 2.f), 0.25f * 0.125f + 0.1f * (stab * -4.f), 0.75f * 0.5f + 0.1f * 0.f, 1.f * 0.125f + 0.1f * (stab * 8.f)},
                              {2.f * 0.25f, 4.f * 0.125f, 0.f, 8.f * 0.125f}};
    const float init[5] = {0.f, 0.f, stab, 0.1f * stab, 0.f};
    for (int kind = RNDE_REG_NONE; kind <= RNDE_REG_STIFF_DT; ++kind)
        for (bool start : {false, true}) {
            int idx[6] = {-7, -7, -7, -7, -7, -7};
            float val[7] = {-7.f, -7.f, -7.f, -7.f, -7.f, -7.f, -7.f};
            const int nsv = gather_saved_values(att.data(), 5, kAccept, kind, start, idx, val);
            CHECK(idx[5] == -7);      // (nothing past n_att)
            if (kind == RNDE_REG_NONE) {
                CHECK(nsv == 0 && val[0] == -7.f);
                for (int n = 0; n < 5; ++n) CHECK(idx[n] == -1);
                continue;
            }
            const int o = start ? 1 : 0;
            CHECK(nsv == 4 + o);
            CHECK(idx[0] == o && idx[1] == -1 && idx[2] == o + 1 && idx[3] == o + 2 && idx[4] == o + 3);
            if (start) CHECK(same_bits(val[0], init[kind]));
            for (int j = 0; j < 4; ++j) CHECK(same_bits(val[o + j], want[kind][j]));
            CHECK(val[nsv] == -7.f);
            // without an output for the values: the same count and indices
            int idx2[5];
            CHECK(gather_saved_values(att.data(), 5, kAccept, kind, start, idx2, nullptr) == nsv);
            for (int n = 0; n < 5; ++n) CHECK(idx2[n] == idx[n]);
        }
    int none = -7;
    CHECK(gather_saved_values((const Att*)nullptr, 0, kAccept, RNDE_REG_ERR, true, &none, nullptr) == 1 && none == -7);      // no attempts: the start's value alone
    CHECK(gather_saved_values((const Att*)nullptr, 0, kAccept, RNDE_REG_ERR, false, &none, nullptr) == 0);
}

// ---- step_end_times: the last accepted step overshoots t1 ----------------------------------------------------------------------------------
static void step_end_checks() {
    const float t = 0.3f, dt = 0.1f, tnew = t + dt;      // (not exact in binary: the end is t + dt as fp32 forms it)
    const std::vector<Att> att = {{0.f, 0.3f, 0, 0, kAccept}, {t, 0.5f, 0, 0, 0}, {t, dt, 0, 0, kAccept}, {tnew, 0.75f, 0, 0, 0}, {tnew, 0.625f, 0, 0, kAccept}};
    const float t1 = 1.f;
    CHECK(att[4].t + att[4].dt > t1);
    for (bool start : {false, true}) {
        const std::vector<float> e = step_end_times(att.data(), 5, kAccept, 0.f, t1, start);
        const size_t o = start ? 1 : 0;
        CHECK(e.size() == 3 + o);
        if (e.size() != 3 + o) continue;
        if (start) CHECK(e[0] == 0.f);
        CHECK(same_bits(e[o], 0.3f) && same_bits(e[o + 1], tnew) && same_bits(e[o + 2], t1));      // rejected attempts absent, the end clamped
    }
    CHECK(step_end_times((const Att*)nullptr, 0, kAccept, 0.5f, 1.f, false).empty());
    CHECK(step_end_times((const Att*)nullptr, 0, kAccept, 0.5f, 1.f, true) == std::vector<float>{0.5f});
    const std::vector<Att> rej = {{0.f, 1.f, 0, 0, 0}, {0.f, 0.5f, 0, 0, 2}};      // (another flag set, not the accepting one)
    CHECK(step_end_times(rej.data(), 2, kAccept, 0.f, 1.f, false).empty());
}

// ---- the sizing rules at their corners -------------------------------------------------------------------------------------------------------
static void sizing_checks() {
    // taped one-launch multi-wave solve: min(cap, max(48, 2 predicted))
    CHECK(mw_taped_attempt_limit(256, 12) == 48 && mw_taped_attempt_limit(256, 24) == 48 && mw_taped_attempt_limit(256, 25) == 50);
    CHECK(mw_taped_attempt_limit(256, 128) == 256 && mw_taped_attempt_limit(256, 200) == 256 && mw_taped_attempt_limit(32, 4) == 32 && mw_taped_attempt_limit(48, 1) == 48);
    // speculative records of the one-launch stage solve: min(cap, max(64, 2 predicted))
    CHECK(stage_speculative_records(256, 12) == 64 && stage_speculative_records(256, 32) == 64 && stage_speculative_records(256, 33) == 66);
    CHECK(stage_speculative_records(256, 128) == 256 && stage_speculative_records(256, 1000) == 256 && stage_speculative_records(16, 12) == 16);
    // chunks: coupled ranks enqueue 16 whatever their history; alone, the prediction (at least 4), then 4
    CHECK(first_chunk(false, 12) == 12 && first_chunk(false, 1) == 4 && first_chunk(false, 4) == 4 && first_chunk(false, 300) == 300);
    CHECK(first_chunk(true, 12) == 16 && first_chunk(true, 1) == 16 && first_chunk(true, 300) == 16);
    CHECK(later_chunk(false) == 4 && later_chunk(true) == 16);
    // retry window: doubles, capped at 1024
    CHECK(next_retry_window(8) == 16 && next_retry_window(511) == 1022 && next_retry_window(512) == 1024 && next_retry_window(513) == 1024 && next_retry_window(1024) == 1024);
    // evaluations: 3 + (S - 1) per attempt
    CHECK(solve_nfe(7, 0) == 3 && solve_nfe(7, 12) == 75 && solve_nfe(13, 10) == 123);
    CHECK(solve_nfe(13, 200000000) == 3 + 12 * (int64_t)200000000);      // (formed in 64 bits)
    // saveat: increasing and inside [t0, t1]
    const float ok[4] = {0.f, 0.25f, 0.5f, 1.f}, one[1] = {0.5f};
    CHECK(saveat_valid(ok, 4, 0.f, 1.f) && saveat_valid(one, 1, 0.f, 1.f) && saveat_valid(one, 1, 0.5f, 0.5f) && saveat_valid(ok, 0, 0.f, 1.f));
    const float below[2] = {-0.125f, 0.5f}, above[2] = {0.5f, 1.125f}, down[3] = {0.25f, 0.75f, 0.5f}, equal[3] = {0.25f, 0.5f, 0.5f}, hole[2] = {0.25f, std::nanf("")};
    CHECK(!saveat_valid(below, 2, 0.f, 1.f));
    CHECK(!saveat_valid(above, 2, 0.f, 1.f));
    CHECK(!saveat_valid(ok, 4, 0.125f, 1.f) && !saveat_valid(ok, 4, 0.f, 0.75f));
    CHECK(!saveat_valid(down, 3, 0.f, 1.f));
    CHECK(!saveat_valid(equal, 3, 0.f, 1.f));
    CHECK(!saveat_valid(hole, 2, 0.f, 1.f) && !saveat_valid(hole + 1, 1, 0.f, 1.f));
}

int main() {
    callback_value_checks();
    eig_cotangent_checks();
    gather_checks();
    step_end_checks();
    sizing_checks();
    if (failures) { std::printf("%d forward plan checks FAILED\n", failures); return 1; }
    std::printf("forward plan checks passed\n");
    return 0;
}
