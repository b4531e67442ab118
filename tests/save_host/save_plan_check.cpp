// What the host derives from an attempt log for the reverse sweeps, checked by a program of its own (tests/test_node_tiled_saveat_host.py
// compiles and runs it; no GPU is touched): csrc/rnde_rev_plan.h -- the save plan on written-down attempt logs, the chain engines' evaluation
// times, the saved-value cotangent gather (the eigen_est cotangent coefficients: fwd_plan_check.cpp, beside the callback's value) -- and the Tsit5 dense-output weights of csrc/rnde_device.h (dense_weights, dense_weights_deriv; host and device functions) against the tableau
// and against central differences.
// Prints one line per failed check; exit status 0 when there is none.
#include "rnde_device.h"
#include "rnde_rev_plan.h"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace rnde;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

struct Att { float t, dt; int flags; };

static std::vector<SaveRange> plan(const std::vector<float>& sv, float t0, const std::vector<Att>& att, int* covered) {
    std::vector<SaveRange> r(att.size() + 1);      // (one more than needed: a write past n_att would land in it and be seen below)
    r[att.size()] = SaveRange{-7, -7};
    *covered = save_plan(sv.data(), (int)sv.size(), t0, att.data(), (int)att.size(), F_ACCEPT, r.data());
    CHECK(r[att.size()].lo == -7 && r[att.size()].hi == -7);
    r.pop_back();
    return r;
}

// the ranges are consecutive and, with the start's index, partition 0 .. covered
static void check_partition(const std::vector<SaveRange>& r, int first, int covered) {
    int at = first;
    for (const SaveRange& g : r) { CHECK(g.lo == at); CHECK(g.hi >= g.lo); at = g.hi; }
    CHECK(at == covered);
}

static void save_plan_checks() {
    // steps end at 0.25, 0.5, 0.75, 1 exactly; attempt 1 is rejected
    const std::vector<Att> att = {{0.f, 0.25f, F_ACCEPT}, {0.25f, 0.5f, 0}, {0.25f, 0.25f, F_ACCEPT}, {0.5f, 0.25f, F_ACCEPT}, {0.75f, 0.25f, F_ACCEPT | F_CLAMP}};
    int cov = 0;
    {   // first time == t0, two times in one step, a time exactly at an interior step end, a step with none, a time == t1
        const std::vector<float> sv = {0.f, 0.1f, 0.2f, 0.25f, 0.6f, 1.f};
        const auto r = plan(sv, 0.f, att, &cov);
        CHECK(cov == 6);
        check_partition(r, 1, cov);
        CHECK(r[0].lo == 1 && r[0].hi == 4);       // 0.1, 0.2 and the step end 0.25: the end belongs to THIS step
        CHECK(r[1].lo == 4 && r[1].hi == 4);       // the rejected attempt: empty
        CHECK(r[2].lo == 4 && r[2].hi == 4);       // (0.25, 0.5]: none
        CHECK(r[3].lo == 4 && r[3].hi == 5);       // 0.6
        CHECK(r[4].lo == 5 && r[4].hi == 6);       // t1
    }
    {   // no start: index 0 belongs to the first step
        const std::vector<float> sv = {0.1f, 0.5f, 0.75f};
        const auto r = plan(sv, 0.f, att, &cov);
        CHECK(cov == 3);
        check_partition(r, 0, cov);
        CHECK(r[0].lo == 0 && r[0].hi == 1 && r[2].lo == 1 && r[2].hi == 2 && r[3].lo == 2 && r[3].hi == 3 && r[4].lo == 3 && r[4].hi == 3);
    }
    {   // n = 1 with [t1]
        const std::vector<float> sv = {1.f};
        const auto r = plan(sv, 0.f, att, &cov);
        CHECK(cov == 1);
        check_partition(r, 0, cov);
        for (int i = 0; i < 4; ++i) CHECK(r[i].lo == 0 && r[i].hi == 0);
        CHECK(r[4].lo == 0 && r[4].hi == 1);
    }
    {   // n = 1 with [t0]: the start alone, no attempt covers anything
        const std::vector<float> sv = {0.f};
        const auto r = plan(sv, 0.f, att, &cov);
        CHECK(cov == 1);
        check_partition(r, 1, cov);
    }
    {   // a solve that stops short (a replay of two attempts): the later times stay uncovered, nothing runs past n_save
        const std::vector<Att> two(att.begin(), att.begin() + 2);
        const std::vector<float> sv = {0.f, 0.1f, 0.6f, 1.f};
        const auto r = plan(sv, 0.f, two, &cov);
        CHECK(cov == 2);
        check_partition(r, 1, cov);
    }
    {   // step ends that are not exact in binary: the comparison is against t + dt as fp32 forms it
        const float t = 0.3f, dt = 0.1f, tnew = t + dt;
        const std::vector<Att> a = {{0.f, 0.3f, F_ACCEPT}, {t, dt, F_ACCEPT}, {tnew, 1.f - tnew, F_ACCEPT}};
        const std::vector<float> sv = {tnew, std::nextafterf(tnew, 2.f)};
        const auto r = plan(sv, 0.f, a, &cov);
        CHECK(cov == 2);
        check_partition(r, 0, cov);
        CHECK(r[1].lo == 0 && r[1].hi == 1 && r[2].lo == 1 && r[2].hi == 2);
    }
    {   // no attempts, no save times
        const auto r = plan({}, 0.f, {}, &cov);
        CHECK(cov == 0 && r.empty());
    }
}

// dense_weights in double: the same polynomials, for the central differences
static void dense_weights64(double th, double (&b)[7]) {
    const double t2 = th * th;
    b[0] = -1.0530884977290216 * th * (th - 1.3299890189751412) * (t2 - 1.4364028541716351 * th + 0.7139816917074209);
    b[1] = 0.1017 * t2 * (t2 - 2.1966568338249754 * th + 1.2949852507374631);
    b[2] = 2.490627285651252793 * t2 * (t2 - 2.38535645472061657 * th + 1.57803468208092486);
    b[3] = -16.54810288924490272 * (th - 1.21712927295533244) * (th - 0.61620406037800089) * t2;
    b[4] = 47.37952196281928122 * (th - 1.203071208372362603) * (th - 0.658047292653547382) * t2;
    b[5] = -34.87065786149660974 * (th - 1.2) * (th - 0.666666666666666667) * t2;
    b[6] = 2.5 * (th - 1.0) * (th - 0.6) * t2;
}

static void dense_weight_checks() {
    float b[7];
    dense_weights(0.f, b);
    for (int j = 0; j < 7; ++j) CHECK(b[j] == 0.f);
    // b(1) is the tableau's last row a_{7,j} (first same as last: unew = uprev + dt sum_j a_7j k_j), whose weight of k7 is 0
    const double b1[7] = {0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774, 0.0};
    dense_weights(1.f, b);
    for (int j = 0; j < 7; ++j) {
        const bool ok = std::fabs((double)b[j] - b1[j]) <= 4e-6;      // fp32 rounding of products of terms up to 47 (a few ulp of 3.3)
        if (!ok) { std::printf("FAILED dense_weights(1)[%d]: %.9g, tableau %.9g\n", j, (double)b[j], b1[j]); ++failures; }
    }
    CHECK(b[6] == 0.f);
    for (double th : {0.05, 0.3, 0.5, 0.77, 0.999}) {
        float w[7], dw[7];
        double w64[7], lo[7], hi[7];
        dense_weights((float)th, w);
        dense_weights_deriv((float)th, dw);
        dense_weights64((double)(float)th, w64);
        const double e = 1e-6;
        dense_weights64((double)(float)th - e, lo);
        dense_weights64((double)(float)th + e, hi);
        for (int j = 0; j < 7; ++j) {
            const double fd = (hi[j] - lo[j]) / (2 * e);
            // the derivative's terms reach 47 * 2.2: fp32 rounding of their sum, 2e-5 absolute; the central difference itself is good to 1e-9
            if (std::fabs((double)dw[j] - fd) > 2e-5 + 1e-5 * std::fabs(fd)) {
                std::printf("FAILED dense_weights_deriv(%g)[%d]: %.9g, central difference %.9g\n", th, j, (double)dw[j], fd); ++failures;
            }
            if (std::fabs((double)w[j] - w64[j]) > 4e-6) { std::printf("FAILED dense_weights(%g)[%d]: %.9g, double %.9g\n", th, j, (double)w[j], w64[j]); ++failures; }
        }
    }
}

// ---- eval_times: a written-down five-attempt log, both positions of the initial pair, 6 and 12 evaluations per attempt -------------------
static void eval_time_checks() {
    const std::vector<Att> att = {{0.f, 0.25f, F_ACCEPT}, {0.25f, 0.5f, 0}, {0.25f, 0.125f, F_ACCEPT}, {0.375f, 0.5f, F_ACCEPT}, {0.875f, 0.125f, F_ACCEPT | F_CLAMP}};
    const int n_att = (int)att.size();
    const float t0 = 0.f, dt0 = 0.03125f;
    float c[13];
    for (int E : {6, 12}) {
        c[0] = 0.f;
        for (int s = 1; s <= E; ++s) c[s] = E == 6 ? tsC(s) : (float)s / 16.f + (s == E ? 0.25f : 0.f);      // (12: nodes exact in binary, the last one 1)
        for (bool init_first : {true, false}) {
            std::vector<float> out((size_t)E * n_att + 3, -7.f);      // (one more than needed: a write past the end would be seen)
            eval_times(att.data(), n_att, E, c, t0, dt0, init_first, out.data());
            CHECK(out.back() == -7.f);
            const int init = init_first ? 0 : E * n_att, ev = init_first ? 2 : 0;
            CHECK(out[init] == t0 && out[init + 1] == t0 + dt0);
            for (int n = 0; n < n_att; ++n)
                for (int s = 1; s <= E; ++s) CHECK(out[ev + E * n + s - 1] == att[n].t + c[s] * att[n].dt);
            // written down: the last stage of every attempt sits at the step's end, the first stage of attempt 2 at 0.25 + c_2 * 0.125
            const float ends[5] = {0.25f, 0.75f, 0.375f, 0.875f, 1.f};
            for (int n = 0; n < n_att; ++n) CHECK(out[ev + E * n + E - 1] == ends[n]);
            CHECK(out[ev + E * 2] == (E == 6 ? 0.25f + 0.161f * 0.125f : 0.2578125f));
        }
    }
    {   // no attempts: the initial pair alone
        float out[3] = {-7.f, -7.f, -7.f}, c1[2] = {0.f, 1.f};
        eval_times((const Att*)nullptr, 0, 6, c1, 0.5f, 0.25f, false, out);
        CHECK(out[0] == 0.5f && out[1] == 0.75f && out[2] == -7.f);
    }
}

// ---- gather_svb --------------------------------------------------------------------------------------------------------------------------
static void gather_checks() {
    const int idx[5] = {0, -1, 1, -1, 2};
    const float bar[3] = {0.5f, -3.f, 7.25f};
    float out[6];
    auto fill = [&] { for (float& v : out) v = -7.f; };
    fill(); gather_svb(idx, 5, 1.f, nullptr, out);      // no cotangent: zeros
    for (int i = 0; i < 5; ++i) CHECK(out[i] == 0.f);
    CHECK(out[5] == -7.f);
    fill(); gather_svb(idx, 5, 1.f, bar, out);          // -1: the callback did not fire for that attempt
    CHECK(out[0] == 0.5f && out[1] == 0.f && out[2] == -3.f && out[3] == 0.f && out[4] == 7.25f && out[5] == -7.f);
    fill(); gather_svb(idx, 5, 2.f, bar, out);          // coupled controller, two ranks
    CHECK(out[0] == 1.f && out[1] == 0.f && out[2] == -6.f && out[3] == 0.f && out[4] == 14.5f && out[5] == -7.f);
    fill(); gather_svb(idx, 0, 2.f, bar, out);
    CHECK(out[0] == -7.f);
}

int main() {
    save_plan_checks();
    eval_time_checks();
    gather_checks();
    dense_weight_checks();
    if (failures) { std::printf("%d save host checks FAILED\n", failures); return 1; }
    std::printf("save host checks passed\n");
    return 0;
}
