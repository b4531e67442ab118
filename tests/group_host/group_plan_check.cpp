// What the host decides around a launch of several TrackedFFJORD batches, checked by a program of its own (tests/test_group_plan_host.py
// compiles and runs it; no GPU is touched): csrc/rnde_group_plan.h -- the group table at its corners against tables written out by hand, and
// every refusal string for every limit.
// Prints one line per failed check; exit status 0 when there is none.
#include "rnde_group_plan.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace rnde;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static bool same(const TileGroup& a, int first_tile, int ntiles, int col0, int B) {
    return a.first_tile == first_tile && a.ntiles == ntiles && a.col0 == col0 && a.B == B;
}
static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

// ---- the table ------------------------------------------------------------------------------------------------------------------------------
static void table_checks() {
    // columns to tiles: the last tile of a group is padded, a full tile is not split
    CHECK(group_tiles(1) == 1 && group_tiles(15) == 1 && group_tiles(16) == 1 && group_tiles(17) == 2 && group_tiles(32) == 2 && group_tiles(33) == 3);
    CHECK(group_tiles(1024) == 64 && group_tiles(4096) == 256);
    CHECK(group_reserved_tiles(1) == 1 && group_reserved_tiles(16) == 1 && group_reserved_tiles(17) == 2 && group_reserved_tiles(96) == 6 &&
          group_reserved_tiles(4096) == 256);
    static_assert(sizeof(TileGroup) == 16, "the device table's entry is four ints");
    {   // one group, each corner of B
        const int32_t b1[1] = {1}, b15[1] = {15}, b16[1] = {16}, b17[1] = {17};
        GroupPlan P = group_plan(1, b1);
        CHECK(P.n_groups == 1 && P.tiles == 1 && P.cols == 1 && P.Bp == 16 && same(P.g[0], 0, 1, 0, 1));
        P = group_plan(1, b15);
        CHECK(P.tiles == 1 && P.cols == 15 && P.Bp == 16 && same(P.g[0], 0, 1, 0, 15));
        P = group_plan(1, b16);
        CHECK(P.tiles == 1 && P.cols == 16 && P.Bp == 16 && same(P.g[0], 0, 1, 0, 16));
        P = group_plan(1, b17);
        CHECK(P.tiles == 2 && P.cols == 17 && P.Bp == 32 && same(P.g[0], 0, 2, 0, 17));
    }
    {   // unequal groups: 16, 40, 23 columns -> 1, 3, 2 tiles; caller columns back to back, tiles back to back, the last two groups padded
        const int32_t B[3] = {16, 40, 23};
        const GroupPlan P = group_plan(3, B);
        CHECK(P.n_groups == 3 && P.tiles == 6 && P.cols == 79 && P.Bp == 96);
        CHECK(same(P.g[0], 0, 1, 0, 16));
        CHECK(same(P.g[1], 1, 3, 16, 40));
        CHECK(same(P.g[2], 4, 2, 56, 23));
        // the padding of a group's last tile: workspace columns [16 first_tile + B, 16 (first_tile + ntiles)) belong to nobody else
        CHECK(16 * P.g[1].first_tile + P.g[1].B == 56 && 16 * (P.g[1].first_tile + P.g[1].ntiles) == 64);      // 8 padded columns
        CHECK(16 * P.g[2].first_tile + P.g[2].B == 87 && 16 * (P.g[2].first_tile + P.g[2].ntiles) == 96);      // 9 padded columns
        const int who[6] = {0, 1, 1, 1, 2, 2};
        for (int t = 0; t < 6; ++t) CHECK(group_of_tile(P, t) == who[t]);
        CHECK(group_of_tile(P, 6) == -1 && group_of_tile(P, -1) == -1);
    }
    {   // the corners side by side: 1, 15, 16, 17 -> 1, 1, 1, 2 tiles
        const int32_t B[4] = {1, 15, 16, 17};
        const GroupPlan P = group_plan(4, B);
        CHECK(P.tiles == 5 && P.cols == 49 && P.Bp == 80);
        CHECK(same(P.g[0], 0, 1, 0, 1) && same(P.g[1], 1, 1, 1, 15) && same(P.g[2], 2, 1, 16, 16) && same(P.g[3], 3, 2, 32, 17));
    }
    {   // four groups of 144: 36 tiles, more than one XCD's 32
        const int32_t B[4] = {144, 144, 144, 144};
        const GroupPlan P = group_plan(4, B);
        CHECK(P.tiles == 36 && P.cols == 576 && P.Bp == 576);
        for (int g = 0; g < 4; ++g) CHECK(same(P.g[g], 9 * g, 9, 144 * g, 144));
    }
    {   // offsets never overlap and cover the launch, whatever the sizes: both the caller columns and the workspace tiles
        const int32_t B[kGroupMax] = {1, 2, 16, 17, 31, 32, 33, 47, 48, 49, 100, 7, 64, 65, 15, 1024};
        const GroupPlan P = group_plan(kGroupMax, B);
        int tiles = 0, cols = 0;
        for (int g = 0; g < kGroupMax; ++g) {
            CHECK(P.g[g].first_tile == tiles && P.g[g].col0 == cols && P.g[g].B == B[g] && P.g[g].ntiles == (B[g] + 15) / 16);
            CHECK(16 * P.g[g].ntiles >= B[g] && 16 * (P.g[g].ntiles - 1) < B[g]);
            tiles += P.g[g].ntiles; cols += B[g];
        }
        CHECK(P.tiles == tiles && P.cols == cols && P.Bp == 16 * tiles && tiles == 104 && cols == 1551);
        std::vector<int> owner(P.tiles, -1);
        for (int g = 0; g < kGroupMax; ++g)
            for (int t = P.g[g].first_tile; t < P.g[g].first_tile + P.g[g].ntiles; ++t) { CHECK(owner[t] == -1); owner[t] = g; }
        for (int t = 0; t < P.tiles; ++t) CHECK(owner[t] == group_of_tile(P, t) && owner[t] >= 0);
    }
}

// ---- the refusals ---------------------------------------------------------------------------------------------------------------------------
static void reserve_checks() {
    CHECK(kGroupMax == 16 && kGroupTilesMax == 256);
    CHECK(group_reserve_refusal(1, false, 3, 96).empty() && group_reserve_refusal(2, false, 1, 1).empty());
    CHECK(group_reserve_refusal(1, false, 16, 4096).empty() && group_reserve_refusal(2, false, 0, 0).empty());
    // engine 0, by name, pointing at the tiled engine -- also for the release
    CHECK(has(group_reserve_refusal(0, false, 3, 96), "one-workgroup engine") && has(group_reserve_refusal(0, false, 3, 96), "rnde_ffjord_create_tiled"));
    CHECK(has(group_reserve_refusal(0, false, 0, 0), "one-workgroup engine"));
    // a tape
    CHECK(has(group_reserve_refusal(1, true, 3, 96), "holds a tape") && has(group_reserve_refusal(2, true, 0, 0), "holds a tape"));
    // max_groups
    for (int bad : {-1, 0, 17, 1000}) {
        const std::string s = group_reserve_refusal(1, false, bad, 96);
        CHECK(has(s, "max_groups must be 1..16") && has(s, ("got " + std::to_string(bad)).c_str()));
    }
    // max_columns: at least a column per group, at most 256 tiles
    for (int bad : {-5, 0, 2, 4097}) {
        const std::string s = group_reserve_refusal(1, false, 3, bad);
        CHECK(has(s, "max_columns must be max_groups..4096") && has(s, "256 resident tiles") && has(s, ("got " + std::to_string(bad)).c_str()));
    }
    CHECK(group_reserve_refusal(1, false, 3, 3).empty());
}

static void call_checks() {
    const int32_t B[3] = {16, 40, 23};
    const int cap_g = 3, cap_t = 6, mb = 64;
    auto call = [&](int cg, int ct, int n, const int32_t* b, float t0, float t1, bool exact, bool serves, bool e, bool s, bool c) {
        return group_call_refusal(cg, ct, mb, n, b, t0, t1, exact, serves, e, s, c);
    };
    CHECK(call(cap_g, cap_t, 3, B, 0.f, 1.f, false, true, true, true, true).empty());
    CHECK(call(cap_g, cap_t, 3, B, 0.f, 1.f, true, true, false, false, false).empty());
    CHECK(call(cap_g, cap_t, 1, B, 0.f, 1.f, false, true, true, false, false).empty());
    // no capacity: the fresh handle's message, whatever else is wrong
    CHECK(call(0, 0, 3, B, 0.f, 1.f, false, true, true, true, true) == kGroupNoCapacity);
    CHECK(call(0, 0, 0, nullptr, 1.f, 0.f, false, true, false, true, false) == kGroupNoCapacity);
    CHECK(has(kGroupNoCapacity, "no group capacity") && has(kGroupNoCapacity, "rnde_ffjord_reserve_groups"));
    // n_groups against the capacity
    for (int bad : {0, -1, 4}) {
        const std::string s = call(cap_g, cap_t, bad, B, 0.f, 1.f, false, true, true, true, true);
        CHECK(has(s, "n_groups must be 1..3") && has(s, "max_groups") && has(s, ("got " + std::to_string(bad)).c_str()));
    }
    CHECK(has(call(cap_g, cap_t, 3, nullptr, 0.f, 1.f, false, true, true, true, true), "B_host"));
    // a B_g of 0, a negative one, one above max_batch: the group's index and the limit
    {
        const int32_t z[3] = {16, 0, 23}, n[3] = {-4, 40, 23}, big[3] = {16, 40, 65};
        std::string s = call(cap_g, cap_t, 3, z, 0.f, 1.f, false, true, true, true, true);
        CHECK(has(s, "group 1: B must be 1..64") && has(s, "max_batch") && has(s, "got 0"));
        s = call(cap_g, cap_t, 3, n, 0.f, 1.f, false, true, true, true, true);
        CHECK(has(s, "group 0: B must be 1..64") && has(s, "got -4"));
        s = call(cap_g, cap_t, 3, big, 0.f, 1.f, false, true, true, true, true);
        CHECK(has(s, "group 2: B must be 1..64") && has(s, "got 65"));
    }
    // tiles above the reservation: 16, 40, 23 need 6 tiles although 79 columns are 5 tiles' worth
    {
        const std::string s = call(cap_g, 5, 3, B, 0.f, 1.f, false, true, true, true, true);
        CHECK(has(s, "need 6 tiles") && has(s, "reservation holds 5") && has(s, "max_columns = 80"));
        CHECK(call(cap_g, 6, 3, B, 0.f, 1.f, false, true, true, true, true).empty());
    }
    // the span (a NaN is no span either)
    CHECK(has(call(cap_g, cap_t, 3, B, 1.f, 1.f, false, true, true, true, true), "t1 > t0"));
    CHECK(has(call(cap_g, cap_t, 3, B, 1.f, 0.f, false, true, true, true, true), "t1 > t0"));
    CHECK(has(call(cap_g, cap_t, 3, B, 0.f, std::nanf(""), false, true, true, true, true), "t1 > t0"));
    // the exact trace and the probe
    CHECK(has(call(cap_g, cap_t, 3, B, 0.f, 1.f, true, false, false, true, true), "does not serve the exact trace"));
    CHECK(has(call(cap_g, cap_t, 3, B, 0.f, 1.f, false, true, false, true, true), "e_dev is required unless exact"));
    CHECK(has(call(cap_g, cap_t, 3, B, 0.f, 1.f, true, true, true, true, true), "e_dev must be NULL with exact"));
    // the accumulators come together
    CHECK(has(call(cap_g, cap_t, 3, B, 0.f, 1.f, false, true, true, true, false), "sum_dev and count_dev come together"));
    CHECK(has(call(cap_g, cap_t, 3, B, 0.f, 1.f, false, true, true, false, true), "sum_dev and count_dev come together"));
    // the failing group's message
    CHECK(group_failure(2, 2) == "TrackedFFJORD groups: group 2: max_attempts reached");
    CHECK(group_failure(0, 3) == "TrackedFFJORD groups: group 0: dt underflow");
    CHECK(group_failure(1, 4) == "TrackedFFJORD groups: group 1: non-finite error estimate or dt");
}

int main() {
    table_checks();
    reserve_checks();
    call_checks();
    if (failures) { std::printf("%d group plan checks FAILED\n", failures); return 1; }
    std::printf("group plan checks passed\n");
    return 0;
}
