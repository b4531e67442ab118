// rnde_group_plan.h -- what the host decides around a launch that carries several independent TrackedFFJORD batches ("groups";
// rnde_ffjord_reserve_groups / rnde_ffjord_forward_groups, include/rnde.h): the group table the kernel reads, the limits and the refusal
// strings.  Kernel-free in the manner of rnde_fwd_plan.h: plain C++, so a host program can include it alone
// (tests/group_host/group_plan_check.cpp).
//
// The table.  Group g holds B_g columns of the call, back to back in the caller layout (D x sum B): its first column there is col0_g = B_0 +
// ... + B_{g-1}.  On the tile layout a group is ntiles_g = ceil(B_g / 16) tiles of its own -- two groups never share a tile, a group's last
// tile is padded -- and the launch's tiles are the groups' tiles back to back: first_tile_g = ntiles_0 + ... + ntiles_{g-1}.  Everything
// the kernel keeps per tile (workspace columns 16 first_tile_g ..., initial-step records, meeting granules) is indexed by the launch's tile
// number, so the ranges of two groups never overlap.  The workspace rows share one stride, Bp = 16 x the launch's tiles.
#pragma once
#include <cstdint>
#include <string>

#include "rnde_fwd_plan.h"      // solve_verdict

namespace rnde {

constexpr int kGroupMax = 16;             // groups one launch carries (the kernel finds its group by walking the table)
constexpr int kGroupTilesMax = 256;       // tiles one launch holds: every one resident (kMwMeetMax, rnde_chainmw.h)

struct TileGroup { int first_tile, ntiles, col0, B; };      // one entry of the device table (16 bytes)

struct GroupPlan {
    int n_groups, tiles, cols, Bp;        // the launch: its groups, tiles (= workgroups), caller columns and padded row stride
    TileGroup g[kGroupMax];
};

inline int group_tiles(int B) { return (B + 15) / 16; }
inline int group_reserved_tiles(int max_columns) { return (max_columns + 15) / 16; }      // what a reservation of max_columns holds

// The table of a call that group_call_refusal has passed (1 <= n_groups <= kGroupMax, every B_g >= 1).
inline GroupPlan group_plan(int n_groups, const int32_t* B) {
    GroupPlan P{};
    P.n_groups = n_groups;
    for (int g = 0; g < n_groups; ++g) {
        P.g[g] = TileGroup{P.tiles, group_tiles(B[g]), P.cols, B[g]};
        P.tiles += P.g[g].ntiles;
        P.cols += B[g];
    }
    P.Bp = 16 * P.tiles;
    return P;
}

// The group of launch tile `tile` (what the kernel does on the device), -1 past the last tile.
inline int group_of_tile(const GroupPlan& P, int tile) {
    for (int g = 0; g < P.n_groups; ++g)
        if (tile >= P.g[g].first_tile && tile < P.g[g].first_tile + P.g[g].ntiles) return g;
    return -1;
}

// ---- refusals: "" when the request is served, otherwise the message (each names the limit) ----
constexpr const char* kGroupNoCapacity =
    "TrackedFFJORD groups: the handle has no group capacity; rnde_ffjord_reserve_groups(h, max_groups, max_columns) reserves it";

// rnde_ffjord_reserve_groups (max_groups = max_columns = 0 releases and is always served on engines 1 and 2 without a tape)
inline std::string group_reserve_refusal(int engine, bool holds_tape, int max_groups, int max_columns) {
    if (engine == 0)
        return "TrackedFFJORD groups: the one-workgroup engine solves a batch in one workgroup and has no tiles to share a launch between; create "
               "the handle with rnde_ffjord_create_tiled (engine = \"tiled\") or rnde_ffjord_create_chain";
    if (holds_tape)
        return "TrackedFFJORD groups: the handle holds a tape (a taped forward waiting for its backward); reserve before the forward or behind "
               "its backward";
    if (max_groups == 0 && max_columns == 0) return "";
    if (max_groups < 1 || max_groups > kGroupMax)
        return "TrackedFFJORD groups: max_groups must be 1.." + std::to_string(kGroupMax) + " (kGroupMax groups in one launch), or 0 with max_columns = 0 to "
               "release the capacity; got " + std::to_string(max_groups);
    if (max_columns < max_groups || max_columns > 16 * kGroupTilesMax)
        return "TrackedFFJORD groups: max_columns must be max_groups.." + std::to_string(16 * kGroupTilesMax) + " (every group holds a column; one launch "
               "holds kGroupTilesMax = " + std::to_string(kGroupTilesMax) + " resident tiles of 16 columns); got " + std::to_string(max_columns);
    return "";
}

// rnde_ffjord_forward_groups, before any launch.  cap_groups / cap_tiles: the reservation (0: none); max_batch: cfg.max_batch.
inline std::string group_call_refusal(int cap_groups, int cap_tiles, int max_batch, int n_groups, const int32_t* B, float t0, float t1, bool exact,
                                      bool serves_exact, bool has_e, bool has_sum, bool has_count) {
    if (cap_groups < 1) return kGroupNoCapacity;
    if (n_groups < 1 || n_groups > cap_groups)
        return "TrackedFFJORD groups: n_groups must be 1.." + std::to_string(cap_groups) + " (the reserved max_groups); got " + std::to_string(n_groups);
    if (!B) return "TrackedFFJORD groups: B_host (n_groups column counts) is required";
    long long tiles = 0;
    for (int g = 0; g < n_groups; ++g) {
        if (B[g] < 1 || B[g] > max_batch)
            return "TrackedFFJORD groups: group " + std::to_string(g) + ": B must be 1.." + std::to_string(max_batch) + " (cfg.max_batch); got " + std::to_string(B[g]);
        tiles += group_tiles(B[g]);
    }
    if (tiles > cap_tiles)
        return "TrackedFFJORD groups: the groups need " + std::to_string(tiles) + " tiles of 16 columns (every group its own), the reservation holds " +
               std::to_string(cap_tiles) + " (max_columns = " + std::to_string(16 * cap_tiles) + ")";
    if (!(t1 > t0)) return "TrackedFFJORD groups: tspan must satisfy t1 > t0";
    if (exact && !serves_exact) return "TrackedFFJORD groups: the handle does not serve the exact trace";
    if (!exact && !has_e) return "TrackedFFJORD groups: e_dev is required unless exact is set (the group call draws no probes of its own)";
    if (exact && has_e) return "TrackedFFJORD groups: e_dev must be NULL with exact set (the exact trace -tr J takes no probe)";
    if (has_sum != has_count) return "TrackedFFJORD groups: sum_dev and count_dev come together, both or neither (one of them is NULL)";
    return "";
}

// The call's status message when group g ended with controller status `status` (nonzero; the words: solve_verdict).
inline std::string group_failure(int g, int status) {
    return "TrackedFFJORD groups: group " + std::to_string(g) + ": " + solve_verdict(status).msg;
}

}  // namespace rnde
