// rnde_tile_host.h -- what the two translation units of the tile layout (rnde_ffjord.hip, rnde_node_tile.hip) do alike on the host around
// the launches of rnde_tile_driver.h: the records a reverse sweep walks, built from a step log, the residency check of a launch whose
// tiles meet, and the message of a meeting that did not hold; the workspace of a solve (TileSolveWs), its StepParams (tile_step_params),
// the run of a launch whose tiles meet (tile_run_met) and the copy of the step log behind a solve (the status map, the
// saved values and the exports are rnde_fwd_plan.h's).  No kernel lives here; a stand-alone host program checks the record builders, tile_step_params and the
// step log's helpers against values written out by hand (tests/track_host/track_host_check.cpp).
#pragma once
#include <algorithm>
#include <climits>
#include <initializer_list>
#include <string>
#include <vector>

#include "rnde_fwd_plan.h"     // gather_saved_values, solve_verdict, the exports
#include "rnde_meet.h"         // MeetRes, meet_verdict; rnde_alloc.h: DevBuf, PinBuf
#include "rnde_track_rec.h"    // FfStepRec, FfAttRec, ff_att_rec

namespace rnde {

// The accepted steps of a step log, in forward order, each with the cotangent of its saved value EEst * dt (saveval_bar: one entry per
// saved value, NULL: zeros; skip_first: the value saved at init, cb_save_start under a regulariser, is a constant and takes entry 0).
inline void tile_step_recs(const StepMeta* meta, int n_att, const float* saveval_bar, bool skip_first, std::vector<FfStepRec>& rec) {
    rec.clear();
    int k = skip_first ? 1 : 0;
    for (int i = 0; i < n_att; ++i) {
        const StepMeta& m = meta[i];
        if (!(m.flags & F_ACCEPT)) continue;
        rec.push_back(FfStepRec{m.t, m.dt, m.eest, saveval_bar ? saveval_bar[k] : 0.f});
        ++k;
    }
}

// One record per attempt of the tracked sweep (rec: tile_step_recs of the same log); a rejected attempt reads the tape record of the
// accepted attempt behind it.  Attempts behind the last accepted one reach nothing and are trimmed.
inline void tile_att_recs(const StepMeta* meta, int n_att, const std::vector<FfStepRec>& rec, std::vector<FfAttRec>& att) {
    att.clear();
    att.reserve(n_att);
    int acc = 0;
    for (int i = 0; i < n_att; ++i) {
        const bool a = (meta[i].flags & F_ACCEPT) != 0;
        att.push_back(ff_att_rec(meta[i], a ? rec[acc].svb : 0.f, acc));
        if (a) ++acc;
    }
    while (!att.empty() && !(att.back().flags & F_ACCEPT)) att.pop_back();
}

// A meeting needs every tile of the largest batch resident at once, on the footprint of the kernels that meet.  "" when ntiles_max tiles
// fit; otherwise prefix + "max_batch needs <n> resident tiles for " + what + ", the device holds <room> workgroups of " + footprint.
// *e: a HIP call that failed (the string is then empty).
inline std::string tile_residency_refusal(std::initializer_list<const void*> kernels, int threads, size_t lds_bytes, int ntiles_max, int device,
                                          const char* prefix, const char* what, const char* footprint, hipError_t* e) {
    *e = hipSuccess;
    int per_cu = kernels.size() ? INT_MAX : 0;
    hipDeviceProp_t prop;
    for (const void* k : kernels) {
        int n = 0;
        if ((*e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, threads, lds_bytes)) != hipSuccess) return "";
        per_cu = std::min(per_cu, n);
    }
    if ((*e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return "";
    // (one XCD: one workgroup on each of its CUs)
    const long long room = ntiles_max > kMeetXcdCus ? (long long)per_cu * prop.multiProcessorCount : (per_cu > 0 ? kMeetXcdCus : 0);
    if (room >= ntiles_max) return "";
    return std::string(prefix) + "max_batch needs " + std::to_string(ntiles_max) + " resident tiles for " + what + ", the device holds " + std::to_string(room) +
           " workgroups of " + footprint;
}

// The verdict of a launch whose tiles met (behind queue_check and the stream's synchronisation).  "" when the meeting held; otherwise the
// abort word is cleared and the message is prefix + "a workgroup meeting of " + what + " timed out (<the cause>); " + tail.
// *e: a HIP call that failed.  There is no fall-back to other arithmetic: the caller fails and says why.
inline std::string tile_meet_refusal(MeetRes& M, const Meet& meet, int nt, hipStream_t s, const char* prefix, const char* what, const char* tail,
                                     hipError_t* e) {
    *e = hipSuccess;
    const bool split = meet_split(M.chk, nt, meet.global != 0);
    if (meet_verdict(M.chk, nt, meet.global != 0) == MEET_OK) return "";
    if ((*e = M.clear_abort(s)) != hipSuccess || (*e = hipStreamSynchronize(s)) != hipSuccess) return "";
    return std::string(prefix) + "a workgroup meeting of " + what + " timed out (" +
           (split ? "the tiles pinned to one XCD by block index landed on different XCDs" : "not every tile was resident") + "); " + tail;
}

// ---- the workspace of a tile solve: the one owner of what a solve needs on the device beside its inputs.  Its three users:
//   the tiled TrackedFFJORD handle   alloc(D + 1, ceil(max_batch / 16), 1, max_attempts, Dyn::scratch_floats(G), kMwMeetMax, false)
//   rnde_ffjord::Groups              alloc(D + 1, ceil(max_columns / 16), max_groups, max_attempts, Dyn::scratch_floats(G), the same tile count, true)
//   the tiled TrackedNeuralODE       alloc(D, ceil(max_batch / 16), 1, max_attempts, 0, kMwMeetMax, false)
// fin_apart: the final states are an allocation of their own (a group call's), not the entries of ctl behind the live ones (a single solve's).
// Every buffer is an owner behind rnde_alloc.h (counted, and poisoned under RNDE_POISON; the meeting place zeroes its own words); a handle
// declares its events ahead of this member (members go in reverse order).  The one-workgroup FFJORD engine, which has no tiles, allocates by
// hand what it uses: ws, norm [512], ctl [3] (n_live stays 2), meta, initrec_t [1], h_fin [1], and sets Bp.  DA, PA: a host check's allocators.
template <class DA = DevAlloc, class PA = PinAlloc>
struct TileSolveWsT {
    Buf<float, DA> ws, norm, scratch;        // [10][rows][Bp]; [tiles][8] + 512, zeroed; [tiles][scratch floats] or empty
    Buf<StepState, DA> ctl, fin_n, ctl_t;    // [n_solves][2] live states, then (not fin_apart) the final ones; [n_solves] (fin_apart); [tiles]
    Buf<StepMeta, DA> meta;                  // [n_solves][max_attempts]
    Buf<InitRec, DA> initrec_t;              // [tiles]
    Buf<StepState, PA> h_fin;                // pinned [n_solves]: where the host reads the final states (an asynchronous copy must not land in a dead stack frame)
    MeetRes meet;                            // (max_attempts + 4) x 3 x meet_tiles granules
    int Bp = 0, n_live = 2;                  // the row stride, 16 x tiles; live states in ctl

    hipError_t alloc(int rows, int n_tiles, int n_solves, int max_attempts, size_t scratch_floats_per_tile, int meet_tiles, bool fin_apart) {
        const size_t NT = (size_t)n_tiles, NS = (size_t)n_solves, MA = (size_t)max_attempts;
        Bp = 16 * n_tiles; n_live = 2 * n_solves;
        hipError_t e = ws.alloc(10 * (size_t)rows * Bp);
        if (e == hipSuccess) e = norm.alloc(8 * NT + 512);
        if (e == hipSuccess) e = hipMemset(norm, 0, (8 * NT + 512) * 4);
        if (e == hipSuccess && scratch_floats_per_tile) e = scratch.alloc(NT * scratch_floats_per_tile);
        if (e == hipSuccess) e = ctl.alloc(fin_apart ? 2 * NS : 3 * NS);
        if (e == hipSuccess && fin_apart) e = fin_n.alloc(NS);
        if (e == hipSuccess) e = ctl_t.alloc(NT);
        if (e == hipSuccess) e = meta.alloc(NS * MA);
        if (e == hipSuccess) e = initrec_t.alloc(NT);
        if (e == hipSuccess) e = h_fin.alloc(NS);
        if (e == hipSuccess) e = meet.create(MA + 4, 3, meet_tiles);
        return e;
    }
    StepState* fin() const { return fin_n ? fin_n.get() : ctl.get() + n_live; }
    // ws for more rows (TrackedFFJORD's kinetic rows), all or nothing with what `beside` allocates for the caller (who swaps its own in behind a success)
    template <class Beside>
    hipError_t grow_rows(int rows, Beside&& beside) {
        Buf<float, DA> w;
        hipError_t e = w.alloc(10 * (size_t)rows * Bp);
        if (e == hipSuccess) e = beside();
        if (e == hipSuccess) ws.swap(w);       // (the old one goes with the local)
        return e;
    }
};
using TileSolveWs = TileSolveWsT<>;

// The StepParams of a tile solve: the one place that fills them.  The tiled NeuralODE sets the saveat fields afterwards, a group call
// overrides Bpad (B is its first group's).
template <class WS>
inline StepParams tile_step_params(const WS& W, const float* x, int rows, int B, float reltol, float abstol, float t0, float t1, int max_attempts,
                                   const float* replay, int n_replay) {
    StepParams P{};
    P.x = x; P.D = rows; P.B = B; P.Bn = B; P.Bpad = W.Bp; P.nwg = 1;
    P.ctl = W.ctl; P.ctl_final = W.fin(); P.meta = W.meta; P.initrec = W.initrec_t; P.initpart = W.norm;
    P.reltol = reltol; P.abstol = abstol; P.t0 = t0; P.t1 = t1;
    P.tape = 1; P.max_attempts = max_attempts; P.reg_kind = 0; P.nsave = 0;
    P.replay = replay; P.n_replay = replay ? n_replay : 0;
    P.beta1 = kBeta1; P.beta2 = kBeta2; P.rk_order = 5.f;
    return P;
}
// What a TileSolveParams takes from the workspace, and a TileSolveParams / TileRevParams from the meeting of its launch.
template <class Params>
inline void tile_bind_ws(Params& T, const TileSolveWs& W) { T.ws = W.ws; T.norm = W.norm; T.initrec_t = W.initrec_t; T.ctl_t = W.ctl_t; T.Bp = W.Bp; }
template <class Params>
inline void tile_bind_meet(Params& T, const MeetRes& M, const Meet& meet) { T.meet = meet; T.xcc = M.xcc; T.xcd_slot = M.slot; }

// ---- the run of a launch.  Event, launch, event: launch() queues the kernels and returns hipGetLastError() behind the last one.
template <class Launch>
inline hipError_t tile_run_timed(hipEvent_t ev0, hipEvent_t ev1, hipStream_t s, Launch&& launch) {
    hipError_t e = hipEventRecord(ev0, s);
    if (e == hipSuccess) e = launch();
    return e == hipSuccess ? hipEventRecord(ev1, s) : e;
}
// One run of a launch whose nt tiles meet at M (allow_local: the one-XCD form while they fit one), to the end of the stream: a new
// epoch, the timed launch (launch(meet)), what the caller queues behind it (behind(): the copy of the final states, a reduction), the
// meeting's check words, the wait for the stream, the verdict (tile_meet_refusal with prefix, what, tail: *refusal is "" when it held).
template <class Launch, class Behind>
inline hipError_t tile_run_met(MeetRes& M, int nt, bool allow_local, hipEvent_t ev0, hipEvent_t ev1, hipStream_t s, Launch&& launch, Behind&& behind,
                               const char* prefix, const char* what, const char* tail, std::string* refusal) {
    refusal->clear();
    const Meet meet = M.begin(nt, allow_local, s);
    hipError_t e = M.err;
    if (e == hipSuccess) e = tile_run_timed(ev0, ev1, s, [&] { return launch(meet); });
    if (e == hipSuccess) e = behind();
    if (e == hipSuccess) e = M.queue_check(meet, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) *refusal = tile_meet_refusal(M, meet, nt, s, prefix, what, tail, &e);
    return e;
}

// ---- behind a solve.  The first n_att records of a device step log, on the host (behind the stream's synchronisation: n_att is the final state's).
inline hipError_t tile_fetch_log(const StepMeta* dev, int n_att, StepMeta* host) {
    return n_att ? hipMemcpy(host, dev, (size_t)n_att * sizeof(StepMeta), hipMemcpyDeviceToHost) : hipSuccess;
}

}  // namespace rnde
