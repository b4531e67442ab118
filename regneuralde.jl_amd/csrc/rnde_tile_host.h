// rnde_tile_host.h -- what the two translation units of the tile layout (rnde_ffjord.hip, rnde_node_tile.hip) do alike on the host around
// the launches of rnde_tile_driver.h: the records a reverse sweep walks, built from a step log, the residency check of a launch whose
// tiles meet, and the message of a meeting that did not hold.  No kernel lives here; a stand-alone host program checks the two record
// builders against records written out by hand (tests/track_host/track_host_check.cpp).
#pragma once
#include <algorithm>
#include <climits>
#include <initializer_list>
#include <string>
#include <vector>

#include "rnde_meet.h"         // MeetRes, meet_verdict
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

}  // namespace rnde
