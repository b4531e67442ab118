// rnde_node_tile.hip -- C ABI of the tiled engine of TrackedNeuralODE (include/rnde.h: rnde_node_create_tiled, engine 4): an rnde_node
// whose solve, reverse sweeps (constant-step and tracked: rnde_node_set_tracking) and feval are the tile driver's kernels
// (rnde_tile_driver.h) over the dynamics NtDyn (rnde_node_tile.h).  The public rnde_node_* entries (rnde.hip, rnde_reverse.hip) hand a handle of this engine to the node_tiled_* functions
// below, or refuse it by name.
// Saved points (rnde_node_forward_saveat / _everystep, the D x n x B backward) are served on a handle with a saveat capacity
// (rnde_node_tiled_reserve_saveat) by the SAVE instantiations of the same kernels; a handle without one refuses them as before.
#include "rnde_node.h"
#include "rnde_node_tile.h"
#include "rnde_tile_driver.h"
#include "rnde_tile_host.h"

static const char kNtPrefix[] = "TrackedNeuralODE tiled engine: ";

struct rnde_node_tiled {
    FcGeo G{};
    int Bp = 0, ntiles_max = 0;
    size_t lds_bytes = 0;
    Event ev[5];                     // (ahead of the buffers: members go in reverse order, the buffers and the meeting place first)
    // (every pointer member is an owner, rnde_alloc.h; h->h_meta, where the host reads the step log, is an owner of the rnde_node)
    TileSolveWs sw;                  // the solve's workspace and the tiles' meeting place (rnde_tile_host.h)
    DevBuf<float> tape, replay, rws, pacc, pcopy;
    DevBuf<FfStepRec> rec;           // [max_attempts]
    // rnde_node_set_tracking: taped forwards are reversed with the controller (and the initial step) differentiated
    bool track_ctrl = false, track_initdt = false;
    DevBuf<FfAttRec> att;            // [max_attempts]: the tracked sweep's attempt records (allocated when tracking is first switched on)
    DevBuf<double> tsb;              // [2]: the tracked sweep's (t0-bar, t1-bar)
    PinBuf<double> h_tsb;            // pinned [2]: where the host reads them (likewise)
    std::vector<FfStepRec> h_rec;    // the accepted steps' records of the last reverse sweep (likewise)
    std::vector<FfAttRec> h_att;     // the attempt records of the last tracked sweep (the source of an asynchronous copy: it outlives the call)
    // the taped forward, kept apart from the last solve (an untaped probe between a taped forward and its backward leaves it alone)
    std::vector<StepMeta> tp_meta;
    int tp_n_att = 0, tp_n_acc = 0, tp_B = 0;
    bool tp_track_ctrl = false, tp_track_initdt = false;      // the tape remembers the setting of its forward
    InitRec tp_init{};
    float tp_t0 = 0.f;
    bool ev_fwd = false, ev_bwd = false;
    // rnde_node_tiled_reserve_saveat: room for up to sv_cap save times per call (0: saving calls are refused, as on a fresh handle)
    int sv_cap = 0;
    DevBuf<float> sv_t;              // [sv_cap]: the save times of the running solve
    DevBuf<float> tp_sv_t;           // [sv_cap]: the tape's own copy (an untaped saving probe between a taped forward and its backward leaves it alone)
    DevBuf<SaveRange> sv_rng;        // [max_attempts]: the save indices of each record the reverse sweep walks (save_plan, formed on the host)
    std::vector<float> h_sv, tp_saveat;      // the running solve's times (the source of an asynchronous copy); the taped forward's (empty: an end-state tape)
    std::vector<SaveRange> h_rng;            // (likewise a copy's source)
};

static FcGeo nt_geo(const rnde_node_config* c) { return fc_geo(c->n_layers, c->dims, c->act, c->time_dep); }
static bool nt_shape_ok(const rnde_node_config* c) {
    if (!c || c->n_layers < 1 || c->n_layers > RNDE_MAX_LAYERS) return false;
    for (int l = 0; l <= c->n_layers; ++l) if (c->dims[l] < 1 || c->dims[l] > 65536) return false;
    return true;
}

extern "C" int64_t rnde_node_tiled_lds_bytes(const rnde_node_config* c) {
    if (!nt_shape_ok(c)) return -1;
    int64_t w = 0, y = 0, mp = 0;      // (in 64 bits: a shape far beyond the limit must not wrap into it)
    auto pad = [](int64_t n) { return (n + 15) / 16 * 16; };
    for (int l = 0; l <= c->n_layers; ++l) mp = std::max(mp, pad(c->dims[l]));
    for (int l = 0; l < c->n_layers; ++l) { w += pad(c->dims[l]) * (pad(c->dims[l + 1]) + 1) + 2 * pad(c->dims[l + 1]); y += pad(c->dims[l + 1]) * 16; }
    return 4 * ((w + 3) / 4 * 4 + pad(c->dims[0]) * 16 + y + 2 * mp * 16 + 128);
}

// What the tiled engine serves; a message that names the limit or the alternative otherwise (no device needed).
static const char* nt_refusal(const rnde_node_config* c) {
    static thread_local std::string msg;
    if (c->n_layers < 1 || c->n_layers > RNDE_MAX_LAYERS) return "TrackedNeuralODE tiled engine: n_layers must be 1..RNDE_MAX_LAYERS (8 Dense layers)";
    const int n = c->n_layers;
    for (int l = 0; l <= n; ++l) if (c->dims[l] < 1) return "TrackedNeuralODE tiled engine: every width must be at least 1";
    if (c->dims[0] != c->dims[n]) return "TrackedNeuralODE tiled engine: dims[0] must equal dims[n_layers] (the dynamics map the state to its own rate)";
    for (int l = 0; l < n; ++l)
        if (c->act[l] < RNDE_ACT_IDENTITY || c->act[l] > RNDE_ACT_ELU)
            return "TrackedNeuralODE tiled engine: an activation code outside rnde_act (identity, tanh, relu, sigmoid, softplus, elu) is not served";
    if (c->solver != RNDE_SOLVER_TSIT5) return "TrackedNeuralODE tiled engine: only Tsit5 is served (DP5 / DOP853 run on the chain engine, rnde_node_create, widths <= 64)";
    if (c->regularize >= RNDE_REG_STIFF && c->regularize <= RNDE_REG_STIFF_DT)
        return "TrackedNeuralODE tiled engine: the stiffness callbacks (RNDE_REG_STIFF, RNDE_REG_ERR_STIFF, RNDE_REG_STIFF_DT) are not served; "
               "regularize is RNDE_REG_NONE or RNDE_REG_ERR (EEst * dt per accepted step)";
    if (c->regularize != RNDE_REG_NONE && c->regularize != RNDE_REG_ERR) return "TrackedNeuralODE tiled engine: regularize: unknown value";
    if (c->pre_act != RNDE_PRE_NONE) return "TrackedNeuralODE tiled engine: pre_act must be RNDE_PRE_NONE (a leading tanh or cube runs on the chain engine, rnde_node_create)";
    if (c->col_tile != 0) return "TrackedNeuralODE tiled engine: col_tile must be 0 (the engine has one layout: four waves per 16 columns)";
    if (c->track_ctrl != 0 || c->track_initdt != 0)
        return "TrackedNeuralODE tiled engine: track_ctrl = 1 and track_initdt = 1 are not served in the create config: a fresh handle's reverse sweep "
               "treats step sizes and times as constants (set track_ctrl = 0 and track_initdt = 0; rnde_node_set_tracking then switches the handle to "
               "the sweep that differentiates the controller and the initial step, as rnde_node_create's engines do)";
    if (c->max_batch < 1 || c->max_attempts < 1 || !(c->reltol > 0.f) || !(c->abstol > 0.f)) return "TrackedNeuralODE tiled engine: bad max_batch / max_attempts / tolerances";
    if (c->max_batch > 16 * kMwMeetMax)
        return "TrackedNeuralODE tiled engine: max_batch above 4096 is not served (one meeting holds kMwMeetMax = 256 resident tiles of 16 columns)";
    if (c->max_attempts > kFtMaxAttempts) return "TrackedNeuralODE tiled engine: max_attempts above 8000 is not served (meeting tags)";
    const int64_t need = rnde_node_tiled_lds_bytes(c);
    if (need < 0 || need > (int64_t)kFtLdsBytes) {
        msg = "TrackedNeuralODE tiled engine: the resident weights and the activations of a tile need " + std::to_string((long long)need) +
              " bytes of LDS, above the limit of " + std::to_string(kFtLdsBytes) + " bytes (160 KB; solve and reverse sweep use the same layout)";
        return msg.c_str();
    }
    return nullptr;
}

void node_tiled_destroy(rnde_node* h) {
    delete h->tiled;
    h->tiled = nullptr;
}

extern "C" rnde_status rnde_node_create_tiled(const rnde_node_config* c, rnde_node** out) {
    if (!c || !out) { rnde_set_create_error("null argument"); return RNDE_ERR_BAD_ARG; }
    *out = nullptr;
    if (const char* why = nt_refusal(c)) { rnde_set_create_error(why); return RNDE_ERR_BAD_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= c->device) { rnde_set_create_error("no HIP device"); return RNDE_ERR_NO_DEVICE; }
    if (hipSetDevice(c->device) != hipSuccess) { rnde_set_create_error("hipSetDevice failed"); return RNDE_ERR_NO_DEVICE; }
    std::unique_ptr<rnde_node, void (*)(rnde_node*)> hold(new rnde_node(), rnde_node_destroy);
    rnde_node* h = hold.get();
    rnde_node_tiled* T = new rnde_node_tiled();
    h->tiled = T;
    h->cfg = *c; h->engine = 4;
    T->G = nt_geo(c);
    h->D = c->dims[0]; h->H = 0; h->P = T->G.P; h->BT = 16;
    T->ntiles_max = (c->max_batch + 15) / 16;
    T->Bp = 16 * T->ntiles_max;
    h->Bpad_max = T->Bp; h->nwg_max = T->ntiles_max;
    T->lds_bytes = (size_t)NtDyn::lds_floats(T->G) * 4;
    if ((int64_t)T->lds_bytes != rnde_node_tiled_lds_bytes(c)) { rnde_set_create_error("internal: LDS byte counts disagree"); return RNDE_ERR_BAD_ARG; }
    auto fail = [&](hipError_t e) { rnde_set_create_error(std::string("HIP: ") + hipGetErrorString(e)); return RNDE_ERR_HIP; };
    hipError_t e;
    const int D = h->D;
    const size_t RB = (size_t)D * T->Bp, MA = (size_t)c->max_attempts, NT = (size_t)T->ntiles_max;
    if ((e = T->sw.alloc(D, T->ntiles_max, 1, c->max_attempts, 0, kMwMeetMax, false)) != hipSuccess) return fail(e);
    if ((e = T->tape.alloc((MA + 1) * RB)) != hipSuccess) return fail(e);
    if ((e = T->replay.alloc(2 * MA)) != hipSuccess) return fail(e);
    if ((e = T->rws.alloc(NT * NtDyn::rev_ws_floats(T->G))) != hipSuccess) return fail(e);
    if ((e = T->pacc.alloc(NT * T->G.P)) != hipSuccess) return fail(e);
    if ((e = T->pcopy.alloc((size_t)T->G.P)) != hipSuccess) return fail(e);
    if ((e = T->rec.alloc(MA)) != hipSuccess) return fail(e);
    if ((e = h->own_h_meta.alloc(MA)) != hipSuccess) return fail(e);
    h->h_meta = h->own_h_meta;
    const void* solve = (const void*)rnde_tile_solve_kernel<NtDyn, false, false>;
    for (const void* k : {solve, (const void*)rnde_tile_reverse_kernel<NtDyn, false, false, false>, (const void*)rnde_tile_feval_kernel<NtDyn, false>})
        if ((e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)T->lds_bytes)) != hipSuccess) return fail(e);
    if (T->ntiles_max > kMeetXcdCus) {      // the agent-scope meeting: every tile of the largest batch must be resident at once
        const std::string why = tile_residency_refusal({solve}, kFtThreads, T->lds_bytes, T->ntiles_max, c->device, kNtPrefix, "the meeting", "this LDS footprint", &e);
        if (e != hipSuccess) return fail(e);
        if (!why.empty()) { rnde_set_create_error(why); return RNDE_ERR_BAD_ARG; }
    }
    for (auto& v : T->ev) if ((e = v.create()) != hipSuccess) return fail(e);
    *out = hold.release();
    return RNDE_OK;
}

rnde_status node_tiled_forward(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1, float* u_out_dev,
                               const float* saveat_host, int32_t n_saveat, float* sv_out_dev, int64_t* nfe_out, float* saveval_host,
                               int32_t* n_saveval_out, int32_t keep_tape, void* stream) {
    rnde_node_tiled* T = h->tiled;
    hipStream_t s = (hipStream_t)stream;
    const bool saving = saveat_host || n_saveat > 0 || sv_out_dev;
    if (saving && T->sv_cap == 0) {      // (a handle without a saveat capacity: rnde_node_tiled_reserve_saveat switches saving on)
        h->err = "TrackedNeuralODE tiled engine: rnde_node_forward_saveat is not served (the end state only; saveat runs on the engines of rnde_node_create)";
        return RNDE_ERR_BAD_ARG;
    }
    if (!x_dev || !p_dev || B < 1 || B > h->cfg.max_batch) { h->err = "bad argument (B must be 1..max_batch)"; return RNDE_ERR_BAD_ARG; }
    if (!(t1 > t0)) { h->err = "bad B or tspan"; return RNDE_ERR_BAD_ARG; }
    if (saving) {
        if (!saveat_host || n_saveat < 1 || !sv_out_dev) { h->err = "TrackedNeuralODE tiled engine: rnde_node_forward_saveat: saveat_host, n_saveat >= 1 and u_saved_dev are required"; return RNDE_ERR_BAD_ARG; }
        if (n_saveat > T->sv_cap) {
            h->err = "TrackedNeuralODE tiled engine: rnde_node_forward_saveat: n_saveat = " + std::to_string(n_saveat) + " is above the handle's saveat capacity of " +
                     std::to_string(T->sv_cap) + " (rnde_node_tiled_reserve_saveat)";
            return RNDE_ERR_BAD_ARG;
        }
        for (int i = 0; i < n_saveat; ++i)
            if (!(saveat_host[i] >= t0 && saveat_host[i] <= t1) || (i > 0 && !(saveat_host[i] > saveat_host[i - 1]))) {
                h->err = "saveat must be increasing and inside [t0, t1]"; return RNDE_ERR_BAD_ARG;
            }
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const float* steps_host = h->replay_host;
    const int n_steps = h->n_replay;
    const bool taped = keep_tape != 0;
    if (taped) {
        h->have_tape = false;
        HIPCHK(h, hipMemcpyAsync(T->pcopy, p_dev, (size_t)h->P * 4, hipMemcpyDeviceToDevice, s));      // (the tape keeps no caller pointer)
    }
    if (steps_host) HIPCHK(h, hipMemcpyAsync(T->replay, steps_host, (size_t)2 * n_steps * 4, hipMemcpyHostToDevice, s));
    if (saving) {
        T->h_sv.assign(saveat_host, saveat_host + n_saveat);
        HIPCHK(h, hipMemcpyAsync(T->sv_t, T->h_sv.data(), (size_t)n_saveat * 4, hipMemcpyHostToDevice, s));
        if (taped) HIPCHK(h, hipMemcpyAsync(T->tp_sv_t, T->h_sv.data(), (size_t)n_saveat * 4, hipMemcpyHostToDevice, s));
    }
    const TileSolveWs& W = T->sw;
    TileSolveParams<FcGeo> Q{};
    Q.F = tile_step_params(W, x_dev, h->D, B, h->cfg.reltol, h->cfg.abstol, t0, t1, h->cfg.max_attempts, steps_host ? (const float*)T->replay : nullptr, n_steps);
    if (saving) { Q.F.sv_t = T->sv_t; Q.F.nsave = n_saveat; Q.F.sv_out = sv_out_dev; }
    tile_bind_ws(Q, W);
    const int nt = (B + 15) / 16;
    Q.G = T->G; Q.p = p_dev; Q.x = x_dev; Q.tape = taped ? T->tape : nullptr; Q.x_out = u_out_dev; Q.dir = 1; Q.ntiles = nt;
    const StepState& fin = *T->sw.h_fin;
    std::string why;
    // every tile resident, one meeting per attempt (one XCD up to 32 tiles, agent scope above)
    HIPCHK(h, tile_run_met(T->sw.meet, nt, true, T->ev[0], T->ev[1], s,
                           [&](const Meet& meet) {
                               tile_bind_meet(Q, T->sw.meet, meet);
                               if (saving) hipLaunchKernelGGL((rnde_tile_solve_kernel<NtDyn, false, true>), dim3(MeetRes::grid(meet)), dim3(kFtThreads), T->lds_bytes, s, Q);
                               else hipLaunchKernelGGL((rnde_tile_solve_kernel<NtDyn, false, false>), dim3(MeetRes::grid(meet)), dim3(kFtThreads), T->lds_bytes, s, Q);
                               return hipGetLastError();
                           },
                           [&] { T->ev_fwd = true; return hipMemcpyAsync(W.h_fin, W.fin(), sizeof(StepState), hipMemcpyDeviceToHost, s); },
                           kNtPrefix, "the solve", "the solve was abandoned", &why));
    if (!why.empty()) { h->n_att = 0; h->err = why; return RNDE_ERR_HIP; }
    h->n_att = fin.n_att; h->B = B; h->Bpad = T->Bp; h->t0 = t0; h->t1 = t1;
    HIPCHK(h, tile_fetch_log(W.meta, fin.n_att, h->h_meta));
    if (const SolveVerdict v = solve_verdict(fin.status); v.st != RNDE_OK) { h->err = v.msg; return v.st; }
    if (nfe_out) *nfe_out = 3 + 6 * (int64_t)fin.n_att;      // 2 (initial dt) + 1 (fsalfirst) + 6 per attempt
    // SavingCallback(EEst * dt): 0 at init when it fires there, then one per accepted step
    const int nsv = gather_saved_values(h->h_meta, fin.n_att, F_ACCEPT, h->cfg.regularize, h->cfg.cb_save_start != 0, nullptr, saveval_host);
    h->n_saveval = nsv;
    if (n_saveval_out) *n_saveval_out = nsv;
    if (taped) {
        T->tp_meta.assign(h->h_meta, h->h_meta + fin.n_att);
        T->tp_n_att = fin.n_att; T->tp_n_acc = fin.n_acc; T->tp_B = B;
        T->tp_track_ctrl = T->track_ctrl; T->tp_track_initdt = T->track_initdt; T->tp_t0 = t0;
        if (saving) T->tp_saveat = T->h_sv; else T->tp_saveat.clear();
        if (T->track_initdt) HIPCHK(h, hipMemcpy(&T->tp_init, W.initrec_t, sizeof(InitRec), hipMemcpyDeviceToHost));      // (every tile's record is tile 0's)
        h->have_tape = true;
    }
    return RNDE_OK;
}

// Behind a sweep (ev[3]): the tiles' partial p-bars summed into p_bar_dev, then ev[4].
static hipError_t node_tiled_reduce(rnde_node* h, int nt, float* p_bar_dev, hipStream_t s) {
    rnde_node_tiled* T = h->tiled;
    hipLaunchKernelGGL(rnde_tile_reduce_kernel, dim3((h->P + 255) / 256), dim3(256), 0, s, (const float*)T->pacc, h->P, nt, p_bar_dev);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(T->ev[4], s);
    if (e == hipSuccess) T->ev_bwd = true;
    return e;
}

// The tracked sweep of a tape whose forward ran under rnde_node_set_tracking(h, 1, *): launched as the solve is, one meeting per attempt
// (and two for the initial step); rec: the accepted steps with their saved values' cotangents.
static rnde_status node_tiled_backward_tracked(rnde_node* h, const std::vector<FfStepRec>& rec, TileRevParams<FcGeo> Q, float* p_bar_dev, float* tspan_bar_host,
                                               hipStream_t s) {
    rnde_node_tiled* T = h->tiled;
    std::vector<FfAttRec>& att = T->h_att;
    tile_att_recs(T->tp_meta.data(), T->tp_n_att, rec, att);
    if (!att.empty()) HIPCHK(h, hipMemcpyAsync(T->att, att.data(), att.size() * sizeof(FfAttRec), hipMemcpyHostToDevice, s));
    const bool saving = !T->tp_saveat.empty();
    if (saving) {                               // one range per attempt (the trimmed ones covered nothing)
        T->h_rng.resize(T->tp_n_att + 1);
        save_plan(T->tp_saveat.data(), (int)T->tp_saveat.size(), T->tp_t0, T->tp_meta.data(), T->tp_n_att, F_ACCEPT, T->h_rng.data());
        if (!att.empty()) HIPCHK(h, hipMemcpyAsync(T->sv_rng, T->h_rng.data(), att.size() * sizeof(SaveRange), hipMemcpyHostToDevice, s));
    }
    const int nt = (T->tp_B + 15) / 16;
    Q.att = T->att; Q.n_att = (int)att.size(); Q.track_initdt = T->tp_track_initdt ? 1 : 0; Q.init = T->tp_init; Q.t0 = T->tp_t0; Q.tspan_out = T->tsb;
    double* tsb = T->h_tsb;
    std::string why;
    // (a new epoch re-arms the rows the solve used; att and tsb are members: a copy still in flight on an error return touches live memory)
    HIPCHK(h, tile_run_met(T->sw.meet, nt, true, T->ev[2], T->ev[3], s,
                           [&](const Meet& meet) {
                               tile_bind_meet(Q, T->sw.meet, meet);
                               if (saving) hipLaunchKernelGGL((rnde_tile_reverse_kernel<NtDyn, false, true, true>), dim3(MeetRes::grid(meet)), dim3(kFtThreads), T->lds_bytes, s, Q);
                               else hipLaunchKernelGGL((rnde_tile_reverse_kernel<NtDyn, false, true, false>), dim3(MeetRes::grid(meet)), dim3(kFtThreads), T->lds_bytes, s, Q);
                               return hipGetLastError();
                           },
                           [&] {
                               const hipError_t e = node_tiled_reduce(h, nt, p_bar_dev, s);
                               return e == hipSuccess ? hipMemcpyAsync(tsb, T->tsb, 2 * sizeof(double), hipMemcpyDeviceToHost, s) : e;
                           },
                           kNtPrefix, "the tracked reverse sweep", "the sweep was abandoned, x_bar, p_bar and tspan_bar are not valid", &why));
    if (!why.empty()) { h->err = why; return RNDE_ERR_HIP; }
    if (tspan_bar_host) { tspan_bar_host[0] = (float)tsb[0]; tspan_bar_host[1] = (float)tsb[1]; }
    return RNDE_OK;
}

// ---- rnde_node_set_tracking: which reverse sweep the taped forwards of a tiled handle get ----
extern "C" rnde_status rnde_node_set_tracking(rnde_node* h, int32_t track_ctrl, int32_t track_initdt) {
    if (!h) return RNDE_ERR_BAD_ARG;
    if (h->engine != 4) {
        h->err = "rnde_node_set_tracking: served on handles of rnde_node_create_tiled; the engines of rnde_node_create take cfg.track_ctrl / cfg.track_initdt "
                 "at creation";
        return RNDE_ERR_BAD_ARG;
    }
    rnde_node_tiled* T = h->tiled;
    if ((track_ctrl != 0 && track_ctrl != 1) || (track_initdt != 0 && track_initdt != 1)) {
        h->err = "TrackedNeuralODE tiled engine: rnde_node_set_tracking: track_ctrl and track_initdt are 0 or 1";
        return RNDE_ERR_BAD_ARG;
    }
    if (!track_ctrl && track_initdt) {
        h->err = "TrackedNeuralODE tiled engine: rnde_node_set_tracking: track_ctrl = 0 with track_initdt = 1 is not served: with the controller a constant "
                 "the proposed step of attempt 0 reaches nothing, so it repairs nothing (the settings are (0, 0), (1, 0) and (1, 1))";
        return RNDE_ERR_BAD_ARG;
    }
    if (h->have_tape) {
        h->err = "TrackedNeuralODE tiled engine: rnde_node_set_tracking: the handle holds a tape (a taped forward waiting for its backward); the tape "
                 "remembers the setting of its forward, change it before the forward or after rnde_node_release_tape";
        return RNDE_ERR_BAD_ARG;
    }
    if (track_ctrl && !T->att) {
        HIPCHK(h, hipSetDevice(h->cfg.device));
        const void* sweep = (const void*)rnde_tile_reverse_kernel<NtDyn, false, true, false>;
        HIPCHK(h, hipFuncSetAttribute(sweep, hipFuncAttributeMaxDynamicSharedMemorySize, (int)T->lds_bytes));
        if (T->ntiles_max > kMeetXcdCus) {      // the agent-scope meeting: every tile of the largest batch resident at once, on the tracked kernel's own footprint
            hipError_t e;
            const std::string why = tile_residency_refusal({sweep}, kFtThreads, T->lds_bytes, T->ntiles_max, h->cfg.device,
                                                           "TrackedNeuralODE tiled engine: rnde_node_set_tracking: ", "the tracked reverse sweep's meeting",
                                                           "the tracked sweep's footprint", &e);
            HIPCHK(h, e);
            if (!why.empty()) { h->err = why; return RNDE_ERR_BAD_ARG; }
        }
        // (att last: it is what marks the switch-on as done, so a call that failed half way is simply made again)
        HIPCHK(h, T->tsb.reserve(2));
        HIPCHK(h, T->h_tsb.reserve(2));
        HIPCHK(h, T->att.alloc((size_t)h->cfg.max_attempts));
    }
    T->track_ctrl = track_ctrl != 0; T->track_initdt = track_initdt != 0;
    return RNDE_OK;
}

extern "C" rnde_status rnde_node_tracking(const rnde_node* h, int32_t* ctrl_out, int32_t* initdt_out) {
    if (!h) return RNDE_ERR_BAD_ARG;
    // (a handle of rnde_node_create: its config's flags, fixed at creation)
    if (ctrl_out) *ctrl_out = h->engine == 4 ? (h->tiled->track_ctrl ? 1 : 0) : h->cfg.track_ctrl;
    if (initdt_out) *initdt_out = h->engine == 4 ? (h->tiled->track_initdt ? 1 : 0) : h->cfg.track_initdt;
    return RNDE_OK;
}

// ---- rnde_node_tiled_reserve_saveat: the per-handle switch of the saving calls (a capacity, which the engine needs anyway) ----
extern "C" int32_t rnde_node_tiled_saveat_capacity(const rnde_node* h) { return (h && h->engine == 4 && h->tiled) ? h->tiled->sv_cap : -1; }

extern "C" rnde_status rnde_node_tiled_reserve_saveat(rnde_node* h, int32_t max_saveat) {
    if (!h) return RNDE_ERR_BAD_ARG;
    if (h->engine != 4) {
        h->err = "rnde_node_tiled_reserve_saveat: served on handles of rnde_node_create_tiled; the engines of rnde_node_create serve "
                 "rnde_node_forward_saveat / _everystep without a reservation";
        return RNDE_ERR_BAD_ARG;
    }
    rnde_node_tiled* T = h->tiled;
    if (h->have_tape) {
        h->err = "TrackedNeuralODE tiled engine: rnde_node_tiled_reserve_saveat: the handle holds a tape (a taped forward waiting for its backward, which "
                 "may own save times); reserve before the forward or after rnde_node_release_tape";
        return RNDE_ERR_BAD_ARG;
    }
    if (max_saveat < 0 || max_saveat > h->cfg.max_attempts + 1) {
        h->err = "TrackedNeuralODE tiled engine: rnde_node_tiled_reserve_saveat: max_saveat = " + std::to_string(max_saveat) + " is outside 0.." +
                 std::to_string(h->cfg.max_attempts + 1) + " (max_attempts + 1: what save_everystep with save_start can need)";
        return RNDE_ERR_BAD_ARG;
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    T->sv_cap = 0;                              // (set last: a call that failed half way leaves a handle that refuses, and is simply made again)
    T->tp_saveat.clear();
    T->sv_t.reset(); T->tp_sv_t.reset(); T->sv_rng.reset();
    if (max_saveat == 0) return RNDE_OK;
    const void *solve = (const void*)rnde_tile_solve_kernel<NtDyn, false, true>, *sweep = (const void*)rnde_tile_reverse_kernel<NtDyn, false, true, true>;
    for (const void* k : {solve, (const void*)rnde_tile_reverse_kernel<NtDyn, false, false, true>, sweep})
        HIPCHK(h, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)T->lds_bytes));
    if (T->ntiles_max > kMeetXcdCus) {          // the agent-scope meeting: every tile of the largest batch resident at once, on the saving kernels' own footprint
        hipError_t e;
        const std::string why = tile_residency_refusal({solve, sweep}, kFtThreads, T->lds_bytes, T->ntiles_max, h->cfg.device,
                                                       "TrackedNeuralODE tiled engine: rnde_node_tiled_reserve_saveat: ",
                                                       "the meeting of the saving solve and sweep", "their footprint", &e);
        HIPCHK(h, e);
        if (!why.empty()) { h->err = why; return RNDE_ERR_BAD_ARG; }
    }
    HIPCHK(h, T->sv_t.reserve((size_t)max_saveat));
    HIPCHK(h, T->tp_sv_t.reserve((size_t)max_saveat));
    HIPCHK(h, T->sv_rng.reserve((size_t)h->cfg.max_attempts));
    T->sv_cap = max_saveat;
    return RNDE_OK;
}

rnde_status node_tiled_backward(rnde_node* h, const float* u_bar_dev, const float* saveval_bar_host, float* x_bar_dev, float* p_bar_dev,
                                float* tspan_bar_host, void* stream) {
    rnde_node_tiled* T = h->tiled;
    if (!u_bar_dev || !p_bar_dev) { h->err = "u_bar_dev and p_bar_dev are required"; return RNDE_ERR_BAD_ARG; }
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const bool reg = h->cfg.regularize == RNDE_REG_ERR;
    std::vector<FfStepRec>& rec = T->h_rec;      // (a member: the source of an asynchronous copy outlives an error return)
    tile_step_recs(T->tp_meta.data(), T->tp_n_att, reg ? saveval_bar_host : nullptr, reg && h->cfg.cb_save_start, rec);
    if ((int)rec.size() != T->tp_n_acc) { h->err = "internal: accepted-step count mismatch"; return RNDE_ERR_BAD_ARG; }
    if (!rec.empty()) HIPCHK(h, hipMemcpyAsync(T->rec, rec.data(), rec.size() * sizeof(FfStepRec), hipMemcpyHostToDevice, s));
    TileRevParams<FcGeo> Q{};
    Q.G = T->G; Q.p = T->pcopy; Q.tape = T->tape; Q.rec = T->rec; Q.out_bar = u_bar_dev; Q.ws = T->rws; Q.pacc = T->pacc; Q.x_bar = x_bar_dev;
    Q.n_acc = T->tp_n_acc; Q.B = T->tp_B; Q.Bp = T->Bp; Q.reltol = h->cfg.reltol; Q.abstol = h->cfg.abstol;
    const bool saving = !T->tp_saveat.empty();
    if (saving) { Q.sv_t = T->tp_sv_t; Q.rng = T->sv_rng; Q.nsave = (int)T->tp_saveat.size(); Q.save_t0 = T->tp_saveat[0] == T->tp_t0 ? 1 : 0; }
    if (T->tp_track_ctrl) return node_tiled_backward_tracked(h, rec, Q, p_bar_dev, tspan_bar_host, s);
    const int nt = (T->tp_B + 15) / 16;
    if (saving) {                               // one range per accepted step, in the order of rec
        std::vector<SaveRange> by_att(T->tp_n_att + 1);
        save_plan(T->tp_saveat.data(), (int)T->tp_saveat.size(), T->tp_t0, T->tp_meta.data(), T->tp_n_att, F_ACCEPT, by_att.data());
        T->h_rng.clear();
        for (int i = 0; i < T->tp_n_att; ++i) if (T->tp_meta[i].flags & F_ACCEPT) T->h_rng.push_back(by_att[i]);
        if (!T->h_rng.empty()) HIPCHK(h, hipMemcpyAsync(T->sv_rng, T->h_rng.data(), T->h_rng.size() * sizeof(SaveRange), hipMemcpyHostToDevice, s));
    }
    HIPCHK(h, tile_run_timed(T->ev[2], T->ev[3], s, [&] {      // (the tiles of this sweep do not meet)
        if (saving) hipLaunchKernelGGL((rnde_tile_reverse_kernel<NtDyn, false, false, true>), dim3(nt), dim3(kFtThreads), T->lds_bytes, s, Q);
        else hipLaunchKernelGGL((rnde_tile_reverse_kernel<NtDyn, false, false, false>), dim3(nt), dim3(kFtThreads), T->lds_bytes, s, Q);
        return hipGetLastError();
    }));
    HIPCHK(h, node_tiled_reduce(h, nt, p_bar_dev, s));
    HIPCHK(h, hipStreamSynchronize(s));      // (rec is a host vector: the copy must have left it)
    if (tspan_bar_host) { tspan_bar_host[0] = 0.f; tspan_bar_host[1] = 0.f; }      // step sizes and times are constants of this sweep
    return RNDE_OK;
}

rnde_status node_tiled_feval(rnde_node* h, const float* u_dev, const float* p_dev, int32_t B, float t, float* out_dev, void* stream) {
    rnde_node_tiled* T = h->tiled;
    if (!u_dev || !p_dev || !out_dev) { h->err = "bad argument"; return RNDE_ERR_BAD_ARG; }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((rnde_tile_feval_kernel<NtDyn, false>), dim3((B + 15) / 16), dim3(kFtThreads), T->lds_bytes, s, T->G, p_dev, u_dev, (const float*)nullptr, t, B, 0,
                       T->rws, (float*)nullptr, out_dev);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(s));
    return RNDE_OK;
}

rnde_status node_tiled_timing(rnde_node* h, float* fwd_ms, float* rev_sweep_ms, float* rev_rest_ms) {
    rnde_node_tiled* T = h->tiled;
    float a = -1.f, b = -1.f, c = -1.f;
    if (T->ev_fwd) { HIPCHK(h, hipEventSynchronize(T->ev[1])); HIPCHK(h, hipEventElapsedTime(&a, T->ev[0], T->ev[1])); }
    if (T->ev_bwd) {
        HIPCHK(h, hipEventSynchronize(T->ev[4]));
        HIPCHK(h, hipEventElapsedTime(&b, T->ev[2], T->ev[3])); HIPCHK(h, hipEventElapsedTime(&c, T->ev[3], T->ev[4]));
    }
    if (fwd_ms) *fwd_ms = a;
    if (rev_sweep_ms) *rev_sweep_ms = b;
    if (rev_rest_ms) *rev_rest_ms = c;
    return RNDE_OK;
}
