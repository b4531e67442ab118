// rnde_ffjord.hip -- C ABI of TrackedFFJORD (include/rnde.h, "TrackedFFJORD" section): create / forward / replay / backward / sample
// over the kernels of rnde_ffjord.h (one-launch solve) and rnde_bffjord.h (one-launch reverse sweep), or, on a handle of the tile layout,
// over the tile driver of rnde_tile_driver.h: rnde_ffjord_create_tiled (engine 1) runs it with the ConcatSquash dynamics FtDyn
// (rnde_ffjordt.h / rnde_bffjordt.h), rnde_ffjord_create_chain (engine 2) with the Dense-chain dynamics FcDyn (rnde_ffjordc.h /
// rnde_bffjordc.h).  The *_kinetic entries run the KIN = true instantiations of the same kernels over D + 3 rows (TrackedFFJORD{false}
// called with regularize = true).  The *_exact entries run the plain instantiations of the tile driver with the exact trace in the forward
// solve, on the tape and in the reverse sweep (engines 1 and 2).
#include <algorithm>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/rnde.h"
#include "rnde_alloc.h"          // first among the project headers: every hipMalloc behind it goes through the RNDE_POISON wrapper
#include "rnde_bffjord.h"
#include "rnde_bffjordt.h"
#include "rnde_bffjordc.h"
#include "rnde_tile_driver.h"
#include "rnde_tile_host.h"
#include "rnde_probe.h"
#include "rnde_ffjord_loss.h"

using namespace rnde;

static thread_local std::string g_ff_create_err;

struct rnde_ffjord {
    rnde_ffjord_config cfg;
    FfGeo G;
    std::string err;
    int Bp = 0, T = 0, R = 0;
    size_t lds_bytes = 0;
    Event ev[4];                     // (ahead of the buffers: members go in reverse order, the buffers first)
    // (every allocated member is an owner, rnde_alloc.h)
    // The solve's workspace (rnde_tile_host.h).  Engines 1 and 2: alloc'ed whole, with the tiles' meeting place; sw.scratch is the exact
    // trace's matrix per tile of engine 1.  Engine 0 fills the members its one workgroup uses (ws, norm [512], ctl [3], meta, initrec_t [1], h_fin, Bp).
    TileSolveWs sw;
    DevBuf<float> tape, e_buf, replay;
    DevBuf<float> rws, pacc;
    DevBuf<FfStepRec> rec;           // [max_attempts]
    std::vector<StepMeta> h_meta;    // step log of the last solve (rnde_ffjord_steps / _timing)
    int n_att = 0, n_acc = 0, B = 0;
    // the taped forward, kept apart from the last solve: an untaped call (an inference probe, sample) between a taped forward and its
    // backward leaves the tape, its step log and its operands as they were
    struct Tape {
        bool valid = false;
        std::vector<StepMeta> meta;
        int n_att = 0, n_acc = 0, B = 0;
        float reltol = 0.f, abstol = 0.f;
        const float* e = nullptr;    // the probe (the caller's, or e_tape)
        const float* p = nullptr;
        bool kin = false;            // a kinetic forward: D + 3 rows per record
        bool exact = false;          // an exact-trace forward (rnde_ffjord_forward_exact): no probe, the reverse sweep's exact variant
        bool trk = false;            // the handle's track_ctrl setting at the forward: backward runs the tracked sweep
    } tp;
    bool kin_ready = false;          // ws / tape / rws hold D + 3 rows (grown by the first kinetic call)
    DevBuf<float> e_tape;            // the library's probe of a taped forward (e_buf serves untaped calls)
    float fwd_ms = -1.f, rev_ms = -1.f;
    // the tile layout (engine = 1, 2): one workgroup per 16 columns, the workgroups meeting once per attempt
    int engine = 0;
    FtGeo TG{};
    int ntiles_max = 0;
    FcGeo CG{};                      // engine = 2: the Dense-chain dynamics on the tile layout (cfg holds the shared fields, in_dims = D)
    bool track_ctrl = false;         // rnde_ffjord_set_track_ctrl: taped forwards are reversed with the controller differentiated
    DevBuf<FfAttRec> att;            // [max_attempts]: the tracked sweep's attempt records (allocated when tracking is first switched on)
    // several batches per launch (rnde_ffjord_reserve_groups): the capacity is the switch, NULL without one.  Everything a group call
    // touches on the device is here; the handle's own workspace, tape and step log are not touched by it.
    struct Groups {
        int max_groups = 0, tiles = 0, max_columns = 0;
        // the groups' columns side by side under the call's row stride; a group's states, step log and meeting granules lie behind those
        // of the groups in front
        TileSolveWs sw;
        DevBuf<TileGroup> table;         // [max_groups]
        PinBuf<TileGroup> h_table;       // pinned: [max_groups]
        std::vector<std::vector<StepMeta>> log;      // the step logs of the last group call
    };
    std::unique_ptr<Groups> gr;
    // rnde_ffjord_nll_grad: logpx when the caller passes NULL, the kinetic rows and the reverse sweep's seeds (allocated at the first fused call)
    DevBuf<float> f_logpx, f_logpx_bar, f_reg, f_reg_bar;      // [max_batch], [max_batch], [2][max_batch], [2][max_batch]
};

#define FCHK(h, x)                                                                                  \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) { (h)->err = std::string("HIP: ") + hipGetErrorString(e_); return RNDE_ERR_HIP; } \
    } while (0)

// The dynamics of a handle of the tile layout: f(DynTag<Dyn>{}, geometry), Dyn = FcDyn with h->CG (engine 2) or FtDyn with h->TG (engine 1).
template <class D> struct DynTag { using type = D; };
template <class F>
static auto with_dyn(rnde_ffjord* h, F&& f) { return h->engine == 2 ? f(DynTag<FcDyn>{}, h->CG) : f(DynTag<FtDyn>{}, h->TG); }
// The KIN instantiation of a kernel: f(std::true_type{}) for the kinetic rows, f(std::false_type{}) without.
template <class F>
static void with_kin(bool kin, F&& f) { if (kin) f(std::true_type{}); else f(std::false_type{}); }

// rnde_debug_elementwise's share of this translation unit (rnde_probe.h): the private softplus of rnde_ffjord.h
struct EwFfjord {
    __device__ float operator()(float a, float) const { return ff_softplus(a); }
};
hipError_t rnde::elementwise_ffjord(const float* in, long long n, float* out, hipStream_t s) {
    return elementwise_launch(EwFfjord{}, in, nullptr, n, out, s);
}

extern "C" const char* rnde_ffjord_last_error(const rnde_ffjord* h) { return h ? h->err.c_str() : g_ff_create_err.c_str(); }

extern "C" int32_t rnde_ffjord_param_count(const rnde_ffjord_config* c) {
    if (!c || c->in_dims < 1 || c->hidden < 1) return -1;
    const int D = c->in_dims, H = c->hidden;
    return ff_layer_params(D, H) + ff_layer_params(H, H) + ff_layer_params(H, D);
}

// What the kernels serve; a message that names the limit otherwise (tiled: the tiled engine's limits).
static const char* ff_refusal(const rnde_ffjord_config* c, bool tiled = false) {
    if (c->dynamics != RNDE_FFJORD_CONCAT_SQUASH)
        return "TrackedFFJORD: this config describes the ConcatSquash MLPDynamics of experiments/ffjord_gaussian.jl (dynamics = forw_n_back) only; "
               "the default forw_n_back (TDChain / Dense dynamics through Tracker.forward) is served by rnde_ffjord_create_chain "
               "(rnde_ffjord_chain_config)";
    if (!tiled && (c->in_dims < 1 || c->in_dims + 1 > kFfMaxW || c->hidden < 1 || c->hidden > kFfMaxW))
        return "TrackedFFJORD: widths above the chain engine's limit of 64 are not served (in_dims + 1 <= 64 and hidden <= 64; "
               "rnde_ffjord_create_tiled / engine = \"tiled\" serves wider models)";
    if (tiled && (c->in_dims < 1 || c->in_dims > kFtMaxD || c->hidden < 1 || c->hidden > kFtMaxH))
        return "TrackedFFJORD tiled engine: widths above its LDS limit are not served (in_dims <= 64 and hidden <= 112: the resident weights "
               "and activations of a tile within 160 KB of LDS)";
    if (c->kinetic_reg)
        return "TrackedFFJORD{false} with regularize = true (kinetic energy and Jacobian norm rows) is not served";
    if (c->regularize != 0 && c->regularize != 1) return "TrackedFFJORD: regularize is 0 ({false}) or 1 ({true}: EEst * dt per accepted step)";
    if (c->solver != RNDE_SOLVER_TSIT5) return "TrackedFFJORD: only Tsit5 is served";
    if (c->max_batch < 1 || c->max_attempts < 1 || !(c->reltol > 0.f) || !(c->abstol > 0.f)) return "TrackedFFJORD: bad max_batch / max_attempts / tolerances";
    if (tiled && c->max_batch > 16 * kMwMeetMax)
        return "TrackedFFJORD tiled engine: max_batch above 4096 is not served (one meeting holds kMwMeetMax = 256 resident tiles of 16 columns)";
    if (tiled && c->max_attempts > kFtMaxAttempts) return "TrackedFFJORD tiled engine: max_attempts above 8000 is not served (meeting tags)";
    return nullptr;
}

using FfHold = std::unique_ptr<rnde_ffjord, void (*)(rnde_ffjord*)>;      // a handle under construction: destroyed unless the last step releases it

// The buffers, kernel attributes and XCD slot of a handle of the tile layout, for the dynamics Dyn with geometry G (h->cfg is filled).
template <class Dyn>
static rnde_status tile_create(FfHold hold, const typename Dyn::Geo& G, rnde_ffjord** out) {
    rnde_ffjord* h = hold.get();
    const rnde_ffjord_config* c = &h->cfg;
    const int D = G.D, R = D + 1;
    h->R = R;
    h->ntiles_max = (c->max_batch + 15) / 16;
    h->Bp = 16 * h->ntiles_max;
    h->T = kFtThreads;
    h->lds_bytes = (size_t)Dyn::lds_floats(G) * 4;
    auto fail = [&](hipError_t e) { g_ff_create_err = std::string("HIP: ") + hipGetErrorString(e); return RNDE_ERR_HIP; };
    hipError_t e;
    const size_t RB = (size_t)R * h->Bp, MA = (size_t)c->max_attempts, NT = (size_t)h->ntiles_max;
    if ((e = h->sw.alloc(R, h->ntiles_max, 1, c->max_attempts, Dyn::scratch_floats(G), kMwMeetMax, false)) != hipSuccess) return fail(e);
    if ((e = h->tape.alloc((MA + 1) * RB)) != hipSuccess) return fail(e);
    if ((e = h->e_buf.alloc((size_t)D * h->Bp)) != hipSuccess) return fail(e);
    if ((e = h->e_tape.alloc((size_t)D * h->Bp)) != hipSuccess) return fail(e);
    if ((e = h->replay.alloc(2 * MA)) != hipSuccess) return fail(e);
    if ((e = h->rws.alloc(NT * Dyn::rev_ws_floats(G))) != hipSuccess) return fail(e);
    if ((e = h->pacc.alloc(NT * G.P)) != hipSuccess) return fail(e);
    if ((e = h->rec.alloc(MA)) != hipSuccess) return fail(e);
    for (const void* k : {(const void*)rnde_tile_solve_kernel<Dyn, false>, (const void*)rnde_tile_reverse_kernel<Dyn, false>,
                          (const void*)rnde_tile_feval_kernel<Dyn, false>, (const void*)rnde_tile_solve_kernel<Dyn, true>,
                          (const void*)rnde_tile_reverse_kernel<Dyn, true>, (const void*)rnde_tile_feval_kernel<Dyn, true>,
                          (const void*)rnde_tile_reverse_kernel<Dyn, false, true>})
        if ((e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes)) != hipSuccess) return fail(e);
    for (auto& v : h->ev) if ((e = v.create()) != hipSuccess) return fail(e);
    *out = hold.release();
    return RNDE_OK;
}

// A handle on the selected device, or NULL with the create error set.
static FfHold ff_new_handle(int device, rnde_status* st) {
    FfHold none(nullptr, rnde_ffjord_destroy);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) { g_ff_create_err = "no HIP device"; *st = RNDE_ERR_NO_DEVICE; return none; }
    if (hipSetDevice(device) != hipSuccess) { g_ff_create_err = "hipSetDevice failed"; *st = RNDE_ERR_NO_DEVICE; return none; }
    return FfHold(new rnde_ffjord(), rnde_ffjord_destroy);
}

extern "C" rnde_status rnde_ffjord_create_tiled(const rnde_ffjord_config* c, rnde_ffjord** out) {
    if (!c || !out) { g_ff_create_err = "null argument"; return RNDE_ERR_BAD_ARG; }
    *out = nullptr;
    if (const char* why = ff_refusal(c, true)) { g_ff_create_err = why; return RNDE_ERR_BAD_ARG; }
    rnde_status st = RNDE_OK;
    FfHold h = ff_new_handle(c->device, &st);
    if (!h) return st;
    h->cfg = *c;
    h->engine = 1;
    h->G = ff_geo(c->in_dims, c->hidden);
    h->TG = ft_geo(c->in_dims, c->hidden);
    if ((size_t)FtDyn::lds_floats(h->TG) * 4 > (size_t)kFtLdsBytes) {
        g_ff_create_err = "TrackedFFJORD tiled engine: a tile does not fit in LDS";
        return RNDE_ERR_BAD_ARG;
    }
    const FtGeo G = h->TG;
    return tile_create<FtDyn>(std::move(h), G, out);
}

extern "C" int32_t rnde_ffjord_engine(const rnde_ffjord* h) { return h ? h->engine : -1; }

// ---- the tracked-controller reverse sweep (engines 1 and 2, regularize = 1) ----
extern "C" rnde_status rnde_ffjord_set_track_ctrl(rnde_ffjord* h, int32_t on) {
    if (!h) return RNDE_ERR_BAD_ARG;
    if (on != 0 && on != 1) { h->err = "TrackedFFJORD track_ctrl: the setting is 0 (step sizes and times are constants of the reverse sweep) or 1"; return RNDE_ERR_BAD_ARG; }
    if (h->engine == 0) {
        h->err = "TrackedFFJORD track_ctrl: the one-workgroup engine does not differentiate the step controller; create the handle with "
                 "rnde_ffjord_create_tiled (engine = \"tiled\") or rnde_ffjord_create_chain";
        return RNDE_ERR_BAD_ARG;
    }
    if (!h->cfg.regularize) {
        h->err = "TrackedFFJORD track_ctrl: a regularize = 0 handle has no saved value EEst * dt, and without one the tracked and the constant-step "
                 "sweep agree to O(tol) (2e-10 to 2e-6 relative, measured with the fp64 oracle); track_ctrl needs regularize = 1";
        return RNDE_ERR_BAD_ARG;
    }
    if (h->tp.valid) {
        h->err = "TrackedFFJORD track_ctrl: the handle holds a tape (a taped forward waiting for its backward); the tape remembers the setting of its "
                 "forward, change it before the forward";
        return RNDE_ERR_BAD_ARG;
    }
    if (on && !h->att) {       // its meeting needs every tile of the largest batch resident at once, on the tracked kernel's own footprint
        hipError_t e;
        const std::string why = with_dyn(h, [&](auto dyn, const auto&) {
            return tile_residency_refusal({(const void*)rnde_tile_reverse_kernel<typename decltype(dyn)::type, false, true>}, kFtThreads, h->lds_bytes, h->ntiles_max,
                                          h->cfg.device, "TrackedFFJORD track_ctrl: ", "the reverse sweep's meeting", "the tracked sweep's footprint", &e);
        });
        FCHK(h, e);
        if (!why.empty()) { h->err = why; return RNDE_ERR_BAD_ARG; }
        FCHK(h, h->att.alloc((size_t)h->cfg.max_attempts));
    }
    h->track_ctrl = on != 0;
    return RNDE_OK;
}

extern "C" int32_t rnde_ffjord_track_ctrl(const rnde_ffjord* h) { return h ? (h->track_ctrl ? 1 : 0) : -1; }

// ---- the Dense-chain dynamics (rnde_ffjord_create_chain) ----
static bool fc_shape_ok(const rnde_ffjord_chain_config* c) {
    if (!c || c->n_layers < 1 || c->n_layers > RNDE_MAX_LAYERS) return false;
    for (int l = 0; l <= c->n_layers; ++l) if (c->dims[l] < 1) return false;
    return true;
}

extern "C" int32_t rnde_ffjord_chain_param_count(const rnde_ffjord_chain_config* c) {
    if (!fc_shape_ok(c)) return -1;
    int64_t P = 0;
    for (int l = 0; l < c->n_layers; ++l) P += (int64_t)(c->dims[l] + (c->time_dep ? 1 : 0)) * c->dims[l + 1] + c->dims[l + 1];
    return P > INT32_MAX ? -1 : (int32_t)P;
}

// What the chain kernels serve; a message that names the limit otherwise (no device needed).
static const char* fc_refusal(const rnde_ffjord_chain_config* c) {
    static thread_local std::string msg;
    if (c->n_layers < 1 || c->n_layers > RNDE_MAX_LAYERS)
        return "TrackedFFJORD chain dynamics: n_layers must be 1..RNDE_MAX_LAYERS (8 Dense layers)";
    const int n = c->n_layers, td = c->time_dep ? 1 : 0;
    for (int l = 0; l <= n; ++l) if (c->dims[l] < 1) return "TrackedFFJORD chain dynamics: every width must be at least 1";
    if (c->dims[0] != c->dims[n])
        return "TrackedFFJORD chain dynamics: dims[0] must equal dims[n_layers] (the dynamics map the state to its own rate)";
    for (int l = 0; l < n; ++l)
        if (c->dims[l + 1] > kFcMaxW || c->dims[l] > kFcMaxW)
            return "TrackedFFJORD chain dynamics: widths above the limit of 64 are not served (no layer's output and no layer's input above 64; "
                   "the time row of a TDChain layer is an epilogue vector and does not count)";
    if (c->dims[0] + 1 > kFcMaxW)
        return "TrackedFFJORD chain dynamics: the state [z; l] must fit the limit of 64 rows (dims[0] + 1 <= 64; dims[0] + 3 <= 64 for the "
               "kinetic energy rows)";
    for (int l = 0; l < n; ++l)
        if (c->act[l] < RNDE_ACT_IDENTITY || c->act[l] > RNDE_ACT_ELU)
            return "TrackedFFJORD chain dynamics: an activation code outside rnde_act (identity, tanh, relu, sigmoid, softplus, elu) is not served";
    if (c->regularize != 0 && c->regularize != 1) return "TrackedFFJORD: regularize is 0 ({false}) or 1 ({true}: EEst * dt per accepted step)";
    if (c->solver != RNDE_SOLVER_TSIT5) return "TrackedFFJORD: only Tsit5 is served";
    if (c->max_batch < 1 || c->max_attempts < 1 || !(c->reltol > 0.f) || !(c->abstol > 0.f)) return "TrackedFFJORD: bad max_batch / max_attempts / tolerances";
    if (c->max_batch > 16 * kMwMeetMax)
        return "TrackedFFJORD chain dynamics: max_batch above 4096 is not served (one meeting holds kMwMeetMax = 256 resident tiles of 16 columns)";
    if (c->max_attempts > kFtMaxAttempts) return "TrackedFFJORD chain dynamics: max_attempts above 8000 is not served (meeting tags)";
    const FcGeo G = fc_geo(n, c->dims, c->act, td);
    const size_t need = (size_t)FcDyn::lds_floats(G) * 4;
    if (need > (size_t)kFtLdsBytes) {
        msg = "TrackedFFJORD chain dynamics: the resident weights and the activations of a tile need " + std::to_string(need) +
              " bytes of LDS, above the limit of " + std::to_string(kFtLdsBytes) + " bytes (160 KB)";
        return msg.c_str();
    }
    return nullptr;
}

extern "C" rnde_status rnde_ffjord_create_chain(const rnde_ffjord_chain_config* c, rnde_ffjord** out) {
    if (!c || !out) { g_ff_create_err = "null argument"; return RNDE_ERR_BAD_ARG; }
    *out = nullptr;
    if (const char* why = fc_refusal(c)) { g_ff_create_err = why; return RNDE_ERR_BAD_ARG; }
    rnde_status st = RNDE_OK;
    FfHold h = ff_new_handle(c->device, &st);
    if (!h) return st;
    h->engine = 2;
    h->CG = fc_geo(c->n_layers, c->dims, c->act, c->time_dep);
    const int D = h->CG.D;
    rnde_ffjord_config& k = h->cfg;        // the fields the shared entries read
    k = rnde_ffjord_config{};
    k.in_dims = D; k.hidden = 0; k.dynamics = RNDE_FFJORD_TRACKER_FORWARD; k.time_dep = c->time_dep; k.regularize = c->regularize;
    k.max_batch = c->max_batch; k.solver = c->solver; k.reltol = c->reltol; k.abstol = c->abstol; k.cb_save_start = c->cb_save_start;
    k.max_attempts = c->max_attempts; k.device = c->device;
    h->G = FfGeo{};
    h->G.D = D; h->G.H = 0; h->G.P = h->CG.P;
    const FcGeo G = h->CG;
    return tile_create<FcDyn>(std::move(h), G, out);
}

extern "C" rnde_status rnde_ffjord_create(const rnde_ffjord_config* c, rnde_ffjord** out) {
    if (!c || !out) { g_ff_create_err = "null argument"; return RNDE_ERR_BAD_ARG; }
    *out = nullptr;
    if (const char* why = ff_refusal(c)) { g_ff_create_err = why; return RNDE_ERR_BAD_ARG; }
    rnde_status st = RNDE_OK;
    FfHold hold = ff_new_handle(c->device, &st);
    if (!hold) return st;
    rnde_ffjord* h = hold.get();
    h->cfg = *c;
    h->G = ff_geo(c->in_dims, c->hidden);
    const int D = c->in_dims, R = D + 1, HS = std::max(c->hidden, D), HR = std::max(c->hidden, R);
    h->R = R;
    h->Bp = (c->max_batch + 63) / 64 * 64;
    // threads of the solve workgroup: the most (<= 512) whose LDS vectors fit next to the parameters
    for (int T = kFfMaxThreads; T >= 64; T /= 2) {
        const size_t bytes = ((size_t)h->G.P + 32 + (size_t)3 * HS * T) * 4;
        if (bytes <= 160 * 1024 && (T <= h->Bp || T == 64)) { h->T = T; h->lds_bytes = bytes; break; }
    }
    auto fail = [&](hipError_t e) { g_ff_create_err = std::string("HIP: ") + hipGetErrorString(e); return RNDE_ERR_HIP; };
    hipError_t e;
    if (!h->T) { g_ff_create_err = "TrackedFFJORD: parameters and per-column vectors do not fit in LDS"; return RNDE_ERR_BAD_ARG; }
    const size_t RB = (size_t)R * h->Bp, MA = (size_t)c->max_attempts;
    h->sw.Bp = h->Bp;
    if ((e = h->sw.ws.alloc(10 * RB)) != hipSuccess) return fail(e);
    if ((e = h->tape.alloc((MA + 1) * RB)) != hipSuccess) return fail(e);
    if ((e = h->sw.norm.alloc(512)) != hipSuccess) return fail(e);
    if ((e = hipMemset(h->sw.norm, 0, 512 * 4)) != hipSuccess) return fail(e);
    if ((e = h->e_buf.alloc((size_t)D * h->Bp)) != hipSuccess) return fail(e);
    if ((e = h->e_tape.alloc((size_t)D * h->Bp)) != hipSuccess) return fail(e);
    if ((e = h->replay.alloc(2 * MA)) != hipSuccess) return fail(e);
    if ((e = h->rws.alloc((size_t)(24 + kFfVjpVecs) * HR * h->Bp)) != hipSuccess) return fail(e);
    if ((e = h->pacc.alloc((size_t)h->G.P * h->Bp)) != hipSuccess) return fail(e);
    if ((e = h->sw.ctl.alloc(3)) != hipSuccess) return fail(e);
    if ((e = h->sw.meta.alloc(MA)) != hipSuccess) return fail(e);
    if ((e = h->sw.initrec_t.alloc(1)) != hipSuccess) return fail(e);
    if ((e = h->rec.alloc(MA)) != hipSuccess) return fail(e);
    for (const void* k : {(const void*)rnde_ffjord_solve_kernel<false>, (const void*)rnde_ffjord_solve_kernel<true>})
        if ((e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes)) != hipSuccess) return fail(e);
    for (auto& v : h->ev) if ((e = v.create()) != hipSuccess) return fail(e);
    if ((e = h->sw.h_fin.alloc(1)) != hipSuccess) return fail(e);
    *out = hold.release();
    return RNDE_OK;
}

extern "C" void rnde_ffjord_destroy(rnde_ffjord* h) { delete h; }      // (every buffer and event is an owner)

// The first kinetic call of a handle: the limits, then state, tape and reverse workspace for D + 3 rows.  Plain calls go on using the
// same buffers with their own D + 1 row layout; a plain tape waiting for its backward is carried over.
static rnde_status ff_kinetic_ready(rnde_ffjord* h) {
    if (h->cfg.regularize) {
        h->err = "TrackedFFJORD{true} has no kinetic energy rows: the reference's {true} method never passes regularize on (ffjord.jl:119); "
                 "create the handle with regularize = 0";
        return RNDE_ERR_BAD_ARG;
    }
    const int D = h->G.D, H = h->G.H, Rk = D + 3;
    if (h->engine == 0 && (Rk > kFfMaxW || H > kFfMaxW)) {
        h->err = "TrackedFFJORD kinetic energy rows: widths above the chain engine's limit of 64 are not served (in_dims + 3 <= 64 and hidden <= 64; "
                 "rnde_ffjord_create_tiled / engine = \"tiled\" serves in_dims <= 64 and hidden <= 112)";
        return RNDE_ERR_BAD_ARG;
    }
    if (h->engine == 2 && Rk > kFcMaxW) {
        h->err = "TrackedFFJORD kinetic energy rows on chain dynamics: the state [z; l; lambda1; lambda2] must fit the limit of 64 rows "
                 "(dims[0] + 3 <= 64)";
        return RNDE_ERR_BAD_ARG;
    }
    if (h->kin_ready) return RNDE_OK;
    const size_t RBk = (size_t)Rk * h->Bp, RB = (size_t)h->R * h->Bp, MA = (size_t)h->cfg.max_attempts;
    const size_t rws = h->engine == 0 ? (size_t)(24 + kFfVjpVecsKin) * std::max(H, Rk) * h->Bp
                                      : with_dyn(h, [&](auto dyn, const auto& G) { return (size_t)h->ntiles_max * decltype(dyn)::type::rev_ws_floats(G, true); });
    FCHK(h, hipDeviceSynchronize());           // (rnde_ffjord_debug_feval does not wait for its launch)
    DevBuf<float> tape, rw;          // (the handle keeps what it has unless all three, the workspace in front, are there)
    const hipError_t e = h->sw.grow_rows(Rk, [&] {
        hipError_t e = tape.alloc((MA + 1) * RBk);
        if (e == hipSuccess) e = rw.alloc(rws);
        if (e == hipSuccess && h->tp.valid) e = hipMemcpy(tape, h->tape, ((size_t)h->tp.n_acc + 1) * RB * 4, hipMemcpyDeviceToDevice);
        return e;
    });
    if (e != hipSuccess) {
        h->err = std::string("TrackedFFJORD kinetic energy rows: HIP: ") + hipGetErrorString(e);
        return RNDE_ERR_HIP;
    }
    h->tape.swap(tape); h->rws.swap(rw);      // (the old two go with the locals)
    h->kin_ready = true;
    return RNDE_OK;
}

// One solve as its entry describes it: dir = +1 the forward (logpx; Hutchinson probe e, or exact: the exact trace and no probe), dir = -1
// sampling (exact trace, tau = t1 - t).  kin: the kinetic forward (D + 3 rows, the two rows to reg_out; ff_kinetic_ready has run).
// The leading members are what every rnde_ffjord_forward* entry takes (an aggregate); an entry then sets what is its own.
struct FfCall {
    const float *x, *p, *e; int32_t B; float t0, t1; uint64_t seed;
    float *logpx, *x_out; int32_t keep_tape; hipStream_t s;
    int dir = +1;
    bool replay = false;                    // a *_replay entry: steps_host (n_steps pairs (dt, accepted)) is required
    const float* steps_host = nullptr; int32_t n_steps = 0;
    bool kin = false, exact = false;
    float* reg_out = nullptr;
    const FfLossSeed* ls = nullptr;         // rnde_ffjord_nll_grad: the loss-and-seed kernel behind the solve
};

static rnde_status ff_solve(rnde_ffjord* h, const FfCall& c) {
    const int dir = c.dir, B = c.B;
    const bool kin = c.kin, exact = c.exact;
    hipStream_t s = c.s;
    if (!c.x || !c.p || B < 1 || B > h->cfg.max_batch) { h->err = "bad argument (B must be 1..max_batch)"; return RNDE_ERR_BAD_ARG; }
    if (!(c.t1 > c.t0)) { h->err = "TrackedFFJORD: tspan must satisfy t1 > t0 (sample() integrates t1 -> t0 itself)"; return RNDE_ERR_BAD_ARG; }
    if (c.steps_host && (c.n_steps < 1 || c.n_steps > h->cfg.max_attempts)) { h->err = "replay: n_steps must be 1..max_attempts"; return RNDE_ERR_BAD_ARG; }
    const bool taped = dir > 0 && c.keep_tape;
    if (taped) h->tp.valid = false;            // (only a taped forward replaces the tape)
    const float* e_dev = c.e;
    if (dir > 0 && !exact && !e_dev) {   // the library's normal stream, drawn once per call (the reference's default argument)
        float* eb = taped ? h->e_tape : h->e_buf;
        rnde_status st = rnde_normal_fill(eb, (int64_t)h->G.D * B, c.seed, 0x46464A4FULL, s);
        if (st != RNDE_OK) { h->err = "rnde_normal_fill failed"; return st; }
        e_dev = eb;
    }
    if (c.steps_host) FCHK(h, hipMemcpyAsync(h->replay, c.steps_host, (size_t)2 * c.n_steps * 4, hipMemcpyHostToDevice, s));
    const TileSolveWs& W = h->sw;
    const StepParams F = tile_step_params(W, c.x, kin ? h->G.D + 3 : h->R, B, h->cfg.reltol, h->cfg.abstol, dir > 0 ? c.t0 : 0.f, dir > 0 ? c.t1 : c.t1 - c.t0,
                                          h->cfg.max_attempts, c.steps_host ? (const float*)h->replay : nullptr, c.n_steps);
    const float* e_solve = (dir > 0 && !exact) ? e_dev : nullptr;
    float *tape = taped ? (float*)h->tape : nullptr, *logpx = dir > 0 ? c.logpx : nullptr;
    const bool tiles = h->engine >= 1;     // engines 1 and 2 share the tile layout, the meeting and its checks
    auto launch = [&](const Meet& meet) {
        if (!tiles) {
            FfSolveParams Q{};
            Q.F = F; Q.G = h->G; Q.p = c.p; Q.x = c.x; Q.e = e_solve; Q.ws = W.ws; Q.tape = tape; Q.logpx = logpx; Q.x_out = c.x_out; Q.norm = W.norm;
            Q.dir = dir; Q.T = h->T; Q.Bp = h->Bp; Q.tbase = c.t1; Q.reg = c.reg_out;
            with_kin(kin, [&](auto K) { hipLaunchKernelGGL(rnde_ffjord_solve_kernel<decltype(K)::value>, dim3(1), dim3(h->T), h->lds_bytes, s, Q); });
        } else with_dyn(h, [&](auto dyn, const auto& G) {
            using Dyn = typename decltype(dyn)::type;
            TileSolveParams<typename Dyn::Geo> T{};
            T.F = F; T.G = G; T.p = c.p; T.x = c.x; T.e = e_solve; T.tape = tape; T.logpx = logpx; T.x_out = c.x_out;
            tile_bind_ws(T, W);
            tile_bind_meet(T, h->sw.meet, meet);
            T.exact = (dir < 0 || exact) ? 1 : 0; T.scratch = T.exact ? (float*)W.scratch : nullptr;
            T.dir = dir; T.ntiles = meet.n; T.tbase = c.t1; T.reg = c.reg_out;
            const dim3 grid(MeetRes::grid(meet));      // one XCD: every eighth block is a tile (the others return at once)
            with_kin(kin, [&](auto K) { hipLaunchKernelGGL((rnde_tile_solve_kernel<Dyn, decltype(K)::value>), grid, dim3(kFtThreads), h->lds_bytes, s, T); });
        });
        return hipGetLastError();
    };
    auto behind = [&] {        // rnde_ffjord_nll_grad: the loss terms and the sweep's seeds, behind the solve and in front of the host wait
        if (c.ls) {
            ff_launch_loss_seed(*c.ls, kin, s);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        return hipMemcpyAsync(W.h_fin, W.fin(), sizeof(StepState), hipMemcpyDeviceToHost, s);
    };
    const StepState& fin = *h->sw.h_fin;
    std::string why;
    if (tiles) {       // every tile resident, one meeting per attempt (one XCD up to 32 tiles, agent scope above)
        FCHK(h, tile_run_met(h->sw.meet, (B + 15) / 16, true, h->ev[0], h->ev[1], s, launch, behind, "TrackedFFJORD tiled engine: ", "the solve", "the solve was abandoned", &why));
    } else {           // the one workgroup meets nobody: the same order without the meeting's steps
        FCHK(h, tile_run_timed(h->ev[0], h->ev[1], s, [&] { return launch(Meet{}); }));
        FCHK(h, behind());
        FCHK(h, hipStreamSynchronize(s));
    }
    (void)hipEventElapsedTime(&h->fwd_ms, h->ev[0], h->ev[1]);
    if (!why.empty()) { h->n_att = h->n_acc = 0; h->h_meta.clear(); h->err = why; return RNDE_ERR_HIP; }
    h->n_att = fin.n_att; h->n_acc = fin.n_acc; h->B = B;
    h->h_meta.resize(fin.n_att);
    FCHK(h, tile_fetch_log(W.meta, fin.n_att, h->h_meta.data()));
    if (const SolveVerdict v = solve_verdict(fin.status); v.st != RNDE_OK) { h->err = v.msg; return v.st; }
    if (taped) {
        rnde_ffjord::Tape& T = h->tp;
        T.meta = h->h_meta; T.n_att = h->n_att; T.n_acc = h->n_acc; T.B = B;
        T.reltol = F.reltol; T.abstol = F.abstol; T.e = exact ? nullptr : e_dev; T.p = c.p; T.kin = kin; T.exact = exact; T.trk = h->track_ctrl; T.valid = true;
    }
    return RNDE_OK;
}

// A forward solve (c.dir = +1) behind its entry's checks, then what the entry hands back: nfe and the saved values.
static rnde_status ff_forward(rnde_ffjord* h, const FfCall& c, int64_t* nfe_out, float* saveval_host, int32_t* n_saveval_out) {
    if (!h) return RNDE_ERR_BAD_ARG;
    const bool exact = c.exact, kin = c.kin;
    if (c.replay && !c.steps_host) { h->err = "replay: steps_host is required"; return RNDE_ERR_BAD_ARG; }
    if (exact && h->engine == 0) {
        h->err = "TrackedFFJORD exact trace: the one-workgroup engine does not serve the exact forward; create the handle with "
                 "rnde_ffjord_create_tiled (engine = \"tiled\") or rnde_ffjord_create_chain";
        return RNDE_ERR_BAD_ARG;
    }
    if (exact && kin) { h->err = "TrackedFFJORD exact trace: the kinetic energy rows are not served with it (the Jacobian norm row is defined on the probe)"; return RNDE_ERR_BAD_ARG; }
    if (!c.logpx) { h->err = "logpx_dev is required"; return RNDE_ERR_BAD_ARG; }
    if (kin) {
        if (!c.reg_out) { h->err = "reg_out_dev (2 x B: the kinetic energy row, then the Jacobian norm row) is required"; return RNDE_ERR_BAD_ARG; }
        if (rnde_status kst = ff_kinetic_ready(h)) return kst;
    }
    rnde_status st = ff_solve(h, c);
    if (st != RNDE_OK) return st;
    if (nfe_out) *nfe_out = 3 + 6 * (int64_t)h->n_att;      // 2 (initial dt) + 1 (fsalfirst) + 6 per attempt, as rnde_node_forward
    // SavingCallback(EEst * dt) (ffjord.jl:116): 0 at init when it fires there, then one per accepted step
    const int nsv = gather_saved_values(h->h_meta.data(), h->n_att, F_ACCEPT, h->cfg.regularize ? RNDE_REG_ERR : RNDE_REG_NONE, h->cfg.cb_save_start != 0, nullptr, saveval_host);
    if (n_saveval_out) *n_saveval_out = nsv;
    return RNDE_OK;
}

extern "C" rnde_status rnde_ffjord_forward(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t B, float t0, float t1,
                                           uint64_t seed, float* logpx_dev, float* z_out_dev, int64_t* nfe_out, float* saveval_host,
                                           int32_t* n_saveval_out, int32_t keep_tape, void* stream) {
    return ff_forward(h, FfCall{x_dev, p_dev, e_dev, B, t0, t1, seed, logpx_dev, z_out_dev, keep_tape, (hipStream_t)stream}, nfe_out, saveval_host, n_saveval_out);
}

extern "C" rnde_status rnde_ffjord_forward_replay(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t B, float t0,
                                                  float t1, uint64_t seed, const float* steps_host, int32_t n_steps, float* logpx_dev, float* z_out_dev,
                                                  int64_t* nfe_out, float* saveval_host, int32_t* n_saveval_out, int32_t keep_tape, void* stream) {
    FfCall c{x_dev, p_dev, e_dev, B, t0, t1, seed, logpx_dev, z_out_dev, keep_tape, (hipStream_t)stream};
    c.replay = true; c.steps_host = steps_host; c.n_steps = n_steps;
    return ff_forward(h, c, nfe_out, saveval_host, n_saveval_out);
}

extern "C" rnde_status rnde_ffjord_forward_kinetic(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t B, float t0,
                                                   float t1, uint64_t seed, float* logpx_dev, float* reg_out_dev, float* z_out_dev, int64_t* nfe_out,
                                                   int32_t keep_tape, void* stream) {
    FfCall c{x_dev, p_dev, e_dev, B, t0, t1, seed, logpx_dev, z_out_dev, keep_tape, (hipStream_t)stream};
    c.kin = true; c.reg_out = reg_out_dev;
    return ff_forward(h, c, nfe_out, nullptr, nullptr);
}

extern "C" rnde_status rnde_ffjord_forward_kinetic_replay(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t B,
                                                          float t0, float t1, uint64_t seed, const float* steps_host, int32_t n_steps,
                                                          float* logpx_dev, float* reg_out_dev, float* z_out_dev, int64_t* nfe_out,
                                                          int32_t keep_tape, void* stream) {
    FfCall c{x_dev, p_dev, e_dev, B, t0, t1, seed, logpx_dev, z_out_dev, keep_tape, (hipStream_t)stream};
    c.replay = true; c.steps_host = steps_host; c.n_steps = n_steps; c.kin = true; c.reg_out = reg_out_dev;
    return ff_forward(h, c, nfe_out, nullptr, nullptr);
}

extern "C" rnde_status rnde_ffjord_forward_exact(rnde_ffjord* h, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1, float* logpx_dev,
                                                 float* z_out_dev, int64_t* nfe_out, float* saveval_host, int32_t* n_saveval_out, int32_t keep_tape,
                                                 void* stream) {
    FfCall c{x_dev, p_dev, nullptr, B, t0, t1, 0, logpx_dev, z_out_dev, keep_tape, (hipStream_t)stream};
    c.exact = true;
    return ff_forward(h, c, nfe_out, saveval_host, n_saveval_out);
}

extern "C" rnde_status rnde_ffjord_forward_exact_replay(rnde_ffjord* h, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1,
                                                        const float* steps_host, int32_t n_steps, float* logpx_dev, float* z_out_dev, int64_t* nfe_out,
                                                        float* saveval_host, int32_t* n_saveval_out, int32_t keep_tape, void* stream) {
    FfCall c{x_dev, p_dev, nullptr, B, t0, t1, 0, logpx_dev, z_out_dev, keep_tape, (hipStream_t)stream};
    c.replay = true; c.steps_host = steps_host; c.n_steps = n_steps; c.exact = true;
    return ff_forward(h, c, nfe_out, saveval_host, n_saveval_out);
}

// The attempt count of a step log and, into out_host (may be NULL), its export: (t, dt, EEst, accepted) when wide, (dt, accepted) otherwise.
static rnde_status ff_export(rnde_ffjord* h, const char* entry, const StepMeta* log, int n_att, bool wide, float* out_host, int32_t capacity, int32_t* n_attempts_out) {
    *n_attempts_out = n_att;
    if (!out_host) return RNDE_OK;
    if (capacity < n_att) { h->err = std::string(entry) + ": capacity below the attempt count"; return RNDE_ERR_BAD_ARG; }
    if (wide) export_step_log(log, n_att, F_ACCEPT, out_host);
    else export_steps(log, n_att, F_ACCEPT, out_host);
    return RNDE_OK;
}

extern "C" rnde_status rnde_ffjord_step_log(rnde_ffjord* h, float* log_host, int32_t capacity, int32_t* n_attempts_out) {
    if (!h || !n_attempts_out) return RNDE_ERR_BAD_ARG;
    return ff_export(h, "step_log", h->h_meta.data(), h->n_att, true, log_host, capacity, n_attempts_out);
}

extern "C" rnde_status rnde_ffjord_steps(rnde_ffjord* h, float* steps_host, int32_t capacity, int32_t* n_attempts_out) {
    if (!h || !n_attempts_out) return RNDE_ERR_BAD_ARG;
    return ff_export(h, "steps", h->h_meta.data(), h->n_att, false, steps_host, capacity, n_attempts_out);
}

// The reverse sweep of the taped forward; a kinetic tape runs the KIN = true kernels with reg_bar_dev (NULL: zeros), an exact tape the
// exact variant of the tile driver's sweep.
static rnde_status ff_backward(rnde_ffjord* h, const float* logpx_bar_dev, const float* saveval_bar_host, const float* reg_bar_dev, float* p_bar_dev,
                               float* x_bar_dev, void* stream) {
    if (!h) return RNDE_ERR_BAD_ARG;
    const rnde_ffjord::Tape& T = h->tp;
    if (!T.valid) { h->err = "backward without a taped forward"; return RNDE_ERR_NO_TAPE; }
    if (!logpx_bar_dev || !p_bar_dev) { h->err = "logpx_bar_dev and p_bar_dev are required"; return RNDE_ERR_BAD_ARG; }
    hipStream_t s = (hipStream_t)stream;
    std::vector<FfStepRec> rec;
    tile_step_recs(T.meta.data(), T.n_att, h->cfg.regularize ? saveval_bar_host : nullptr, h->cfg.regularize && h->cfg.cb_save_start, rec);
    if ((int)rec.size() != T.n_acc) { h->err = "internal: accepted-step count mismatch"; return RNDE_ERR_BAD_ARG; }
    if (!rec.empty()) FCHK(h, hipMemcpyAsync(h->rec, rec.data(), rec.size() * sizeof(FfStepRec), hipMemcpyHostToDevice, s));
    const bool trk = T.trk && h->engine >= 1 && !T.kin;
    std::vector<FfAttRec> att;
    const int nt = (T.B + 15) / 16;
    if (trk) {
        tile_att_recs(T.meta.data(), T.n_att, rec, att);
        if (!att.empty()) FCHK(h, hipMemcpyAsync(h->att, att.data(), att.size() * sizeof(FfAttRec), hipMemcpyHostToDevice, s));
    }
    // The sweep and the sum of its partial p-bars.  meet != NULL: the tracked sweep (the step records are unused; the attempt records
    // are in h->att), placed as the solve is.
    auto sweep = [&](const Meet* meet) {
        auto fill = [&](auto& Q) {       // (what FfRevParams and TileRevParams share; the cotangent of logpx is set beside it)
            Q.p = T.p; Q.e = T.e; Q.tape = h->tape; Q.rec = h->rec; Q.ws = h->rws; Q.pacc = h->pacc; Q.x_bar = x_bar_dev; Q.n_acc = T.n_acc; Q.B = T.B;
            Q.Bp = h->Bp; Q.reltol = T.reltol; Q.abstol = T.abstol; Q.reg_bar = reg_bar_dev;
        };
        if (h->engine == 0) {
            FfRevParams Q{};
            fill(Q);
            Q.G = h->G; Q.logpx_bar = logpx_bar_dev;
            with_kin(T.kin, [&](auto K) { hipLaunchKernelGGL(rnde_ffjord_reverse_kernel<decltype(K)::value>, dim3((T.B + 255) / 256), dim3(256), 0, s, Q); });
        } else with_dyn(h, [&](auto dyn, const auto& G) {
            using Dyn = typename decltype(dyn)::type;
            TileRevParams<typename Dyn::Geo> Q{};
            fill(Q);
            Q.G = G; Q.out_bar = logpx_bar_dev; Q.exact = T.exact ? 1 : 0; Q.scratch = T.exact ? (float*)h->sw.scratch : nullptr;
            if (meet) {
                Q.att = h->att; Q.n_att = (int)att.size();
                tile_bind_meet(Q, h->sw.meet, *meet);
                hipLaunchKernelGGL((rnde_tile_reverse_kernel<Dyn, false, true>), dim3(MeetRes::grid(*meet)), dim3(kFtThreads), h->lds_bytes, s, Q);
            } else
                with_kin(T.kin, [&](auto K) { hipLaunchKernelGGL((rnde_tile_reverse_kernel<Dyn, decltype(K)::value>), dim3(nt), dim3(kFtThreads), h->lds_bytes, s, Q); });
        });
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (h->engine == 0) hipLaunchKernelGGL(rnde_ffjord_reduce_kernel, dim3((h->G.P + 255) / 256), dim3(256), 0, s, (const float*)h->pacc, h->G.P, T.B, h->Bp, p_bar_dev);
        else hipLaunchKernelGGL(rnde_tile_reduce_kernel, dim3((h->G.P + 255) / 256), dim3(256), 0, s, (const float*)h->pacc, h->G.P, nt, p_bar_dev);
        return hipGetLastError();
    };
    std::string why;
    FCHK(h, trk ? tile_run_met(h->sw.meet, nt, true, h->ev[2], h->ev[3], s, [&](const Meet& meet) { return sweep(&meet); }, [] { return hipSuccess; },
                               "TrackedFFJORD track_ctrl: ", "the tracked reverse sweep", "the sweep was abandoned, p_bar and x_bar are not valid", &why)
                : tile_run_timed(h->ev[2], h->ev[3], s, [&] { return sweep(nullptr); }));      // (the tiles of the constant-step sweep do not meet)
    FCHK(h, hipEventSynchronize(h->ev[3]));
    (void)hipEventElapsedTime(&h->rev_ms, h->ev[2], h->ev[3]);
    if (!why.empty()) { h->err = why; return RNDE_ERR_HIP; }
    return RNDE_OK;
}

extern "C" rnde_status rnde_ffjord_backward(rnde_ffjord* h, const float* logpx_bar_dev, const float* saveval_bar_host, float* p_bar_dev,
                                            float* x_bar_dev, void* stream) {
    return ff_backward(h, logpx_bar_dev, saveval_bar_host, nullptr, p_bar_dev, x_bar_dev, stream);
}

extern "C" rnde_status rnde_ffjord_backward_kinetic(rnde_ffjord* h, const float* logpx_bar_dev, const float* reg_bar_dev, float* p_bar_dev,
                                                    float* x_bar_dev, void* stream) {
    if (!h) return RNDE_ERR_BAD_ARG;
    if (h->tp.valid && h->tp.exact) {
        h->err = "backward_kinetic: the taped forward is an exact-trace one, which has no kinetic energy rows (use rnde_ffjord_backward)";
        return RNDE_ERR_BAD_ARG;
    }
    if (h->tp.valid && !h->tp.kin) { h->err = "backward_kinetic: the taped forward has no kinetic energy rows (use rnde_ffjord_backward)"; return RNDE_ERR_BAD_ARG; }
    return ff_backward(h, logpx_bar_dev, nullptr, reg_bar_dev, p_bar_dev, x_bar_dev, stream);
}

// The training step's gradient in one call (include/rnde.h; the formulas: rnde_ffjord_loss.h): the taped forward with the loss-and-seed
// kernel behind its solve launch, the saved values' term on the host, the reverse sweep.  The call consumes its own tape.
extern "C" rnde_status rnde_ffjord_nll_grad(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t B, float t0, float t1,
                                            uint64_t seed, int32_t mode, float lambda_r, float lambda_k, float lambda_j, float* p_bar_dev,
                                            float* x_bar_dev, float* logpx_dev, float* terms_dev, float* reg_out_host, int64_t* nfe_out, void* stream) {
    if (!h) return RNDE_ERR_BAD_ARG;
    auto refuse = [&](const char* why) { h->err = why; return RNDE_ERR_BAD_ARG; };
    if (mode < 0 || mode > 2) return refuse("nll_grad: mode must be 0 (Hutchinson probe), 1 (exact trace) or 2 (kinetic energy and Jacobian norm rows)");
    if (mode == 1 && h->engine == 0)
        return refuse("nll_grad mode 1: TrackedFFJORD exact trace: the one-workgroup engine does not serve the exact forward; create the handle with "
                      "rnde_ffjord_create_tiled (engine = \"tiled\") or rnde_ffjord_create_chain");
    if (mode == 1 && e_dev) return refuse("nll_grad mode 1: the exact trace takes no probe; e_dev must be NULL");
    if (mode != 2 && (lambda_k != 0.f || lambda_j != 0.f))
        return refuse("nll_grad: lambda_k and lambda_j weigh the kinetic energy and Jacobian norm rows, which exist in mode 2 only; they must be 0 outside it");
    if (lambda_r != 0.f && !h->cfg.regularize)
        return refuse("nll_grad: lambda_r weighs the saved values EEst * dt, which a regularize = 0 handle does not have; it must be 0 there");
    if (!p_bar_dev || !terms_dev || !reg_out_host || !nfe_out) return refuse("nll_grad: p_bar_dev, terms_dev, reg_out_host and nfe_out are required");
    if (!x_dev || !p_dev || B < 1 || B > h->cfg.max_batch) return refuse("nll_grad: bad argument (x_dev and p_dev are required, B must be 1..max_batch)");
    if (!(t1 > t0)) return refuse("nll_grad: TrackedFFJORD: tspan must satisfy t1 > t0");
    if (mode == 2)
        if (rnde_status kst = ff_kinetic_ready(h)) return kst;
    const bool kin = mode == 2;
    const size_t MB = (size_t)h->cfg.max_batch;
    if (!h->f_logpx_bar) {
        DevBuf<float> a, b, c, d;      // (the handle takes all four or none)
        hipError_t e = a.alloc(MB);
        if (e == hipSuccess) e = b.alloc(MB);
        if (e == hipSuccess) e = c.alloc(2 * MB);
        if (e == hipSuccess) e = d.alloc(2 * MB);
        FCHK(h, e);
        h->f_logpx.swap(a); h->f_logpx_bar.swap(b); h->f_reg.swap(c); h->f_reg_bar.swap(d);
    }
    float* logpx = logpx_dev ? logpx_dev : (float*)h->f_logpx;
    FfLossSeed ls{};
    ls.logpx = logpx; ls.reg = kin ? (float*)h->f_reg : nullptr; ls.terms = terms_dev; ls.logpx_bar = h->f_logpx_bar;
    ls.reg_bar = kin ? (float*)h->f_reg_bar : nullptr; ls.B = B; ls.lambda_k = lambda_k; ls.lambda_j = lambda_j;
    std::vector<float> sv((size_t)h->cfg.max_attempts + 1), sv_bar;
    int32_t nsv = 0;
    FfCall c{x_dev, p_dev, mode == 1 ? nullptr : e_dev, B, t0, t1, seed, logpx, nullptr, 1, (hipStream_t)stream};
    c.kin = kin; c.reg_out = kin ? (float*)h->f_reg : nullptr; c.exact = mode == 1; c.ls = &ls;
    rnde_status st = ff_forward(h, c, nfe_out, sv.data(), &nsv);
    if (st != RNDE_OK) { h->tp.valid = false; return st; }      // (no sweep behind a solve that failed)
    *reg_out_host = h->cfg.regularize ? ff_saveval_term(sv.data(), nsv, lambda_r, sv_bar) : 0.f;
    st = ff_backward(h, h->f_logpx_bar, h->cfg.regularize && nsv ? sv_bar.data() : nullptr, kin ? (const float*)h->f_reg_bar : nullptr, p_bar_dev, x_bar_dev,
                     stream);
    h->tp.valid = false;
    return st;
}

extern "C" rnde_status rnde_ffjord_sample(rnde_ffjord* h, const float* p_dev, const float* z_dev, int32_t n, float t0, float t1, uint64_t seed,
                                          float* x_out_dev, void* stream) {
    if (!h) return RNDE_ERR_BAD_ARG;
    if (!x_out_dev) { h->err = "x_out_dev is required"; return RNDE_ERR_BAD_ARG; }
    hipStream_t s = (hipStream_t)stream;
    if (!z_dev) {      // z ~ N(0, I) from the library's normal stream
        if (n < 1 || n > h->cfg.max_batch) { h->err = "bad argument (n must be 1..max_batch)"; return RNDE_ERR_BAD_ARG; }
        rnde_status st = rnde_normal_fill(h->e_buf, (int64_t)h->G.D * n, seed, 0x53414D50ULL, s);
        if (st != RNDE_OK) { h->err = "rnde_normal_fill failed"; return st; }
        z_dev = h->e_buf;
    }
    FfCall c{z_dev, p_dev, nullptr, n, t0, t1, seed, nullptr, x_out_dev, 0, s};
    c.dir = -1;
    return ff_solve(h, c);
}

// One evaluation of the dynamics on the handle's engine (the launch is not waited for).
static rnde_status ff_feval(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t B, float t, int32_t exact, bool kin,
                            float* out_dev, hipStream_t s) {
    if (h->engine == 0) with_kin(kin, [&](auto K) {
        hipLaunchKernelGGL(rnde_ffjord_feval_kernel<decltype(K)::value>, dim3((B + 255) / 256), dim3(256), 0, s, h->G, p_dev, x_dev, e_dev, t, B, exact, h->rws, out_dev);
    });
    else with_dyn(h, [&](auto dyn, const auto& G) { with_kin(kin, [&](auto K) {
        hipLaunchKernelGGL((rnde_tile_feval_kernel<typename decltype(dyn)::type, decltype(K)::value>), dim3((B + 15) / 16), dim3(kFtThreads), h->lds_bytes, s, G, p_dev,
                           x_dev, e_dev, t, B, exact, h->rws, h->sw.scratch, out_dev);
    }); });
    FCHK(h, hipGetLastError());
    return RNDE_OK;
}

extern "C" rnde_status rnde_ffjord_debug_feval(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t B, float t,
                                               int32_t exact, float* out_dev, void* stream) {
    if (!h || !x_dev || !p_dev || !out_dev || B < 1 || B > h->cfg.max_batch || (!exact && !e_dev)) { if (h) h->err = "bad argument"; return RNDE_ERR_BAD_ARG; }
    return ff_feval(h, x_dev, p_dev, e_dev, B, t, exact, false, out_dev, (hipStream_t)stream);
}

extern "C" rnde_status rnde_ffjord_debug_feval_kinetic(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t B, float t,
                                                       float* out_dev, void* stream) {
    if (!h || !x_dev || !p_dev || !e_dev || !out_dev || B < 1 || B > h->cfg.max_batch) { if (h) h->err = "bad argument"; return RNDE_ERR_BAD_ARG; }
    if (rnde_status kst = ff_kinetic_ready(h)) return kst;
    return ff_feval(h, x_dev, p_dev, e_dev, B, t, 0, true, out_dev, (hipStream_t)stream);
}

// ---- several batches per launch (engines 1 and 2; the plan: rnde_group_plan.h, the kernel: rnde_tile_group_solve_kernel) ----
extern "C" rnde_status rnde_ffjord_reserve_groups(rnde_ffjord* h, int32_t max_groups, int32_t max_columns) {
    if (!h) return RNDE_ERR_BAD_ARG;
    const std::string why = group_reserve_refusal(h->engine, h->tp.valid, max_groups, max_columns);
    if (!why.empty()) { h->err = why; return RNDE_ERR_BAD_ARG; }
    FCHK(h, hipDeviceSynchronize());           // (nothing of a call in flight reads what is released here)
    h->gr.reset();
    if (max_groups == 0) return RNDE_OK;
    const int tiles = group_reserved_tiles(max_columns);
    return with_dyn(h, [&](auto dyn, const auto& G) {
        using Dyn = typename decltype(dyn)::type;
        const void* kern = (const void*)rnde_tile_group_solve_kernel<Dyn>;
        FCHK(h, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes));
        hipError_t e;
        // (up to 32 tiles the check counts one workgroup on each CU of an XCD, which the whole device holds as well: the launch is at agent scope)
        const std::string full = tile_residency_refusal({kern}, kFtThreads, h->lds_bytes, tiles, h->cfg.device, "TrackedFFJORD groups: max_columns / 16: ",
                                                        "the group solve's meetings", "the group kernel's footprint", &e);
        FCHK(h, e);
        if (!full.empty()) { h->err = full; return RNDE_ERR_BAD_ARG; }
        auto gr = std::make_unique<rnde_ffjord::Groups>();
        FCHK(h, gr->sw.alloc(h->R, tiles, max_groups, h->cfg.max_attempts, Dyn::scratch_floats(G), tiles, true));
        FCHK(h, gr->table.alloc((size_t)max_groups));
        FCHK(h, gr->h_table.alloc((size_t)max_groups));
        gr->max_groups = max_groups; gr->tiles = tiles; gr->max_columns = max_columns;
        h->gr = std::move(gr);
        return RNDE_OK;
    });
}

extern "C" rnde_status rnde_ffjord_group_capacity(const rnde_ffjord* h, int32_t* max_groups_out, int32_t* max_columns_out) {
    if (!h) return RNDE_ERR_BAD_ARG;
    if (max_groups_out) *max_groups_out = h->gr ? h->gr->max_groups : 0;
    if (max_columns_out) *max_columns_out = h->gr ? h->gr->max_columns : 0;
    return RNDE_OK;
}

extern "C" rnde_status rnde_ffjord_forward_groups(rnde_ffjord* h, const float* x_dev, const float* p_dev, const float* e_dev, int32_t n_groups,
                                                  const int32_t* B_host, float t0, float t1, int32_t exact, float* logpx_dev, int64_t* nfe_out_host,
                                                  int32_t* status_out_host, double* sum_dev, int64_t* count_dev, void* stream) {
    if (!h) return RNDE_ERR_BAD_ARG;
    if (h->engine == 0) { h->err = group_reserve_refusal(0, false, 0, 0); return RNDE_ERR_BAD_ARG; }
    const std::string why = group_call_refusal(h->gr ? h->gr->max_groups : 0, h->gr ? h->gr->tiles : 0, h->cfg.max_batch, n_groups, B_host, t0, t1, exact != 0,
                                               h->engine >= 1, e_dev != nullptr, sum_dev != nullptr, count_dev != nullptr);
    if (!why.empty()) { h->err = why; return RNDE_ERR_BAD_ARG; }
    if (!x_dev || !p_dev || !logpx_dev) { h->err = "TrackedFFJORD groups: x_dev, p_dev and logpx_dev are required"; return RNDE_ERR_BAD_ARG; }
    rnde_ffjord::Groups& GR = *h->gr;
    hipStream_t s = (hipStream_t)stream;
    const GroupPlan plan = group_plan(n_groups, B_host);
    for (int g = 0; g < n_groups; ++g) GR.h_table[g] = plan.g[g];
    FCHK(h, hipMemcpyAsync(GR.table, GR.h_table, (size_t)n_groups * sizeof(TileGroup), hipMemcpyHostToDevice, s));
    GR.log.clear();
    const TileSolveWs& W = GR.sw;
    // (the fields of ff_solve's forward under the call's row stride; B, Bn and the per-group pointers are set per group on the device)
    StepParams F = tile_step_params(W, x_dev, h->R, plan.g[0].B, h->cfg.reltol, h->cfg.abstol, t0, t1, h->cfg.max_attempts, nullptr, 0);
    F.Bpad = plan.Bp;
    auto launch = [&](const Meet& meet) {
        with_dyn(h, [&](auto dyn, const auto& G) {
            using Dyn = typename decltype(dyn)::type;
            TileGroupParams<typename Dyn::Geo> Q{};
            TileSolveParams<typename Dyn::Geo>& T = Q.T;
            T.F = F; T.G = G; T.p = p_dev; T.x = x_dev; T.e = exact ? nullptr : e_dev; T.logpx = logpx_dev;
            tile_bind_ws(T, W);
            tile_bind_meet(T, GR.sw.meet, meet);
            T.exact = exact ? 1 : 0; T.scratch = exact ? (float*)W.scratch : nullptr; T.dir = 1; T.Bp = plan.Bp; T.ntiles = plan.g[0].ntiles; T.tbase = t1;
            Q.table = GR.table; Q.n_groups = plan.n_groups; Q.meet_rows = h->cfg.max_attempts + 4; Q.meta_stride = h->cfg.max_attempts;
            Q.scratch_floats = Dyn::scratch_floats(G);
            hipLaunchKernelGGL((rnde_tile_group_solve_kernel<Dyn>), dim3(plan.tiles), dim3(kFtThreads), h->lds_bytes, s, Q);
        });
        return hipGetLastError();
    };
    std::string bad;
    FCHK(h, tile_run_met(GR.sw.meet, plan.tiles, false, h->ev[0], h->ev[1], s, launch,      // agent scope whatever the count
                         [&] { return hipMemcpyAsync(W.h_fin, W.fin(), (size_t)n_groups * sizeof(StepState), hipMemcpyDeviceToHost, s); },
                         "TrackedFFJORD groups: ", "the group solve", "every group was abandoned", &bad));
    (void)hipEventElapsedTime(&h->fwd_ms, h->ev[0], h->ev[1]);
    if (!bad.empty()) { h->err = bad; return RNDE_ERR_HIP; }
    GR.log.resize(n_groups);
    int first_bad = -1;
    for (int g = 0; g < n_groups; ++g) {
        const StepState& fin = GR.sw.h_fin[g];
        GR.log[g].resize(fin.n_att);
        FCHK(h, tile_fetch_log(W.meta + (size_t)g * h->cfg.max_attempts, fin.n_att, GR.log[g].data()));
        if (nfe_out_host) nfe_out_host[g] = 3 + 6 * (int64_t)fin.n_att;
        const rnde_status st = solve_verdict(fin.status).st;
        if (status_out_host) status_out_host[g] = st;
        if (st != RNDE_OK && first_bad < 0) first_bad = g;
    }
    if (first_bad >= 0) {
        const int cs = GR.sw.h_fin[first_bad].status;
        h->err = group_failure(first_bad, cs);
        return solve_verdict(cs).st;
    }
    if (sum_dev) {                   // behind the final states, and only when every group ended well: a failed call adds nothing
        hipLaunchKernelGGL(rnde_group_sum_kernel, dim3(1), dim3(256), 0, s, (const float*)logpx_dev, plan.cols, sum_dev, (long long*)count_dev);
        FCHK(h, hipGetLastError());
    }
    return RNDE_OK;
}

extern "C" rnde_status rnde_ffjord_group_steps(rnde_ffjord* h, int32_t g, float* steps_host, int32_t capacity, int32_t* n_attempts_out) {
    if (!h || !n_attempts_out) return RNDE_ERR_BAD_ARG;
    if (!h->gr || g < 0 || g >= (int)h->gr->log.size()) {
        h->err = "group_steps: g must be a group of the last group call on this handle";
        return RNDE_ERR_BAD_ARG;
    }
    const std::vector<StepMeta>& log = h->gr->log[g];
    return ff_export(h, "group_steps", log.data(), (int)log.size(), false, steps_host, capacity, n_attempts_out);
}

extern "C" rnde_status rnde_ffjord_timing(rnde_ffjord* h, float* solve_ms, float* reverse_ms, int32_t* attempts, int32_t* accepted) {
    if (!h) return RNDE_ERR_BAD_ARG;
    if (solve_ms) *solve_ms = h->fwd_ms;
    if (reverse_ms) *reverse_ms = h->rev_ms;
    if (attempts) *attempts = h->n_att;
    if (accepted) *accepted = h->n_acc;
    return RNDE_OK;
}
