// rnde_node.h -- what the translation units of the C ABI over the ODE engines share: the handle, the allocation and error-check macros and the
// helpers one side offers the other (rnde.hip: creation, forward solves, debug / bench entry points; rnde_reverse.hip: the reverse passes, the
// classifier head and the optimiser steps).  Not an interface: include/rnde.h is.
#pragma once
#include "../../include/rnde.h"
// The device allocations of the translation units that include this header (rnde.hip, rnde_reverse.hip, rnde_node_tile.hip) go through
// rnde_alloc.h's wrapper (RNDE_POISON), first among the project headers; the other allocating units (rnde_ffjord.hip, rnde_sde.hip,
// rnde_latent.hip, rnde_comm.hip) include that header themselves.  MeetRes::create (rnde_meet.h) stays outside the fill on purpose (it is
// counted like the rest).  The same header has the owning types the handle's members are made of.
#include "rnde_alloc.h"
#include "rnde_fwd.h"
#include "rnde_bwd.h"
#include "rnde_stage.h"
#include "rnde_bstage.h"
#include "rnde_stage_persist2.h"
#include "rnde_bstage_persist.h"
#include "rnde_solve_sync.h"
#include "rnde_meet.h"
#include "rnde_binit_stage.h"
#include "rnde_head.h"
#include "rnde_chain.h"
#include "rk_tables.h"
#include "rnde_bchain.h"
#include "rnde_chainmw.h"
#include "rnde_bchainmw.h"
#include "rnde_rev_plan.h"
#include "rnde_probe.h"

#include <chrono>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>


// rnde_stage_solve.hip (its own translation unit, parameter blocks by address: the same struct definitions on both sides)
extern "C" hipError_t rnde_launch_stage_solve(const void* stage_params, const void* persist_sync, const void* solve_sync, int act2, int x3, hipStream_t s);
extern "C" hipError_t rnde_launch_x3_pack(const float* p, void* x3B, void* x3D, void* x3Bt, void* x3Dt, int D, int H, int MT, int WT, int R, int HT, hipStream_t s);
using namespace rnde;

struct rnde_node {
    rnde_node_config cfg{};
    int D = 0, H = 0, P = 0, BT = 8, act2 = 1;
    int Bpad_max = 0, nwg_max = 0;
    // stage engine (rnde_stage.h)
    // Owners (rnde_alloc.h): every allocated member is a DevBuf / PinBuf / Event / Stream and goes with the handle; a member that points into
    // another allocation is a raw pointer marked "view", and nothing is freed through it.  The stream and the events come first: members go
    // in reverse order, the buffers before them.
    Stream wstream;                       // (experimental overlap path of the weight-gradient GEMMs)
    Event wevents[66];
    Event tev[5];                         // rnde_node_set_timing: around the attempt loop of the forward, the reverse sweep and the rest of the reverse pass
    Event ev_host;                        // rnde_node_classifier_grad: what the forward's host wait uses
    int engine = 0;                       // set at creation: 2 stage kernels, 3 chain engine (rnde_chain.h), 4 tiled engine (rnde_node_tile.h)
    struct rnde_node_tiled* tiled = nullptr;   // engine 4: everything of that engine (rnde_node_tile.hip); the fields below it uses are cfg, D, P, h_meta, n_att, B, have_tape, err
    ChainGeo cg{}; DevBuf<float> cfrags; int NKD = 0, chain_alt = 0;
    int chain_ga = 0;             // a layer's activation is other than identity / tanh: the kernel variants that serve every rnde_act (ALT / LAT = 2)
    size_t chain_lds_f = 0, chain_lds_b = 0;
    // multi-wave kernels of the chain engine (rnde_chainmw.h): 4 waves per 16 columns, activations taped in the slab by the forward
    rnde_comm* couple = nullptr; int couple_batch = 0, couple_world = 1;   // SURVEY 8e mode 2 (rnde_node_set_coupling)
    int rk_tab = 0; RkTab rk{};   // explicit RK pair as data: 1 = a 7-stage pair (DP5, or Tsit5 through the same path when RNDE_CHAIN_TAB=1), 2 = S stages (DOP853)
    // chain engine, multi-wave kernels: the whole adaptive solve as ONE launch (rnde_chainmw.h MW_SOLVE) while the tiles fit one XCD (<= 32)
    int mw_clean = 0, mw_retry_after = 8;   // non-sticky fallback of those kernels, as persist_clean / persist_retry_after of the stage engine
    int mw_solve = 1; MeetRes mw_meet;   // the meeting place of both one-launch kernels (rnde_meet.h); its XCD slot moves on after a failure
    int mw_bsweep = 1; DevBuf<int> mw_bargs; PinBuf<int> h_mw_bargs; PinBuf<unsigned> h_mw_bchk; bool pending_bsweep = false; int bsweep_nt = 0; bool bsweep_global = false;   // (the pending sweep's OWN check words, tile count and meeting kind: a later forward may overwrite h->B and the meeting's own check buffer before the verdict is read)
      // the reverse sweep as one launch (rnde_bchainmw.h SWEEP): per-attempt arguments [sv_lo | sv_hi | eig_c], check words
    int rk_S = 7, rk_order = 5;   // stages of the pair in first-same-as-last form (evaluations per attempted step = rk_S - 1), controller order
    int mw_lat = 0;               // the reference's latent-ODE shape (20 <-> 50, 8 layers): forward kernels with register-stationary weights
    int mw = 0; MwGeo mg{}; DevBuf<float> mw_tab; DevBuf<float> mw_slab; long long mw_slab_evals = 0; size_t mw_lds_f = 0, mw_lds_b = 0;
    DevBuf<float> cslab; DevBuf<float> ev_t; PinBuf<float> h_ev_t;   // chain reverse: (H, Z) dump, evaluation times
    int sMT = 0, sWT = 0, sR = 0, sHT = 0, sK2b = 0, sKHb = 0;
    DevBuf<f32x4> spwB, spwD, spwBt, spwDt;
    DevBuf<float> slab2;
    size_t stage_lds = 0;
    DevBuf<float> head_ws;   // fused classifier head scratch
    // rnde_node_classifier_grad: work the forward enqueues BEHIND the copy its host wait needs (so it runs while the host wakes up),
    // (the event that wait uses: ev_host above), the caller-independent buffers of the fused step, and "the reverse sweep's weight packs are already queued"
    std::function<rnde_status(hipStream_t)> after_solve; bool rev_packed = false;
    DevBuf<float> cg_ws; std::vector<float> cg_sv;
    DevBuf<float> sv_t_dev; std::vector<float> saveat;   // saveat times of the last forward
    DevBuf<float> replay_dev; const float* replay_host = nullptr; int n_replay = 0;   // rnde_node_forward_replay (set for one forward)
    std::vector<float> replay_armed;   // rnde_debug_arm_replay: the sequence the next rnde_node_forward_saveat runs along (then cleared)
    // persistent attempt kernel (rnde_stage_persist.h): 1 = in use, 0 = off (RNDE_PERSIST=0), -1 = disabled after a failure
    int wgrad_side_pct = 30, stage_generic = 0;
    int persist_clean = 0, persist_retry_after = 8, persist_fallbacks = 0;   // non-sticky fallback: clean multi-launch solves since the last failure, when to try again   // fixed at creation (config fields; RNDE_* environment overrides are read once, there)
    int persist2 = -1;   // two column tiles per workgroup in the forward attempt kernel: -1 automatic (by tile count), 0 never, 1 whenever possible (RNDE_PERSIST2, read at creation)
    int persist = 0, persist_spins = kPersistMaxSpins; int tslab_Bpad = -1; size_t tslab_bytes = 0; DevBuf<float> tslab; unsigned *pabort = nullptr, *pxcc = nullptr; unsigned* h_pchk = nullptr;   // pabort, pxcc: views into mbox; h_pchk: view into h_mbox
    // the whole forward solve as one launch (rnde_stage_solve.h): 1 = use it where it applies, 0 = off (RNDE_STAGE_SOLVE=0 at creation); meeting granules and the epoch of their tags
    // (the abort word and the XCC ids of that kernel are PersistSync's)
    long long tail_folds[4] = {0, 0, 0, 0};      // launches that took a folded form (rnde_node_tail_folds: reduce fold, weight-gradient pair, x3 pack fold, binit pairs)
    int stage_solve = 1; MeetRes s_meet; int one_launch_solves = 0;
    // the one-launch solve's Dense layers on the matrix cores (rnde_x3.h): 1 = on (RNDE_X3 at creation / rnde_node_set_matrix_mode), split weight images, "packed for the current p"
    int x3 = 0; DevBuf<unsigned char> x3B, x3D, x3Bt, x3Dt; bool x3_packed = false, x3_fwd = false;      // x3_fwd: this forward's stage kernels run with x3 (weights split by its pack launch); x3_packed: the last forward ran the x3 solve, the four images hold ITS parameters (the reverse pass may use the transposed pair)
    // device
    DevBuf<float> f0, h0, u1, f1, h1, arena;      // arena: arena.cap() / rec_stride records
    DevBuf<float> xcopy;     // private copy of x (the tape must not alias caller memory)
    long long rec_stride = 0;
    DevBuf<float> pcopy;
    DevBuf<StepState> ctl;
    DevBuf<unsigned char> mbox; PinBuf<unsigned char> h_mbox; size_t mbox_meta_off = 0;   // stage engine: everything the host reads per chunk, contiguous (one copy)
    // Views.  Stage engine: into mbox / h_mbox.  Chain and tiled engines: onto the own_* allocations below, which no other code names.
    StepState* ctl_final = nullptr;
    StepMeta* meta = nullptr;
    InitRec* initrec = nullptr;
    StepState* h_ctl = nullptr;
    StepMeta* h_meta = nullptr;
    InitRec* h_init = nullptr;
    DevBuf<StepState> own_ctl_final; DevBuf<StepMeta> own_meta; DevBuf<InitRec> own_initrec;
    PinBuf<StepState> own_h_ctl; PinBuf<StepMeta> own_h_meta; PinBuf<InitRec> own_h_init;
    DevBuf<float> errpart, initpart;
    BwdBuffers bw;
    PinBuf<float> h_scal;    // pinned host
    // last forward
    int B = 0, Bpad = 0, nwg = 0, n_att = 0, predicted = 0;
    float t0 = 0, t1 = 0;
    bool have_tape = false;
    bool pending_bwd = false;
    DevBuf<float> diag_buf;   // (RNDE_DIAG builds) cycle stamps   // an asynchronous reverse pass whose health words have not been looked at yet
    std::vector<int> sv_index;  // per attempt: index into saveval or -1
    int n_saveval = 0;
    int timing = 0; bool tev_fwd = false, tev_bwd = false;
    std::string err;
};

#define HIPCHK(h, call)                                                                              \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess) {                                                                     \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e__);                           \
            return RNDE_ERR_HIP;                                                                     \
        }                                                                                            \
    } while (0)

// ---- rnde_node_tile.hip: the tiled engine (engine 4) behind the public entries of rnde.hip / rnde_reverse.hip ----
void rnde_set_create_error(const std::string& msg);      // (rnde.hip: what rnde_last_error(NULL) returns on this thread)
void node_tiled_destroy(rnde_node* h);
rnde_status node_tiled_forward(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1, float* u_out_dev,
                               const float* saveat_host, int32_t n_saveat, float* sv_out_dev, int64_t* nfe_out, float* saveval_host,
                               int32_t* n_saveval_out, int32_t keep_tape, void* stream);
rnde_status node_tiled_backward(rnde_node* h, const float* u_bar_dev, const float* saveval_bar_host, float* x_bar_dev, float* p_bar_dev,
                                float* tspan_bar_host, void* stream);
rnde_status node_tiled_feval(rnde_node* h, const float* u_dev, const float* p_dev, int32_t B, float t, float* out_dev, void* stream);
rnde_status node_tiled_timing(rnde_node* h, float* fwd_ms, float* rev_sweep_ms, float* rev_rest_ms);
// an entry the tiled engine does not serve: the message names the entry and the alternative
#define RNDE_TILED_REFUSE(h, what)                                                                                                       \
    do {                                                                                                                                 \
        if ((h) && (h)->engine == 4) {                                                                                                   \
            (h)->err = std::string("TrackedNeuralODE tiled engine: ") + what;                                                            \
            return RNDE_ERR_BAD_ARG;                                                                                                     \
        }                                                                                                                                \
    } while (0)

// ---- handle -> kernel instantiation, stated once per kernel family: the forward (rnde.hip) and the reverse (rnde_reverse.hip) of one handle launch
// the same variant.  f is a generic lambda; it receives the template arguments as std::integral_constant values and is instantiated for the
// combinations listed here and no other.
template <int V> using IC = std::integral_constant<int, V>;
// one-wave chain kernels (rnde_chain.h, rnde_bchain.h): f(NKD, ALT); ALT 2 serves every rnde_act, ALT 1 is the compile-time latent-ODE shape
template <class F>
static auto chain_variant(const rnde_node* h, F&& f) {
    if (h->chain_ga) switch (h->NKD) {
        case 4: return f(IC<4>{}, IC<2>{});
        case 8: return f(IC<8>{}, IC<2>{});
        default: return f(IC<16>{}, IC<2>{});
    }
    switch (h->NKD) {
        case 4: return f(IC<4>{}, IC<0>{});
        case 8: return h->chain_alt ? f(IC<8>{}, IC<1>{}) : f(IC<8>{}, IC<0>{});
        default: return f(IC<16>{}, IC<0>{});
    }
}
// multi-wave chain kernels (rnde_chainmw.h, rnde_bchainmw.h): f(NR, TAB, LAT); TAB 0 constant-folded Tsit5, 1 a 7-stage table, 2 an S-stage table;
// LAT 2 serves every rnde_act, LAT 1 is the latent-ODE shape with register-stationary weights (NR 2, 7-stage pairs only)
template <class F>
static auto mw_variant(const rnde_node* h, F&& f) {
    auto by_nr = [&](auto tab, auto lat) {
        switch (h->NKD) {
            case 4: return f(IC<1>{}, tab, lat);
            case 8: return f(IC<2>{}, tab, lat);
            default: return f(IC<4>{}, tab, lat);
        }
    };
    auto by_tab = [&](auto lat) { return h->rk_tab == 2 ? by_nr(IC<2>{}, lat) : (h->rk_tab ? by_nr(IC<1>{}, lat) : by_nr(IC<0>{}, lat)); };
    if (h->chain_ga) return by_tab(IC<2>{});
    if (h->rk_tab != 2 && h->mw_lat) return h->rk_tab ? f(IC<2>{}, IC<1>{}, IC<1>{}) : f(IC<2>{}, IC<0>{}, IC<1>{});
    return by_tab(IC<0>{});
}

// the headline geometry ([784, 100, 784] as 7 row blocks of 7 waves, 7 hidden tiles, 7 k-blocks) the fixed-shape stage kernels, forward and reverse, are
// compiled for; Kb: the k-blocks of the side in question (StageParams::K2b forward, BwdStageParams::KHb reverse)
static inline bool stage_fix(const rnde_node* h, int WT, int HT, int Kb, int MT, int R) { return WT == 7 && HT == 7 && Kb == 7 && MT == 49 && R == 7 && h->D == 784 && h->H == 100 && !h->stage_generic; }
static const rnde_status RNDE_INTERNAL_RETRY = static_cast<rnde_status>(100);
// The launches around the two sweeps that are folded into a neighbour, one host switch each, read per call like RNDE_SOLVE_FOLD (tests and A/B
// runs flip them inside one process; 0 = off, anything else = on): RNDE_REDUCE_FOLD (the two passes of the weight-gradient reduction as one launch),
// RNDE_WGRAD_PAIR (both layers' full-width weight-gradient launches as one), RNDE_BINIT_PAIR (the reverse of the initial-step rule as two paired launches)
// -- on unless set to 0 -- and RNDE_X3_PACK_FOLD (the x3 weight split inside the pack launch), off unless set: its own A/B did not separate from the
// run-to-run spread.  Every one of them leaves the results bit for bit what they were.
static inline bool tail_switch(const char* name, bool by_default = true) { const char* e = getenv(name); return e ? e[0] != '0' : by_default; }
// ---- rnde.hip, used by rnde_reverse.hip ----
StepParams make_params(rnde_node* h, const float* x, int B, float t0, float t1, int tape);
MwParams make_mw_params(rnde_node* h, const StepParams& P);
ChainParams make_chain_params(rnde_node* h, const StepParams& P);
rnde_status couple_sum(rnde_node* h, float* partials, long long count, hipStream_t s);
hipError_t stage_pack(rnde_node* h, const float* p, f32x4* dst, int which, int MTrows, int Kb, hipStream_t st);
rnde_status stage_pack_all(rnde_node* h, const float* p_dev, hipStream_t s, const float* x_src = nullptr, long long x_floats = 0);
hipError_t slab_prepare(rnde_node* h, int Bpad, hipStream_t s);
void persist_check_enqueue(rnde_node* h, int grid, hipStream_t s);
bool persist_check_result(rnde_node* h, int C, int R, hipStream_t s);
bool bsweep_failed(rnde_node* h, hipStream_t s);
rnde_status forward_impl(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1,
                         float* u_out_dev, const float* saveat_host, int32_t n_saveat, float* sv_out_dev,
                         int64_t* nfe_out, float* saveval_host, int32_t* n_saveval_out, int32_t keep_tape, void* stream);
