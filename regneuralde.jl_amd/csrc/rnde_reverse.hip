// rnde_reverse.hip -- C ABI (include/rnde.h), the reverse side: discretise-then-optimise reverse passes of the three ODE engines, the weight-gradient
// GEMMs, the classifier head and its fused training step, the optimiser steps.  The handle and what rnde.hip offers this file: rnde_node.h.
#include "rnde_node.h"
#include "rnde_wgradx.h"
#include "rnde_head_eval.h"

static rnde_status chain_bwd_run(rnde_node* h, const float* u_bar_dev, const float* saveval_bar_host, float* x_bar_dev,
                                 float* p_bar_dev, float* tspan_bar_host, hipStream_t s, bool sync = true, float* tspan_bar_dev = nullptr);
static rnde_status bwd_run(rnde_node* h, const float* u_bar_dev, const float* saveval_bar_host, float* x_bar_dev,
                           float* p_bar_dev, float* tspan_bar_host, hipStream_t s, bool sync = true, float* tspan_bar_dev = nullptr);


extern "C" rnde_status rnde_node_backward_async(rnde_node* h, const float* u_bar_dev, const float* saveval_bar_host, float* x_bar_dev,
                                                float* p_bar_dev, float* tspan_bar_dev, void* stream) {
    if (!h) return RNDE_ERR_BAD_ARG;
    RNDE_TILED_REFUSE(h, "rnde_node_backward_async is not served (rnde_node_backward runs its reverse sweep and waits for it)");
    if (!h->have_tape) { h->err = "no recorded forward"; return RNDE_ERR_NO_TAPE; }
    if (h->engine == 3) return chain_bwd_run(h, u_bar_dev, saveval_bar_host, x_bar_dev, p_bar_dev, nullptr, (hipStream_t)stream, false, tspan_bar_dev);
    return bwd_run(h, u_bar_dev, saveval_bar_host, x_bar_dev, p_bar_dev, nullptr, (hipStream_t)stream, false, tspan_bar_dev);
}

extern "C" rnde_status rnde_node_backward(rnde_node* h, const float* u_bar_dev, const float* saveval_bar_host,
                                          float* x_bar_dev, float* p_bar_dev, float* tspan_bar_host, void* stream) {
    if (!h) return RNDE_ERR_BAD_ARG;
    if (!h->have_tape) { h->err = "no recorded forward"; return RNDE_ERR_NO_TAPE; }
    if (h->engine == 4) return node_tiled_backward(h, u_bar_dev, saveval_bar_host, x_bar_dev, p_bar_dev, tspan_bar_host, stream);
    if (h->engine == 3) return chain_bwd_run(h, u_bar_dev, saveval_bar_host, x_bar_dev, p_bar_dev, tspan_bar_host, (hipStream_t)stream);
    return bwd_run(h, u_bar_dev, saveval_bar_host, x_bar_dev, p_bar_dev, tspan_bar_host, (hipStream_t)stream);
}
extern "C" rnde_status rnde_node_backward_host(rnde_node* h, const float* u_bar, const float* saveval_bar, float* x_bar,
                                               float* p_bar, float* tspan_bar) {
    if (!h) return RNDE_ERR_BAD_ARG;
    DevBuf<float> ub, xb, pb;
    const size_t nb = (size_t)h->D * h->B * 4;
    HIPCHK(h, ub.alloc(nb / 4)); HIPCHK(h, xb.alloc(nb / 4)); HIPCHK(h, pb.alloc((size_t)h->P));
    HIPCHK(h, hipMemcpy(ub, u_bar, nb, hipMemcpyHostToDevice));
    rnde_status st = rnde_node_backward(h, ub, saveval_bar, xb, pb, tspan_bar, nullptr);
    if (st == RNDE_OK) { hipMemcpy(x_bar, xb, nb, hipMemcpyDeviceToHost); hipMemcpy(p_bar, pb, (size_t)h->P * 4, hipMemcpyDeviceToHost); }
    return st;
}

// ---- reverse pass driver ------------------------------------------------------------------------
static rnde_status bwd_prepare(rnde_node* h) {
    BwdBuffers& b = h->bw;
    if (b.ready) return RNDE_OK;
    const size_t A = (size_t)h->D * h->Bpad_max, HB = (size_t)h->H * h->Bpad_max;
    const int cap = h->cfg.max_attempts;
    // (reserve: a call that failed half way is simply made again)
    HIPCHK(h, b.U.reserve(A)); HIPCHK(h, b.K1.reserve(A)); HIPCHK(h, b.UB1.reserve(A));
    HIPCHK(h, b.zi2.reserve(2 * A)); HIPCHK(h, b.zi1.reserve(2 * HB));
    HIPCHK(h, b.svb_att.reserve((size_t)cap));
    HIPCHK(h, b.bstate_mem.reserve(2 * sizeof(BState) + 64)); b.bstate = (BState*)b.bstate_mem.get(); HIPCHK(h, b.ibstate.reserve(2));      // (+ 64 bytes: the [2][4] sums of rnde_bpart_reduce_kernel)
    HIPCHK(h, b.bpart.reserve((size_t)(2 * h->nwg_max + 256) * 4)); HIPCHK(h, b.ipart.reserve((size_t)2 * h->nwg_max * 4));   // (+256 entries: finish_attempt_scalars reads whole 256-entry blocks)
    HIPCHK(h, b.tspan_out.reserve(2));
    const size_t nev = (size_t)6 * cap + 2;
    // (ev1 / h_ev1 are sized for [ev1 | ev2 | svb] back to back: bwd_run lays the three out contiguously and sends them in ONE copy)
    const size_t desc_blob = 2 * nev * sizeof(EvalDesc) + (size_t)cap * 4 + 64;
    HIPCHK(h, b.ev1_mem.reserve(desc_blob)); b.ev1 = (EvalDesc*)b.ev1_mem.get(); HIPCHK(h, b.ev2.reserve(nev));
    HIPCHK(h, b.h_ev1_mem.reserve(desc_blob)); b.h_ev1 = (EvalDesc*)b.h_ev1_mem.get(); HIPCHK(h, b.h_ev2.reserve(nev));
    HIPCHK(h, b.h_svb.reserve((size_t)cap));
    const size_t seg = std::max((size_t)h->H * (h->D + 2), (size_t)h->D * (h->H + 2));
    b.slab_floats = seg * 256;              // per layer; two layers back to back
    HIPCHK(h, b.slab.reserve(2 * b.slab_floats));
    HIPCHK(h, b.slab_r.reserve(2 * 16 * seg));      // second-level partials, one region per layer
    if (!h->wstream) {
        int prio_least = 0, prio_greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
        HIPCHK(h, hipStreamCreateWithPriority(&h->wstream.s, hipStreamNonBlocking, prio_least));   // never ahead of the sweep
        for (auto& e : h->wevents) HIPCHK(h, e.create(hipEventDisableTiming));
    }
    HIPCHK(h, b.UTB.reserve(A)); HIPCHK(h, b.UNB.reserve(A)); HIPCHK(h, b.UPB0.reserve(A));
    HIPCHK(h, b.GB.reserve(15 * A));   // gbar_1..6, EXK, EXG (stiffness extras), W_1..7 (saveat)
    b.ready = true;
    return RNDE_OK;
}

static bool wgrad3_ok(int M, int Nx) {
    const bool tall = M >= Nx;
    const int wide = tall ? M : Nx + 2, narrow = tall ? Nx + 2 : M;
    return getenv("RNDE_WGRAD_LEGACY") == nullptr && getenv("RNDE_WGRAD_V2") == nullptr && M % 4 == 0 && Nx % 4 == 0 && wide > 656 &&
           wide <= 800 && narrow <= 112;
}
// Does the quarter form of the bf16x3 weight-gradient kernel (rnde_wgrad4x_kernel) serve this launch, and with which chunks (steps per chunk, number of chunks)
// and operand feed?  One place for launch_wgrad_part and launch_wgrad_pair: the chunks fix the summation order.
struct Wx4Plan { bool ok; int spc4, sc4, feed; };
static Wx4Plan wgrad4_plan(const rnde_node* h, int n_evals, int M, int Nx, int Bpad, int max_chunks) {
    Wx4Plan q{false, 0, 0, 0};
    if (n_evals <= 0 || !wgrad3_ok(M, Nx)) return q;
    const bool tall = M >= Nx;
    const int total_steps = n_evals * ((Bpad + 31) / 32);
    // matrix mode 1 in effect for this step (the forward ran the x3 solve): the GEMMs on the matrix cores too (rnde_wgradx.h; RNDE_X3_WGRAD_OFF=1: A/B)
    const bool x3_off = getenv("RNDE_X3_WGRAD_OFF") != nullptr;            // (read per call: A/B runs and tests switch inside one process)
    const bool x3_half = getenv("RNDE_X3_WGRAD_HALF") != nullptr;         // (A/B: the single-buffered half form)
    const int TT4 = ((tall ? M : Nx + 2) + 15) / 16;
    if (!(h->x3_packed && !x3_off && !x3_half && TT4 >= 28 && TT4 <= 52)) return q;
    static const int target4 = getenv("RNDE_WGRAD4_CHUNKS") ? atoi(getenv("RNDE_WGRAD4_CHUNKS")) : 64;
    int sc4 = std::max(1, std::min({max_chunks > 0 ? max_chunks / 2 : target4, total_steps, 256}));
    const int spc4 = (total_steps + sc4 - 1) / sc4;
    sc4 = (total_steps + spc4 - 1) / spc4;
#if RNDE_WX4_ABL == 7 || RNDE_WX4_ABL == 8      // (these two timing ablations exist in the first form only: such a build always launches it)
    const bool q0 = true;
#else
    // which operand feed (rnde_wgradx.h; same chunks, same bits), read per call for A/B runs and tests: RNDE_X3_WGRAD_Q0=1 the quarter form as first built
    // (FEED 0), RNDE_X3_WGRAD_FEED=1 the coalesced, unrepeated feed (FEED 1); neither set: kWx4DefaultFeed
    const char* ef = getenv("RNDE_X3_WGRAD_FEED");
    const bool q0 = getenv("RNDE_X3_WGRAD_Q0") != nullptr || (ef ? ef[0] == '0' : kWx4DefaultFeed == 0);
#endif
    q.ok = true; q.spc4 = spc4; q.sc4 = sc4; q.feed = q0 ? 0 : 1;
    return q;
}
// The instantiations of one kernel template share a signature: each launch below picks its kernel as a function pointer from a small table.
using WgradKern = decltype(&rnde_wgrad3_kernel<true>);      // (rnde_wgrad_kernel, rnde_wgrad2_kernel, rnde_wgrad3_kernel, rnde_wgrad3x_kernel)
// `max_chunks` > 0 caps the number of chunks (two workgroups each) of the 16x16x4 kernel: 16 for the launches that run
// underneath the sweep on the CUs it leaves idle, see bwd_run
static rnde_status launch_wgrad_part(rnde_node* h, const EvalDesc* ev, int n_evals, int per_chunk, int M, int Nx, int Bpad,
                                     float* slab, int* chunk_cursor, hipStream_t s, int max_chunks = 0) {
    if (n_evals <= 0) return RNDE_OK;
    const int mtiles = (M + 31) / 32, ntiles = (Nx + 2 + 31) / 32;
    const bool tall = M >= Nx;  // layer 2: M = D; layer 1: M = H
    const int MB = tall ? 2 : 4, NB = tall ? 4 : 2;
    const int blocks = ((mtiles + MB - 1) / MB) * ((ntiles + NB - 1) / NB);
    const long long len = (long long)M * (Nx + 2);
    const int chunks = (n_evals + per_chunk - 1) / per_chunk;      // (chunking of the direct-from-global kernels only; checked where they are launched)
    float* dst = slab + (size_t)(*chunk_cursor) * len;
    static const bool legacy = getenv("RNDE_WGRAD_LEGACY") != nullptr;   // direct-from-global variant, kept for A/B runs
    const bool fits = tall ? (Nx + 2 <= 128) : (M <= 128);                // the staged kernel covers 128 on the un-split side
    if (wgrad3_ok(M, Nx)) {                                               // (RNDE_WGRAD_V2, read per call, keeps the 32x32x2 staged kernel: A/B)
        // 16x16x4 kernel: two workgroups (the halves of the wide side) per chunk of 32-column steps
        const int total_steps = n_evals * ((Bpad + 31) / 32);
        static const int target_chunks = getenv("RNDE_WGRAD3_CHUNKS") ? atoi(getenv("RNDE_WGRAD3_CHUNKS")) : 128;
        int sc = std::max(1, std::min({max_chunks > 0 ? max_chunks : target_chunks, total_steps, 256}));
        const int steps_per_chunk = (total_steps + sc - 1) / sc;
        sc = (total_steps + steps_per_chunk - 1) / steps_per_chunk;
        if ((size_t)(*chunk_cursor + sc) * (size_t)len > h->bw.slab_floats) { h->err = "weight-gradient slab overflow"; return RNDE_ERR_BAD_ARG; }
        // matrix mode 1 in effect for this step (the forward ran the x3 solve): the GEMMs on the matrix cores too (rnde_wgradx.h; RNDE_X3_WGRAD_OFF=1: A/B)
        const bool x3_off = getenv("RNDE_X3_WGRAD_OFF") != nullptr;            // (read per call: A/B runs and tests switch inside one process)
        const Wx4Plan q4 = wgrad4_plan(h, n_evals, M, Nx, Bpad, max_chunks);
        if (q4.ok) {
            // quarter form (rnde_wgrad4x_kernel): four workgroups per chunk, two LDS images; the launches underneath the sweep stay at 32 workgroups (8 chunks)
            const int sc4 = q4.sc4, spc4 = q4.spc4, feed = q4.feed;
            if ((size_t)(*chunk_cursor + sc4) * (size_t)len > h->bw.slab_floats) { h->err = "weight-gradient slab overflow"; return RNDE_ERR_BAD_ARG; }
            static constexpr decltype(&rnde_wgrad4x_kernel<true, 0>) kern4[2][2] = {{rnde_wgrad4x_kernel<false, 0>, rnde_wgrad4x_kernel<false, 1>},
                                                                                    {rnde_wgrad4x_kernel<true, 0>, rnde_wgrad4x_kernel<true, 1>}};      // [tall][FEED]
            static constexpr size_t lds4[2] = {kWx4LdsBytes, kWx4fLdsBytes};                                                                       // [FEED]
            static DeviceOnce attr4;
            if (attr4.need()) {
                for (int t = 0; t < 2; ++t)
                    for (int f = 0; f < 2; ++f) HIPCHK(h, hipFuncSetAttribute((const void*)kern4[t][f], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds4[f]));
                attr4.done();
            }
            const dim3 g4(32 * ((sc4 + 7) / 8));
            hipLaunchKernelGGL(kern4[tall][feed], g4, dim3(448), lds4[feed], s, ev, n_evals, spc4, sc4, M, Nx, Bpad, dst);
            HIPCHK(h, hipGetLastError());
            *chunk_cursor += sc4;
            return RNDE_OK;
        }
        // the 16x16x4 kernel proper, bf16x3 (rnde_wgradx.h) or fp32 inputs (rnde_bwd.h): [x3][tall]
        static constexpr WgradKern kern3[2][2] = {{rnde_wgrad3_kernel<false>, rnde_wgrad3_kernel<true>}, {rnde_wgrad3x_kernel<false>, rnde_wgrad3x_kernel<true>}};
        static constexpr size_t lds3[2] = {(size_t)2 * 32 * (464 + 144) * sizeof(float) /* two buffers */, kWxLdsBytes};
        static DeviceOnce attr3[2];
        const int x3 = (h->x3_packed && !x3_off) ? 1 : 0;
        if (attr3[x3].need()) {
            for (int t = 0; t < 2; ++t) HIPCHK(h, hipFuncSetAttribute((const void*)kern3[x3][t], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3[x3]));
            attr3[x3].done();
        }
        hipLaunchKernelGGL(kern3[x3][tall], dim3(2, sc), dim3(448), lds3[x3], s, ev, n_evals, steps_per_chunk, M, Nx, Bpad, dst);
        HIPCHK(h, hipGetLastError());
        *chunk_cursor += sc;
        return RNDE_OK;
    }
    if (!legacy && fits) {
        // staged kernel: chunks are ranges of 32-column steps; pick the count that fills the chip in whole rounds
        // (3 workgroups per CU -> 768 resident: one round; measured 768 / 1100 / 1536 / 1792 -> 4.44 / 4.57 / 4.51 / 4.54 ms per step)
        const int pblocks = tall ? (M + 127) / 128 : (Nx + 2 + 127) / 128;
        const int total_steps = n_evals * ((Bpad + 31) / 32);
        static const int target_wgs = getenv("RNDE_WGRAD_WGS") ? atoi(getenv("RNDE_WGRAD_WGS")) : 768;
        int sc = std::max(1, std::min({target_wgs / pblocks, total_steps, 256}));
        const int steps_per_chunk = (total_steps + sc - 1) / sc;
        sc = (total_steps + steps_per_chunk - 1) / steps_per_chunk;
        if ((size_t)(*chunk_cursor + sc) * (size_t)len > h->bw.slab_floats) { h->err = "weight-gradient slab overflow"; return RNDE_ERR_BAD_ARG; }
        static constexpr WgradKern kern2[2] = {rnde_wgrad2_kernel<false>, rnde_wgrad2_kernel<true>};      // [tall]
        hipLaunchKernelGGL(kern2[tall], dim3(pblocks, sc), dim3(256), 0, s, ev, n_evals, steps_per_chunk, M, Nx, Bpad, dst);
        HIPCHK(h, hipGetLastError());
        *chunk_cursor += sc;
        return RNDE_OK;
    } else {
        // (this check used to sit in front of ALL paths with the direct kernels' chunk count -- up to 240 -- and refused solves of more than ~65
        //  attempts on the 16x16x4 path, which needs 127 chunks behind the sweep: "slab overflow" in a training run whose step count had grown)
        if ((size_t)(*chunk_cursor + chunks) * (size_t)len > h->bw.slab_floats) { h->err = "weight-gradient slab overflow"; return RNDE_ERR_BAD_ARG; }
        static constexpr WgradKern kern[2] = {rnde_wgrad_kernel<4, 2>, rnde_wgrad_kernel<2, 4>};      // [tall]: <MB, NB>
        hipLaunchKernelGGL(kern[tall], dim3(blocks, chunks), dim3(64), 0, s, ev, n_evals, per_chunk, M, Nx, Bpad, dst);
    }
    HIPCHK(h, hipGetLastError());
    *chunk_cursor += chunks;
    return RNDE_OK;
}
// The full-width launches behind the sweep, layer 1 then layer 2, over the same evaluations.  Where both are the quarter form with FEED 1 they go out as ONE launch
// (rnde_wgrad4x_pair_kernel: the two grids back to back; host switch RNDE_WGRAD_PAIR, read per call): each layer's chunk table, steps per chunk, number of chunks,
// chunk-to-XCD map (a layer's grid is a multiple of 32 workgroups, so the second layer's linear ids keep their id % 8) and slab positions are those of the two
// launches, which serve every other case.
static rnde_status launch_wgrad_pair(rnde_node* h, const EvalDesc* ev1, const EvalDesc* ev2, int n_evals, int per_chunk, int Bpad, float* slab1, int* cur1,
                                     float* slab2, int* cur2, hipStream_t s) {
    const int H = h->H, D = h->D;
    const Wx4Plan q1 = wgrad4_plan(h, n_evals, H, D, Bpad, 0), q2 = wgrad4_plan(h, n_evals, D, H, Bpad, 0);
    const long long len1 = (long long)H * (D + 2), len2 = (long long)D * (H + 2);
    // (launch_wgrad_part checks the slab against the 16x16x4 kernel's chunk count in front of the quarter form's own: a call it would refuse is left to it)
    const int most = std::max({q1.sc4, q2.sc4, std::min({128, n_evals * ((Bpad + 31) / 32), 256})});
    const bool fits = (size_t)(*cur1 + most) * (size_t)len1 <= h->bw.slab_floats && (size_t)(*cur2 + most) * (size_t)len2 <= h->bw.slab_floats;
    static const bool chunks_env = getenv("RNDE_WGRAD3_CHUNKS") != nullptr;      // (an A/B run that moves that count: the two launches, which read it)
    if (!(q1.ok && q2.ok && q1.feed == 1 && q2.feed == 1 && fits && !chunks_env && tail_switch("RNDE_WGRAD_PAIR"))) {
        rnde_status r = launch_wgrad_part(h, ev1, n_evals, per_chunk, H, D, Bpad, slab1, cur1, s);
        if (r != RNDE_OK) return r;
        return launch_wgrad_part(h, ev2, n_evals, per_chunk, D, H, Bpad, slab2, cur2, s);
    }
    static DeviceOnce attrp;
    if (attrp.need()) {
        HIPCHK(h, hipFuncSetAttribute((const void*)rnde_wgrad4x_pair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWx4fLdsBytes));
        attrp.done();
    }
    const Wx4Job j1{ev1, n_evals, q1.spc4, q1.sc4, H, D, slab1 + (size_t)(*cur1) * len1};
    const Wx4Job j2{ev2, n_evals, q2.spc4, q2.sc4, D, H, slab2 + (size_t)(*cur2) * len2};
    const int g1 = 32 * ((q1.sc4 + 7) / 8), g2 = 32 * ((q2.sc4 + 7) / 8);
    hipLaunchKernelGGL(rnde_wgrad4x_pair_kernel, dim3(g1 + g2), dim3(448), kWx4fLdsBytes, s, j1, j2, g1, Bpad);
    HIPCHK(h, hipGetLastError());
    *cur1 += q1.sc4; *cur2 += q2.sc4; ++h->tail_folds[1];
    return RNDE_OK;
}

// ---- what the three engines' run functions share ------------------------------------------------------------------------------------
// the saved-value cotangent per attempt into h_svb (coupled controller: every rank passes the cotangent of its own loss; the shared scalars then
// carry `world` times the single-device cotangent, like everything else -- see rnde_node_set_coupling)
static void gather_saveval_bar(rnde_node* h, const float* saveval_bar_host) {
    gather_svb(h->sv_index.data(), h->n_att, h->couple ? (float)h->couple_world : 1.f, saveval_bar_host, h->bw.h_svb);
}
// which saveat indices each attempt of the recorded solve covers (all empty without saveat)
static std::vector<SaveRange> save_ranges(const rnde_node* h) {
    std::vector<SaveRange> rng((size_t)std::max(1, h->n_att), SaveRange{0, 0});
    save_plan(h->saveat.data(), (int)h->saveat.size(), h->t0, h->h_meta, h->n_att, F_ACCEPT, rng.data());
    return rng;
}
// the parameter block every reverse kernel starts from (the stage engine replaces svb_att by its place in the one host-to-device copy)
static BwdParams fill_bwd_params(rnde_node* h, const float* u_bar_dev, float* x_bar_dev) {
    const BwdBuffers& b = h->bw;
    BwdParams Q{};
    Q.F = make_params(h, h->xcopy, h->B, h->t0, h->t1, 1);
    Q.U = b.U; Q.K1 = b.K1; Q.UB1 = b.UB1; Q.zi2 = b.zi2; Q.zi1 = b.zi1; Q.svb_att = b.svb_att;
    Q.bstate = b.bstate; Q.ibstate = b.ibstate; Q.bpart = b.bpart; Q.ipart = b.ipart;
    Q.ubar = u_bar_dev; Q.xbar = x_bar_dev; Q.tspan_out = b.tspan_out;
    Q.n_att = h->n_att; Q.track_ctrl = h->cfg.track_ctrl; Q.track_initdt = h->cfg.track_initdt; Q.reg_kind = h->cfg.regularize;
    Q.bpart_n = Q.F.nwg;
    Q.tspan_scale = h->couple ? 1.f / (float)h->couple_world : 1.f;
    Q.sv_T = (int)h->saveat.size();
    Q.sv_ubar0 = (!h->saveat.empty() && h->saveat[0] == h->t0) ? u_bar_dev : nullptr;
    return Q;
}
static rnde_status bwd_run(rnde_node* h, const float* u_bar_dev, const float* saveval_bar_host, float* x_bar_dev,
                           float* p_bar_dev, float* tspan_bar_host, hipStream_t s, bool sync, float* tspan_bar_dev) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    rnde_status st = bwd_prepare(h);
    if (st != RNDE_OK) return st;
    BwdBuffers& b = h->bw;
    int n_att = h->n_att;
    gather_saveval_bar(h, saveval_bar_host);
    // one host-to-device copy for everything the reverse pass reads from the host: [ev1 (ne) | ev2 (ne) | svb (n_att)], ne = 2 + 6 n_att
    const int ne_all = 2 + 6 * n_att;
    EvalDesc* const h_ev1 = b.h_ev1; EvalDesc* const h_ev2 = b.h_ev1 + ne_all; float* const h_svb_blob = (float*)(b.h_ev1 + 2 * (size_t)ne_all);
    EvalDesc* const d_ev1 = b.ev1;   EvalDesc* const d_ev2 = b.ev1 + ne_all;   float* const d_svb = (float*)(b.ev1 + 2 * (size_t)ne_all);
    memcpy(h_svb_blob, b.h_svb, (size_t)n_att * 4);
    BwdParams Q = fill_bwd_params(h, u_bar_dev, x_bar_dev);
    Q.svb_att = d_svb;
#ifdef RNDE_DIAG
    if (getenv("RNDE_DIAG_BWD")) { (void)h->diag_buf.reserve(2048); hipMemset(h->diag_buf, 0, 512); Q.F.dbg_out = h->diag_buf; }
#endif
    // ---- evaluation descriptors for the parameter-gradient GEMMs (all pointers are known before the sweep) ----
    const long long A = (long long)h->D * Q.F.Bpad, HB = (long long)h->H * Q.F.Bpad;
    RecLayout L{A, HB};
    // order: the two evaluations of the initial-step heuristic, then 6 per attempt -- so that "everything up to attempt n" is
    // one contiguous range for the launch that runs after the sweep
    int ne = 2;
    h_ev2[0] = EvalDesc{b.zi2, h->h0, h->t0, 0};           h_ev1[0] = EvalDesc{b.zi1, h->xcopy, h->t0, 0};
    h_ev2[1] = EvalDesc{b.zi2 + A, h->h1, h->t0 + h->h_init->dt0, 0}; h_ev1[1] = EvalDesc{b.zi1 + HB, h->u1, h->t0 + h->h_init->dt0, 0};
    for (int n = 0; n < n_att; ++n) {
        const StepMeta& m = h->h_meta[n];
        const float* R = h->arena + (long long)m.rec * h->rec_stride;
        for (int sidx = 2; sidx <= 7; ++sidx) {
            const float ts = m.t + tsC(sidx - 1) * m.dt;
            h_ev2[ne] = EvalDesc{R + L.k(sidx), R + L.h(sidx), ts, 0};
            h_ev1[ne] = EvalDesc{R + L.z1(sidx), sidx < 7 ? R + L.g(sidx) : R + L.unew(), ts, 0};
            ++ne;
        }
    }
    HIPCHK(h, hipMemcpyAsync(b.ev1, b.h_ev1, 2 * (size_t)ne * sizeof(EvalDesc) + (size_t)n_att * 4, hipMemcpyHostToDevice, s));
    float* slab1 = b.slab;
    float* slab2w = b.slab + b.slab_floats;
    int cur1 = 0, cur2 = 0, evi = 0;
    const int per_chunk = std::max(1, (ne + 239) / 240);          // (chunking of the 32x32x2 kernels; the 16x16x4 kernel chunks by steps)
    // ---- weight-gradient GEMMs underneath the sweep ----
    // The persistent reverse kernel occupies 8 * R * ceil(C / 8) CUs (224 of 256 at B = 512: one workgroup per CU, 28 per XCD)
    // and is latency bound; the 32 CUs it cannot use sit idle for the whole sweep (~1.7 ms).  A launch of 16 chunks x 2
    // workgroups of rnde_wgrad3_kernel lands 4 per XCD (round-robin dispatch) and, at 155 KB of LDS and 238 VGPRs per workgroup,
    // exactly one per CU -- it takes those idle CUs and nothing else.  So the evaluations of the attempts reversed first
    // (`side_frac` of them, in groups) go to a second stream as such 32-workgroup launches, each waiting on an event recorded
    // after its last reverse launch; the rest runs on all CUs after the sweep as before.  An earlier form of this overlap with
    // unrestricted grids was a net loss (the GEMM waves took CUs the sweep's workgroups needed: 6.4 -> 8.4..9.8 ms per step).
    const int side_pct = h->wgrad_side_pct;
    const int sweep_cus = 8 * h->sR * ((Q.F.Bpad / 16 + 7) / 8);
    const bool side = h->persist == 1 && side_pct > 0 && n_att >= 8 && sweep_cus <= 224 &&
                      wgrad3_ok(h->H, h->D) && wgrad3_ok(h->D, h->H);
    const int side_att = side ? std::min(n_att, n_att * side_pct / 100) : 0;      // attempts [n_att - side_att, n_att)
    const int group = std::max(4, (side_att + 5) / 6);                             // <= 6 side launches per layer (slab space: 16 chunks each)
    bool used_side = false;
    auto wgrad_group = [&](int lo, int hi, bool on_side) -> rnde_status {
        if (hi <= lo) return RNDE_OK;
        hipStream_t ws = s;
        if (on_side) {
            hipEvent_t ev = h->wevents[evi++ % 64];
            HIPCHK(h, hipEventRecord(ev, s));
            HIPCHK(h, hipStreamWaitEvent(h->wstream, ev, 0));
            ws = h->wstream; used_side = true;
        } else return launch_wgrad_pair(h, d_ev1 + lo, d_ev2 + lo, hi - lo, per_chunk, h->B, slab1, &cur1, slab2w, &cur2, s);      // (behind the sweep: both layers in one launch where the quarter form serves them)
        rnde_status r = launch_wgrad_part(h, d_ev1 + lo, hi - lo, per_chunk, h->H, h->D, h->B, slab1, &cur1, ws, on_side ? 16 : 0);
        if (r != RNDE_OK) return r;
        return launch_wgrad_part(h, d_ev2 + lo, hi - lo, per_chunk, h->D, h->H, h->B, slab2w, &cur2, ws, on_side ? 16 : 0);
    };
    int hi_att = n_att;                                           // evaluations of attempts >= hi_att are already launched
    hipError_t e;
    h->tev_bwd = false;
    if (h->timing) HIPCHK(h, hipEventRecord(h->tev[2], s));
    {
        // the sweep: one persistent launch per reversed attempt (fallback: 7 launches); then the kernels for the initialisation part
        if (!h->rev_packed) {
            HIPCHK(h, stage_pack(h, h->pcopy, h->spwBt, 2, h->sMT, h->sKHb, s));
            HIPCHK(h, stage_pack(h, h->pcopy, h->spwDt, 3, h->sHT, h->sMT, s));
        }
        h->rev_packed = false;
        BStageParams BQ{};
        BQ.B = Q; BQ.p = h->pcopy; BQ.pwBt = h->spwBt; BQ.pwDt = h->spwDt; BQ.slab = h->slab2; BQ.x3Bt = h->x3Bt; BQ.x3Dt = h->x3Dt;
        BQ.UTB = b.UTB; BQ.UNB = b.UNB; BQ.UPB0 = b.UPB0; BQ.GB = b.GB;
        BQ.EXK = b.GB + 6 * A; BQ.EXG = b.GB + 7 * A; BQ.SVW = b.GB + 8 * A;
        BQ.sv_t = h->saveat.empty() ? nullptr : h->sv_t_dev; BQ.sv_ubar = u_bar_dev; BQ.nsave = (int)h->saveat.size();
        BQ.MT = h->sMT; BQ.WT = h->sWT; BQ.R = h->sR; BQ.C = Q.F.Bpad / 16; BQ.HT = h->sHT; BQ.KHb = h->sKHb;
        // large batches: the partials of attempt n + 1 are summed ONCE behind its launch (rnde_bpart_reduce_kernel) instead of in the START of every
        // workgroup of attempt n -- pays from ~900 partials on (B >= 2048: a 4 us launch against 7+ us of dependent cold loads in every workgroup)
        double* const bsum = (double*)(b.bstate + 2);
        const bool pre_reduce = h->persist == 1 && Q.bpart_n >= 896 && !getenv("RNDE_NO_BPART_REDUCE");
        if (pre_reduce) BQ.B.bsum = bsum;
        const dim3 grid(BQ.R * BQ.C), blk(64 * BQ.WT);
        const std::vector<SaveRange> rng = save_ranges(h);
        const int a2 = h->act2 ? 1 : 0;
        // the instantiations of each kernel template share a signature: the kernel is a function pointer from a table, one launch statement per family
        using BAttemptKern = decltype(&rnde_bstage_attempt_kernel<0, 0>);
        static constexpr BAttemptKern kAttempt[2][2] = {{rnde_bstage_attempt_kernel<0, 0>, rnde_bstage_attempt_kernel<0, 1>},
                                                        {rnde_bstage_attempt_kernel<1, 0>, rnde_bstage_attempt_kernel<1, 1>}};      // [ACT2][FIX]
        static constexpr BAttemptKern kAttemptX3[2][4] = {      // [ACT2][EX]: the fixed geometry in matrix mode 1
            {rnde_bstage_attempt_kernel<0, 1, 1, 0>, rnde_bstage_attempt_kernel<0, 1, 1, 1>, rnde_bstage_attempt_kernel<0, 1, 1, 2>, rnde_bstage_attempt_kernel<0, 1, 1, 3>},
            {rnde_bstage_attempt_kernel<1, 1, 1, 0>, rnde_bstage_attempt_kernel<1, 1, 1, 1>, rnde_bstage_attempt_kernel<1, 1, 1, 2>, rnde_bstage_attempt_kernel<1, 1, 1, 3>}};
        static constexpr decltype(&rnde_bstage_kernel<0, BM_START>) kStage[2][2] = {{rnde_bstage_kernel<0, BM_START>, rnde_bstage_kernel<0, BM_STAGE>},
                                                                                   {rnde_bstage_kernel<1, BM_START>, rnde_bstage_kernel<1, BM_STAGE>}};      // [ACT2][MODE]
        static constexpr decltype(&rnde_binit_stage_kernel<0, 0>) kInit[2][4] = {      // [ACT2][STEP]
            {rnde_binit_stage_kernel<0, 0>, rnde_binit_stage_kernel<0, 1>, rnde_binit_stage_kernel<0, 2>, rnde_binit_stage_kernel<0, 3>},
            {rnde_binit_stage_kernel<1, 0>, rnde_binit_stage_kernel<1, 1>, rnde_binit_stage_kernel<1, 2>, rnde_binit_stage_kernel<1, 3>}};
        for (int n = n_att - 1; n >= 0; --n) {
            float c1 = 0.f, c2 = 0.f;      // cotangent coefficients of eigen_est (host-known: saveval cotangent, callback form, recorded norms)
            eig_cotangent(h->cfg.regularize, b.h_svb[n], h->h_meta[n], &c1, &c2);
            const double qo = pow((double)h->h_meta[n].qold_in, (double)kBeta2);   // for the scalar adjoint chain of the attempt
            if (h->persist == 1) {   // the attempt's 7 reverse launches as one (rnde_bstage_persist.h)
                PersistSync Y{h->tslab, h->pabort, h->pxcc, h->persist_spins};
                HIPCHK(h, slab_prepare(h, Q.F.Bpad, s));
                const dim3 pgrid(8 * BQ.R * ((BQ.C + 7) / 8));
                const bool fix = stage_fix(h, BQ.WT, BQ.HT, BQ.KHb, BQ.MT, BQ.R);
                BAttemptKern kern = kAttempt[a2][fix];
                size_t lds = h->stage_lds;
                if (fix) {
                    // (+ the START-staged tape operands of the six stages, rnde_bstage_persist.h: 6 x 7 waves x 2 arrays x 1 KiB)
                    lds = h->stage_lds + (size_t)(RNDE_BSTAGE_HDMA ? 1 : 0) * 6 * 7 * 2 * 1024;
                    static DeviceOnce attr;
                    if (attr.need()) {
                        for (int a = 0; a < 2; ++a) HIPCHK(h, hipFuncSetAttribute((const void*)kAttempt[a][1], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
                        attr.done();
                    }
                    // matrix mode 1 (rnde_x3.h): the forward ran the x3 solve and split the transposed weights too; the x3 form serves every callback of the
                    // experiments (the eigen_est cotangents fit since the partial sums became scalars: 198 VGPRs), and saveat in an instantiation of its own (256)
                    const bool x3 = h->x3_packed && h->x3Bt && h->x3Dt && !getenv("RNDE_X3_REV_OFF");
                    if (x3) {
                        lds = sizeof(float) * ((size_t)2 * kX3ImageFloats + 64) + (size_t)(RNDE_BSTAGE_HDMA ? 1 : 0) * 6 * 7 * 2 * 1024;
                        static DeviceOnce attr3;
                        if (attr3.need()) {
                            for (int a = 0; a < 2; ++a)
                                for (int e = 0; e < 4; ++e) HIPCHK(h, hipFuncSetAttribute((const void*)kAttemptX3[a][e], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
                            attr3.done();
                        }
                        // the instantiation by what this reverse pass needs: saveat cotangents (bit 0), eigen_est cotangents (bit 1: the three stiffness callbacks)
                        kern = kAttemptX3[a2][(h->saveat.empty() ? 0 : 1) | (h->cfg.regularize >= RNDE_REG_STIFF ? 2 : 0)];
                    }
                }
                hipLaunchKernelGGL(kern, pgrid, blk, lds, s, BQ, n, h->h_meta[n], c1, c2, rng[n].lo, rng[n].hi, Y, qo, b.h_svb[n]);
                if ((st = couple_sum(h, b.bpart + (size_t)(n & 1) * Q.bpart_n * 4, 4LL * Q.bpart_n, s)) != RNDE_OK) return st;
                if (pre_reduce && n > 0) hipLaunchKernelGGL(rnde_bpart_reduce_kernel, dim3(1), dim3(64), 0, s, Q, n, bsum);      // (attempt 0's partials go to the reverse of the initial-step rule, which sums them itself)
                if (n >= n_att - side_att && (hi_att - n >= group || n == n_att - side_att)) {   // attempts [n, hi_att) are final
                    st = wgrad_group(2 + 6 * n, 2 + 6 * hi_att, true);
                    if (st != RNDE_OK) return st;
                    hi_att = n;
                }
                continue;
            }
            hipLaunchKernelGGL(kStage[a2][BM_START], grid, blk, h->stage_lds, s, BQ, n, 0, h->h_meta[n], c1, c2, rng[n].lo, rng[n].hi, qo);
            for (int j = 6; j >= 1; --j) hipLaunchKernelGGL(kStage[a2][BM_STAGE], grid, blk, h->stage_lds, s, BQ, n, j, h->h_meta[n], c1, c2, rng[n].lo, rng[n].hi, qo);
            if ((st = couple_sum(h, b.bpart + (size_t)(n & 1) * Q.bpart_n * 4, 4LL * Q.bpart_n, s)) != RNDE_OK) return st;
        }
        HIPCHK(h, hipGetLastError());
        {   // reverse of the initial-step rule (rnde_binit_stage.h): four stage-engine steps, each pair of them -- STEP 0 + 1, STEP 2 + 3: nothing but a hand-off
            // inside the column tile between them -- as one launch on the persistent grid while the persistent kernels are in use (a hand-off that gives up is
            // found by persist_check_* behind this pass, as for the attempt kernel: the handle then falls back to the four launches); RNDE_BINIT_PAIR=0, read per
            // call: the four launches.  The sums over all workgroups (ipart; the coupled controller's all-reduce) stay between the pairs.
            const bool pairs = h->persist == 1 && tail_switch("RNDE_BINIT_PAIR");
            if (pairs) {
                static constexpr decltype(&rnde_binit_pair_kernel<0, 1>) kPair[2][2] = {{rnde_binit_pair_kernel<0, 1>, rnde_binit_pair_kernel<0, 2>},
                                                                                      {rnde_binit_pair_kernel<1, 1>, rnde_binit_pair_kernel<1, 2>}};      // [ACT2][PHASE - 1]
                PersistSync Y{h->tslab, h->pabort, h->pxcc, h->persist_spins};
                HIPCHK(h, slab_prepare(h, Q.F.Bpad, s));
                const dim3 pgrid(8 * BQ.R * ((BQ.C + 7) / 8));
                for (int ph = 0; ph < 2; ++ph) {
                    hipLaunchKernelGGL(kPair[a2][ph], pgrid, blk, h->stage_lds, s, BQ, Y);
                    ++h->tail_folds[3];
                    // (coupled controller) after phase 1: dot, tau of the reversed second evaluation; after phase 2: tau of the first
                    if ((st = couple_sum(h, Q.ipart + ph * 4LL * Q.F.nwg, 4LL * Q.F.nwg, s)) != RNDE_OK) return st;
                }
            }
            for (int step = 0; step < 4 && !pairs; ++step) {
                hipLaunchKernelGGL(kInit[a2][step], grid, blk, h->stage_lds, s, BQ);
                // (coupled controller) after step 1: dot, tau of the reversed second evaluation; after step 3: tau of the first
                if ((step & 1) && (st = couple_sum(h, Q.ipart + (step / 2) * 4LL * Q.F.nwg, 4LL * Q.F.nwg, s)) != RNDE_OK) return st;
            }
            hipLaunchKernelGGL(rnde_bfin_kernel, dim3(1), dim3(64), 0, s, Q);
            HIPCHK(h, hipGetLastError());
        }
    }
    if (h->timing) HIPCHK(h, hipEventRecord(h->tev[3], s));
    // remaining evaluations on all CUs (everything that did not go to the side stream, incl. the two initialisation evaluations)
    st = wgrad_group(0, 2 + 6 * hi_att, false);
    if (st != RNDE_OK) return st;
    if (used_side) {
        hipEvent_t ev = h->wevents[64];
        HIPCHK(h, hipEventRecord(ev, h->wstream));
        HIPCHK(h, hipStreamWaitEvent(s, ev, 0));
    }
    if (cur1 > 16 && cur2 > 16) {   // both layers in one launch per pass (same sums in the same order as launch_wgrad_reduce)
        const long long len1 = (long long)h->H * (h->D + 2), len2 = (long long)h->D * (h->H + 2);
        const size_t seg_r = std::max((size_t)len1, (size_t)len2);
        float* r1 = b.slab_r; float* r2 = b.slab_r + 16 * seg_r;
        const int pg1 = (cur1 + 15) / 16, g1 = (cur1 + pg1 - 1) / pg1, pg2 = (cur2 + 15) / 16, g2 = (cur2 + pg2 - 1) / pg2;
        const int grid = (int)std::min<long long>((std::max(len1, len2) + 255) / 256, 2048);
        if (tail_switch("RNDE_REDUCE_FOLD")) {      // the two passes as one launch, the group sums in registers (rnde_wgrad_reduce_fold_pair: same sums, same order)
            ReducePair F{{{slab1, p_bar_dev, len1, cur1, pg1}, {slab2w, p_bar_dev + (size_t)h->H * (h->D + 2), len2, cur2, pg2}}};
            hipLaunchKernelGGL(rnde_wgrad_reduce_fold_pair, dim3(grid, 1, 2), dim3(256), 0, s, F);
            ++h->tail_folds[0];
        } else {
            ReducePair A{{{slab1, r1, len1, cur1, pg1}, {slab2w, r2, len2, cur2, pg2}}};
            hipLaunchKernelGGL(rnde_wgrad_reduce_pair, dim3(grid, std::max(g1, g2), 2), dim3(256), 0, s, A);
            ReducePair Bp{{{r1, p_bar_dev, len1, g1, g1}, {r2, p_bar_dev + (size_t)h->H * (h->D + 2), len2, g2, g2}}};
            hipLaunchKernelGGL(rnde_wgrad_reduce_pair, dim3(grid, 1, 2), dim3(256), 0, s, Bp);
        }
        HIPCHK(h, hipGetLastError());
    } else {
        HIPCHK(h, launch_wgrad_reduce(slab1, cur1, (long long)h->H * (h->D + 2), b.slab_r, p_bar_dev, s));                                       // [W1; b1]
        HIPCHK(h, launch_wgrad_reduce(slab2w, cur2, (long long)h->D * (h->H + 2), b.slab_r, p_bar_dev + (size_t)h->H * (h->D + 2), s));      // [W2; b2]
    }
    if (h->timing) { HIPCHK(h, hipEventRecord(h->tev[4], s)); h->tev_bwd = true; }
#ifdef RNDE_DIAG
    if (h->persist == 1 && getenv("RNDE_DIAG_BWD")) {
        unsigned long long hst[64] = {0};
        hipStreamSynchronize(s);
        hipMemcpy(hst, h->diag_buf, sizeof(hst), hipMemcpyDeviceToHost);
        fprintf(stderr, "persistent reverse attempt (workgroup 0 thread 0, cycles): START %lld (entry->weights issued %lld, ->w1t %lld, ->array loads issued %lld, finish_attempt_scalars %lld, scalar chain %lld, vector part %lld), its phase D + put %lld\n", (long long)(hst[1]-hst[0]), (long long)(hst[43]-hst[0]), (long long)(hst[44]-hst[43]), (long long)(hst[40]-hst[44]), (long long)(hst[41]-hst[40]), (long long)(hst[42]-hst[41]), (long long)(hst[1]-hst[42]), (long long)(hst[2]-hst[1]));
        for (int st = 0; st < 6; ++st) { const unsigned long long* q = hst + 3 + 5 * st; const unsigned long long prev = st == 0 ? hst[2] : hst[7 + 5 * (st - 1)];
            fprintf(stderr, "  stage j=%d: poll %lld A %lld B %lld C %lld D+put %lld\n", 6 - st, (long long)(q[0]-prev), (long long)(q[1]-q[0]), (long long)(q[2]-q[1]), (long long)(q[3]-q[2]), st < 5 ? (long long)(q[4]-q[3]) : 0LL); }
        fprintf(stderr, "  total %lld cycles to the end of stage 1, END (reduction of the 21 partial sums) %lld; in START's vector part the wait for the record's k arrays %lld\n",
                (long long)(hst[34]-hst[0]), (long long)(hst[35]-hst[34]), (long long)(hst[45]-hst[42]));
    }
#endif
    if (!sync) {   // rnde_node_backward_async: no host round trip; the health words are looked at by the next synchronising call
        if (tspan_bar_dev) HIPCHK(h, hipMemcpyAsync(tspan_bar_dev, b.tspan_out, 8, hipMemcpyDeviceToDevice, s));
        h->have_tape = false;
        h->pending_bwd = h->persist == 1;
        return RNDE_OK;
    }
    HIPCHK(h, hipMemcpyAsync(h->h_scal, b.tspan_out, 8, hipMemcpyDeviceToHost, s));
    persist_check_enqueue(h, h->sR * (Q.F.Bpad / 16), s);
    HIPCHK(h, hipStreamSynchronize(s));
    if (h->couple && rnde_comm_health(h->couple) != RNDE_OK) { h->err = std::string("coupled controller: ") + rnde_comm_last_error(h->couple); return RNDE_ERR_HIP; }
    if (tspan_bar_host) { tspan_bar_host[0] = h->h_scal[0]; tspan_bar_host[1] = h->h_scal[1]; }
    h->have_tape = false;  // z2bar overwrote k_s in place: the tape is consumed
    if (persist_check_result(h, Q.F.Bpad / 16, h->sR, s)) {
        h->err = "persistent reverse kernel abandoned its hand-off (tape consumed): rerun forward + backward, the multi-launch kernels are now in use";
        return RNDE_ERR_HIP;
    }
    return RNDE_OK;
}

// ---- fused classifier head ------------------------------------------------------
static rnde_status head_reserve(rnde_node* h, int32_t B, int32_t n_classes) {
    const size_t need = (size_t)B * n_classes + B + (size_t)kHeadChunks * n_classes * h->D;
    HIPCHK(h, h->head_ws.reserve(need));
    return RNDE_OK;
}
extern "C" rnde_status rnde_classifier_head(rnde_node* h, const float* u_dev, const float* p3_dev, const float* y_dev,
                                            int32_t B, int32_t n_classes, float* logits_out_dev, float* u_bar_dev,
                                            float* p3_bar_dev, float* ce_out_dev, void* stream) {
    if (!h || B < 1 || n_classes < 1 || n_classes > kHeadMaxC) return RNDE_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const rnde_status rs = head_reserve(h, B, n_classes);
    if (rs != RNDE_OK) return rs;
    float* delta = h->head_ws;
    float* ce_col = h->head_ws + (size_t)B * n_classes;
    if (h->D > 256 * kHeadRowsPerThread) { h->err = "classifier head: D <= 1024"; return RNDE_ERR_BAD_ARG; }
    if (n_classes == 10) hipLaunchKernelGGL((rnde_head_col_kernel<10>), dim3(B), dim3(256), 0, s, u_dev, p3_dev, y_dev, h->D, n_classes, B,
                       logits_out_dev, u_bar_dev, delta, ce_col);
    else hipLaunchKernelGGL((rnde_head_col_kernel<0>), dim3(B), dim3(256), 0, s, u_dev, p3_dev, y_dev, h->D, n_classes, B,
                       logits_out_dev, u_bar_dev, delta, ce_col);
    float* partial = ce_col + B;
    hipLaunchKernelGGL(rnde_head_wgrad_kernel, dim3((h->D + 255) / 256, kHeadChunks), dim3(256), 0, s, u_dev, (const float*)delta,
                       h->D, n_classes, B, partial);
    hipLaunchKernelGGL(rnde_head_reduce_kernel, dim3((n_classes * h->D + 255) / 256), dim3(256), 0, s, (const float*)partial,
                       (const float*)delta, (const float*)ce_col, h->D, n_classes, B, p3_bar_dev, ce_out_dev);
    HIPCHK(h, hipGetLastError());
    return RNDE_OK;
}

// ---- one training-step gradient in ONE call (forward solve -> head -> reverse solve), SURVEY.md 8f rank 1 ------------------
// The three calls above chained by the caller leave the GPU idle between the solve and its reverse (~80 us of a 2.4 ms step at
// B = 512): the forward ends in a host wait (the host needs the step log to launch the reverse sweep), and only then does the
// caller queue the head and the reverse pass.  Here the head and the weight packs of the reverse sweep are queued BEFORE that
// wait (they do not depend on the step log), so they run while the host wakes up and prepares the sweep.
extern "C" rnde_status rnde_node_classifier_grad(rnde_node* h, const float* x_dev, const float* p2_dev, const float* p3_dev,
                                                 const float* y_dev, int32_t B, int32_t n_classes, float t0, float t1,
                                                 float lambda, float* p2_bar_dev, float* p3_bar_dev, float* x_bar_dev,
                                                 float* ce_out_dev, float* reg_out_host, int64_t* nfe_out, rnde_comm* comm,
                                                 void* stream) {
    if (!h || !x_dev || !p2_dev || !p3_dev || !y_dev || !p2_bar_dev || !p3_bar_dev || !ce_out_dev) return RNDE_ERR_BAD_ARG;
    RNDE_TILED_REFUSE(h, "rnde_node_classifier_grad is not served (the fused training step runs on the stage engine: two-layer dynamics, rnde_node_create with col_tile 0)");
    if (h->engine != 2) { h->err = "rnde_node_classifier_grad: two-layer dynamics on the stage engine (col_tile 0)"; return RNDE_ERR_BAD_ARG; }
    if (B < 1 || B > h->cfg.max_batch) { h->err = "bad B or tspan"; return RNDE_ERR_BAD_ARG; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t A = (size_t)h->D * B;
    HIPCHK(h, h->cg_ws.reserve(3 * A));
    HIPCHK(h, h->ev_host.create(hipEventDisableTiming));
    if (n_classes < 1 || n_classes > kHeadMaxC) return RNDE_ERR_BAD_ARG;
    rnde_status st = head_reserve(h, B, n_classes);   // (the hook below runs between an event record and the host's wait on it: it only enqueues)
    if (st != RNDE_OK) return st;
    float* u = h->cg_ws; float* ubar = h->cg_ws + A; float* xbar = x_bar_dev ? x_bar_dev : h->cg_ws + 2 * A;
    h->cg_sv.resize((size_t)h->cfg.max_attempts + 1);
    int32_t nsv = 0;
    int64_t nfe = 0;
    h->after_solve = [&](hipStream_t s) -> rnde_status {
        const rnde_status r = rnde_classifier_head(h, u, p3_dev, y_dev, B, n_classes, nullptr, ubar, p3_bar_dev, ce_out_dev, s);
        return r;
    };
    st = forward_impl(h, x_dev, p2_dev, B, t0, t1, u, nullptr, 0, nullptr, &nfe, h->cg_sv.data(), &nsv, 1, stream);
    h->after_solve = nullptr;
    if (st != RNDE_OK) { h->rev_packed = false; return st; }
    // lambda * mean(sv.saveval) (experiments/mnist_node.jl:135): every saved value carries the cotangent lambda / n
    double reg = 0.0;
    const bool regularize = lambda != 0.f && nsv > 0 && h->cfg.regularize != RNDE_REG_NONE;
    if (regularize) {
        for (int i = 0; i < nsv; ++i) reg += h->cg_sv[i];
        reg = (double)lambda * reg / nsv;
        for (int i = 0; i < nsv; ++i) h->cg_sv[i] = lambda / (float)nsv;
    }
    if (reg_out_host) *reg_out_host = (float)reg;
    if (nfe_out) *nfe_out = nfe;
    const int64_t n3 = (int64_t)n_classes * h->D + n_classes;
    st = bwd_run(h, ubar, regularize ? h->cg_sv.data() : nullptr, xbar, p2_bar_dev, nullptr, (hipStream_t)stream, false, nullptr);
    h->rev_packed = false;
    if (st != RNDE_OK) return st;
    if (comm) {   // ONE collective per step when the two gradients sit back to back ([p2-bar | p3-bar], the flat buffer of a data-parallel caller):
        // on the caller's stream everything is serial anyway, and a second call is a second RCCL launch latency
        if (p3_bar_dev == p2_bar_dev + h->P) st = rnde_comm_allreduce(comm, p2_bar_dev, (int64_t)h->P + n3, 0, stream);
        else if ((st = rnde_comm_allreduce(comm, p2_bar_dev, (int64_t)h->P, 0, stream)) == RNDE_OK) st = rnde_comm_allreduce(comm, p3_bar_dev, n3, 0, stream);
        if (st != RNDE_OK) { h->err = std::string("all-reduce: ") + rnde_comm_last_error(comm); return st; }
    }
    return RNDE_OK;
}

// ---- the evaluation call of ClassifierNODE (reference src/metrics.jl:2-18 around src/models/supervised_classification.jl:40-46) ------------
// The untaped solve into a workspace of the handle, then ONE head launch (rnde_head_eval.h): logits, both argmaxes and the count.  Which
// variant is queued where: without labels the launch only overwrites logits_out_dev, so it goes through h->after_solve in front of the host's
// wait (as rnde_node_classifier_grad queues its head; a solve that is redone queues it again).  With labels the fused count is kept and the
// counting variant is queued EXACTLY ONCE, behind the solve's final status: the counter accumulates, a redone solve must not count twice.
// The tiled engine's solve does not pass through wait_for_host: its head is queued behind the solve in both cases.
static rnde_status launch_head_eval(rnde_node* h, const float* u, const float* p3, const float* y, int32_t B, int32_t C, float* logits, int64_t* correct,
                                    hipStream_t s) {
    unsigned long long* cnt = (unsigned long long*)correct;
    const dim3 grid(B), blk(256);
    if (y && cnt) {
        if (C == 10) hipLaunchKernelGGL((rnde_head_eval_kernel<10, true>), grid, blk, 0, s, u, p3, y, h->D, C, logits, cnt);
        else hipLaunchKernelGGL((rnde_head_eval_kernel<0, true>), grid, blk, 0, s, u, p3, y, h->D, C, logits, cnt);
    } else {
        if (C == 10) hipLaunchKernelGGL((rnde_head_eval_kernel<10, false>), grid, blk, 0, s, u, p3, (const float*)nullptr, h->D, C, logits, (unsigned long long*)nullptr);
        else hipLaunchKernelGGL((rnde_head_eval_kernel<0, false>), grid, blk, 0, s, u, p3, (const float*)nullptr, h->D, C, logits, (unsigned long long*)nullptr);
    }
    HIPCHK(h, hipGetLastError());
    return RNDE_OK;
}
extern "C" rnde_status rnde_node_classifier_predict(rnde_node* h, const float* x_dev, const float* p2_dev, const float* p3_dev, const float* y_dev,
                                                    int32_t B, int32_t n_classes, float t0, float t1, float* logits_out_dev, int64_t* correct_dev,
                                                    int64_t* nfe_out, void* stream) {
    if (!h) return RNDE_ERR_BAD_ARG;
    if (!x_dev || !p2_dev || !p3_dev || !logits_out_dev) { h->err = "rnde_node_classifier_predict: null pointer"; return RNDE_ERR_BAD_ARG; }
    if (!y_dev && correct_dev) { h->err = "rnde_node_classifier_predict: correct_dev without y_dev (nothing to count against)"; return RNDE_ERR_BAD_ARG; }
    if (B < 1 || B > h->cfg.max_batch) { h->err = "rnde_node_classifier_predict: 1 <= B <= max_batch = " + std::to_string(h->cfg.max_batch); return RNDE_ERR_BAD_ARG; }
    if (n_classes < 2 || n_classes > kHeadMaxC) { h->err = "rnde_node_classifier_predict: 2 <= n_classes <= " + std::to_string(kHeadMaxC); return RNDE_ERR_BAD_ARG; }
    if (h->D > 256 * kHeadRowsPerThread) { h->err = "rnde_node_classifier_predict: D <= " + std::to_string(256 * kHeadRowsPerThread) + " (the head keeps its rows of W in registers)"; return RNDE_ERR_BAD_ARG; }
    if (!(t1 > t0)) { h->err = "rnde_node_classifier_predict: t1 > t0"; return RNDE_ERR_BAD_ARG; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, h->cg_ws.reserve((size_t)h->D * B));
    HIPCHK(h, h->ev_host.create(hipEventDisableTiming));
    float* u = h->cg_ws;
    const bool counting = y_dev && correct_dev;
    const bool hooked = !counting && h->engine != 4;
    if (hooked) h->after_solve = [&](hipStream_t s) -> rnde_status { return launch_head_eval(h, u, p3_dev, nullptr, B, n_classes, logits_out_dev, nullptr, s); };
    const rnde_status st = forward_impl(h, x_dev, p2_dev, B, t0, t1, u, nullptr, 0, nullptr, nfe_out, nullptr, nullptr, 0, stream);
    h->after_solve = nullptr;
    if (st != RNDE_OK || hooked) return st;
    return launch_head_eval(h, u, p3_dev, y_dev, B, n_classes, logits_out_dev, correct_dev, (hipStream_t)stream);
}

// ---- chain engine reverse pass ----------------------------------------------------------------------------
template <int NKD, int ALT = 0>
static hipError_t launch_bchain_t(rnde_node* h, const BChainParams& Q, const SaveRange* rng, hipStream_t s) {
    const size_t lds = h->chain_lds_b;
    static DeviceOnce attr_set;
    if (attr_set.need()) {
        hipError_t e = hipFuncSetAttribute((const void*)rnde_bchain_kernel<NKD, ALT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)rnde_bchain_init_kernel<NKD, 1, ALT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)rnde_bchain_init_kernel<NKD, 2, ALT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        attr_set.done();
    }
    const dim3 grid(Q.B.F.nwg), blk(64 * kCW);
    for (int n = Q.B.n_att - 1; n >= 0; --n) {
        float c1 = 0.f, c2 = 0.f;   // cotangent of eigen_est for this attempt
        const StepMeta& mm = h->h_meta[n];
        eig_cotangent(h->cfg.regularize, h->bw.h_svb[n], mm, &c1, &c2);
        hipLaunchKernelGGL((rnde_bchain_kernel<NKD, ALT>), grid, blk, lds, s, Q, n, mm, rng[n].lo, rng[n].hi, c1, c2);
    }
    hipLaunchKernelGGL((rnde_bchain_init_kernel<NKD, 1, ALT>), grid, blk, lds, s, Q);
    hipLaunchKernelGGL((rnde_bchain_init_kernel<NKD, 2, ALT>), grid, blk, lds, s, Q);
    hipLaunchKernelGGL(rnde_bfin_kernel, dim3(1), dim3(64), 0, s, Q.B);
    return hipGetLastError();
}


// ---- chain engine, multi-wave kernels: reverse pass (rnde_bchainmw.h) ------------------------------------------------------
template <int NR, int TAB, int LAT = 0>
static rnde_status launch_bmw_t(rnde_node* h, const BMwParams& Q, const SaveRange* rng, hipStream_t s) {
    const BwdBuffers& b = h->bw;
    const size_t lds = h->mw_lds_b;
    static DeviceOnce attr_set;
    if (attr_set.need()) {
        hipError_t e = hipFuncSetAttribute((const void*)rnde_bchainmw_kernel<NR, TAB, LAT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)rnde_bchainmw_kernel<NR, TAB, LAT, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)rnde_bchainmw_init_kernel<NR, 1, LAT == 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)rnde_bchainmw_init_kernel<NR, 2, LAT == 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        HIPCHK(h, e);
        attr_set.done();
    }
    const dim3 grid(Q.ntiles), blk(kMwThreads);
    rnde_status st = RNDE_OK;
    // the whole sweep as ONE launch (rnde_bchainmw.h SWEEP): every workgroup resident (<= 256 column tiles; more than 32: meeting through the
    // memory side, as the forward solve), no shared controller, more than one attempt
    const bool sweep = h->mw_bsweep > 0 && !h->couple && Q.ntiles <= kMwMeetMax && Q.B.n_att >= 2 && h->mw_meet.xch;
    int* a_lo = h->h_mw_bargs; int* a_hi = a_lo + h->cfg.max_attempts; float* a_eig = (float*)(a_hi + h->cfg.max_attempts);
    for (int n = Q.B.n_att - 1; n >= 0; --n) {
        float c1 = 0.f, c2 = 0.f;   // cotangent of eigen_est for this attempt
        const StepMeta& mm = h->h_meta[n];
        eig_cotangent(h->cfg.regularize, b.h_svb[n], mm, &c1, &c2);
        if (sweep) { a_lo[n] = rng[n].lo; a_hi[n] = rng[n].hi; a_eig[2 * n] = c1; a_eig[2 * n + 1] = c2; continue; }
        hipLaunchKernelGGL((rnde_bchainmw_kernel<NR, TAB, LAT>), grid, blk, lds, s, Q, n, mm, rng[n].lo, rng[n].hi, c1, c2);
        // (coupled controller, SURVEY 8e mode 2: the S, tau, c-tau partials of attempt n summed over the ranks before attempt n - 1 reads them)
        if ((st = couple_sum(h, b.bpart + (size_t)(n & 1) * Q.B.bpart_n * 4, 4LL * Q.B.bpart_n, s)) != RNDE_OK) return st;
    }
    if (sweep) {
        const int cap = h->cfg.max_attempts;
        HIPCHK(h, hipMemcpyAsync(h->mw_bargs, h->h_mw_bargs, (size_t)cap * 16, hipMemcpyHostToDevice, s));
        BMwParams W = Q;
        W.meet = h->mw_meet.begin(Q.ntiles, true, s);
        HIPCHK(h, h->mw_meet.err);
        W.sv_lo = h->mw_bargs; W.sv_hi = h->mw_bargs + cap; W.eig_c = (const float*)(h->mw_bargs + 2 * cap);
        W.xcc = h->mw_meet.xcc; W.xcd_slot = h->mw_meet.slot;
        hipLaunchKernelGGL((rnde_bchainmw_kernel<NR, TAB, LAT, 1>), dim3(MeetRes::grid(W.meet)), blk, lds, s, W, Q.B.n_att - 1, h->h_meta[Q.B.n_att - 1], 0, 0, 0.f, 0.f);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, h->mw_meet.queue_check(W.meet, s, h->h_mw_bchk));      // (a buffer of the sweep's own: the verdict is read after a later synchronisation)
        h->pending_bsweep = true; h->bsweep_nt = Q.ntiles; h->bsweep_global = W.meet.global != 0;
    }
    hipLaunchKernelGGL((rnde_bchainmw_init_kernel<NR, 1, LAT == 2>), grid, blk, lds, s, Q);
    if ((st = couple_sum(h, Q.B.ipart, 4LL * Q.B.F.nwg, s)) != RNDE_OK) return st;                        // dot, tau of the reversed second evaluation
    hipLaunchKernelGGL((rnde_bchainmw_init_kernel<NR, 2, LAT == 2>), grid, blk, lds, s, Q);
    if ((st = couple_sum(h, Q.B.ipart + 4LL * Q.B.F.nwg, 4LL * Q.B.F.nwg, s)) != RNDE_OK) return st;      // tau of the first
    hipLaunchKernelGGL(rnde_bfin_kernel, dim3(1), dim3(64), 0, s, Q.B);
    HIPCHK(h, hipGetLastError());
    return RNDE_OK;
}

// ---- what the two chain run functions share ----------------------------------------------------------------------------------------------
static const float kTsit5C[7] = {tsC(0), tsC(1), tsC(2), tsC(3), tsC(4), tsC(5), tsC(6)};      // nodes of the constant-folded pair, as RkTab::c holds a table's

// the buffers of a chain handle's reverse pass, allocated once; E: evaluations per attempted step (6; S - 1 for an S-stage table)
static rnde_status chain_bwd_prepare(rnde_node* h, int E) {
    BwdBuffers& b = h->bw;
    if (b.ready) return RNDE_OK;
    const int cap = h->cfg.max_attempts, ntiles_max = h->Bpad_max / 16;
    const size_t Ac = (size_t)ntiles_max * h->NKD * 64;
    HIPCHK(h, b.U.reserve(Ac)); HIPCHK(h, b.K1.reserve(Ac)); HIPCHK(h, b.UB1.reserve(Ac));
    HIPCHK(h, b.svb_att.reserve((size_t)cap));
    HIPCHK(h, b.bstate_mem.reserve(2 * sizeof(BState))); b.bstate = (BState*)b.bstate_mem.get(); HIPCHK(h, b.ibstate.reserve(2));
    HIPCHK(h, b.bpart.reserve((size_t)(2 * h->nwg_max + 256) * 4)); HIPCHK(h, b.ipart.reserve((size_t)2 * h->nwg_max * 4));   // (+256 entries: finish_attempt_scalars reads whole 256-entry blocks)
    HIPCHK(h, b.tspan_out.reserve(2));
    HIPCHK(h, b.h_svb.reserve((size_t)cap));
    HIPCHK(h, b.slab.reserve((size_t)96 * h->P)); HIPCHK(h, b.slab_r.reserve((size_t)16 * h->P));
    HIPCHK(h, h->ev_t.reserve((size_t)E * cap + 2)); HIPCHK(h, h->h_ev_t.reserve((size_t)E * cap + 2));
    b.ready = true;
    return RNDE_OK;
}
// what a chain sweep reads from the host, sent ahead of it: the saved-value cotangent per attempt and the evaluation times (rnde_rev_plan.h)
static rnde_status chain_bwd_inputs(rnde_node* h, const float* saveval_bar_host, int E, const float* nodes, bool init_first, hipStream_t s) {
    BwdBuffers& b = h->bw;
    gather_saveval_bar(h, saveval_bar_host);
    HIPCHK(h, hipMemcpyAsync(b.svb_att, b.h_svb, (size_t)std::max(1, h->n_att) * 4, hipMemcpyHostToDevice, s));
    eval_times(h->h_meta, h->n_att, E, nodes, h->t0, h->h_init->dt0, init_first, h->h_ev_t);
    HIPCHK(h, hipMemcpyAsync(h->ev_t, h->h_ev_t, (size_t)(E * h->n_att + 2) * 4, hipMemcpyHostToDevice, s));
    return RNDE_OK;
}
// behind the sweep: the parameter gradients of all layers over all evaluations (W: the slab as rnde_chain_wgrad_kernel reads it) and their
// fixed-order reduction; then tspan-bar to the device (async) or, behind a synchronisation, to the host.  The tape is consumed either way.
static rnde_status chain_bwd_finish(rnde_node* h, const BChainParams& W, int n_evals, float* p_bar_dev, float* tspan_bar_host, hipStream_t s, bool sync,
                                    float* tspan_bar_dev) {
    BwdBuffers& b = h->bw;
    const int n_units = n_evals * W.ntiles;
    const int chunks = std::max(1, std::min(96, n_units / 8));
    const int per_chunk = (n_units + chunks - 1) / chunks;
    hipLaunchKernelGGL(rnde_chain_wgrad_kernel, dim3(W.G.n_layers, chunks), dim3(64 * kCW), 0, s, W, (const float*)h->ev_t, n_units, per_chunk, b.slab, h->P);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, launch_wgrad_reduce(b.slab, chunks, h->P, b.slab_r, p_bar_dev, s));
    h->have_tape = false;
    if (!sync) {
        if (tspan_bar_dev) HIPCHK(h, hipMemcpyAsync(tspan_bar_dev, b.tspan_out, 8, hipMemcpyDeviceToDevice, s));
        return RNDE_OK;
    }
    HIPCHK(h, hipMemcpyAsync(h->h_scal, b.tspan_out, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (tspan_bar_host) { tspan_bar_host[0] = h->h_scal[0]; tspan_bar_host[1] = h->h_scal[1]; }
    return RNDE_OK;
}

static rnde_status chain_mw_bwd_run(rnde_node* h, const float* u_bar_dev, const float* saveval_bar_host, float* x_bar_dev,
                                    float* p_bar_dev, float* tspan_bar_host, hipStream_t s, bool sync, float* tspan_bar_dev) {
    const ChainGeo& G = h->cg;
    const int E = h->rk_S - 1;      // evaluations per attempted step (6; S - 1 for an S-stage table)
    rnde_status st = chain_bwd_prepare(h, E);
    if (st != RNDE_OK) return st;
    const int n_evals = E * h->n_att + 2;
    if (!h->mw_slab || h->mw_slab_evals < n_evals) { h->err = "activation slab missing: the forward was not taped on the multi-wave kernels"; return RNDE_ERR_NO_TAPE; }
    // evaluation times in slab order: 0: f(u0,t0), 1: f(u1,t0+dt0), 2 + E n + (s-2): stage s of attempt n
    if ((st = chain_bwd_inputs(h, saveval_bar_host, E, h->rk_tab ? h->rk.c : kTsit5C, true, s)) != RNDE_OK) return st;
    BMwParams Q{};
    Q.B = fill_bwd_params(h, u_bar_dev, x_bar_dev);
    Q.G = h->mg; Q.rk = h->rk; Q.tab = h->mw_tab; Q.ntiles = Q.B.F.Bpad / 16;
    Q.slab = h->mw_slab; Q.ev_stride = (long long)Q.ntiles * h->mg.RS * 64;
    Q.sv_t = h->saveat.empty() ? nullptr : h->sv_t_dev; Q.sv_ubar = u_bar_dev; Q.nsave = (int)h->saveat.size();
    const std::vector<SaveRange> rng = save_ranges(h);
    st = mw_variant(h, [&](auto nr, auto tab, auto lat) { return launch_bmw_t<nr(), tab(), lat()>(h, Q, rng.data(), s); });
    if (st != RNDE_OK) return st;
    // parameter gradients of all layers over all evaluations: the one-wave engine's kernel on the same slab format
    BChainParams W{};
    W.G = G; W.ntiles = Q.ntiles; W.slab = h->mw_slab; W.ev_stride = Q.ev_stride; W.RS = h->mg.RS;
    for (int l = 0; l <= G.n_layers; ++l) { W.hrow[l] = h->mg.hrow[l]; if (l < G.n_layers) W.zrow[l] = h->mg.zrow[l]; }
    st = chain_bwd_finish(h, W, n_evals, p_bar_dev, tspan_bar_host, s, sync, tspan_bar_dev);
    if (st == RNDE_OK && sync && bsweep_failed(h, s))     // nothing the sweep reads was consumed: the same reverse pass again, one launch per attempt
        return chain_mw_bwd_run(h, u_bar_dev, saveval_bar_host, x_bar_dev, p_bar_dev, tspan_bar_host, s, sync, tspan_bar_dev);
    return st;
}

static rnde_status chain_bwd_run(rnde_node* h, const float* u_bar_dev, const float* saveval_bar_host, float* x_bar_dev,
                                 float* p_bar_dev, float* tspan_bar_host, hipStream_t s, bool sync, float* tspan_bar_dev) {
    if (h->mw) { HIPCHK(h, hipSetDevice(h->cfg.device)); return chain_mw_bwd_run(h, u_bar_dev, saveval_bar_host, x_bar_dev, p_bar_dev, tspan_bar_host, s, sync, tspan_bar_dev); }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const ChainGeo& G = h->cg;
    const int E = 6;      // evaluations per attempted step
    rnde_status st = chain_bwd_prepare(h, E);
    if (st != RNDE_OK) return st;
    const int n_evals = E * h->n_att + 2;
    // evaluation times in slab order: E n + (s-2): stage s of attempt n; then f(u0,t0), f(u1,t0+dt0)
    if ((st = chain_bwd_inputs(h, saveval_bar_host, E, kTsit5C, false, s)) != RNDE_OK) return st;
    BChainParams Q{};
    Q.B = fill_bwd_params(h, u_bar_dev, x_bar_dev);
    Q.G = G; Q.frags = h->cfrags; Q.ntiles = Q.B.F.Bpad / 16;
    int row = 0;
    auto pad4 = [](int k) { return 4 * ((k + 3) / 4); };
    for (int l = 0; l < G.n_layers; ++l) { Q.hrow[l] = row; row += pad4(G.nks[l]); Q.zrow[l] = row; row += pad4(G.nks[l + 1]); }
    Q.hrow[G.n_layers] = row; row += pad4(G.nks[G.n_layers]);
    Q.RS = row; Q.ev_stride = (long long)Q.ntiles * row * 64;
    Q.sv_t = h->saveat.empty() ? nullptr : h->sv_t_dev; Q.sv_ubar = u_bar_dev; Q.nsave = (int)h->saveat.size();
    const size_t need = (size_t)n_evals * Q.ev_stride;
    if (h->cslab.cap() < need && h->cslab.reserve(need + need / 2) != hipSuccess)      // (head room: a step count that creeps up while a model trains must not free + allocate every step)
        HIPCHK(h, h->cslab.reserve(need));
    Q.slab = h->cslab;
    const std::vector<SaveRange> rng = save_ranges(h);
    const hipError_t e = chain_variant(h, [&](auto nkd, auto alt) { return launch_bchain_t<nkd(), alt()>(h, Q, rng.data(), s); });
    HIPCHK(h, e);
    return chain_bwd_finish(h, Q, n_evals, p_bar_dev, tspan_bar_host, s, sync, tspan_bar_dev);
}

extern "C" rnde_status rnde_adam_step(float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t len, int64_t t, float eta, float beta1,
                                      float beta2, float eps, float gscale, void* stream) {
    if (!p_dev || !g_dev || !m_dev || !v_dev || len < 0 || t < 1) return RNDE_ERR_BAD_ARG;
    if (len == 0) return RNDE_OK;
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)t)), bc2 = (float)(1.0 - pow((double)beta2, (double)t));
    hipLaunchKernelGGL(rnde::rnde_adam_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p_dev, g_dev, m_dev, v_dev,
                       (long long)len, gscale, eta, beta1, beta2, bc1, bc2, eps);
    return hipGetLastError() == hipSuccess ? RNDE_OK : RNDE_ERR_HIP;
}
extern "C" rnde_status rnde_adam_wd_step(float* p_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t len, int64_t t, float eta, float beta1,
                                         float beta2, float eps, float gscale, float wd, void* stream) {
    if (!p_dev || !g_dev || !m_dev || !v_dev || len < 0 || t < 1) return RNDE_ERR_BAD_ARG;
    if (len == 0) return RNDE_OK;
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)t)), bc2 = (float)(1.0 - pow((double)beta2, (double)t));
    hipLaunchKernelGGL(rnde::rnde_adam_wd_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p_dev, g_dev, m_dev, v_dev,
                       (long long)len, gscale, wd, eta, beta1, beta2, bc1, bc2, eps);
    return hipGetLastError() == hipSuccess ? RNDE_OK : RNDE_ERR_HIP;
}
extern "C" rnde_status rnde_momentum_step_scaled(float* p_dev, const float* g_dev, float* v_dev, int64_t len, int64_t n, float gamma,
                                                 float eta, float rho, float gscale, void* stream);
extern "C" rnde_status rnde_momentum_step(float* p_dev, const float* g_dev, float* v_dev, int64_t len, int64_t n, float gamma,
                                          float eta, float rho, void* stream) {
    return rnde_momentum_step_scaled(p_dev, g_dev, v_dev, len, n, gamma, eta, rho, 1.0f, stream);
}
extern "C" rnde_status rnde_momentum_step_scaled(float* p_dev, const float* g_dev, float* v_dev, int64_t len, int64_t n, float gamma,
                                                 float eta, float rho, float gscale, void* stream) {
    if (!p_dev || !g_dev || !v_dev || len < 0 || n < 1) return RNDE_ERR_BAD_ARG;
    if (len == 0) return RNDE_OK;
    const float inv_decay = gscale / (1.0f + gamma * (float)n);
    hipLaunchKernelGGL(rnde::rnde_momentum_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p_dev, g_dev,
                       v_dev, (long long)len, inv_decay, eta, rho);
    return hipGetLastError() == hipSuccess ? RNDE_OK : RNDE_ERR_HIP;
}

