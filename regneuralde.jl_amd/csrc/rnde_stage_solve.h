// rnde_stage_solve.h -- the stage engine's WHOLE adaptive solve as ONE launch (headline geometry: D = 784, H = 100, 7 x 7 row tiles).
//
// rnde_stage_attempt_kernel (rnde_stage_persist.h) already runs the seven stages of an attempted step in one launch; what it still pays
// per attempt is the kernel boundary the error norm needs: launch ramp, the controller's cold loads (state, 224 partials), 64 VGPRs of
// weights per lane re-read from the Infinity Cache, the state arrays (uprev, k1) re-read from the tape -- ~4 us of a 27 us attempt at
// B = 512, 39 times per forward solve (reference call site: `solve(prob, Tsit5(); ...)`, src/models/neural_ode.jl:131-137).
// Here the attempt loop itself is in the kernel:
//   * the weight slice, w1t / b1, uprev and k1 (= unew and k7 of the last accepted attempt) never leave registers;
//   * the error norm meets through memory: after stage 7 every workgroup publishes its partial sums as 8-byte {value, tag} granules
//     (ONE agent-scope store each: the data is its own validity, `cdna_hip_programming.md` Guideline 16, form R2), wave 0 of every
//     workgroup sweeps all of them with agent-scope loads and forms the sums in the order `sum_partials` forms them -- so the solve is
//     bit-identical to the one-launch-per-attempt path (tests/test_gpu_solve.py);
//   * the PI controller (advance_state_t, rnde_fwd.h) runs between the meeting and the next attempt's first stage, as it does in the
//     prologue of the attempt kernel; StepMeta / StepState records are written exactly as before (the reverse pass reads them).
// The workgroups of a column tile still hand the layer-1 partials to each other through their XCD's L2 (slab_put / slab_poll_sum);
// the meeting crosses XCDs, which is why it uses agent-scope (sc1) stores and loads on granules every workgroup writes once per solve
// (rnde_meet.h, the form with a fixed stride of 256: entry index = attempt number, nothing is ever reused inside a launch, nothing needs clearing).
// All workgroups must be resident at once (<= 256, one per CU); every spin is bounded, a time-out raises the abort word the attempt
// kernels use and the host redoes the solve launch by launch.
// The launches that used to stand around it are inside it too (SolveSync::fold, host switch RNDE_SOLVE_FOLD): in front of the attempt loop the
// initial-step rule -- the four SM_I* launches of rnde_stage_kernel, through the functions that kernel calls (rnde_stage.h), with hand-off buffers and
// granule rows of its own -- and at the end the final state, stored to the caller's buffer from the registers that hold it (rnde_stage_finish_kernel's copy).
#pragma once
#ifndef RNDE_SOLVE_DEFER_TAPE
#define RNDE_SOLVE_DEFER_TAPE 1
#endif
#ifndef RNDE_SOLVE_LOCAL_LAYOUT
#define RNDE_SOLVE_LOCAL_LAYOUT 1
#endif
#include "rnde_stage_persist.h"
#include "rnde_solve_sync.h"
#include "rnde_meet.h"
#include "rnde_x3.h"

namespace rnde {

// the controller state through LDS: written by one lane, read back by every wave as scalars (twelve words)
static_assert(sizeof(StepState) == 48, "StepState is twelve 4-byte words");
__device__ __forceinline__ void solve_state_put(int* ss, const StepState& S) {
    const int* src = (const int*)&S;
#pragma unroll
    for (int i = 0; i < 12; ++i) ss[i] = src[i];
}
__device__ __forceinline__ StepState solve_state_get(const int* ss) {
    StepState S;
    int* dst = (int*)&S;
#pragma unroll
    for (int i = 0; i < 12; ++i) dst[i] = __builtin_amdgcn_readfirstlane(ss[i]);
    return S;
}

// The two Dense-layer products of a stage in their fp32-input-MFMA form (headline geometry, LDS operand images [16][116] with permuted k): used by every
// stage of the X3 = 0 kernel and by the start-up of both (the initial-step rule is fp32-input-MFMA arithmetic in both matrix modes).
// layer 1: this row block's partial of W1 * v for the wave's hidden tile; v goes through the image GL (one barrier inside)
__device__ __forceinline__ f32x4 solve_f32_layer1(float* GL, const f32x4 (&wD)[7], const f32x4& v, int own_gl0, int col, int lane) {
    constexpr int KG = 16 * 7 + 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) GL[own_gl0 + 4 * i] = v[i];
    __syncthreads();
    const float* gbp = GL + col * KG + 4 * (lane >> 4);
    f32x4 bg[7];
#pragma unroll
    for (int kb = 0; kb < 7; ++kb) bg[kb] = *(const f32x4*)(gbp + 16 * kb);
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < 7; ++kb) {
        acc0 = mfma16(wD[kb][0], bg[kb][0], acc0);
        acc1 = mfma16(wD[kb][1], bg[kb][1], acc1);
        acc0 = mfma16(wD[kb][2], bg[kb][2], acc0);
        acc1 = mfma16(wD[kb][3], bg[kb][3], acc1);
    }
    return acc0 + acc1;
}
// layer 2: the wave's 16 rows of W2ext * [h; t; 1] from the image HL (k-steps from 104 on multiply zeros and are left out, as in the attempt kernel)
__device__ __forceinline__ f32x4 solve_f32_layer2(const float* HL, const f32x4 (&wB)[7], int col, int lane) {
    constexpr int KH = 16 * 7 + 4, gH = 100;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const float* hb = HL + col * KH + 4 * (lane >> 4);
    f32x4 bf[7];
#pragma unroll
    for (int kb = 0; kb < 7; ++kb) bf[kb] = *(const f32x4*)(hb + 16 * kb);
#pragma unroll
    for (int kb = 0; kb < 7; ++kb) {
        acc0 = mfma16(wB[kb][0], bf[kb][0], acc0);
        if (16 * kb + 4 < gH + 2) acc1 = mfma16(wB[kb][1], bf[kb][1], acc1);
        if (16 * kb + 8 < gH + 2) acc0 = mfma16(wB[kb][2], bf[kb][2], acc0);
        if (16 * kb + 12 < gH + 2) acc1 = mfma16(wB[kb][3], bf[kb][3], acc1);
    }
    return acc0 + acc1;
}

// where Z.u_out lies in rnde_stage_solve_kernel's kernel-argument segment (the arguments follow each other as the members of a struct would)
struct SolveKernelArgs { StageParams Q; PersistSync Y; SolveSync Z; };
constexpr size_t kSolveArgUOut = offsetof(SolveKernelArgs, Z) + offsetof(SolveSync, u_out);

// X3 = 1: the two Dense-layer products of every stage on the matrix cores (rnde_x3.h: exact three-way bf16 split of both operands, six
// v_mfma_f32_16x16x32_bf16 per 32 k-values) instead of the fp32-input MFMA, which this part executes on its vector ALUs.  Everything else -- hand-off,
// meeting, controller, tape layout, the state in registers -- is the same code.  The products are rounded differently (more accurately: rnde_x3.h), so
// an X3 solve is NOT bit-identical to the fp32-MFMA kernels; its parity is stated against the fp64 restatement (tests/test_gpu_x3.py).
template <int ACT2, int X3>
__global__ __launch_bounds__(64 * 7) void rnde_stage_solve_kernel(const StageParams Q, const PersistSync Y, const SolveSync Z) {
    const StepParams& P = Q.F;
    constexpr int gWT = 7, gHT = 7, gK2b = 7, gR = 7, gD = 784, gH = 100;
    constexpr int KH = 16 * gK2b + 4, KG = 16 * gWT + 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* HL = smem;
    float* GL = HL + (X3 ? kX3ImageFloats : kSCB * KH);
    float* RED = GL + (X3 ? kX3ImageFloats : kSCB * KG);         // [32]; RED[24] = "a wave of this workgroup gave up"
    unsigned short* HX = (unsigned short*)HL;      // X3: the operand images [plane][column][kX3K] of bf16 in place of the fp32 images
    unsigned short* GX = (unsigned short*)GL;
    double* SUMS = (double*)(RED + 32);  // [4]: the three cross-workgroup sums of the meeting, [3] != 0: the meeting failed
    float* QP = (float*)(SUMS + 4);      // [2] (by attempt parity: a fast wave writes the next one while a slow wave still reads this one): powf(qold, beta2) of the state the running attempt started from (evaluated off the critical path)
    int* SS = (int*)(QP + 2);            // [12] the controller state before the next attempt, as wave 0 derived it behind the meeting (see solve_state_put / _get)
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    __builtin_assume(w >= 0 && w < 7);
    const int rb = (blockIdx.x >> 3) % gR, ct = 8 * ((blockIdx.x >> 3) / gR) + (blockIdx.x & 7);      // a tile's row blocks share blockIdx % 8 (one XCD)
    if (ct >= Q.C) return;
    const int wg = rb * Q.C + ct;
    const int col = lane & 15, gcol = ct * kSCB + col;
    const bool colok = gcol < P.B;
    constexpr bool vec = true;
    const bool writer = (wg == 0 && tid == 0);
    const int T = rb * gWT + w;
    const int r0 = 16 * T + 4 * (lane >> 4);
#if RNDE_SOLVE_LOCAL_LAYOUT
    const RecLayout LL{(long long)gD * P.Bpad, (long long)gH * P.Bpad};
#else
    const RecLayout L{(long long)gD * P.Bpad, (long long)gH * P.Bpad};
#endif
    if (tid == 0) Y.xcc[wg] = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 15;   // HW_REG_XCC_ID
    const size_t co = (size_t)gcol * gD;

    // ---- once per solve: the state the first attempt starts from, this block's weight slice, the bias / time column of this wave's hidden tile ----
    f32x4 c_up = ld4(P.x + co, r0, gD, colok, P.xvec != 0), c_k[7];
    c_k[0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (!Z.fold) c_k[0] = ld4(P.f0 + co, r0, gD, true, vec);      // (Z.fold: f0 comes out of the start-up below)
#pragma unroll
    for (int j = 1; j < 7; ++j) c_k[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float w1t_own[4] = {0.f, 0.f, 0.f, 0.f}, b1_own[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int hr = 16 * w + 4 * (lane >> 4) + i;
        if (hr < gH) { w1t_own[i] = Q.p[(size_t)gH * gD + hr]; b1_own[i] = Q.p[(size_t)gH * (gD + 1) + hr]; }
    }
    f32x4 wB[X3 ? 1 : 7], wD[X3 ? 1 : 7];
    x3u4 xB[X3 ? 4 : 1][3], xD[X3 ? 4 : 1][3];
    // the fp32 fragments of this block's weight slice: the X3 = 0 kernel's operands for the whole solve; the X3 = 1 kernel needs them for the start-up
    // only and loads its split weights behind it (the two fragment sets are never live together)
    auto load_f32_weights = [&](f32x4 (&fB)[7], f32x4 (&fD)[7]) {
        const f32x4* pB = Q.pwB + ((size_t)T * gK2b) * 64 + lane;
        const f32x4* pD = Q.pwD + ((size_t)w * 49 + rb * gWT) * 64 + lane;
#pragma unroll
        for (int kb = 0; kb < 7; ++kb) fD[kb] = pD[(size_t)kb * 64];
#pragma unroll
        for (int kb = 0; kb < 7; ++kb) fB[kb] = pB[(size_t)kb * 64];
        fB[6][2] = 0.f; fB[6][3] = 0.f;      // (k-steps 104.. multiply zeros and are left out, as in the attempt kernel)
    };
    if constexpr (!X3) load_f32_weights(wB, wD);

    // loop-invariant addressing of this lane's four rows of its own hidden tile (phase A) and row tile (phase D)
    int own_kind[4];
    float own_c1[4], own_c0[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int hr = 16 * w + 4 * (lane >> 4) + i;
        own_kind[i] = hr < gH ? 0 : (hr == gH ? 1 : (hr == gH + 1 ? 2 : 3));
        own_c1[i] = own_kind[i] == 1 ? 1.f : 0.f; own_c0[i] = own_kind[i] == 2 ? 1.f : 0.f;
    }
    const int own_hl0 = col * KH + kperm(16 * w + 4 * (lane >> 4));
    const int own_gl0 = col * KG + kperm(16 * w + 4 * (lane >> 4));
    const size_t own_hd0 = (size_t)gcol * gH + 16 * w + 4 * (lane >> 4);
    // (the hidden activations are computed identically by all seven row blocks of a tile: row block rb tapes hidden tile rb -- one store per
    //  stage and workgroup instead of seven in row block 0, whose workgroups would otherwise reach every meeting last)
    const bool own_hstore = rb == w && own_kind[3] == 0;
    if (tid == 0) { RED[24] = 0.f; SUMS[0] = SUMS[1] = SUMS[2] = SUMS[3] = 0.0; }
    __syncthreads();

    // phase D: this row block's layer-1 partial of the stage input v -> slab, exchange number `ex`
    auto phase_d = [&](const f32x4& v, unsigned ex) {
        if constexpr (X3) {
            x3_store4(GX, col, 16 * w + 4 * (lane >> 4), v);
            __syncthreads();
            const size_t tile0x = (((size_t)slab_buf(ex) * Q.C + ct) * gR + rb) * gHT;
            slab_put(Y.tslab, tile0x + w, lane, x3_tile<4>(xD, GX, lane));
        } else {
            const size_t tile0 = (((size_t)slab_buf(ex) * Q.C + ct) * gR + rb) * gHT;
            slab_put(Y.tslab, tile0 + w, lane, solve_f32_layer1(GL, wD, v, own_gl0, col, lane));
        }
    };
    // phase A's arithmetic: the wave's hidden tile (rows beyond H: the time row, the bias row's 1, zeros) from the summed layer-1 partials
    auto hidden_of = [&](const f32x4& zs, float ts) {
        float pre[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) pre[i] = fmaf(w1t_own[i], ts, zs[i]) + b1_own[i];
        const f32x2 t01 = tanh_fast2((f32x2){pre[0], pre[1]}), t23 = tanh_fast2((f32x2){pre[2], pre[3]});
        f32x4 hv = {t01.x, t01.y, t23.x, t23.y};
        if (w == 6) {
#pragma unroll
            for (int i = 0; i < 4; ++i) hv[i] = own_kind[i] == 0 ? hv[i] : fmaf(own_c1[i], ts, own_c0[i]);
        }
        return hv;
    };
    auto act2_of = [&](f32x4 kv) {
        if (ACT2) {
            const f32x2 a01 = tanh_fast2((f32x2){kv[0], kv[1]}), a23 = tanh_fast2((f32x2){kv[2], kv[3]});
            kv = (f32x4){a01.x, a01.y, a23.x, a23.y};
        }
        return kv;
    };

    // ---- the start-up (Z.fold): the initial-step rule, i.e. what the launches SM_I1 .. SM_I4 of rnde_stage_kernel compute in front of a solve -- f0 = f(u0, t0),
    // dt0 from ||u0|| and ||f0||, f1 = f(u0 + dt0 f0, t0 + dt0), ||f1 - f0|| -- through the same functions (rnde_stage.h) and the same fp32-input-MFMA products,
    // with everything those launches leave for the reverse pass (f0, h0, u1, f1, h1, initpart, InitRec).  The two hand-offs inside a column tile use slab
    // buffers of their own (3 and 4: the attempts cycle through 0 .. 2), emptied by their producers once every consumer is known to be through; the two
    // cross-workgroup sums meet on the granule rows behind the attempts' (Z.n_limit, Z.n_limit + 1), formed in sum_partials' order.
    InitFold IF{0.0, 0.f, 0.f, Z.fold};      // (wave 0) for the controller of attempt 0
    auto startup = [&](const f32x4 (&fB)[7], const f32x4 (&fD)[7]) __attribute__((always_inline)) -> bool {
        const f32x4 xv = c_up;
        // f at (v, ts): layer-1 partials through start-up buffer `buf`, hidden activations to hdst; false: a hand-off gave up
        auto feval = [&](const f32x4& v, float ts, int buf, float* hdst, f32x4& kv) __attribute__((always_inline)) -> bool {
            const size_t tile0 = (((size_t)buf * Q.C + ct) * gR + rb) * gHT;
            slab_put(Y.tslab, tile0 + w, lane, solve_f32_layer1(GL, fD, v, own_gl0, col, lane));
            f32x4 zs = {0.f, 0.f, 0.f, 0.f};
            const bool dead = !slab_poll_sum(Y, buf, Q.C, gR, gHT, ct, w, lane, zs);
            const f32x4 hv = hidden_of(zs, ts);
            if (own_hstore) *(f32x4*)(hdst + own_hd0) = hv;
#pragma unroll
            for (int i = 0; i < 4; ++i) HL[own_hl0 + 4 * i] = hv[i];
            if (dead && lane == 0) RED[24] = 1.f;
            __syncthreads();
            if (RED[24] != 0.f) return false;
            kv = act2_of(solve_f32_layer2(HL, fB, col, lane));
            return true;
        };
        // the workgroup's partial sums (summed as rnde_stage_kernel sums them) to initpart rows prow.., everybody's sums from granule row Z.n_limit + row (wave 0)
        auto meet = [&](int nval, float p0, float p1, int prow, int row, double (&o)[3]) __attribute__((always_inline)) -> bool {
            p0 = wave_sum_f(p0); p1 = wave_sum_f(p1);
            if (lane == 0) { RED[w] = p0; RED[8 + w] = p1; }
            __syncthreads();
            if (w != 0) return true;
            float mine[3] = {0.f, 0.f, 0.f};
            for (int i = 0; i < gWT; ++i) { mine[0] += RED[i]; mine[1] += RED[8 + i]; }
            if (lane == 0) { P.initpart[(size_t)prow * P.nwg + wg] = mine[0]; if (nval > 1) P.initpart[(size_t)(prow + 1) * P.nwg + wg] = mine[1]; }
            return meet_exchange_256(Z.xch, Z.epoch, Y.abort_flag, Y.max_spins, Z.n_limit + row, P.nwg, wg, nval, mine, o, lane);
        };
        const size_t tileA = (((size_t)(kSlabBufs - 2) * Q.C + ct) * gR + rb) * gHT, tileB = (((size_t)(kSlabBufs - 1) * Q.C + ct) * gR + rb) * gHT;
        double o[3] = {0.0, 0.0, 0.0};
        // SM_I1, SM_I2: f0, h0, the partials of ||u0|| and ||f0||
        f32x4 f0;
        if (!feval(xv, P.t0, kSlabBufs - 2, P.h0, f0)) return false;
        st4(P.f0 + co, r0, gD, true, vec, f0);
        c_k[0] = f0;
        float p0 = 0.f, p1 = 0.f;
        init_norm_parts_u0_f0(P, xv, f0, r0, colok, p0, p1);
        bool ok = meet(2, p0, p1, 0, 0, o);
        // SM_I3: dt0, the Euler step
        if (w == 0) {
            float d1; IF.dt0 = init_dt0_rule(P, o[0], o[1], writer, &d1); IF.d1 = d1;
            if (lane == 0) { RED[25] = IF.dt0; if (!ok) SUMS[3] = 1.0; }
        }
        __syncthreads();
        if (SUMS[3] != 0.0) return false;
        const float dt0 = RED[25];
        const f32x4 u1 = init_euler_step(xv, dt0, f0);
        st4(P.u1 + co, r0, gD, true, vec, u1);
        // SM_I4: f1, h1, the partial of ||f1 - f0||
        f32x4 f1;
        if (!feval(u1, P.t0 + dt0, kSlabBufs - 1, P.h1, f1)) return false;
        slab_clear(Y.tslab, tileA + w, lane);      // (this wave's poll of the second exchange succeeded: every row block's wave w has produced it, hence consumed the first)
        st4(P.f1 + co, r0, gD, true, vec, f1);
        p0 = 0.f;
        init_norm_part_df(P, xv, f0, f1, r0, colok, p0);
        ok = meet(1, p0, 0.f, 2, 1, o);
        if (w == 0) { IF.s2 = o[0]; if (lane == 0 && !ok) SUMS[3] = 1.0; }
        __syncthreads();
        if (SUMS[3] != 0.0) return false;
        slab_clear(Y.tslab, tileB + w, lane);      // (every workgroup has come to the second meeting, hence consumed the second exchange; acknowledged before the first put of attempt 0)
        return true;
    };
    if (Z.fold) {
        if constexpr (X3) {
            f32x4 fB[7], fD[7];
            load_f32_weights(fB, fD);
            if (!startup(fB, fD)) return;
        } else {
            if (!startup(wB, wD)) return;
        }
    }
    if constexpr (X3) {
        const x3u4* pB = (const x3u4*)Z.x3B + ((size_t)T * 4 * 3) * 64 + lane;
        const x3u4* pD = (const x3u4*)Z.x3D + ((size_t)(w * gR + rb) * 4 * 3) * 64 + lane;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) { xD[s][pl] = pD[(size_t)(s * 3 + pl) * 64]; xB[s][pl] = pB[(size_t)(s * 3 + pl) * 64]; }
        }
        // the operand images start as zeros: k-values nobody writes (102 .. 127 of the hidden layer's, 112 .. 127 of the row block's) multiply zero weights
        for (int i = tid; i < 2 * kX3ImageFloats; i += 64 * 7) HL[i] = 0.f;
        __syncthreads();
    }

#ifdef RNDE_DIAG      // cycle stamps of workgroup 0, eight per attempt (tools/diag_solve.py)
#define ZSTAMP(k) do { if (P.dbg_out && wg == 0 && tid == 0 && n < 120) ((unsigned long long*)P.dbg_out)[n * 8 + (k)] = clock64(); } while (0)
// every workgroup's arrival at the meeting of attempt 10 and its way out of it (s_memrealtime: one clock for all XCDs, 100 MHz)
#define ZARRIVE(k) do { if (P.dbg_out && tid == 0 && n == 10) ((unsigned long long*)P.dbg_out)[1024 + wg * 2 + (k)] = wall_clock64(); } while (0)
#else
#define ZSTAMP(k) do { } while (0)
#define ZARRIVE(k) do { } while (0)
#endif
    // ---- controller: ONE wave per workgroup derives the state before an attempt (wave 0: it holds the meeting's sums in registers and is alone on its
    // SIMD while wave 4 waits at the barrier), the others pick the twelve words up from LDS.  Round 4 had every wave derive it redundantly from the
    // sums in LDS: the same function on the same arguments -- the same bits -- at seven times the vector instructions (the controller's float arithmetic,
    // two pow and the double-precision norms, runs on the vector ALU: this part has no scalar float unit), two waves per SIMD taking turns.
    const float none[4] = {0.f, 0.f, 0.f, 0.f};
    StepState S{};
    if (w == 0) {
        const StepState nop{};
        S = advance_state_t<true>(P, 0, lane, writer, &P.ctl[0], none, nop, nullptr, nullptr, &IF);
        if (lane == 0) solve_state_put(SS, S);
    }
    __syncthreads();
    S = solve_state_get(SS);
    f32x4 c_un = {0.f, 0.f, 0.f, 0.f};
    // the tape stores of a stage (k_{s+1}, g_{s+2} / u_new) are issued BEHIND the next stage's poll: a wave's polling load cannot complete before every
    // older store of the wave is acknowledged (vmcnt counts both), so a store in front of a poll puts its acknowledgement on the hand-off's critical path;
    // behind the poll it has a whole stage to come back.  The values are in registers anyway (c_k[s]; the stage input is carried in `pend`).  Matrix mode 1
    // only: there it takes 0.3 us off an attempt in-step; the fp32-input-MFMA form's stages got 3 % LONGER with it (41.8 k against 40.5 k cycles, stamps).
    constexpr bool DEFER = RNDE_SOLVE_DEFER_TAPE && X3;
    f32x4 pend = {0.f, 0.f, 0.f, 0.f};
    for (int n = 0;; ++n) {
        ZSTAMP(0);
        // the controller of the NEXT attempt divides by qold^beta2, and qold is known now: wave 3 -- alone on its SIMD -- evaluates the power while
        // the stages run, the others pick it up after the meeting (the barriers in between order the LDS word); same function, same argument, same bits
        if (w == 3 && lane == 0) QP[(n + 1) & 1] = powf(S.qold, P.beta2);
        ZSTAMP(1);
        if (S.done || n >= Z.n_limit) {
            if (writer) *P.ctl_final = S;
            // the final state -- x when nothing was accepted, else unew of the live record: what c_up holds after the accept hand-over -- from registers
            // (the pointer is read from the kernel-argument segment HERE: taken from Z it stays in scalar registers across the attempt loop, which has none to spare)
            float* const uo = *(float* volatile const*)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + kSolveArgUOut);
            if (uo) st_tile(uo + (size_t)gcol * gD, r0, gD, colok, (reinterpret_cast<size_t>(uo) & 15) == 0, c_up);
            return;
        }
        const float t = S.t, dt = (P.t1 - S.t < S.dtp) ? (P.t1 - S.t) : S.dtp;
        const int rec = P.tape ? n : (S.live == 0 ? 1 : 0);
        float* R = P.arena + (long long)rec * P.rec_stride;
#if RNDE_SOLVE_LOCAL_LAYOUT
        // the record's array offsets are formed from (A, HB) where they are used, every attempt: left to itself the compiler keeps the ~19 loop-invariant 64-bit
        // offsets in scalar registers across the attempt loop and spills them (75-81 SGPR spills, 143 v_readlane per attempt); the empty asm hides the invariance
        long long A_n = LL.A, HB_n = LL.HB;
        asm volatile("" : "+s"(A_n), "+s"(HB_n));
        const RecLayout L{A_n, HB_n};
#endif

        // ---- the attempt kernel's START: g2, exchange 1 ----
        {
            const f32x4 v = fma4(dt, tsA(1, 0) * c_k[0], c_up);
            // the clears of the previous attempt's last stage are acknowledged before this attempt's first put -- they were issued before the meeting, so
            // nothing waits here; BEHIND the tape store below the same wait would sit on that store's acknowledgement (vmcnt counts stores too)
            slab_clears_done();
            if constexpr (DEFER) pend = v;
            else if (P.tape) st4(R + L.g(2) + co, r0, gD, true, vec, v);
            phase_d(v, 1u);
        }
        ZSTAMP(2);

        float part0 = 0.f, part1 = 0.f, part2 = 0.f;
        bool alive = true;
        auto stage = [&](auto sc) {
            constexpr int s = decltype(sc)::value;
            if (!alive) return;
            const float ts = fmaf(tsC(s), dt, t);
            float* hdst = R + L.h(s + 1);
            float* kdst = R + L.k(s + 1);
            const int buf = slab_buf((unsigned)s);
            // ---- phase A: poll this wave's hidden tile of the 7 row blocks (the polling load is the data load) ----
            f32x4 zs = {0.f, 0.f, 0.f, 0.f};
            const bool dead = !slab_poll_sum(Y, buf, Q.C, gR, gHT, ct, w, lane, zs);
            const size_t tprev0 = (((size_t)slab_buf((unsigned)(s + 2)) * Q.C + ct) * gR + rb) * gHT;
            if (!dead) slab_clear(Y.tslab, tprev0 + w, lane);
            if constexpr (DEFER) {
                if constexpr (s >= 2) st4(R + L.k(s) + co, r0, gD, true, vec, c_k[s - 1]);
                if constexpr (s == 6) st4(R + L.unew() + co, r0, gD, true, vec, pend);
                else if (P.tape) st4(R + L.g(s + 1) + co, r0, gD, true, vec, pend);
            }
            const f32x4 hv = hidden_of(zs, ts);
            if (own_hstore) *(f32x4*)(hdst + own_hd0) = hv;
            if constexpr (X3) x3_store4(HX, col, 16 * w + 4 * (lane >> 4), hv);
            else {
#pragma unroll
                for (int i = 0; i < 4; ++i) HL[own_hl0 + 4 * i] = hv[i];
            }
            if (dead && lane == 0) RED[24] = 1.f;
            __syncthreads();
            if constexpr (!X3) { if (RED[24] != 0.f) { alive = false; return; } }
            // ---- phase B ----
            f32x4 kv;
            if constexpr (X3) {
                const float gave_up = RED[24];      // (requested in front of the fragments -- x3_tile's first scheduling barrier keeps it there -- and looked at behind the products)
                kv = x3_tile<4>(xB, HX, lane);
                if (gave_up != 0.f) { alive = false; return; }      // (X3: the flag is read with the fragments, not in front of them -- an LDS round trip per stage less on the chain; a workgroup that gives up has multiplied for nothing)
                kv = act2_of(kv);
            } else kv = act2_of(solve_f32_layer2(HL, wB, col, lane));
            // ---- phase C ----
            if constexpr (s < 6) {
                slab_clears_done();      // (issued two phases ago: nothing to wait for in practice) before this stage's put, see slab_put
                if constexpr (!DEFER) st4(kdst + co, r0, gD, true, vec, kv);
                f32x4 acc = tsA(s + 1, 0) * c_k[0];
#pragma unroll
                for (int j = 1; j < 6; ++j) if (j < s) acc = fma4(tsA(s + 1, j), c_k[j], acc);
                acc = fma4(tsA(s + 1, s), kv, acc);
                const f32x4 v = fma4(dt, acc, c_up);
                if constexpr (DEFER) { pend = v; if (s == 5) c_un = v; }
                else {
                    if (s == 5) { st4(R + L.unew() + co, r0, gD, true, vec, v); c_un = v; }
                    else if (P.tape) st4(R + L.g(s + 2) + co, r0, gD, true, vec, v);
                }
                c_k[s] = kv;
                phase_d(v, (unsigned)(s + 1));
            } else {
                st4(kdst + co, r0, gD, true, vec, kv);
                c_k[6] = kv;      // k7: k1 of the next attempt if this one is accepted
                const f32x4 up = c_up, un = c_un;
                f32x4 acc = tsBt(0) * c_k[0];
#pragma unroll
                for (int j = 1; j < 6; ++j) acc = fma4(tsBt(j), c_k[j], acc);
                acc = fma4(tsBt(6), kv, acc);
                if (colok) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float ut = dt * acc[i];
                        const float sk = P.abstol + fmaxf(fabsf(up[i]), fabsf(un[i])) * P.reltol;
                        const float r = ut / sk;
                        part0 = add_square_unfused(part0, r);
                    }
                    if (P.reg_kind >= 2) {
                        f32x4 g6 = tsA(5, 0) * c_k[0];
#pragma unroll
                        for (int j = 1; j < 5; ++j) g6 = fma4(tsA(5, j), c_k[j], g6);
                        g6 = fma4(dt, g6, up);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float d1 = kv[i] - c_k[5][i], d2 = un[i] - g6[i];
                            part1 = add_square_unfused(part1, d1); part2 = add_square_unfused(part2, d2);
                        }
                    }
                }
            }
        };
        stage(std::integral_constant<int, 1>{});
        stage(std::integral_constant<int, 2>{});
        stage(std::integral_constant<int, 3>{});
        stage(std::integral_constant<int, 4>{});
        stage(std::integral_constant<int, 5>{});
        stage(std::integral_constant<int, 6>{});
        if (!alive) return;
        ZSTAMP(3);

        // ---- the meeting: this workgroup's partials (same reduction order as the attempt kernel), everybody's sums ----
        const bool three = P.reg_kind >= 2;      // (the two norms of the stiffness estimate travel only when it is asked for)
        part0 = wave_sum_f(part0);
        if (three) { part1 = wave_sum_f(part1); part2 = wave_sum_f(part2); }
        if (lane == 0) { RED[w] = part0; if (three) { RED[8 + w] = part1; RED[16 + w] = part2; } }
        __syncthreads();
        ZSTAMP(4); ZARRIVE(0);
        if (w == 0) {
            float mine[3] = {0.f, 0.f, 0.f};
            for (int i = 0; i < gWT; ++i) { mine[0] += RED[i]; if (three) { mine[1] += RED[8 + i]; mine[2] += RED[16 + i]; } }
            double o[3];
            const bool ok = meet_exchange_256(Z.xch, Z.epoch, Y.abort_flag, Y.max_spins, n, P.nwg, wg, P.reg_kind >= 2 ? 3 : 1, mine, o, lane);
            ZSTAMP(5); ZARRIVE(1);
            // the state before attempt n + 1, from the sums just formed (qold^beta2 of the state this attempt started from: wave 3 left it in QP while
            // the stages ran; the barrier in front of the meeting ordered it)
            const float qp = QP[(n + 1) & 1];
            const StepState nxt = advance_state_t<true>(P, n + 1, lane, writer, &P.ctl[(n + 1) & 1], none, S, o, &qp);
            if (lane == 0) { solve_state_put(SS, nxt); if (!ok) SUMS[3] = 1.0; }
        }
        __syncthreads();
        ZSTAMP(6);
        if (SUMS[3] != 0.0) return;      // the meeting timed out: abort word raised, the host redoes the solve launch by launch
        {
            const StepState nxt = solve_state_get(SS);
            if (nxt.n_acc != S.n_acc) { c_up = c_un; c_k[0] = c_k[6]; }      // accepted: the next attempt starts from (unew, k7) -- already here
            S = nxt;
        }
    }
}

}  // namespace rnde
