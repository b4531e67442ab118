// Reverse of the initial-step rule (k1 = f(u0, t0), u1 = u0 + dt0 k1, f1 = f(u1, t0 + dt0), the three norms) on the STAGE engine:
// weight-stationary workgroups (row block rb x column tile ct, one 16-row tile per wave) as rnde_bstage_kernel, four launches
//   STEP 0   scalars of phase 1, z2bar of f1, phase D (hbar partial -> slab, parity 0)
//   STEP 1   phase A (hbar, z1bar of f1), phase B (u1-bar), partial sums {<u1-bar, f0>, tau}
//   STEP 2   scalars of phase 2 (sums of those partials), z2bar of f0 and the direct part of x-bar, phase D (parity 1)
//   STEP 3   phase A, phase B, x-bar += u0-bar of f0, partial sum {tau}
// in place of the two column-owner launches (rnde_binit_kernel, 2 x ~32 us on 64 workgroups that stream the weights through L2 and triple that
// the moment anything else streams beside them).  Same arithmetic per element (rnde_bwd.h: rnde_binit_kernel / f_bwd); the sums over workgroups
// run over the stage engine's R x C partials instead of the column owner's B / 8 -- a different association of the same terms.
//
// STEP 0 -> STEP 1 and STEP 2 -> STEP 3 are separated by nothing but the hand-off of the hbar partials between the R row blocks of a column tile; the sums over
// ALL workgroups (ipart, and with it the coupled controller's all-reduce) sit behind STEP 1 and behind STEP 3.  rnde_binit_pair_kernel<ACT2, PHASE> runs a pair as
// one launch, the way rnde_bstage_attempt_kernel runs an attempt's seven: the same grid and (rb, ct) decoding (a column tile's row blocks on one XCD), the partials
// through the hand-off slabs of rnde_stage_persist.h (slab_put / slab_poll_sum, bounded spins, the abort word), the weights of both phases and the state arrays
// requested once.  The two steps of a pair are the bodies below (binit_phase_d, binit_phase_ab), which the four stand-alone launches run too: the same
// instructions on the same values, the partials summed over r = 0 .. R - 1 from zero in both forms, so the same bits.
//   Which slab buffers (the attempt kernels' invariant, rnde_stage_persist.h: a launch finds buffers 1 and 2 empty and buffer 0 holding some launch's last
// exchange, which whoever exchanges first empties before buffer 0 is used again): phase 1 exchanges through buffer 1 and every workgroup empties ITS entries of
// buffer 0 (their readers finished launches ago); phase 2 exchanges through buffer 0 -- emptied a kernel boundary earlier -- and every workgroup empties its
// entries of buffer 1 (phase 1's exchange: consumed a kernel boundary earlier).  Behind phase 2 buffers 1 and 2 are empty and buffer 0 holds the last exchange:
// the state every launch starts from.  No wait on a clear anywhere: each is followed by a kernel boundary before the buffer is written again.
#pragma once
#include "rnde_bstage.h"
#include "rnde_stage_persist.h"      // PersistSync, slab_put, slab_poll_sum, slab_clear

namespace rnde {

// what a workgroup (row block rb, column tile ct; wg = rb * C + ct in both launch forms) and its lanes are to the two bodies
struct BinitGeo {
    int tid, lane, w, rb, ct, wg, col, gcol, T, r0, KZ, KG;
    bool colok, vec, writer, tile_ok;
    long long A, HB;
    size_t co;
    float *ZL, *GL, *RED;
};
__device__ __forceinline__ BinitGeo binit_geo(const BStageParams& Q, float* smem, int rb, int ct) {
    const StepParams& P = Q.B.F;
    BinitGeo g;
    g.KZ = 16 * Q.KHb + 4; g.KG = 16 * Q.WT + 4;
    g.ZL = smem;                        // [16][KZ]  z1bar (K = hidden), permuted k
    g.GL = g.ZL + kSCB * g.KZ;          // [16][KG]  this block's rows of z2bar, permuted k
    g.RED = g.GL + kSCB * g.KG;         // [32]
    g.tid = threadIdx.x; g.lane = g.tid & 63;
    g.w = __builtin_amdgcn_readfirstlane(g.tid >> 6);
    g.rb = rb; g.ct = ct; g.wg = rb * Q.C + ct;
    g.col = g.lane & 15; g.gcol = ct * kSCB + g.col;
    g.colok = g.gcol < P.B;
    g.vec = (P.D & 3) == 0;
    g.writer = (g.wg == 0 && g.tid == 0);
    g.T = rb * Q.WT + g.w;
    g.r0 = 16 * g.T + 4 * (g.lane >> 4);
    g.tile_ok = g.T < Q.MT;
    g.A = (long long)P.D * P.Bpad; g.HB = (long long)P.H * P.Bpad;
    g.co = (size_t)g.gcol * P.D;
    return g;
}
// the slab buffer a paired phase exchanges through, and the one whose entries it empties (header above)
__device__ __forceinline__ constexpr int binit_pair_buf(int phase) { return phase == 1 ? 1 : 0; }
__device__ __forceinline__ constexpr int binit_pair_clear(int phase) { return phase == 1 ? 0 : 1; }

// A fragments of phases A + B (W1x^T rows of this wave's row tile): requested by the stand-alone STEP 1 / 3 at their start, by a pair in front of its phase D
__device__ __forceinline__ void binit_load_wB(const BStageParams& Q, const BinitGeo& g, f32x4 (&wB)[kSMaxHT]) {
#pragma unroll
    for (int kb = 0; kb < kSMaxHT; ++kb)
        if (kb < Q.KHb && g.tile_ok) wB[kb] = Q.pwBt[((size_t)g.T * Q.KHb + kb) * 64 + g.lane];
}

// ---- STEP 0 (kPhase 1) / STEP 2 (kPhase 2): the phase's scalars, z2bar, phase D.  PAIR: the hbar partials go to the hand-off slab (slab_put) instead of Q.slab.
// f0v_out: the lane's rows of f0, which phases A + B of kPhase 1 need again.
template <int ACT2, int kPhase, bool PAIR>
__device__ __forceinline__ void binit_phase_d(const BStageParams& Q, const PersistSync& Y, const BinitGeo& g, f32x4& f0v_out) {
#pragma clang fp contract(off)
    const BwdParams& Bq = Q.B;
    const StepParams& P = Bq.F;
    const int lane = g.lane, w = g.w, rb = g.rb, ct = g.ct, col = g.col, gcol = g.gcol, r0 = g.r0, KG = g.KG;
    const bool colok = g.colok, vec = g.vec, writer = g.writer, tile_ok = g.tile_ok;
    const long long A = g.A;
    const size_t co = g.co;
    float* GL = g.GL;
    const double N = (double)P.D * (double)P.Bn;
    const InitRec ir = *P.initrec;
    const float dt0 = ir.dt0;
    constexpr int par = kPhase == 1 ? 0 : 1;              // slab parity of the phase
    {
        f32x4 wD[kSMaxW];
#pragma unroll
        for (int kb = 0; kb < kSMaxW; ++kb)
            if (kb < Q.WT && w < Q.HT && rb * Q.WT + kb < Q.MT) wD[kb] = Q.pwDt[((size_t)w * Q.MT + rb * Q.WT + kb) * 64 + lane];
        f32x4 xv = {0.f, 0.f, 0.f, 0.f}, f0v = xv, f1v = xv, ub1 = xv, Uv = xv, K1v = xv;
        if (tile_ok) {
            xv = ld4(P.x + co, r0, P.D, colok, P.xvec != 0);
            f0v = ld4(P.f0 + co, r0, P.D, true, vec);
            f1v = ld4(P.f1 + co, r0, P.D, true, vec);
            if constexpr (kPhase == 2) {
                ub1 = ld4(Bq.UB1 + co, r0, P.D, true, vec);
                Uv = ld4(Bq.U + co, r0, P.D, true, vec);
                K1v = ld4(Bq.K1 + co, r0, P.D, true, vec);
            }
        }
        f0v_out = f0v;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};                 // z2bar of this lane's four rows
        if constexpr (kPhase == 1) {
            // ---- scalars of phase 1 (rnde_binit_kernel, PHASE == 1), identical in every wave ----
            double tb, dtpb, qoldb, t1b, t0b;
            finish_attempt_scalars(Bq, 0, lane, tb, dtpb, qoldb, t1b, t0b);
            const double dtb = Bq.track_initdt ? dtpb : 0.0;
            double dt0b = 0, d1b = 0, d2b = 0;
            if (ir.sel == 2) { t1b += dtb; t0b -= dtb; }
            else if (ir.sel == 0) dt0b += 100.0 * dtb;
            else if (!ir.dt1_const) {
                const double mm = ir.max_is_d2 ? (double)ir.d2 : (double)ir.d1;
                const double mb = dtb * (-0.2) * (double)ir.dt1 / mm;
                if (ir.max_is_d2) d2b += mb; else d1b += mb;
            } else if (dt0 * 1e-3f > 1e-6f) dt0b += 1e-3 * dtb;
            const double n2 = (double)ir.d2 * (double)dt0, n2b = d2b / (double)dt0;
            dt0b += -d2b * (double)ir.d2 / (double)dt0;
            const double coef_w = n2 > 0 ? n2b / (N * n2) : 0.0;
            if (writer) { IBState b; b.tb = tb; b.t1b = t1b; b.t0b = t0b; b.dt0b = dt0b; b.d1b = d1b; b.d2b = d2b; b.coef_w = coef_w; b.pad = 0; Bq.ibstate[0] = b; }
            const float cw = (float)coef_w;
            if (tile_ok) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float sk = P.abstol + fabsf(xv[i]) * P.reltol;
                    const float wv = (f1v[i] - f0v[i]) / sk;
                    const float f1b = (colok && r0 + i < P.D ? cw * wv : 0.f) / sk;
                    v[i] = ACT2 ? f1b * (1.f - f1v[i] * f1v[i]) : f1b;
                }
                st4(Bq.zi2 + A + co, r0, P.D, true, vec, v);
            }
        } else {
            // ---- scalars of phase 2 (rnde_binit_kernel, PHASE == 2) ----
            const IBState ib = Bq.ibstate[0];
            double dot1 = 0, tau1 = 0;
            for (int i = lane; i < P.nwg; i += 64) { dot1 += (double)Bq.ipart[4 * i]; tau1 += (double)Bq.ipart[4 * i + 1]; }
            dot1 = wave_sum_d(dot1); tau1 = wave_sum_d(tau1);
            double dt0b = ib.dt0b + tau1 + dot1, t0b = ib.t0b + tau1, t1b = ib.t1b, d1b = ib.d1b, d0b = 0;
            if (ir.dt0_clamped) { t1b += dt0b; t0b -= dt0b; }
            else if (!ir.dt0_const) { d0b = dt0b / (100.0 * (double)ir.d1); d1b += -dt0b * (double)dt0 / (double)ir.d1; }
            const float cv = ir.d1 > 0.f ? (float)(d1b / (N * (double)ir.d1)) : 0.f;
            const float cz = ir.d0 > 0.f ? (float)(d0b / (N * (double)ir.d0)) : 0.f;
            const float cw = (float)ib.coef_w;
            if (writer) { IBState b = ib; b.t1b = t1b; b.t0b = t0b; Bq.ibstate[1] = b; }
            if (tile_ok) {
                f32x4 u0b = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool ok = colok && r0 + i < P.D;
                    const float sk = P.abstol + fabsf(xv[i]) * P.reltol;
                    const float wv = (f1v[i] - f0v[i]) / sk, vv = f0v[i] / sk, z = xv[i] / sk;
                    const float wb = ok ? cw * wv : 0.f, vb = ok ? cv * vv : 0.f, zb = ok ? cz * z : 0.f;
                    const float skb = -(wb * wv + vb * vv + zb * z) / sk;
                    const float f0b = K1v[i] + dt0 * ub1[i] + (vb - wb) / sk;
                    u0b[i] = Uv[i] + ub1[i] + zb / sk + skb * P.reltol * sgnf(xv[i]);
                    if (Bq.sv_ubar0 && ok) u0b[i] += Bq.sv_ubar0[((size_t)gcol * Bq.sv_T) * P.D + r0 + i];
                    v[i] = ACT2 ? f0b * (1.f - f0v[i] * f0v[i]) : f0b;
                }
                st4(Bq.zi2 + co, r0, P.D, true, vec, v);
                st_tile(Bq.xbar + co, r0, P.D, colok, false, u0b);      // the direct part of x-bar; STEP 3 adds the part through f0
            }
        }
        // ---- phase D: hbar partial (and layer-2 time row) of this row block -> slab[par] (PAIR: -> the hand-off slab) ----
#pragma unroll
        for (int i = 0; i < 4; ++i) GL[col * KG + kperm(16 * w + 4 * (lane >> 4) + i)] = tile_ok ? v[i] : 0.f;
        __syncthreads();
        f32x4* sl = (f32x4*)Q.slab + ((((size_t)par * Q.C + ct) * Q.R + rb) * Q.HT) * 64;
        const size_t tile0 = (((size_t)binit_pair_buf(kPhase) * Q.C + ct) * Q.R + rb) * Q.HT;
        const float* gbp = GL + col * KG + 4 * (lane >> 4);
        f32x4 bg[kSMaxW];
#pragma unroll
        for (int kb = 0; kb < kSMaxW; ++kb) if (kb < Q.WT) bg[kb] = *(const f32x4*)(gbp + 16 * kb);
        if (w < Q.HT) {
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < kSMaxW; ++kb) {
                if (kb < Q.WT && rb * Q.WT + kb < Q.MT) {
                    acc0 = mfma16(wD[kb][0], bg[kb][0], acc0);
                    acc1 = mfma16(wD[kb][1], bg[kb][1], acc1);
                    acc0 = mfma16(wD[kb][2], bg[kb][2], acc0);
                    acc1 = mfma16(wD[kb][3], bg[kb][3], acc1);
                }
            }
            if constexpr (PAIR) slab_put(Y.tslab, tile0 + w, lane, acc0 + acc1);
            else sl[(size_t)w * 64 + lane] = acc0 + acc1;
        }
        for (int ht = w + Q.WT; ht < Q.HT; ht += Q.WT) {
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < kSMaxW; ++kb) {
                if (kb < Q.WT && rb * Q.WT + kb < Q.MT) {
                    const f32x4 a = Q.pwDt[((size_t)ht * Q.MT + rb * Q.WT + kb) * 64 + lane];
                    acc0 = mfma16(a[0], bg[kb][0], acc0);
                    acc1 = mfma16(a[1], bg[kb][1], acc1);
                    acc0 = mfma16(a[2], bg[kb][2], acc0);
                    acc1 = mfma16(a[3], bg[kb][3], acc1);
                }
            }
            if constexpr (PAIR) slab_put(Y.tslab, tile0 + ht, lane, acc0 + acc1);
            else sl[(size_t)ht * 64 + lane] = acc0 + acc1;
        }
    }
}

// ---- STEP 1 (kPhase 1) / STEP 3 (kPhase 2): phases A + B of the evaluation (f1 at (u1, t0 + dt0): hidden activations h1; f0 at (u0, t0): h0) and the
// workgroup's partial sums.  PAIR: the sum over the row blocks' partials is the poll of the hand-off (slab_poll_sum: from zero, r = 0 .. R - 1, as the loop over
// Q.slab), and the workgroup empties its entries of the other buffer (header above).  A hand-off that times out raises the abort word and leaves zeros: the
// workgroup finishes (nothing waits behind this poll) and the host, which looks at that word behind every reverse pass, refuses the result.
template <int ACT2, int kPhase, bool PAIR>
__device__ __forceinline__ void binit_phase_ab(const BStageParams& Q, const PersistSync& Y, const BinitGeo& g, const f32x4 (&wB)[kSMaxHT], const f32x4& f0v) {
#pragma clang fp contract(off)
    const BwdParams& Bq = Q.B;
    const StepParams& P = Bq.F;
    const int tid = g.tid, lane = g.lane, w = g.w, rb = g.rb, ct = g.ct, wg = g.wg, col = g.col, gcol = g.gcol, r0 = g.r0, KZ = g.KZ;
    const bool colok = g.colok, vec = g.vec, tile_ok = g.tile_ok;
    const long long HB = g.HB;
    const size_t co = g.co;
    float* ZL = g.ZL; float* RED = g.RED;
    constexpr int par = kPhase == 1 ? 0 : 1;
    float dot = 0.f, tau = 0.f;
    {
        const float* hsrc = kPhase == 1 ? P.h1 : P.h0;
        float* z1dst = kPhase == 1 ? Bq.zi1 + HB : Bq.zi1;
        const float* W1t = Q.p + (size_t)P.H * P.D;
        const f32x4* sl = (const f32x4*)Q.slab + (((size_t)par * Q.C + ct) * Q.R) * Q.HT * 64;
        const size_t tclr0 = (((size_t)binit_pair_clear(kPhase) * Q.C + ct) * Q.R + rb) * Q.HT;
        for (int ht = w; ht < Q.HT; ht += Q.WT) {
            f32x4 z = {0.f, 0.f, 0.f, 0.f};
            if constexpr (PAIR) {
                if (slab_poll_sum(Y, binit_pair_buf(kPhase), Q.C, Q.R, Q.HT, ct, ht, lane, z)) slab_clear(Y.tslab, tclr0 + ht, lane);
            } else {
                for (int r = 0; r < Q.R; ++r) z += sl[((size_t)r * Q.HT + ht) * 64 + lane];
            }
            const int h0 = 16 * ht + 4 * (lane >> 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int hr = h0 + i;
                float zv = 0.f;
                if (hr < P.H) {
                    const float hv = hsrc[(size_t)gcol * P.H + hr];
                    zv = z[i] * (1.f - hv * hv);
                    if (rb == 0) { z1dst[(size_t)gcol * P.H + hr] = zv; tau += W1t[hr] * zv; }
                } else if (hr == P.H) {
                    if (rb == 0) tau += z[i];          // layer-2 time cotangent (row H of [W2x^T; w2t^T] z2bar)
                }
                if (hr < 16 * Q.KHb) ZL[col * KZ + kperm(hr)] = zv;
            }
        }
        if (Q.KHb > Q.HT) {
            for (int i = tid; i < kSCB * 16 * Q.KHb; i += blockDim.x) {
                const int c = i / (16 * Q.KHb), k = i - c * 16 * Q.KHb;
                if (k >= 16 * Q.HT) ZL[c * KZ + kperm(k)] = 0.f;
            }
        }
        __syncthreads();
        f32x4 gb = {0.f, 0.f, 0.f, 0.f};
        if (tile_ok) {
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            const float* zb = ZL + col * KZ + 4 * (lane >> 4);
            f32x4 bf[kSMaxHT];
#pragma unroll
            for (int kb = 0; kb < kSMaxHT; ++kb) if (kb < Q.KHb) bf[kb] = *(const f32x4*)(zb + 16 * kb);
#pragma unroll
            for (int kb = 0; kb < kSMaxHT; ++kb) {
                if (kb < Q.KHb) {
                    acc0 = mfma16(wB[kb][0], bf[kb][0], acc0);
                    acc1 = mfma16(wB[kb][1], bf[kb][1], acc1);
                    acc0 = mfma16(wB[kb][2], bf[kb][2], acc0);
                    acc1 = mfma16(wB[kb][3], bf[kb][3], acc1);
                }
            }
            gb = acc0 + acc1;
#pragma unroll
            for (int i = 0; i < 4; ++i) if (r0 + i >= P.D) gb[i] = 0.f;
            if constexpr (kPhase == 1) {
                st4(Bq.UB1 + co, r0, P.D, true, vec, gb);
#pragma unroll
                for (int i = 0; i < 4; ++i) dot += gb[i] * f0v[i];
            } else {
                const f32x4 u0b = ld_tile(Bq.xbar + co, r0, P.D, colok, false);    // (written by STEP 2 of this same lane's counterpart: same rows, same column)
                st_tile(Bq.xbar + co, r0, P.D, colok, false, u0b + gb);
            }
        }
        if (!colok) tau = 0.f;
        dot = wave_sum_f(dot); tau = wave_sum_f(tau);
        __syncthreads();
        if (lane == 0) { RED[w] = dot; RED[8 + w] = tau; }
        __syncthreads();
        if (tid == 0) {
            float sa = 0.f, ta = 0.f;
            for (int i = 0; i < Q.WT; ++i) { sa += RED[i]; ta += RED[8 + i]; }
            if constexpr (kPhase == 1) { float* o = Bq.ipart + (size_t)wg * 4; o[0] = sa; o[1] = ta; o[2] = 0.f; o[3] = 0.f; }
            else { float* o = Bq.ipart + ((size_t)P.nwg + wg) * 4; o[0] = ta; o[1] = 0.f; o[2] = 0.f; o[3] = 0.f; }
        }
    }
}

// the four stand-alone launches (the fallback of the pairs, RNDE_PERSIST=0, RNDE_BINIT_PAIR=0): workgroup blockIdx.x = rb * C + ct
template <int ACT2, int STEP>
__global__ __launch_bounds__(64 * kSMaxW) void rnde_binit_stage_kernel(const BStageParams Q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int rb = blockIdx.x / Q.C, ct = blockIdx.x - rb * Q.C;
    const BinitGeo g = binit_geo(Q, smem, rb, ct);
    constexpr int kPhase = STEP < 2 ? 1 : 2;
    const PersistSync none{};
    f32x4 f0v = {0.f, 0.f, 0.f, 0.f};
    if constexpr (STEP == 0 || STEP == 2) {      // the launches that end in phase D
        binit_phase_d<ACT2, kPhase, false>(Q, none, g, f0v);
    } else {
        const StepParams& P = Q.B.F;
        f32x4 wB[kSMaxHT];
        binit_load_wB(Q, g, wB);
        if (kPhase == 1 && g.tile_ok) f0v = ld4(P.f0 + g.co, g.r0, P.D, true, g.vec);
        binit_phase_ab<ACT2, kPhase, false>(Q, none, g, wB, f0v);
    }
}

// STEP 0 + STEP 1 (PHASE 1) or STEP 2 + STEP 3 (PHASE 2) as one launch: grid 8 * R * ceil(C / 8), the attempt kernel's (rb, ct) decoding (rnde_stage_persist.h)
template <int ACT2, int PHASE>
__global__ __launch_bounds__(64 * kSMaxW) void rnde_binit_pair_kernel(const BStageParams Q, const PersistSync Y) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int rb = (blockIdx.x >> 3) % Q.R, ct = 8 * ((blockIdx.x >> 3) / Q.R) + (blockIdx.x & 7);
    if (ct >= Q.C) return;
    const BinitGeo g = binit_geo(Q, smem, rb, ct);
    if (g.tid == 0) Y.xcc[g.wg] = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 15;      // (as the attempt kernels: the host checks that a column tile sits on one XCD)
    f32x4 wB[kSMaxHT];
    binit_load_wB(Q, g, wB);      // both phases' weights are in flight before the first of them is multiplied
    f32x4 f0v;
    binit_phase_d<ACT2, PHASE, true>(Q, Y, g, f0v);
    binit_phase_ab<ACT2, PHASE, true>(Q, Y, g, wB, f0v);
}

}  // namespace rnde
