// rnde_bnode_tile.h -- the reverse sweep of rnde_node_tile_solve_kernel: discretise-then-optimise through every Tsit5 stage of every accepted
// step, one workgroup per tile, one launch.
//
// The default sweep (rnde_node_tile_reverse_kernel<false>) treats step sizes and times as constants (track_ctrl = track_initdt = 0): once
// the step log is fixed no column depends on another, the cotangent of a saved value EEst * dt reaches the stages through EEst, whose value
// comes from the step log, and no tile meets another.
//
// The tracked sweep (<true>, rnde_node_set_tracking) restates rnde_ffjord_tile_reverse_kernel<Dyn, KIN, true> for a state of D rows: it walks
// ATTEMPTS, last to first; every tile carries the cotangents of (t, the proposed dt, qold) and of the span (t0, t1) in double registers and
// computes them identically.  A rejected attempt recomputes its stages from the uprev it shares with the accepted attempt behind it, has no
// unew cotangent and ADDS to the running uprev cotangent.  The cotangent of dt needs three sums over the whole batch (sum <k_j, k_j-bar>,
// sum tau_s, sum c_s tau_s with tau_s = <df/dt at stage s, k_s-bar>): one tile_meet per attempt, in tile order in double, under the solve's
// launch placement (one XCD up to 32 tiles, agent scope above).  Behind attempt 0 the proposed dt is the initial-step rule's (track_initdt):
// f0, u1 = x + dt0 f0 and f1 are recomputed, two VJPs and two more meetings reverse it (rnde_track_rec.h has the scalars).  The cotangent of
// t in front of attempt 0 and the clamps (dt = t1 - t, dtp' = t1 - t0) give (t0-bar, t1-bar).
//
// The stages are recomputed from the taped uprev with the forward's own evaluation (NtDyn::eval).  One stage's VJP, cotangent kb of
// f(y, t), notation of rnde_ffjordc.h (d_l = phi_l' taken from the layer's output):
//     v_n = d_n .* kb,   v_l = d_l .* W_{l+1}' v_{l+1},   yb += W_1' v_1
//     W_l-bar += v_l y_{l-1}',   wt_l-bar += t sum_c v_l,   b_l-bar += sum_c v_l        (outer products over the tile's 16 columns)
// The transposed products are ft_tr, the outer products one v_mfma_f32_16x16x4_f32 chain per 16 x 16 block of W_l (k = the 16 columns).
// Parameter cotangents accumulate in the tile's own row of pacc ([ntiles][P]) by plain read-modify-write: every entry has one owner lane
// for the whole sweep, no atomics; rnde_node_tile_reduce_kernel then sums the tiles in tile order in double (the arithmetic of
// rnde_ffjordt_reduce_kernel, restated here: that header defines kernels only one translation unit may hold).
#pragma once
#include "rnde_node_tile.h"

namespace rnde {

// dW[o][i] += sum_c A[o][c] Bm[i][c] (both [feature][16]) into pw[i * out + o]; output blocks dealt to the waves
__device__ __forceinline__ void nt_wgrad(const float* A, const float* Bm, int outp, int inp, int out, int in, float* pw, int wave, int lane) {
    const int c = lane & 15, g = lane >> 4, nti = inp >> 4, nt = (outp >> 4) * nti;
    for (int tt = wave; tt < nt; tt += kFtWaves) {
        const int mo = tt / nti, mi = tt - mo * nti;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int ao = (16 * mo + c) * 16 + g, bo = (16 * mi + c) * 16 + g;
#pragma unroll
        for (int kc = 0; kc < 16; kc += 4) acc = mfma16(A[ao + kc], Bm[bo + kc], acc);
        const int i = 16 * mi + c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = 16 * mo + 4 * g + j;
            if (o < out && i < in) pw[(size_t)i * out + o] += acc[j];
        }
    }
}

// yb[0:D] += (df/dy)' kb and pacc += (df/dp)' kb at the stage input y ([D][16]) for the tile's 16 columns.  Every thread of the workgroup
// calls it; ends behind a barrier.  TAU (the tracked sweep): returns the calling thread's share of <df/dt, kb> over the tile's columns,
// sum_l sum_o wt_l[o] sum_c v_l[o][c], from the per-output column sums formed for the bias anyway (zero for a plain Chain), and adds its share
// of <f(y, t), kb> to kdot: the chain's last output, recomputed here in LDS, is f itself, and kb is read for v_n anyway, so the sum
// <k_s, k_s-bar> of the dt cotangent costs no pass over global memory.  Without TAU the function returns 0 and forms neither.
template <bool TAU = false>
__device__ __forceinline__ float nt_vjp(const FcGeo& G, const NtLds& L, float t, const float* y, const float* kb, float* yb, float* pacc, int tid,
                                        float* kdot = nullptr) {
    const int lane = tid & 63, wave = tid >> 6, c = lane & 15, D = G.D, n = G.n;
    float tsum = 0.f;
    for (int idx = tid; idx < D * 16; idx += kFtThreads) L.X[idx] = y[idx];      // (rows >= D of L.X are zero and stay so)
    __syncthreads();
    fc_chain(G, L.W, L.X, L.Y, t, wave, lane, [](int, int, float) {});
    float *va = L.V0, *vb = L.V1;
    {
        const float* yn = L.Y + G.yoff[n - 1];
        const int code = G.act[n - 1];
        if constexpr (TAU) {
            float kd = 0.f;
            for (int idx = tid; idx < G.outp[n - 1] * 16; idx += kFtThreads) {
                float v = 0.f;
                if ((idx >> 4) < D) { const float f = yn[idx], b = kb[idx]; v = act_dy(code, f) * b; kd = fmaf(f, b, kd); }
                va[idx] = v;
            }
            if (kdot) *kdot += kd;
        } else {
            for (int idx = tid; idx < G.outp[n - 1] * 16; idx += kFtThreads) va[idx] = (idx >> 4) < D ? act_dy(code, yn[idx]) * kb[idx] : 0.f;
        }
    }
    __syncthreads();
    for (int l = n - 1; l >= 0; --l) {      // layer l (0-based): input y_{l-1} (L.X for l = 0), cotangent of its pre-activation in va
        const int in = G.dims[l], out = G.dims[l + 1];
        const float* yin = l ? L.Y + G.yoff[l - 1] : L.X;
        float* pl = pacc + G.off[l];
        nt_wgrad(va, yin, G.outp[l], G.inp[l], out, in, pl, wave, lane);
        for (int o = tid; o < out; o += kFtThreads) {
            float s = 0.f;
            for (int k = 0; k < 16; ++k) s += va[o * 16 + k];
            if (G.td) {
                pl[in * out + o] += t * s;
                if constexpr (TAU) tsum = fmaf(L.W[G.voff[l] + o], s, tsum);
            }
            pl[(in + G.td) * out + o] += s;
        }
        if (l > 0) {
            const int code = G.act[l - 1];
            ft_tr(L.W + G.woff[l], G.ld[l], G.inp[l], G.outp[l], va, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int ix = (r0 + j) * 16 + c; vb[ix] = v[j] * act_dy(code, yin[ix]); }
            });
        } else {
            ft_tr(L.W + G.woff[0], G.ld[0], G.inp[0], G.outp[0], va, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int r = r0 + j; if (r < D) yb[r * 16 + c] += v[j]; }
            });
        }
        __syncthreads();
        float* s = va; va = vb; vb = s;
    }
    return tsum;
}

// TRK: the tracked sweep (the header); launched as the solve is (MeetRes::grid), one loop iteration per attempt, then the initial step.
// SAVE: a saving tape.  The only outputs are the saved points: the running uprev cotangent starts at zero, and behind the seeds of an
// accepted attempt the cotangent of each of its save indices (Q.rng, formed on the host by save_plan) enters -- at the step's end into the
// unew cotangent, inside the step into the uprev cotangent and, times dt b_j(theta), into every stage cotangent (the reverse of the dense
// output, rnde_bchain.h).  TRK adds the theta terms to the attempt's sums: -<u_s-bar, sum_j b_j'(theta) k_j> to the t sum and theta times it
// to the dt sum (theta = (ts - t) / dt); the dt b_j part of the dt cotangent is in sum <k_j, k_j-bar> already.  The meeting carries them:
// no meeting is added.  The cotangent of index 0 under save_start goes straight to x-bar.
template <bool TRK = false, bool SAVE = false>
__global__ __launch_bounds__(kFtThreads) void rnde_node_tile_reverse_kernel(const NodeTileRevParams Q) {
    extern __shared__ float nt_smem[];
    const FcGeo& G = Q.G;
    if constexpr (TRK)
        if (!Q.meet.global && (int)(blockIdx.x & 7) != Q.xcd_slot) return;
    const int tile = (TRK && !Q.meet.global) ? (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    const int tid = threadIdx.x, D = G.D, Bp = Q.Bp, col0 = tile * 16, nel = D * 16;
    if constexpr (TRK)
        if (!Q.meet.global && tid == 0) Q.xcc[tile] = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 15;
    const NtLds L = NtDyn::lds(G, nt_smem);
    FcDyn::load_params(G, Q.p, L.W, tid);
    for (int idx = tid; idx < G.DP * 16; idx += kFtThreads) L.X[idx] = 0.f;
    float* ws = Q.ws + (size_t)tile * NtDyn::rev_ws_floats(G);
    const size_t RS = (size_t)nel;
    auto Ys = [&](int s) { return ws + (size_t)s * RS; };
    auto Ks = [&](int s) { return ws + (size_t)(7 + s) * RS; };
    auto Kb = [&](int s) { return ws + (size_t)(14 + s) * RS; };
    float *UB = ws + 21 * RS, *UBn = ws + 22 * RS, *Yb = ws + 23 * RS;
    float* pacc = Q.pacc + (size_t)tile * G.P;
    for (int q = tid; q < G.P; q += kFtThreads) pacc[q] = 0.f;
    const size_t RB = (size_t)D * Bp;
    for (int idx = tid; idx < nel; idx += kFtThreads) {
        const int r = idx >> 4, col = col0 + (idx & 15);
        UB[idx] = (!SAVE && col < Q.B) ? Q.u_bar[(size_t)col * D + r] : 0.f;
    }
    __syncthreads();      // pacc and L.X are next touched by other threads (the entries' owner lanes, the stage loop)
    const double N = (double)D * (double)Q.B;
    double tb = 0.0, dtpb = 0.0, qoldb = 0.0, t1b = 0.0, t0b = 0.0;      // TRK: the cotangents of (t, the proposed dt, qold) behind attempt n, of the span
    for (int n = (TRK ? Q.n_att : Q.n_acc) - 1; n >= 0; --n) {
        NtStepRec st;
        FfAttRec a;                   // TRK: the attempt's record, loaded once
        int flags = F_ACCEPT, urec = n;
        if constexpr (TRK) { a = Q.att[n]; st.t = a.t; st.dt = a.dt; st.eest = a.eest; st.svb = 0.f; flags = a.flags; urec = a.rec; }
        else st = Q.rec[n];
        const float t = st.t, dt = st.dt;
        const bool accepted = (flags & F_ACCEPT) != 0;
        const float* U = Q.tape + (size_t)urec * RB + col0;
        // ---- recompute the stages ----
        for (int s = 0; s < 7; ++s) {
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const int r = idx >> 4, c = idx & 15;
                float acc = 0.f;
                for (int j = 0; j < s; ++j) acc = fmaf(tsA_rt(s, j), Ks(j)[idx], acc);
                const float y = U[(size_t)r * Bp + c] + dt * acc;
                Ys(s)[idx] = y;
                L.X[idx] = y;
            }
            NtDyn::eval(G, L, t + kTsC[s] * dt, Ks(s), 16, tid);
        }
        for (int idx = tid; idx < nel; idx += kFtThreads) {
            for (int s = 0; s < 7; ++s) Kb(s)[idx] = 0.f;
            UBn[idx] = 0.f;
            Yb[idx] = accepted ? UB[idx] : 0.f;               // cotangent of unew = stage-7 input (a rejected attempt has none)
        }
        float pS = 0.f, ptau = 0.f, pctau = 0.f;              // TRK: this thread's shares of the three sums of the dt cotangent
        if constexpr (SAVE) {         // ---- the saved points of this step (every array below is touched by its entry's owner thread alone) ----
            const SaveRange rg = Q.rng[n];
            for (int si = rg.lo; si < rg.hi; ++si) {
                const float ts = Q.sv_t[si], th = (ts - t) / dt;
                const bool at_end = ts == t + dt;
                float bw[7], dbw[7];
                dense_weights(th, bw);
                if constexpr (TRK) dense_weights_deriv(th, dbw);
                for (int idx = tid; idx < nel; idx += kFtThreads) {
                    const int r = idx >> 4, col = col0 + (idx & 15);
                    if (col >= Q.B) continue;
                    const float ub = Q.u_bar[((size_t)col * Q.nsave + si) * D + r];
                    if (at_end) { Yb[idx] += ub; continue; }
                    UBn[idx] += ub;
#pragma unroll
                    for (int j = 0; j < 7; ++j) Kb(j)[idx] += dt * bw[j] * ub;      // (unrolled: bw, dbw stay in registers)
                    if constexpr (TRK) {
                        float dacc = dbw[0] * Ks(0)[idx];
#pragma unroll
                        for (int j = 1; j < 7; ++j) dacc += dbw[j] * Ks(j)[idx];
                        const float v = -ub * dacc;
                        ptau += v; pctau = fmaf(th, v, pctau);
                    }
                }
            }
        }
        // ---- TRK: the scalar reverse of the controller (FfAttRec); dtp' = t1 - t0 under F_DTMAXCLAMP ----
        double eb = 0.0, dtb_pre = 0.0, qoldb_in = 0.0;
        if constexpr (TRK) {
            eb = a.e0 + a.e_dtp * dtpb + a.e_q * qoldb;
            dtb_pre = a.d0 + a.d_t * tb + a.d_dtp * dtpb;
            qoldb_in = a.c_dtp * dtpb + a.c_q * qoldb;
            if (accepted && (flags & F_DTMAXCLAMP)) { t1b += dtpb; t0b -= dtpb; }
        }
        // ---- A: reverse of the error estimate (the saved value EEst * dt; rnde_ffjord_tile.h.  TRK: every attempt, with the coefficient eb) ----
        if (TRK ? (eb != 0.0 && st.eest > 0.f) : (st.svb != 0.f && st.eest > 0.f)) {
            const float coef = TRK ? (float)(eb / (N * (double)st.eest)) : (float)(((double)st.svb * (double)dt) / (N * (double)st.eest));
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                if (col0 + (idx & 15) >= Q.B) continue;
                float E = 0.f;
                for (int j = 0; j < 7; ++j) E += kTsBt[j] * Ks(j)[idx];
                const float up = U[(size_t)(idx >> 4) * Bp + (idx & 15)], un = Ys(6)[idx];
                const float au = fabsf(up), an = fabsf(un);
                const bool use_new = !(au > an);
                const float sk = Q.abstol + (use_new ? an : au) * Q.reltol;
                const float rr = dt * E / sk, rb = coef * rr, utb = rb / sk, skb = -rb * rr / sk;
                for (int j = 0; j < 7; ++j) Kb(j)[idx] += dt * kTsBt[j] * utb;
                if (use_new) Yb[idx] += skb * Q.reltol * (un > 0.f ? 1.f : (un < 0.f ? -1.f : 0.f));
                else UBn[idx] += skb * Q.reltol * (up > 0.f ? 1.f : (up < 0.f ? -1.f : 0.f));
            }
        }
        __syncthreads();
        // ---- B: the stages, last to first ----
        for (int s = 6; s >= 0; --s) {
            if (s != 6) {
                for (int idx = tid; idx < nel; idx += kFtThreads) Yb[idx] = 0.f;
                __syncthreads();
            }
            if constexpr (TRK) {      // (k_s-bar is complete here: nt_vjp adds <k_s, k_s-bar> to pS as it reads it)
                const float ts = nt_vjp<true>(G, L, t + kTsC[s] * dt, Ys(s), Kb(s), Yb, pacc, tid, &pS);
                ptau += ts; pctau = fmaf(kTsC[s], ts, pctau);
            } else {
                nt_vjp(G, L, t + kTsC[s] * dt, Ys(s), Kb(s), Yb, pacc, tid);
            }
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const float y = Yb[idx];
                UBn[idx] += y;
                for (int j = 0; j < s; ++j) Kb(j)[idx] += dt * tsA_rt(s, j) * y;
            }
            __syncthreads();
        }
        for (int idx = tid; idx < nel; idx += kFtThreads) UB[idx] = accepted ? UBn[idx] : UB[idx] + UBn[idx];
        __syncthreads();
        if constexpr (TRK) {          // the meeting, then the scalar tail (finish_attempt_scalars_sums, rnde_bwd.h): dt = min(dtp, t1 - t), t' = t + dt
            double xs[3];
            if (!tile_meet(Q.meet, L.red, n, pS, ptau, pctau, xs, tile, tid)) return;
            const double dtb = dtb_pre + xs[0] / (double)dt + xs[2];
            tb += xs[1];
            if (flags & F_CLAMP) { t1b += dtb; tb -= dtb; dtpb = 0.0; } else dtpb = dtb;
            qoldb = qoldb_in;
        }
    }
    if constexpr (TRK) {
        if (Q.track_initdt) {         // ---- the initial-step rule behind attempt 0 (rnde_bchain_init_kernel's two phases; scalars: rnde_track_rec.h) ----
            const InitRec& ir = Q.init;
            const float dt0 = ir.dt0, rt = Q.reltol, at = Q.abstol;
            const float* X0 = Q.tape + col0;                  // tape record 0: x (padded columns zero)
            const InitBar1 b1 = init_rev_phase1(ir, dtpb, N);
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const float xv = X0[(size_t)(idx >> 4) * Bp + (idx & 15)];
                Ys(0)[idx] = xv;
                L.X[idx] = xv;
            }
            NtDyn::eval(G, L, Q.t0 + 0.f, Ks(0), 16, tid);                   // f0 = f(x, t0)
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const float y = Ys(0)[idx] + dt0 * Ks(0)[idx];
                Ys(1)[idx] = y;
                L.X[idx] = y;
            }
            NtDyn::eval(G, L, Q.t0 + dt0, Ks(1), 16, tid);                   // f1 = f(u1, t0 + dt0)
            const float cw = (float)b1.coef_w;
            for (int idx = tid; idx < nel; idx += kFtThreads) {              // phase 1: f1-bar = coef_w (f1 - f0) / sk^2
                float f1b = 0.f;
                if (col0 + (idx & 15) < Q.B) { const float sk = at + fabsf(Ys(0)[idx]) * rt; f1b = cw * ((Ks(1)[idx] - Ks(0)[idx]) / sk) / sk; }
                Kb(1)[idx] = f1b;
                Yb[idx] = 0.f;
            }
            __syncthreads();
            float ptau = nt_vjp<true>(G, L, Q.t0 + dt0, Ys(1), Kb(1), Yb, pacc, tid);
            float pdot = 0.f;
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const float g = Yb[idx];                                     // u1-bar
                UBn[idx] = g;
                pdot = fmaf(g, Ks(0)[idx], pdot);
            }
            double xs[3];
            if (!tile_meet(Q.meet, L.red, Q.n_att, pdot, ptau, 0.f, xs, tile, tid)) return;
            const InitBar2 b2 = init_rev_phase2(ir, b1, xs[0], xs[1]);
            t0b += b2.t0b; t1b += b2.t1b;
            const float cv = ir.d1 > 0.f ? (float)(b2.d1b / (N * (double)ir.d1)) : 0.f;
            const float cz = ir.d0 > 0.f ? (float)(b2.d0b / (N * (double)ir.d0)) : 0.f;
            for (int idx = tid; idx < nel; idx += kFtThreads) {              // phase 2: f0-bar = dt0 u1-bar + (v-bar - w-bar) / sk, the x-bar terms of the three norms
                const float xv = Ys(0)[idx], f0 = Ks(0)[idx], ub1 = UBn[idx];
                float f0b = dt0 * ub1, u0b = UB[idx] + ub1;
                if (col0 + (idx & 15) < Q.B) {
                    const float sk = at + fabsf(xv) * rt;
                    const float w = (Ks(1)[idx] - f0) / sk, v = f0 / sk, z = xv / sk;
                    const float wb = cw * w, vb = cv * v, zb = cz * z;
                    const float skb = -(wb * w + vb * v + zb * z) / sk;
                    f0b += (vb - wb) / sk;
                    u0b += zb / sk + skb * rt * (xv > 0.f ? 1.f : (xv < 0.f ? -1.f : 0.f));
                }
                Kb(0)[idx] = f0b;
                UB[idx] = u0b;
                Yb[idx] = 0.f;
            }
            __syncthreads();
            ptau = nt_vjp<true>(G, L, Q.t0 + 0.f, Ys(0), Kb(0), Yb, pacc, tid);
            for (int idx = tid; idx < nel; idx += kFtThreads) UB[idx] += Yb[idx];
            if (!tile_meet(Q.meet, L.red, Q.n_att + 1, ptau, 0.f, 0.f, xs, tile, tid)) return;
            t0b += xs[0];
        }
        if (tile == 0 && tid == 0) { Q.tspan_out[0] = t0b + tb; Q.tspan_out[1] = t1b; }      // t-bar in front of attempt 0 is t0's
    }
    if (Q.x_bar)
        for (int idx = tid; idx < nel; idx += kFtThreads) {
            const int r = idx >> 4, col = col0 + (idx & 15);
            if (col >= Q.B) continue;
            float v = UB[idx];
            if constexpr (SAVE)
                if (Q.save_t0) v += Q.u_bar[((size_t)col * Q.nsave) * D + r];
            Q.x_bar[(size_t)col * D + r] = v;
        }
}

// p_bar[q] = sum over tiles of pacc[tile][q], in tile order, carried in double
static __global__ __launch_bounds__(256) void rnde_node_tile_reduce_kernel(const float* __restrict__ pacc, int P, int ntiles, float* __restrict__ p_bar) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= P) return;
    double s = 0.0;
    for (int t = 0; t < ntiles; ++t) s += (double)pacc[(size_t)t * P + q];
    p_bar[q] = (float)s;
}

}  // namespace rnde
