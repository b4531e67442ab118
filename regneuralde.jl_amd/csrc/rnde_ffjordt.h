// rnde_ffjordt.h -- the tiled TrackedFFJORD engine (rnde_ffjord_create_tiled): the ConcatSquash dynamics of rnde_ffjord.h at widths the
// one-workgroup engine does not serve (the tabular experiment's 43 -> 100), with the layer products on the matrix cores.
//
// Geometry (rnde_chainmw.h's layout): one workgroup of four waves per 16 batch columns (a tile).  The padded parameters stay resident in LDS,
// each layer's weights as Wl[in][ld] (ld = outp + 1: the transposed products read rows, the forward products columns, neither conflicts),
// zero outside the layer.  Activations live in LDS as [feature][16 columns]; a layer product is v_mfma_f32_16x16x4_f32 (exact fp32
// products), wave w owning output tiles w, w + 4, ...; its epilogue applies gate / shift / softplus in registers and writes the next
// activation.  Padded feature rows are written as zero by every epilogue, padded columns of a partial last tile carry zero probes and zero
// cotangents and are left out of every norm.
//
// Forward solve (rnde_ffjordt_solve_kernel): the whole adaptive Tsit5 solve in one launch.  The Runge-Kutta state is [R][Bp] in global memory
// (R = D + 1 augmented rows, each tile touching its own 16 columns).  Once per attempt every tile forms its partial of the error norm and the
// tiles meet through rnde_chainmw.h's bounded mw_exchange3 (one XCD up to 32 tiles, agent scope above): partials are summed in tile order in
// double, so every tile runs the same controller (advance_state_t over R rows) on the same bits, and a solve is bit-identical run to run.
// A meeting that times out raises the abort word and ends the launch; the host reports it by name.
//
// Exact trace (sample, feval exact): with a1 = sig(h1) .* g1, a2 = sig(h2) .* g2,
//     tr J = a2' (W2 .* M') a1,   M(t) = W1 diag(g3(t)) W3   (H x H)
// Each tile forms QT = (W2 .* M')' once per evaluation on the matrix cores into a tile-private global buffer; each column then costs one
// H x H product.
//
// Kinetic variant (template parameter KIN; rnde_ffjord.h): R = D + 3 rows, the two regulariser rates sum f^2 and sum eJ^2 formed where the
// trace is formed -- per-lane partials in the epilogues of the layer-3 product and of the last transposed product, then the same per-column
// reduction.  No LDS beyond the plain kernels' (135 KB at (43, 100)), so the limits are the plain ones: in_dims <= 64, hidden <= 112.
#pragma once
#include "rnde_chainmw.h"     // MwMeet, mw_exchange3, kMwMeetMax, mfma16
#include "rnde_ffjord.h"

namespace rnde {

constexpr int kFtWaves = 4;
constexpr int kFtThreads = 64 * kFtWaves;
constexpr int kFtMaxD = 64;            // the tiled engine's width limit (LDS: weights + activations of the solve within 160 KB)
constexpr int kFtMaxH = 112;
constexpr int kFtLdsBytes = 160 * 1024;
constexpr int kFtMaxAttempts = 8000;   // meeting tags are epoch * 8192 + sequence + 1 (two initial meetings + one per attempt)

struct FtGeo {
    int D, H, P, DP, HP;
    int off[3], in[3], out[3];         // parameter offsets and widths (as FfGeo)
    int inp[3], outp[3], ld[3];        // padded widths (16), LDS row stride of Wl
    int woff[3], voff[3];              // LDS offsets (floats) of Wl and of the four vectors b, bw, bb, gw (outp each)
    int wfloats;                       // LDS floats of the parameters
};

__host__ __device__ inline int ft_pad16(int n) { return (n + 15) / 16 * 16; }
__host__ inline FtGeo ft_geo(int D, int H) {
    FtGeo G;
    const FfGeo F = ff_geo(D, H);
    G.D = D; G.H = H; G.P = F.P; G.DP = ft_pad16(D); G.HP = ft_pad16(H);
    int o = 0;
    for (int l = 0; l < 3; ++l) {
        G.off[l] = F.off[l]; G.in[l] = F.in[l]; G.out[l] = F.out[l];
        G.inp[l] = ft_pad16(F.in[l]); G.outp[l] = ft_pad16(F.out[l]); G.ld[l] = G.outp[l] + 1;
        G.woff[l] = o; o += G.inp[l] * G.ld[l];
    }
    for (int l = 0; l < 3; ++l) { G.voff[l] = o; o += 4 * G.outp[l]; }
    G.wfloats = o;
    return G;
}
// LDS floats of the solve / feval / reverse kernels: parameters, gates, six activation buffers, reduction scratch
__host__ __device__ inline int ft_gt_floats(const FtGeo& G) { return 2 * G.HP + G.DP; }
__host__ __device__ inline int ft_align4(int n) { return (n + 3) & ~3; }
__host__ __device__ inline int ft_lds_floats(const FtGeo& G) { return ft_align4(G.wfloats) + ft_align4(ft_gt_floats(G)) + (2 * G.DP + 4 * G.HP) * 16 + 128; }

struct FtLds {
    float* W;                          // parameters (ft_geo layout)
    float* GT;                         // gates at the evaluation time: g1 [HP], g2 [HP], g3 [DP] (zero on padded rows)
    float *X, *E;                      // [DP][16]: the layer-1 input / Hutchinson scratch, the probe
    float *S1, *A1, *S2, *A2;          // [HP][16]: softplus(h_l), sig(h_l) .* g_l (then the VJP's v2, v1 in S1, S2)
    float* red;                        // 64 floats (+ 64 for the meeting)
};
__device__ inline FtLds ft_lds(const FtGeo& G, float* smem) {
    FtLds L;
    L.W = smem; L.GT = smem + ft_align4(G.wfloats);
    float* b = L.GT + ft_align4(ft_gt_floats(G));      // (the meeting keeps doubles at red + 64: 8-byte aligned)
    L.X = b; b += G.DP * 16; L.E = b; b += G.DP * 16;
    L.S1 = b; b += G.HP * 16; L.A1 = b; b += G.HP * 16; L.S2 = b; b += G.HP * 16; L.A2 = b; b += G.HP * 16;
    L.red = b;
    return L;
}

// parameters into LDS, zero-padded (every thread of the workgroup)
__device__ inline void ft_load_params(const FtGeo& G, const float* __restrict__ p, float* W, int tid) {
    for (int l = 0; l < 3; ++l) {
        const int ld = G.ld[l], in = G.in[l], out = G.out[l], n = G.inp[l] * ld;
        float* w = W + G.woff[l];
        for (int idx = tid; idx < n; idx += kFtThreads) {
            const int i = idx / ld, o = idx - i * ld;
            w[idx] = (i < in && o < out) ? p[G.off[l] + i * out + o] : 0.f;
        }
        float* v = W + G.voff[l];
        for (int idx = tid; idx < 4 * G.outp[l]; idx += kFtThreads) {
            const int k = idx / G.outp[l], o = idx - k * G.outp[l];
            v[idx] = o < out ? p[G.off[l] + in * out + k * out + o] : 0.f;
        }
    }
}
__device__ __forceinline__ const float* ft_vec(const FtGeo& G, const float* W, int l, int k) { return W + G.voff[l] + k * G.outp[l]; }

__device__ inline void ft_gates(const FtGeo& G, const float* W, float* GT, float t, int tid) {
    const int n = ft_gt_floats(G);
    for (int idx = tid; idx < n; idx += kFtThreads) {
        int l, o;
        if (idx < G.HP) { l = 0; o = idx; } else if (idx < 2 * G.HP) { l = 1; o = idx - G.HP; } else { l = 2; o = idx - 2 * G.HP; }
        GT[idx] = o < G.out[l] ? ff_sig(ft_vec(G, W, l, 3)[o] * t) : 0.f;
    }
}

// Y = W_l X (forward product): output tiles over outp, k over inp; X [inp][16].  epi(row0, v): rows row0 + j (j < 4), column lane & 15.
template <class Epi>
__device__ __forceinline__ void ft_fwd(const float* Wl, int ld, int inp, int outp, const float* X, int wave, int lane, Epi&& epi) {
    const int c = lane & 15, g = lane >> 4;
    for (int mo = wave; mo < (outp >> 4); mo += kFtWaves) {
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
        const float* wp = Wl + 16 * mo + c + g * ld;
        const float* xp = X + g * 16 + c;
        for (int k = 0; k < inp; k += 8) {
            a0 = mfma16(wp[k * ld], xp[k * 16], a0);
            a1 = mfma16(wp[(k + 4) * ld], xp[(k + 4) * 16], a1);
        }
        epi(16 * mo + 4 * g, a0 + a1);
    }
}
// Y = W_l' X (transposed product): output tiles over inp, k over outp; X [outp][16]
template <class Epi>
__device__ __forceinline__ void ft_tr(const float* Wl, int ld, int inp, int outp, const float* X, int wave, int lane, Epi&& epi) {
    const int c = lane & 15, g = lane >> 4;
    for (int mi = wave; mi < (inp >> 4); mi += kFtWaves) {
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
        const float* wp = Wl + (16 * mi + c) * ld + g;
        const float* xp = X + g * 16 + c;
        for (int k = 0; k < outp; k += 8) {
            a0 = mfma16(wp[k], xp[k * 16], a0);
            a1 = mfma16(wp[k + 4], xp[(k + 4) * 16], a1);
        }
        epi(16 * mi + 4 * g, a0 + a1);
    }
}

// Per-column sum over rows of a product formed in registers (every wave's lanes hold partials of column lane & 15): butterfly inside the
// wave, then the waves in order.  Returns the sum on threads tid < 16 (column tid); ends behind a barrier.
__device__ __forceinline__ float ft_colsum(float v, float* red, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (lane < 16) red[wave * 16 + lane] = v;
    __syncthreads();
    float s = 0.f;
    if (tid < 16) s = ((red[tid] + red[16 + tid]) + red[32 + tid]) + red[48 + tid];
    __syncthreads();
    return s;
}

// One evaluation of the augmented right-hand side for the 16 columns of a tile.
//   pre: L.X holds the data rows of the input ([DP][16], padded rows zero), L.E the probe (Hutchinson; zero columns where not valid).
//   out: kout[r * ks + c] = fsign * f_r (r < D), kout[D * ks + c] = tsign * tr.  exact: the closed-form trace (QT: this tile's H x H buffer).
//   KIN (Hutchinson only): kout[(D + 1) * ks + c] = sum f^2, kout[(D + 2) * ks + c] = sum eJ^2.
//   Every thread of the workgroup calls it; it ends behind a barrier.
template <bool KIN = false>
__device__ __forceinline__ void ft_eval(const FtGeo& G, const FtLds& L, float t, float* kout, int ks, int exact, float fsign, float tsign, float* QT, int tid) {
    const int lane = tid & 63, wave = tid >> 6, c = lane & 15, D = G.D, H = G.H, HP = G.HP;
    const float *W1 = L.W + G.woff[0], *W2 = L.W + G.woff[1], *W3 = L.W + G.woff[2];
    const float *g1 = L.GT, *g2 = L.GT + HP, *g3 = L.GT + 2 * HP;
    ft_gates(G, L.W, L.GT, t, tid);
    __syncthreads();
    if (exact) {   // QT[j][k] = W2[k][j] M[j][k], M[j][k] = sum_i W1[j][i] g3_i W3[i][k]
        const int g = lane >> 4, nt = HP >> 4, ld1 = G.ld[0], ld2 = G.ld[1], ld3 = G.ld[2];
        for (int tt = wave; tt < nt * nt; tt += kFtWaves) {
            const int mj = tt / nt, mk = tt - mj * nt;
            f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
            for (int i = 0; i < G.DP; i += 8) {
                a0 = mfma16(W1[(i + g) * ld1 + 16 * mj + c], g3[i + g] * W3[(16 * mk + c) * ld3 + i + g], a0);
                a1 = mfma16(W1[(i + 4 + g) * ld1 + 16 * mj + c], g3[i + 4 + g] * W3[(16 * mk + c) * ld3 + i + 4 + g], a1);
            }
            const f32x4 m = a0 + a1;
            const int k = 16 * mk + c;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int j = 16 * mj + 4 * g + jj;
                QT[(size_t)j * HP + k] = W2[j * ld2 + k] * m[jj];
            }
        }
    }
    // layer 1 -> S1, A1
    ft_fwd(W1, G.ld[0], G.inp[0], G.outp[0], L.X, wave, lane, [&](int r0, f32x4 v) {
        const float *b = ft_vec(G, L.W, 0, 0), *bw = ft_vec(G, L.W, 0, 1), *bb = ft_vec(G, L.W, 0, 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = r0 + j;
            float s = 0.f, a = 0.f;
            if (o < H) { const float h = fmaf(v[j] + b[o], g1[o], fmaf(bw[o], t, bb[o])); s = ff_softplus(h); a = ff_sig(h) * g1[o]; }
            L.S1[o * 16 + c] = s; L.A1[o * 16 + c] = a;
        }
    });
    __syncthreads();
    // layer 2 -> S2, A2
    ft_fwd(W2, G.ld[1], G.inp[1], G.outp[1], L.S1, wave, lane, [&](int r0, f32x4 v) {
        const float *b = ft_vec(G, L.W, 1, 0), *bw = ft_vec(G, L.W, 1, 1), *bb = ft_vec(G, L.W, 1, 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = r0 + j;
            float s = 0.f, a = 0.f;
            if (o < H) { const float h = fmaf(v[j] + b[o], g2[o], fmaf(bw[o], t, bb[o])); s = ff_softplus(h); a = ff_sig(h) * g2[o]; }
            L.S2[o * 16 + c] = s; L.A2[o * 16 + c] = a;
        }
    });
    __syncthreads();
    // layer 3 -> f;  Hutchinson: X <- g3 .* e;  exact: tr = a2 . (Q a1)
    float pke = 0.f, pjn = 0.f;
    ft_fwd(W3, G.ld[2], G.inp[2], G.outp[2], L.S2, wave, lane, [&](int r0, f32x4 v) {
        const float *b = ft_vec(G, L.W, 2, 0), *bw = ft_vec(G, L.W, 2, 1), *bb = ft_vec(G, L.W, 2, 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = r0 + j;
            if (o < D) {
                const float f = fmaf(v[j] + b[o], g3[o], fmaf(bw[o], t, bb[o]));
                kout[(size_t)o * ks + c] = fsign * f;
                if constexpr (KIN) pke = fmaf(f, f, pke);
            }
        }
    });
    float part = 0.f;
    if (exact) {
        ft_fwd(QT, HP, HP, HP, L.A1, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) part = fmaf(L.A2[(r0 + j) * 16 + c], v[j], part);
        });
    } else {
        for (int idx = tid; idx < G.DP * 16; idx += kFtThreads) L.X[idx] = g3[idx >> 4] * L.E[idx];
        __syncthreads();
        // v2 = a2 .* W3' (g3 .* e) -> S1
        ft_tr(W3, G.ld[2], G.inp[2], G.outp[2], L.X, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int o = r0 + j; L.S1[o * 16 + c] = v[j] * L.A2[o * 16 + c]; }
        });
        __syncthreads();
        // v1 = a1 .* W2' v2 -> S2
        ft_tr(W2, G.ld[1], G.inp[1], G.outp[1], L.S1, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int o = r0 + j; L.S2[o * 16 + c] = v[j] * L.A1[o * 16 + c]; }
        });
        __syncthreads();
        // tr = e . W1' v1
        ft_tr(W1, G.ld[0], G.inp[0], G.outp[0], L.S2, wave, lane, [&](int r0, f32x4 v) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                part = fmaf(L.E[(r0 + j) * 16 + c], v[j], part);
                if constexpr (KIN) pjn = fmaf(v[j], v[j], pjn);      // (rows >= D: W1's padded rows are zero)
            }
        });
    }
    const float tr = ft_colsum(part, L.red, tid);
    if (tid < 16) kout[(size_t)D * ks + tid] = tsign * tr;
    if constexpr (KIN) {
        const float ke = ft_colsum(pke, L.red, tid);
        const float jn = ft_colsum(pjn, L.red, tid);
        if (tid < 16) { kout[(size_t)(D + 1) * ks + tid] = ke; kout[(size_t)(D + 2) * ks + tid] = jn; }
    }
    __syncthreads();
}

struct FtSolveParams {
    StepParams F;                    // the controller's view (F.D = R rows; F.ctl / meta / initrec / ctl_final: tile 0's)
    FtGeo G;
    const float* p;
    const float* x;                  // D x B caller layout
    const float* e;                  // D x B caller layout (dir = +1), NULL (dir = -1: exact trace)
    float* ws;                       // [10][R][Bp]: uprev, unew, (unused), k1..k7
    float* tape;                     // [max_attempts + 1][R][Bp] or NULL
    float* logpx;                    // B (dir = +1) or NULL
    float* x_out;                    // D x B caller layout or NULL
    float* norm;                     // [ntiles][8] + 512: each tile's initial-step norms (advance_state reads the third as a one-entry partial)
    InitRec* initrec_t;              // [ntiles]: each tile's copy of the initial-step record (tile 0's is F.initrec)
    StepState* ctl_t;                // [ntiles]: where tiles other than 0 write the state before attempt 0
    float* qt;                       // [ntiles][HP][HP] (exact trace)
    MwMeet meet;
    unsigned* xcc;                   // [ntiles] (one-XCD meeting: the host checks they agree)
    int xcd_slot;
    int dir, Bp, ntiles;
    float tbase;                     // dir = -1: t1
    float* reg;                      // kinetic solves: 2 x B (lambda1 row, then lambda2 row); NULL otherwise
};

// Publish this tile's three partials (wave 0), collect everybody's sums in tile order; false when the meeting timed out (every thread).
__device__ __forceinline__ bool ft_meet(const FtSolveParams& Q, float* red, int seq, float a, float b, float c, double (&out)[3], int tile, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    a = wave_sum_f(a); b = wave_sum_f(b); c = wave_sum_f(c);
    if (lane == 0) { red[wave] = a; red[4 + wave] = b; red[8 + wave] = c; }
    __syncthreads();
    double* RD = (double*)(red + 64);
    if (wave == 0) {
        float mine[3] = {0.f, 0.f, 0.f};
        for (int w = 0; w < kFtWaves; ++w) { mine[0] += red[w]; mine[1] += red[4 + w]; mine[2] += red[8 + w]; }
        double o[3];
        const bool ok = mw_exchange3(Q.meet, seq, mine, o, tile, lane);
        if (lane == 0) { RD[0] = o[0]; RD[1] = o[1]; RD[2] = o[2]; red[70] = ok ? 1.f : 0.f; }
    }
    __syncthreads();
    const bool ok = red[70] != 0.f;
    out[0] = RD[0]; out[1] = RD[1]; out[2] = RD[2];
    __syncthreads();
    return ok;
}

// The whole adaptive solve in one launch: forward (dir = +1, Hutchinson), replay along P.replay, sampling (dir = -1, exact trace, tau = t1 - t).
template <bool KIN>
__global__ __launch_bounds__(kFtThreads) void rnde_ffjordt_solve_kernel(const FtSolveParams Q) {
    extern __shared__ float ft_smem[];
    if (!Q.meet.global && (int)(blockIdx.x & 7) != Q.xcd_slot) return;
    const int tile = Q.meet.global ? (int)blockIdx.x : (int)(blockIdx.x >> 3);
    const int tid = threadIdx.x, lane = tid & 63;
    const FtGeo& G = Q.G;
    const int D = G.D, R = D + (KIN ? 3 : 1), Bp = Q.Bp, B = Q.F.B, col0 = tile * 16;
    if (!Q.meet.global && tid == 0) Q.xcc[tile] = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 15;
    StepParams P = Q.F;
    P.initpart = Q.norm + 8 * tile;
    P.initrec = Q.initrec_t + tile;
    const bool lead = tile == 0 && tid == 0;
    const FtLds L = ft_lds(G, ft_smem);
    ft_load_params(G, Q.p, L.W, tid);
    for (int idx = tid; idx < G.DP * 16; idx += kFtThreads) {
        const int r = idx >> 4, col = col0 + (idx & 15);
        L.E[idx] = (Q.dir > 0 && r < D && col < B) ? Q.e[(size_t)col * D + r] : 0.f;
        L.X[idx] = 0.f;
    }
    const size_t RB = (size_t)R * Bp;
    float* U = Q.ws + col0;
    float* UN = Q.ws + RB + col0;
    auto K = [&](int s) { return Q.ws + (size_t)(3 + s) * RB + col0; };
    const int exact = Q.dir < 0 ? 1 : 0;
    const float fsign = Q.dir > 0 ? 1.f : -1.f, tsign = Q.dir > 0 ? -1.f : 1.f;
    float* qt = Q.qt ? Q.qt + (size_t)tile * G.HP * G.HP : nullptr;
    auto eval = [&](float time, float* kout) { ft_eval<KIN>(G, L, Q.dir > 0 ? time : Q.tbase - time, kout, Bp, exact, fsign, tsign, qt, tid); };
    const float rt = P.reltol, at = P.abstol;
    const double N = (double)R * (double)B;
    const int nel = R * 16;
    __syncthreads();

    // ---- initial state, f(u0), the initial-step rule (the arithmetic of rnde_ffjord_solve_kernel) ----
    for (int idx = tid; idx < nel; idx += kFtThreads) {
        const int r = idx >> 4, c = idx & 15, col = col0 + c;
        const float v = (r < D && col < B) ? Q.x[(size_t)col * D + r] : 0.f;
        U[(size_t)r * Bp + c] = v;
        if (r < D) L.X[r * 16 + c] = v;
    }
    eval(P.t0 + 0.f, K(0));
    float pa = 0.f, pb = 0.f;
    for (int idx = tid; idx < nel; idx += kFtThreads) {
        const int r = idx >> 4, c = idx & 15;
        if (col0 + c >= B) continue;
        const size_t ix = (size_t)r * Bp + c;
        const float xv = U[ix], kv = K(0)[ix], sk = at + fabsf(xv) * rt;
        const float a = xv / sk, b = kv / sk;
        pa += a * a; pb += b * b;
    }
    double sm[3];
    if (!ft_meet(Q, L.red, 0, pa, pb, 0.f, sm, tile, tid)) return;
    float dt0;
    {
        const float d0 = (float)sqrt(sm[0] / N), d1 = (float)sqrt(sm[1] / N), dtmax = P.t1 - P.t0;
        int c0 = 0, cl = 0;
        if (d0 < 1e-5f || d1 < 1e-5f) { dt0 = 1e-6f; c0 = 1; }
        else dt0 = (d0 / d1) / 100.f;
        if (dtmax < dt0) { dt0 = dtmax; cl = 1; }
        if (tid == 0) { P.initrec->d0 = d0; P.initrec->d1 = d1; P.initrec->dt0 = dt0; P.initrec->dt0_const = c0; P.initrec->dt0_clamped = cl; }
    }
    for (int idx = tid; idx < nel; idx += kFtThreads) {
        const int r = idx >> 4, c = idx & 15;
        const size_t ix = (size_t)r * Bp + c;
        if (r < D) L.X[r * 16 + c] = U[ix] + dt0 * K(0)[ix];
    }
    eval(P.t0 + dt0, K(1));
    float pc = 0.f;
    for (int idx = tid; idx < nel; idx += kFtThreads) {
        const int r = idx >> 4, c = idx & 15;
        if (col0 + c >= B) continue;
        const size_t ix = (size_t)r * Bp + c;
        const float sk = at + fabsf(U[ix]) * rt;
        const float a = (K(1)[ix] - K(0)[ix]) / sk;
        pc += a * a;
    }
    if (!ft_meet(Q, L.red, 1, pc, 0.f, 0.f, sm, tile, tid)) return;
    if (tid == 0) P.initpart[2] = (float)sm[0];       // advance_state reads the third initial norm as a one-entry partial
    __syncthreads();
    __threadfence_block();
    StepState S = advance_state(P, 0, lane, tid == 0, tile == 0 ? &P.ctl[0] : Q.ctl_t + tile);
    int n_acc = 0;
    for (int n = 0; !S.done; ++n) {
        const float t = S.t;
        const float dt = (P.t1 - S.t < S.dtp) ? (P.t1 - S.t) : S.dtp;
        for (int s = 1; s < 7; ++s) {                      // stage s + 1: input uprev + dt sum_j a_{s+1, j} k_j
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const int r = idx >> 4, c = idx & 15;
                const size_t ix = (size_t)r * Bp + c;
                float acc = 0.f;
                for (int j = 0; j < s; ++j) acc = fmaf(tsA_rt(s, j), K(j)[ix], acc);
                const float g = U[ix] + dt * acc;
                if (r < D) L.X[r * 16 + c] = g;
                if (s == 6) UN[ix] = g;
            }
            eval(t + kTsC[s] * dt, K(s));
        }
        float part = 0.f;
        for (int idx = tid; idx < nel; idx += kFtThreads) {   // embedded error estimate, SURVEY.md B.3
            const int r = idx >> 4, c = idx & 15;
            if (col0 + c >= B) continue;
            const size_t ix = (size_t)r * Bp + c;
            float E = 0.f;
            for (int j = 0; j < 7; ++j) E += kTsBt[j] * K(j)[ix];
            const float ut = dt * E, sk = at + fmaxf(fabsf(U[ix]), fabsf(UN[ix])) * rt, rr = ut / sk;
            part += rr * rr;
        }
        double xs[3];
        if (!ft_meet(Q, L.red, 2 + n, part, 0.f, 0.f, xs, tile, tid)) return;
        const float none[4] = {0.f, 0.f, 0.f, 0.f};
        const StepState Sn = advance_state_t<true>(P, n + 1, lane, lead, &P.ctl[(n + 1) & 1], none, S, xs);
        if (Sn.n_acc > S.n_acc) {                          // accepted: tape uprev, then unew -> uprev, k7 -> k1
            for (int idx = tid; idx < nel; idx += kFtThreads) {
                const int r = idx >> 4, c = idx & 15;
                const size_t ix = (size_t)r * Bp + c;
                if (Q.tape) Q.tape[(size_t)n_acc * RB + col0 + ix] = U[ix];
                U[ix] = UN[ix];
                K(0)[ix] = K(6)[ix];
            }
            ++n_acc;
        }
        S = Sn;
    }
    if (lead) *P.ctl_final = S;
    __syncthreads();
    for (int idx = tid; idx < nel; idx += kFtThreads) {
        const int r = idx >> 4, c = idx & 15;
        const size_t ix = (size_t)r * Bp + c;
        if (Q.tape) Q.tape[(size_t)n_acc * RB + col0 + ix] = U[ix];
        if (r < D && col0 + c < B && Q.x_out) Q.x_out[(size_t)(col0 + c) * D + r] = U[ix];
    }
    if (tid < 16 && col0 + tid < B && Q.logpx) {
        float lp = 0.f;
        for (int r = 0; r < D; ++r) {
            const float z = U[(size_t)r * Bp + tid];
            lp += -(1.8378770664093453f + z * z) * 0.5f;
        }
        Q.logpx[col0 + tid] = lp - U[(size_t)D * Bp + tid];
    }
    if constexpr (KIN)
        if (tid < 16 && col0 + tid < B) {
            Q.reg[col0 + tid] = U[(size_t)(D + 1) * Bp + tid];
            Q.reg[(size_t)B + col0 + tid] = U[(size_t)(D + 2) * Bp + tid];
        }
}

// One evaluation of the augmented right-hand side per column (the parity instrument): out (D + 1) x B caller layout, the trace row -e . eJ
// (exact: -tr J).  One workgroup per tile; ws: [ntiles][R][16].  KIN: (D + 3) x B, Hutchinson only.
template <bool KIN>
__global__ __launch_bounds__(kFtThreads) void rnde_ffjordt_feval_kernel(const FtGeo G, const float* __restrict__ p, const float* __restrict__ x,
                                                                       const float* __restrict__ e, float t, int B, int exact, float* __restrict__ ws,
                                                                       float* __restrict__ qt, float* __restrict__ out) {
    extern __shared__ float ft_smem[];
    const int tile = blockIdx.x, tid = threadIdx.x, D = G.D, R = D + (KIN ? 3 : 1), col0 = tile * 16;
    const FtLds L = ft_lds(G, ft_smem);
    ft_load_params(G, p, L.W, tid);
    for (int idx = tid; idx < G.DP * 16; idx += kFtThreads) {
        const int r = idx >> 4, col = col0 + (idx & 15);
        const bool ok = r < D && col < B;
        L.X[idx] = ok ? x[(size_t)col * D + r] : 0.f;
        L.E[idx] = (ok && !exact) ? e[(size_t)col * D + r] : 0.f;
    }
    __syncthreads();                                          // (ft_eval's gates read gate_W from LDS)
    float* k = ws + (size_t)tile * R * 16;
    ft_eval<KIN>(G, L, t, k, 16, exact, 1.f, -1.f, exact ? qt + (size_t)tile * G.HP * G.HP : nullptr, tid);
    for (int idx = tid; idx < R * 16; idx += kFtThreads) {
        const int r = idx >> 4, col = col0 + (idx & 15);
        if (col < B) out[(size_t)col * R + r] = k[idx];
    }
}

}  // namespace rnde
