// rnde.hip -- C ABI (include/rnde.h) over the gfx950 kernels.  No torch, no oracle, no CPU fallback:
// every entry point either runs the HIP kernels or returns an error status.
#include "rnde_node.h"

static thread_local std::string g_create_err;   // last create error of the calling thread (rnde_last_error(NULL)); no process-wide mutable state
void rnde_set_create_error(const std::string& msg) { g_create_err = msg; }
extern "C" const char* rnde_version(void) { return "rnde 0.1.0 (gfx950)"; }
extern "C" int64_t rnde_debug_poison_allocs(void) { return (int64_t)rnde_g_poison_allocs.load(); }      // rnde_alloc.h
extern "C" int64_t rnde_debug_poison_bytes(void) { return (int64_t)rnde_g_poison_bytes.load(); }
extern "C" int64_t rnde_debug_live_allocs(void) { return (int64_t)rnde_g_live_allocs.load(); }
extern "C" int64_t rnde_debug_live_bytes(void) { return (int64_t)rnde_g_live_bytes.load(); }
extern "C" const char* rnde_last_error(const rnde_node* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

extern "C" int32_t rnde_param_count(const rnde_node_config* c) {
    int n = 0;
    for (int l = 0; l < c->n_layers; ++l) n += (c->dims[l] + (c->time_dep ? 1 : 0)) * c->dims[l + 1] + c->dims[l + 1];
    return n;
}

StepParams make_params(rnde_node* h, const float* x, int B, float t0, float t1, int tape) {
    StepParams P{};
    P.x = x;
    P.f0 = h->f0; P.h0 = h->h0; P.u1 = h->u1; P.f1 = h->f1; P.h1 = h->h1;
    P.arena = h->arena; P.rec_stride = h->rec_stride;
    P.ctl = h->ctl; P.ctl_final = h->ctl_final; P.meta = h->meta; P.initrec = h->initrec;
    P.errpart = h->errpart; P.initpart = h->initpart; P.dbg_out = nullptr;
    P.D = h->D; P.H = h->H; P.B = B; P.Bn = h->couple ? h->couple_batch : B;
    P.Bpad = ((B + 15) / 16) * 16;   // both engines pad the batch to 16 columns (one tape format)
    P.nwg = h->engine == 2 ? h->sR * (P.Bpad / 16) : (h->engine == 3 ? (h->mw ? P.Bpad / 16 : (P.Bpad / 16 + kCW - 1) / kCW) : P.Bpad / h->BT);
    P.reltol = h->cfg.reltol; P.abstol = h->cfg.abstol; P.t0 = t0; P.t1 = t1;
    P.tape = tape; P.max_attempts = h->cfg.max_attempts;
    P.forced = 0; P.forced_t = 0; P.forced_dt = 0;
    P.xvec = ((h->D & 3) == 0 && ((uintptr_t)x & 15) == 0) ? 1 : 0;
    P.reg_kind = h->cfg.regularize;
    P.replay = nullptr; P.n_replay = 0;
    P.beta1 = (float)(7.0 / (10.0 * h->rk_order)); P.beta2 = (float)(2.0 / (5.0 * h->rk_order)); P.rk_order = (float)h->rk_order;   // (order 5: kBeta1, kBeta2 bit for bit)
    return P;
}

static_assert(kCMaxL == RNDE_MAX_LAYERS, "chain engine layer limit");
static_assert(ACT_IDENTITY == RNDE_ACT_IDENTITY && ACT_TANH == RNDE_ACT_TANH && ACT_RELU == RNDE_ACT_RELU && ACT_SIGMOID == RNDE_ACT_SIGMOID &&
              ACT_SOFTPLUS == RNDE_ACT_SOFTPLUS && ACT_ELU == RNDE_ACT_ELU, "rnde_act codes of the kernels (rnde_device.h)");
static bool chain_geo(const rnde_node_config* c, ChainGeo& G) {
    G = ChainGeo{};
    G.n_layers = c->n_layers; G.time_dep = c->time_dep ? 1 : 0; G.pre_act = c->pre_act;   // rnde_pre_act, checked by rnde_node_create
    int po = 0, fo = 0, bo = 0, to = 0;
    for (int l = 0; l <= c->n_layers; ++l) {
        if (c->dims[l] < 1 || c->dims[l] > 4 * kCMaxKs) return false;
        G.width[l] = c->dims[l]; G.nks[l] = (c->dims[l] + 3) / 4;
    }
    for (int l = 0; l < c->n_layers; ++l) {
        G.act[l] = c->act[l];
        G.poff[l] = po; po += (G.width[l] + G.time_dep) * G.width[l + 1] + G.width[l + 1];
        G.foff[l] = fo; fo += ((G.nks[l + 1] + 3) / 4) * G.nks[l];
        G.boff[l] = bo; bo += 4 * ((G.nks[l + 1] + 3) / 4) * (1 + G.time_dep);   // padded to whole tiles
        G.toff[l] = to; to += ((G.nks[l] + 3) / 4) * G.nks[l + 1];
    }
    G.nfrag_f = fo; G.nfrag_b = bo; G.nfrag_t = to; G.nksD = G.nks[0];
    return true;
}
static rnde_status chain_create(const rnde_node_config* c, rnde_node** out) {
    ChainGeo G;
    if (!chain_geo(c, G)) { g_create_err = "unsupported dynamics: beyond the 2-layer time-dependent form the kernels cover Dense chains of width <= 64 (rnde_node_create_tiled / engine = \"tiled\" serves wider Dense chains whose weights fit LDS, with track_ctrl = track_initdt = 0; a tape pool, rnde_tapes_create, holds rnde_node_create instances only)"; return RNDE_ERR_BAD_ARG; }
    // LDS: fragment tables rounded up to whole 1 KiB DMA units, then 64 floats of reduction scratch
    size_t lds_f = ((size_t)((G.nfrag_f + G.nfrag_b + 3) / 4) * 256 + 64) * 4, lds_b = ((size_t)((G.nfrag_f + G.nfrag_b + G.nfrag_t + 3) / 4) * 256 + 64) * 4;
    if (lds_b > 160 * 1024) { g_create_err = "chain too large: its weight fragments must fit the 160 KB LDS of a CU"; return RNDE_ERR_BAD_ARG; }
    if (c->regularize < RNDE_REG_NONE || c->regularize > RNDE_REG_STIFF_DT) { g_create_err = "regularize: unknown value"; return RNDE_ERR_BAD_ARG; }
    if (c->col_tile != 0 && c->col_tile != 64 && c->col_tile != 65) { g_create_err = "col_tile: this network runs on the chain engine (0 = auto, 64 = one wave per column tile, 65 = four waves per column tile)"; return RNDE_ERR_BAD_ARG; }
    if (c->max_batch < 1 || c->max_attempts < 1) { g_create_err = "max_batch / max_attempts"; return RNDE_ERR_BAD_ARG; }
    std::unique_ptr<rnde_node, void (*)(rnde_node*)> hold(new rnde_node(), rnde_node_destroy);      // (until the last step has succeeded)
    rnde_node* h = hold.get();
    h->cfg = *c; h->engine = 3; h->cg = G;
    h->D = c->dims[0]; h->H = 0; h->P = rnde_param_count(c); h->BT = 16;
    h->NKD = G.nksD <= 4 ? 4 : (G.nksD <= 8 ? 8 : 16);
    // the kernels with compile-time shapes below (ALT, mw_lat) serve identity / tanh only: any other activation takes the generic kernels' variant
    bool plain_acts = true;
    for (int l = 0; l < G.n_layers; ++l) plain_acts = plain_acts && (G.act[l] == RNDE_ACT_IDENTITY || G.act[l] == RNDE_ACT_TANH);
    h->chain_ga = plain_acts ? 0 : 1;      // (the identity / tanh kernels are compiled without the other maps: ALT / LAT = 2 serve them)
    {   // compile-time shape specialisation for the reference's own latent-ODE widths (rnde_chain.h: ALT)
        bool alt = plain_acts && G.nksD == kAltA && !getenv("RNDE_CHAIN_GENERIC");
        for (int l = 0; l <= G.n_layers && alt; ++l) alt = G.nks[l] == ((l & 1) ? kAltB : kAltA);
        h->chain_alt = alt ? 1 : 0;
    }
    h->Bpad_max = ((c->max_batch + 15) / 16) * 16;
    const int ntiles = h->Bpad_max / 16;
    h->nwg_max = (ntiles + kCW - 1) / kCW;
    {   // multi-wave kernels: geometry, LDS budget, who runs (col_tile 0 = auto -> multi-wave, 64 = one wave per tile, 65 = multi-wave)
        MwGeo& M = h->mg;
        M = MwGeo{};
        M.n_layers = G.n_layers; M.time_dep = G.time_dep; M.pre_act = G.pre_act; M.D = c->dims[0];
        int fo = 0, to = 0, row = 0;
        for (int l = 0; l <= G.n_layers; ++l) { M.width[l] = G.width[l]; M.mt[l] = (G.width[l] + 15) / 16; }
        for (int l = 0; l < G.n_layers; ++l) {
            M.act[l] = G.act[l]; M.poff[l] = G.poff[l];
            M.foff[l] = fo; fo += M.mt[l] * M.mt[l + 1] * 4;
            M.toff[l] = to; to += M.mt[l] * M.mt[l + 1] * 4;
            M.hrow[l] = row; row += 4 * M.mt[l]; M.zrow[l] = row; row += 4 * M.mt[l + 1];
        }
        M.hrow[G.n_layers] = row; row += 4 * M.mt[G.n_layers];
        M.RS = row; M.nfrag_f = (fo + 3) / 4 * 4; M.nfrag_t = (to + 3) / 4 * 4;
        h->mw_lds_f = ((size_t)M.nfrag_f * 64 + 1024 + 2048 + 64) * 4;
        h->mw_lds_b = ((size_t)M.nfrag_t * 64 + 1024 + 2048 + 64) * 4;
        const bool fits = h->mw_lds_f <= 160 * 1024 && h->mw_lds_b <= 160 * 1024;
        const char* e = getenv("RNDE_CHAIN_MW");
        h->mw = (fits && c->col_tile != 64 && !(e && e[0] == '0')) ? 1 : 0;
        if (c->col_tile == 65 && !fits) { g_create_err = "col_tile 65: the multi-wave kernels need the padded weight fragments in 160 KB of LDS"; return RNDE_ERR_BAD_ARG; }
        if (h->mw) h->nwg_max = ntiles;
        {   // experiments/latent_ode.jl:113-124 exactly: eight time-independent layers of widths 20 <-> 50
            bool lat = plain_acts && h->mw && c->n_layers == kLatLayers && !c->time_dep && h->NKD == 8;
            for (int i = 0; i <= kLatLayers && lat; ++i) lat = c->dims[i] == lat_width(i);      // (the kernels leave out the k-steps of the padding: exact widths)
            const char* e = getenv("RNDE_CHAIN_LAT");
            h->mw_lat = (lat && !(e && e[0] == '0')) ? 1 : 0;
        }
        if ((c->solver == RNDE_SOLVER_DP5 || c->solver == RNDE_SOLVER_DOP853) && !h->mw) { g_create_err = "DP5 / DOP853 need the multi-wave kernels (weights must fit LDS)"; return RNDE_ERR_BAD_ARG; }
        h->rk_tab = (h->mw && (c->solver == RNDE_SOLVER_DP5 || getenv("RNDE_CHAIN_TAB") != nullptr)) ? 1 : 0;
        if (c->solver == RNDE_SOLVER_DOP853) {
            // an S-stage pair as a table (csrc/rk_tables.h): the kernels take stage count, tape layout and evaluation counts from it.  Neither a
            // dense output nor the stiffness estimate (k_S - k_{S-1} is not an eigenvalue estimate for an arbitrary pair) exist for it.
            if (c->regularize >= 2) { g_create_err = "DOP853: callbacks none / error_est only (no stiffness estimate for a table pair)"; return RNDE_ERR_BAD_ARG; }
            h->rk_tab = 2; h->mw_lat = 0; h->rk_S = kDop853S; h->rk_order = kDop853Order;
            RkTab& T = h->rk;
            T = RkTab{};
            T.S = h->rk_S; T.order = h->rk_order;
            for (int sI = 0; sI < T.S; ++sI) {
                T.c[sI] = (float)kDop853C[sI]; T.bt[sI] = (float)kDop853Bt[sI];
                for (int i = 0; i < kRkSMax - 1; ++i) {
                    T.fwd[sI][i] = (sI + 1 + i < T.S) ? (float)kDop853A[sI + 1 + i][sI] : 0.f;
                    T.bwd[sI][i] = (sI - 1 - i >= 0) ? (float)kDop853A[sI][sI - 1 - i] : 0.f;
                }
            }
            for (int j = 0; j < T.S; ++j) T.aN[j] = (float)kDop853A[T.S - 1][j];
        }
        if (h->rk_tab == 1) {
            double A[7][7] = {{0}}, Cn[7], BT[7], Dn[7][4];
            if (c->solver == RNDE_SOLVER_DP5) {   // Dormand & Prince 1980; dense output: Shampine 1986 (the matrix scipy's RK45 uses)
                const double a[7][7] = {{0}, {1.0 / 5}, {3.0 / 40, 9.0 / 40}, {44.0 / 45, -56.0 / 15, 32.0 / 9}, {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729},
                                        {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}, {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84, 0}};
                const double cc[7] = {0, 0.2, 0.3, 0.8, 8.0 / 9, 1, 1};
                const double bt[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};
                const double dn[7][4] = {{1.0, -8048581381.0 / 2820520608.0, 8663915743.0 / 2820520608.0, -12715105075.0 / 11282082432.0}, {0, 0, 0, 0},
                                         {0, 131558114200.0 / 32700410799.0, -68118460800.0 / 10900136933.0, 87487479700.0 / 32700410799.0},
                                         {0, -1754552775.0 / 470086768.0, 14199869525.0 / 1410260304.0, -10690763975.0 / 1880347072.0},
                                         {0, 127303824393.0 / 49829197408.0, -318862633887.0 / 49829197408.0, 701980252875.0 / 199316789632.0},
                                         {0, -282668133.0 / 205662961.0, 2019193451.0 / 616988883.0, -1453857185.0 / 822651844.0},
                                         {0, 40617522.0 / 29380423.0, -110615467.0 / 29380423.0, 69997945.0 / 29380423.0}};
                memcpy(A, a, sizeof(A)); memcpy(Cn, cc, sizeof(Cn)); memcpy(BT, bt, sizeof(BT)); memcpy(Dn, dn, sizeof(Dn));
            } else {   // Tsit5 through the data path (cross-check of the path itself): tableau of rnde_device.h, dense output expanded to monomials
                for (int sI = 0; sI < 7; ++sI) { Cn[sI] = tsC(sI); BT[sI] = tsBt(sI); for (int j = 0; j < 7; ++j) A[sI][j] = tsA(sI, j); }
                auto mul = [](const double* a, int na, const double* b, int nb, double* o) { for (int i = 0; i < na + nb - 1; ++i) o[i] = 0; for (int i = 0; i < na; ++i) for (int j = 0; j < nb; ++j) o[i + j] += a[i] * b[j]; };
                auto put = [&](int i, double cf, const double* poly5) { for (int j = 0; j < 4; ++j) Dn[i][j] = cf * poly5[j + 1]; };   // poly5[k] = coefficient of theta^k, k = 0..4
                {   // b1 = c th (th - r)(th^2 - p th + q)
                    const double f1[2] = {-1.3299890189751412, 1.0}, f2[3] = {0.7139816917074209, -1.4364028541716351, 1.0}; double t3[4], t5[5], th[2] = {0.0, 1.0};
                    mul(f1, 2, f2, 3, t3); mul(th, 2, t3, 4, t5); put(0, -1.0530884977290216, t5);
                }
                const double cq[2] = {0.1017, 2.490627285651252793}, pq[2] = {2.1966568338249754, 2.38535645472061657}, qq[2] = {1.2949852507374631, 1.57803468208092486};
                for (int i = 0; i < 2; ++i) { const double t5[5] = {0, 0, qq[i], -pq[i], 1.0}; put(1 + i, cq[i], t5); }   // c th^2 (th^2 - p th + q)
                const double c4[4] = {-16.54810288924490272, 47.37952196281928122, -34.87065786149660974, 2.5}, r4[4] = {1.21712927295533244, 1.203071208372362603, 1.2, 1.0},
                             s4[4] = {0.61620406037800089, 0.658047292653547382, 0.666666666666666667, 0.6};
                for (int i = 0; i < 4; ++i) { const double t5[5] = {0, 0, r4[i] * s4[i], -(r4[i] + s4[i]), 1.0}; put(3 + i, c4[i], t5); }   // c (th - r)(th - s) th^2
            }
            RkTab& T = h->rk;
            T = RkTab{};
            T.S = 7; T.order = 5;
            for (int sI = 0; sI < 7; ++sI) {
                T.c[sI] = (float)Cn[sI]; T.bt[sI] = (float)BT[sI];
                for (int i = 0; i < 6; ++i) { T.fwd[sI][i] = (sI + 1 + i < 7) ? (float)A[sI + 1 + i][sI] : 0.f; T.bwd[sI][i] = (sI - 1 - i >= 0) ? (float)A[sI][sI - 1 - i] : 0.f; }
                for (int j = 0; j < 4; ++j) T.dense[sI][j] = (float)Dn[sI][j];
            }
            for (int j = 0; j < 7; ++j) T.aN[j] = (float)A[6][j];
        }
    }
    h->chain_lds_f = lds_f; h->chain_lds_b = lds_b;
    if (hipSetDevice(c->device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return RNDE_ERR_HIP; }
    const size_t Ac = (size_t)ntiles * h->NKD * 64;   // fragment-order arrays are padded to NKD k-steps
    h->rec_stride = ChainRec{(long long)Ac, h->rk_S}.total();
    auto dm = [](auto& buf, size_t n) { return buf.alloc(n) == hipSuccess; };      // (n elements)
    bool ok = true;
    ok &= dm(h->f0, Ac) && dm(h->u1, Ac) && dm(h->f1, Ac) && dm(h->xcopy, (size_t)h->D * h->Bpad_max);
    ok &= dm(h->pcopy, (size_t)h->P) && dm(h->cfrags, (size_t)(G.nfrag_f + G.nfrag_b + G.nfrag_t + 4) * 64);
    if (h->mw) ok &= dm(h->mw_tab, mw_tab_floats(h->mg));
    if (h->mw) {
        ok &= h->mw_meet.create((size_t)c->max_attempts + 4, 3, kMwMeetMax) == hipSuccess;
        ok &= dm(h->h_mw_bchk, kMwMeetMax + 8) && dm(h->mw_bargs, (size_t)c->max_attempts * 4) && dm(h->h_mw_bargs, (size_t)c->max_attempts * 4);
        if (ok) memset(h->h_mw_bchk, 0, (kMwMeetMax + 8) * 4);
        if (const char* eb = getenv("RNDE_CHAIN_BSWEEP")) h->mw_bsweep = atoi(eb);
        const char* e = getenv("RNDE_CHAIN_SOLVE");
        if (e && e[0] == '0') h->mw_solve = 0;
    }
    ok &= dm(h->ctl, 2) && dm(h->own_ctl_final, 1);
    ok &= dm(h->own_meta, (size_t)(c->max_attempts + 1)) && dm(h->own_initrec, 1);
    ok &= dm(h->errpart, (size_t)(6 * h->nwg_max + 256 + 16)) && dm(h->initpart, (size_t)(3 * h->nwg_max + 256));   // (+256: sum_partials reads whole 256-entry blocks; +16: the [2][4] doubles of rnde_epart_reduce_kernel)
    ok &= dm(h->arena, (size_t)2 * h->rec_stride);
    ok &= dm(h->own_h_ctl, 1);
    ok &= dm(h->own_h_meta, (size_t)(c->max_attempts + 1));
    ok &= dm(h->own_h_init, 1);
    ok &= dm(h->h_scal, 64);
    if (!ok) { g_create_err = "device allocation failed"; return RNDE_ERR_HIP; }
    h->ctl_final = h->own_ctl_final; h->meta = h->own_meta; h->initrec = h->own_initrec;
    h->h_ctl = h->own_h_ctl; h->h_meta = h->own_h_meta; h->h_init = h->own_h_init;
    hipMemset(h->initrec, 0, sizeof(InitRec));
    h->predicted = 12;
    *out = hold.release();
    return RNDE_OK;
}
ChainParams make_chain_params(rnde_node* h, const StepParams& P) {
    ChainParams Q{};
    Q.F = P; Q.G = h->cg; Q.frags = h->cfrags; Q.ntiles = P.Bpad / 16;
    return Q;
}
template <int NKD, int MODE, int ALT = 0>
static hipError_t launch_chain_t(rnde_node* h, const ChainParams& Q, int n, float* u_out, hipStream_t s) {
    auto kern = rnde_chain_kernel<NKD, MODE, ALT>;
    static DeviceOnce attr_set;
    if (attr_set.need()) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        attr_set.done();
    }
    hipLaunchKernelGGL(kern, dim3(Q.F.nwg), dim3(64 * kCW), MODE == CM_FINISH ? 0 : h->chain_lds_f, s, Q, n, u_out);
    return hipGetLastError();
}
template <int MODE>
static hipError_t launch_chain(rnde_node* h, const ChainParams& Q, int n, float* u_out, hipStream_t s) {
    return chain_variant(h, [&](auto nkd, auto alt) { return launch_chain_t<nkd(), MODE, alt()>(h, Q, n, u_out, s); });
}
MwParams make_mw_params(rnde_node* h, const StepParams& P) {
    MwParams Q{};
    Q.F = P; Q.G = h->mg; Q.rk = h->rk; Q.tab = h->mw_tab; Q.ntiles = P.Bpad / 16; Q.u_out = nullptr;
    Q.ev_stride = (long long)Q.ntiles * h->mg.RS * 64;
    Q.slab = P.tape ? h->mw_slab : nullptr;
    return Q;
}
template <int NR, int MODE, int TAB, int LAT = 0>
static hipError_t launch_mw_t(rnde_node* h, const MwParams& Q, int n, hipStream_t s) {
    static DeviceOnce attr_set;
    if (attr_set.need()) {
        hipError_t e = hipFuncSetAttribute((const void*)rnde_chainmw_kernel<NR, MODE, TAB, LAT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        attr_set.done();
    }
    hipLaunchKernelGGL((rnde_chainmw_kernel<NR, MODE, TAB, LAT>), dim3(MODE == MW_SOLVE ? MeetRes::grid(Q.meet) : Q.ntiles), dim3(kMwThreads), MODE == MW_FINISH ? 0 : h->mw_lds_f, s, Q, n);
    return hipGetLastError();
}
template <int MODE>
static hipError_t launch_mw(rnde_node* h, const MwParams& Q, int n, hipStream_t s) {
    return mw_variant(h, [&](auto nr, auto tab, auto lat) { return launch_mw_t<nr(), MODE, tab(), lat()>(h, Q, n, s); });
}
// the forward tapes every layer input of every evaluation into the slab: make room for `evals` evaluations (growing keeps what is there)
static rnde_status ensure_mw_slab(rnde_node* h, long long evals, hipStream_t s) {
    const long long per_eval = (long long)(h->Bpad_max / 16) * h->mg.RS * 64;   // sized for max_batch so that ev_stride changes never outgrow it
    if (h->mw_slab_evals >= evals) return RNDE_OK;
    long long want = std::max(evals, 2 * h->mw_slab_evals);
    {   // 288 GB of HBM: when the slab of a max_attempts solve is small next to what is free, take that at once -- growing it later costs a stream
        // synchronisation, a multi-GB hipMalloc, a copy and a hipFree (~40 ms), and while a model trains its step count creeps across the doubling
        // thresholds in the middle of a run (seen in bench.py's latent_e2e record: one 45 ms step among 3.5 ms ones).  Bounded: the memory is invisible to
        // the caller's own allocator (torch's caching allocator), several handles per layer and several ranks may share one device -- at most
        // RNDE_EAGER_SLAB_MB (default 8192: the config-4 slab at B = 512, max_attempts 256 is 6.8 GB) and at most an eighth of what is free; beyond that the slab grows by doubling as before.
        const long long full = 2 + (long long)(h->rk_S - 1) * h->cfg.max_attempts;
        long long cap_mb = 8192;
        if (const char* e = getenv("RNDE_EAGER_SLAB_MB")) cap_mb = atoll(e);
        size_t fr = 0, tot = 0;
        const size_t full_bytes = (size_t)full * per_eval * 4;
        if (full > want && cap_mb > 0 && full_bytes <= (size_t)cap_mb << 20 && hipMemGetInfo(&fr, &tot) == hipSuccess && full_bytes <= fr / 8) want = full;
    }
    DevBuf<float> nb;
    HIPCHK(h, hipStreamSynchronize(s));
    if (nb.alloc((size_t)want * per_eval) != hipSuccess) {      // the eager size did not fit after all (fragmentation, a neighbour): what the call needs, no more
        (void)hipGetLastError();
        want = evals;
        HIPCHK(h, nb.alloc((size_t)want * per_eval));
    }
    if (h->mw_slab) HIPCHK(h, hipMemcpy(nb, h->mw_slab, (size_t)h->mw_slab_evals * per_eval * 4, hipMemcpyDeviceToDevice));
    h->mw_slab.swap(nb); h->mw_slab_evals = want;      // (nb goes with what the slab held)
    return RNDE_OK;
}

static rnde_status chain_pack(rnde_node* h, const float* p_dev, hipStream_t s) {
    if (h->mw) {
        const long long tm = (long long)mw_tab_floats(h->mg);
        hipLaunchKernelGGL(rnde_chainmw_pack_kernel, dim3((int)std::min<long long>((tm + 255) / 256, 512)), dim3(256), 0, s, p_dev, h->mw_tab, h->mg);
        HIPCHK(h, hipGetLastError());
        return RNDE_OK;
    }
    const long long total = (long long)(h->cg.nfrag_f + h->cg.nfrag_b + h->cg.nfrag_t) * 64;
    hipLaunchKernelGGL(rnde_chain_pack_kernel, dim3((int)std::min<long long>((total + 255) / 256, 512)), dim3(256), 0, s, p_dev, h->cfrags, h->cg);
    HIPCHK(h, hipGetLastError());
    return RNDE_OK;
}
static hipError_t chain_convert(const float* src, float* dst, int D, int B, int ntiles, int nksD, int to_caller, hipStream_t s) {
    const long long total = (long long)ntiles * nksD * 64;
    hipLaunchKernelGGL(rnde_chain_convert_kernel, dim3((int)std::min<long long>((total + 255) / 256, 512)), dim3(256), 0, s, src, dst, D, B, ntiles, nksD, to_caller);
    return hipGetLastError();
}

extern "C" rnde_status rnde_node_create(const rnde_node_config* c, rnde_node** out) {
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= c->device) { g_create_err = "no HIP device"; return RNDE_ERR_NO_DEVICE; }
    if ((c->solver != RNDE_SOLVER_TSIT5 && c->solver != RNDE_SOLVER_DP5 && c->solver != RNDE_SOLVER_DOP853) || c->n_layers < 1 || c->n_layers > RNDE_MAX_LAYERS || c->dims[0] != c->dims[c->n_layers]) {
        g_create_err = "unsupported configuration: Tsit5 (or DP5) over a Dense chain with dims[0] == dims[n_layers]"; return RNDE_ERR_BAD_ARG;
    }
    if (c->pre_act != RNDE_PRE_NONE && c->pre_act != RNDE_PRE_TANH && c->pre_act != RNDE_PRE_CUBE) {
        g_create_err = "pre_act: RNDE_PRE_NONE, RNDE_PRE_TANH or RNDE_PRE_CUBE"; return RNDE_ERR_BAD_ARG;
    }
    if (!rnde_check_acts(c->n_layers, c->act, "act", g_create_err)) return RNDE_ERR_BAD_ARG;
    const bool mnist_form = c->n_layers == 2 && c->time_dep && !c->pre_act && c->act[0] == RNDE_ACT_TANH;
    if (mnist_form && c->col_tile != 64 && c->col_tile != 65 && c->act[1] != RNDE_ACT_IDENTITY && c->act[1] != RNDE_ACT_TANH) {
        // (not handed to the chain engine instead: this form is the one for widths beyond its limit of 64)
        g_create_err = std::string("act[1] = ") + rnde_act_name(c->act[1]) + ": the stage engine (two time-dependent layers, act[0] = tanh, no pre_act, col_tile 0 / 16) "
                       "serves identity or tanh in its second layer; a chain of width <= 64 runs any served activation on the chain engine (col_tile 64 / 65)";
        return RNDE_ERR_BAD_ARG;
    }
    if ((c->solver == RNDE_SOLVER_DP5 || c->solver == RNDE_SOLVER_DOP853) && ((mnist_form && c->col_tile != 65) || c->col_tile == 64 || c->regularize >= RNDE_REG_STIFF)) {
        g_create_err = "DP5 / DOP853 run on the tableau-as-data kernels of the chain engine (col_tile 0 for Dense chains of width <= 64, or 65), callbacks none / EEst*dt";
        return RNDE_ERR_BAD_ARG;
    }
    if (c->col_tile == 64 || c->col_tile == 65 || !mnist_form) return chain_create(c, out);   // small-width chains (latent_ode.jl:113-124): rnde_chain.h
    if (c->regularize < RNDE_REG_NONE || c->regularize > RNDE_REG_STIFF_DT) { g_create_err = "regularize: unknown value"; return RNDE_ERR_BAD_ARG; }
    std::unique_ptr<rnde_node, void (*)(rnde_node*)> hold(new rnde_node(), rnde_node_destroy);      // (until the last step has succeeded)
    rnde_node* h = hold.get();
    h->cfg = *c;
    h->D = c->dims[0]; h->H = c->dims[1]; h->P = rnde_param_count(c); h->act2 = c->act[1];
    h->BT = 8;   // (column granularity of the batch padding the tape's copy of x is zero-filled to)
    if (c->col_tile != 0 && c->col_tile != 16) {
        g_create_err = "col_tile must be 0 (auto) or 16 (stage engine) for the two-layer TDChain form; 64 / 65 select the chain engine.  (The round-1 column-owner "
                       "engine, col_tile 4 / 8, was retired in round 4: 126 us per attempted step against 24; its sources are kept under tools/experiments/column_owner/.)";
        return RNDE_ERR_BAD_ARG;
    }
    if (h->H + 2 > 128 || h->D < 1 || h->H < 1 || (h->D + 15) / 16 > 64 || c->max_batch < 1 || c->max_attempts < 1) {
        g_create_err = "shape outside the kernel limits (H <= 126, D <= 1024)"; return RNDE_ERR_BAD_ARG;
    }
    h->Bpad_max = ((c->max_batch + 15) / 16) * 16;
    // stage engine geometry: WT row tiles (waves) per block chosen to minimise padding, preferring more waves
    h->sMT = (h->D + 15) / 16; h->sHT = (h->H + 1 + 15) / 16; h->sK2b = (h->H + 2 + 15) / 16; h->sKHb = (h->H + 15) / 16;
    { int best = 1, bw = 1 << 30;
      for (int wt = std::min(8, h->sMT); wt >= std::max(1, std::min(4, h->sMT)); --wt) { int R = (h->sMT + wt - 1) / wt; int waste = R * wt - h->sMT; if (waste < bw) { bw = waste; best = wt; } }
      if (const char* e = getenv("RNDE_STAGE_WT")) { const int v = atoi(e); if (v >= 1 && v <= 8) best = std::min(v, h->sMT); }   // (experiments: row tiles per workgroup)
      h->sWT = best; h->sR = (h->sMT + best - 1) / best; }
    h->engine = 2;
    h->nwg_max = std::max(h->Bpad_max / h->BT, h->sR * (h->Bpad_max / 16));
    h->stage_lds = sizeof(float) * ((size_t)16 * (16 * std::max(h->sK2b, h->sHT) + 4) + (size_t)16 * (16 * std::max(h->sWT, h->sKHb) + 4) + 64);
    if (hipSetDevice(c->device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return RNDE_ERR_HIP; }
    const size_t A = (size_t)h->D * h->Bpad_max, HB = (size_t)h->H * h->Bpad_max;
    RecLayout L{(long long)A, (long long)HB};
    h->rec_stride = L.total();
    auto dm = [](auto& buf, size_t n) { return buf.alloc(n) == hipSuccess; };      // (n elements)
    bool ok = true;
    ok &= dm(h->f0, A) && dm(h->u1, A) && dm(h->f1, A) && dm(h->xcopy, A);
    ok &= dm(h->h0, HB) && dm(h->h1, HB);
    ok &= dm(h->pcopy, (size_t)h->P);
    ok &= dm(h->spwB, (size_t)h->sMT * h->sK2b * 64) && dm(h->spwD, (size_t)h->sHT * h->sMT * 64);
    ok &= dm(h->spwBt, (size_t)h->sMT * h->sKHb * 64) && dm(h->spwDt, (size_t)h->sHT * h->sMT * 64);
    ok &= dm(h->slab2, (size_t)2 * (h->Bpad_max / 16) * h->sR * h->sHT * 64 * 4);
    const size_t tslab_bytes = (size_t)kSlabBufs * (h->Bpad_max / 16) * h->sR * h->sHT * 64 * 16;    // buffers of one 16-byte entry per lane and tile: three for the attempts, two for the one-launch solve's start-up
    h->tslab_bytes = tslab_bytes;
    ok &= dm(h->tslab, tslab_bytes / 4);
    // mailbox: [0) final controller state | [512) initial-step record | [1016) abort word of the persistent kernels, [1024) their
    // XCC ids | [meta_off) step metadata -- read by the host with ONE copy per chunk (was five)
    static_assert(sizeof(StepState) <= 512 && sizeof(InitRec) <= 504, "mailbox layout");
    h->mbox_meta_off = (1024 + (size_t)h->nwg_max * 4 + 255) / 256 * 256;
    const size_t mbox_bytes = h->mbox_meta_off + (size_t)(c->max_attempts + 1) * sizeof(StepMeta);
    ok &= dm(h->mbox, mbox_bytes) && dm(h->h_mbox, mbox_bytes);
    if (ok) {
        hipMemset(h->mbox, 0, mbox_bytes);
        h->ctl_final = (StepState*)h->mbox.get(); h->initrec = (InitRec*)(h->mbox + 512);
        h->pabort = (unsigned*)(h->mbox + 1016); h->pxcc = (unsigned*)(h->mbox + 1024); h->meta = (StepMeta*)(h->mbox + h->mbox_meta_off);
        h->h_ctl = (StepState*)h->h_mbox.get(); h->h_init = (InitRec*)(h->h_mbox + 512);
        h->h_pchk = (unsigned*)(h->h_mbox + 1016); h->h_meta = (StepMeta*)(h->h_mbox + h->mbox_meta_off);
    }
    ok &= dm(h->ctl, 2);
    ok &= dm(h->errpart, (size_t)(6 * h->nwg_max + 256 + 16)) && dm(h->initpart, (size_t)(3 * h->nwg_max + 256));   // (+256: sum_partials reads whole 256-entry blocks; +16: the [2][4] doubles of rnde_epart_reduce_kernel)
    // scratch records: 2 (no-tape ring); grown to max_attempts on the first taped forward
    ok &= dm(h->arena, (size_t)2 * h->rec_stride);
    ok &= dm(h->h_scal, 64);
    if (!ok) { g_create_err = "device allocation failed"; return RNDE_ERR_HIP; }
    hipMemset(h->tslab, 0xFF, tslab_bytes); hipMemset(h->pabort, 0, 8); hipMemset(h->pxcc, 0, (size_t)h->nwg_max * 4);
    {   // tuning knobs: config fields, each with a create-time environment override for A/B tooling (never read per solve)
        const char* e = getenv("RNDE_PERSIST");
        const bool off = c->persist < 0 || (e && e[0] == '0');
        h->persist = (h->engine == 2 && h->sR <= 8 && !off) ? 1 : 0;
        if (const char* e2 = getenv("RNDE_PERSIST_SPINS")) h->persist_spins = atoi(e2);
        if (const char* e3 = getenv("RNDE_PERSIST2")) h->persist2 = atoi(e3);
        h->wgrad_side_pct = c->wgrad_side_pct < 0 ? 0 : (c->wgrad_side_pct == 0 ? 30 : std::min(100, c->wgrad_side_pct));
        if (const char* e3 = getenv("RNDE_WGRAD_SIDE")) h->wgrad_side_pct = atoi(e3);
        h->stage_generic = (c->stage_generic != 0 || getenv("RNDE_STAGE_GENERIC") != nullptr) ? 1 : 0;
        if (const char* e6 = getenv("RNDE_STAGE_SOLVE")) h->stage_solve = atoi(e6);
    }
    if (h->persist == 1 && h->stage_solve && c->max_attempts + kSolveInitRows < (int)kMeetRows) {      // meeting granules of the one-launch solve: [attempt | the start-up's two meetings][3][256] x 8 bytes
        if (h->s_meet.create_granules((size_t)c->max_attempts + kSolveInitRows, 3, 256) != hipSuccess) { g_create_err = "device allocation failed"; return RNDE_ERR_HIP; }
    }
    // the stage kernels' Dense layers on the matrix cores (rnde_x3.h): split weight images for the headline geometry (49 row tiles, 7 x 7 (hidden tile, row
    // block) pairs) whenever the one-launch-per-attempt kernels are in use (persist == 1) -- with or without the one-launch solve
    if (h->persist == 1) {
        h->x3 = 1;      // default where the geometry fits (include/rnde.h: rnde_node_set_matrix_mode)
        if (const char* e7 = getenv("RNDE_X3")) h->x3 = atoi(e7) != 0;
        if (stage_fix(h, h->sWT, h->sHT, h->sK2b, h->sMT, h->sR)) {
            const size_t img = (size_t)49 * 4 * 3 * 64 * 16;
            if (!(dm(h->x3B, img) && dm(h->x3D, img) && dm(h->x3Bt, img) && dm(h->x3Dt, img))) { g_create_err = "device allocation failed"; return RNDE_ERR_HIP; }
        } else h->x3 = 0;
    }
    h->predicted = 12;
    *out = hold.release();
    return RNDE_OK;
}

extern "C" void rnde_node_destroy(rnde_node* h) {
    if (!h) return;
    node_tiled_destroy(h);
    delete h;      // (every buffer, event and stream is an owner: rnde_node.h)
}

// ---- SURVEY 8e mode 2: one controller for all shards (include/rnde.h: rnde_node_set_coupling).  Every launch that leaves per-workgroup
// partial sums of a batch-wide norm is followed by an all-reduce of that partial array over the shards, on the same stream: the kernels
// that consume the partials are unchanged (they sum the array in a fixed order, which now holds the element-wise sums over the ranks).
rnde_status couple_sum(rnde_node* h, float* partials, long long count, hipStream_t s) {
    if (!h->couple) return RNDE_OK;
    const rnde_status st = rnde_comm_allreduce(h->couple, partials, count, 0, (void*)s);
    if (st != RNDE_OK) h->err = std::string("coupled controller: ") + rnde_comm_last_error(h->couple);
    return st;
}
extern "C" rnde_status rnde_node_set_coupling(rnde_node* h, rnde_comm* c, int32_t global_batch) {
    if (!h) return RNDE_ERR_BAD_ARG;
    RNDE_TILED_REFUSE(h, "rnde_node_set_coupling is not served (one controller over several shards: the stage engine and the chain engine's multi-wave kernels, rnde_node_create)");
    if (!c) { h->couple = nullptr; h->couple_batch = 0; h->couple_world = 1; return RNDE_OK; }
    const int world = rnde_comm_world(c);
    if (h->engine != 2 && !(h->engine == 3 && h->mw)) { h->err = "coupled controller: the stage engine (MNIST form, col_tile 0 or 16) and the chain engine's multi-wave kernels only"; return RNDE_ERR_BAD_ARG; }
    if (global_batch < world || world < 1) { h->err = "coupled controller: global_batch must cover every rank"; return RNDE_ERR_BAD_ARG; }
    h->couple = c; h->couple_batch = global_batch; h->couple_world = world;
    return RNDE_OK;
}

static rnde_status ensure_arena(rnde_node* h, long long recs) {
    HIPCHK(h, h->arena.reserve((size_t)recs * h->rec_stride));
    return RNDE_OK;
}

static StageParams make_stage_params(rnde_node* h, const StepParams& P, const float* p_dev) {
    StageParams Q{};
    Q.F = P; Q.p = p_dev; Q.pwB = h->spwB; Q.pwD = h->spwD; Q.slab = h->slab2;
    Q.MT = h->sMT; Q.WT = h->sWT; Q.R = h->sR; Q.C = P.Bpad / 16; Q.HT = h->sHT; Q.K2b = h->sK2b; Q.Bpad16 = P.Bpad;
    return Q;
}
template <int ACT2, int MODE>
static hipError_t launch_stage_t(rnde_node* h, const StageParams& Q, int n, int s, hipStream_t st) {
    hipLaunchKernelGGL((rnde_stage_kernel<ACT2, MODE>), dim3(Q.R * Q.C), dim3(64 * Q.WT), h->stage_lds, st, Q, n, s);
    return hipGetLastError();
}
template <int MODE>
static hipError_t launch_stage(rnde_node* h, const StageParams& Q, int n, int s, hipStream_t st) {
    return h->act2 ? launch_stage_t<1, MODE>(h, Q, n, s, st) : launch_stage_t<0, MODE>(h, Q, n, s, st);
}
hipError_t stage_pack(rnde_node* h, const float* p, f32x4* dst, int which, int MTrows, int Kb, hipStream_t st) {
    const long long total = (long long)MTrows * Kb * 64;
    const int grid = (int)std::min<long long>((total + 255) / 256, 1024);
    hipLaunchKernelGGL(rnde_stage_pack_kernel, dim3(grid), dim3(256), 0, st, p, dst, which, h->D, h->H, MTrows, Kb);
    return hipGetLastError();
}
// matrix mode 1 (rnde_x3.h): the weights split into three bf16 planes for the x3 kernels, in front of every forward (p changes between training steps);
// with_rev: the transposed pair of the reverse attempt kernel in the same launch.  Sets "this forward's stage kernels run with x3".
static rnde_status x3_pack(rnde_node* h, const float* p_dev, bool with_rev, hipStream_t s) {
    h->x3_fwd = false;
    if (!(h->x3 && h->x3B && h->x3D && h->persist == 1 && !h->stage_generic)) return RNDE_OK;
    HIPCHK(h, rnde_launch_x3_pack(p_dev, h->x3B, h->x3D, with_rev ? h->x3Bt : nullptr, with_rev ? h->x3Dt : nullptr, h->D, h->H, h->sMT, h->sWT, h->sR, h->sHT, s));
    h->x3_fwd = true;
    h->x3_packed = with_rev;
    return RNDE_OK;
}
static rnde_status stage_pack_weights(rnde_node* h, const float* p_dev, hipStream_t s) {
    HIPCHK(h, stage_pack(h, p_dev, h->spwB, 0, h->sMT, h->sK2b, s));
    HIPCHK(h, stage_pack(h, p_dev, h->spwD, 1, h->sHT, h->sMT, s));
    return x3_pack(h, p_dev, false, s);
}
rnde_status stage_pack_all(rnde_node* h, const float* p_dev, hipStream_t s, const float* x_src, long long x_floats) {
    PackJobs J{};
    int n = 0;
    auto add = [&](void* dst, long long total, int kind, int which, int kdim, const float* src = nullptr) { J.j[n++] = PackJob{dst, src, total, kind, which, kdim, 0}; };
    add(h->spwB, (long long)h->sMT * h->sK2b * 64, 0, 0, h->sK2b);
    add(h->spwD, (long long)h->sHT * h->sMT * 64, 0, 1, h->sMT);
    add(h->spwBt, (long long)h->sMT * h->sKHb * 64, 0, 2, h->sKHb);
    add(h->spwDt, (long long)h->sHT * h->sMT * 64, 0, 3, h->sMT);
    auto add_copy = [&](float* dst, const float* src, long long floats) {     // 16-byte copies where sizes and addresses allow
        const bool v4 = floats % 4 == 0 && ((uintptr_t)dst % 16 == 0) && ((uintptr_t)(src ? src : p_dev) % 16 == 0);
        add(dst, v4 ? floats / 4 : floats, v4 ? 3 : 2, 0, 0, src);
    };
    add_copy(h->pcopy, nullptr, (long long)h->P);
    if (x_src) add_copy(h->xcopy, x_src, x_floats);           // the tape's copy of x rides along (was a launch of its own)
    // matrix mode 1 in effect (x3_pack's condition) and RNDE_X3_PACK_FOLD=1 (read per call; off by default): the split weights ride along too,
    // transposed pair included, instead of rnde_x3_pack_kernel behind this launch -- byte for byte the same images
    const bool x3_in = h->x3 && h->x3B && h->x3D && h->persist == 1 && !h->stage_generic && tail_switch("RNDE_X3_PACK_FOLD", false);
    if (x3_in) {
        const bool rev = h->x3Bt && h->x3Dt;
        J.x3 = X3PackDst{{(x3u4*)h->x3B.get(), (x3u4*)h->x3D.get(), rev ? (x3u4*)h->x3Bt.get() : nullptr, rev ? (x3u4*)h->x3Dt.get() : nullptr}};
        J.MT = h->sMT; J.WT = h->sWT; J.R = h->sR; J.HT = h->sHT;
        add(nullptr, x3_pack_count(J.x3, J.MT, J.R, J.HT), 4, 0, 0);
    }
    long long most = 0;
    for (int i = 0; i < n; ++i) most = std::max(most, J.j[i].total);
    const int grid = (int)std::min<long long>((most + 255) / 256, 256);
    hipLaunchKernelGGL(rnde_pack_all_kernel, dim3(grid, n), dim3(256), 0, s, p_dev, J, h->D, h->H);
    HIPCHK(h, hipGetLastError());
    h->rev_packed = true;
    if (x3_in) { h->x3_fwd = true; h->x3_packed = true; ++h->tail_folds[2]; return RNDE_OK; }      // (what x3_pack records behind its launch)
    return x3_pack(h, p_dev, true, s);
}
// The hand-off slabs must read "empty" wherever the persistent kernels have not written in the current tile indexing: at
// creation, and whenever the padded batch width (= number of column tiles) differs from the last persistent launch's.
hipError_t slab_prepare(rnde_node* h, int Bpad, hipStream_t s) {
    if (h->tslab_Bpad == Bpad) return hipSuccess;
    h->tslab_Bpad = Bpad;
    return hipMemsetAsync(h->tslab, 0xFF, h->tslab_bytes, s);
}
// the two-tile attempt kernel serves this geometry (rnde_stage_persist2.h): the headline network, an even number of column tiles, enough of them
static bool stage_two_tile(const rnde_node* h, const StageParams& Q) {
    return h->persist == 1 && stage_fix(h, Q.WT, Q.HT, Q.K2b, Q.MT, Q.R) && Q.C % 2 == 0 && h->persist2 != 0 && (Q.C >= kPersist2MinTiles || h->persist2 >= 1);
}
// large batches: the error partials of an attempt summed once behind its launch (rnde_epart_reduce_kernel) instead of in every workgroup's prologue of the next --
// from ~900 partials on (B >= 2048), where the two-tile kernel runs; RNDE_NO_EPART_REDUCE=1: A/B
static bool stage_epart_reduce(const rnde_node* h, const StageParams& Q) {
    return stage_two_tile(h, Q) && Q.F.nwg >= 896 && !getenv("RNDE_NO_EPART_REDUCE");
}
static hipError_t stage_attempt(rnde_node* h, const StageParams& Q, int n, hipStream_t s) {
    if (h->persist != 1) {
        hipError_t e = launch_stage<SM_START>(h, Q, n, 0, s);
        for (int st = 1; st <= 5 && e == hipSuccess; ++st) e = launch_stage<SM_STAGE>(h, Q, n, st, s);
        if (e == hipSuccess) e = launch_stage<SM_LAST>(h, Q, n, 6, s);
        return e;
    }
    // one launch per attempt, slab hand-offs inside the kernel (rnde_stage_persist.h)
    using AttemptKern = void (*)(StageParams, int, PersistSync, const void*, const void*);
    // batches that fill the chip more than once: two column tiles per workgroup (rnde_stage_persist2.h; bit-identical results).
    // RNDE_PERSIST2=0 keeps one tile per workgroup (A/B and the bit-identity test), =1 takes two whenever the tile count is even.
    static constexpr AttemptKern kTwoTile[2][2] = {{rnde_stage_attempt_mt_kernel<0, 2>, rnde_stage_attempt_mt_kernel<0, 2, 1>},
                                                   {rnde_stage_attempt_mt_kernel<1, 2>, rnde_stage_attempt_mt_kernel<1, 2, 1>}};      // [ACT2][x3]
    static constexpr size_t lds2[2] = {sizeof(float) * (2 * 2 * 16 * (16 * 7 + 4) + 32 * 3), sizeof(float) * ((size_t)2 * 2 * kX3ImageFloats + 32 * 3)};      // [x3]
    // one tile: the generic kernel, the headline geometry, and the headline geometry in matrix mode 1 -- the same instruction sequence as the x3
    // one-launch solve (bit-identical to it)
    static constexpr AttemptKern kOneTile[2][3] = {{rnde_stage_attempt_kernel<0, 0>, rnde_stage_attempt_kernel<0, 1>, rnde_stage_attempt_kernel<0, 1, 1>},
                                                   {rnde_stage_attempt_kernel<1, 0>, rnde_stage_attempt_kernel<1, 1>, rnde_stage_attempt_kernel<1, 1, 1>}};      // [ACT2][generic | fixed | fixed x3]
    const size_t lds1[3] = {h->stage_lds, h->stage_lds, sizeof(float) * ((size_t)2 * kX3ImageFloats + 64)};
    PersistSync Y{h->tslab, h->pabort, h->pxcc, h->persist_spins};
    if (hipError_t e = slab_prepare(h, Q.Bpad16, s); e != hipSuccess) return e;
    static const bool x3_over_mt = !(getenv("RNDE_X3_MT") && atoi(getenv("RNDE_X3_MT")) == 0);      // (A/B: 0 = keep the fp32 two-tile kernel for large batches even in matrix mode 1)
    const int a2 = h->act2 ? 1 : 0;
    const bool two = stage_two_tile(h, Q);
    const bool x3 = h->x3_fwd && (two ? x3_over_mt : stage_fix(h, Q.WT, Q.HT, Q.K2b, Q.MT, Q.R));
    const void* const xB = x3 ? (const void*)h->x3B : nullptr;
    const void* const xD = x3 ? (const void*)h->x3D : nullptr;
    if (two) hipLaunchKernelGGL(kTwoTile[a2][x3], dim3(8 * Q.R * ((Q.C / 2 + 7) / 8)), dim3(64 * 7), lds2[x3], s, Q, n, Y, xB, xD);
    else {
        const int form = x3 ? 2 : (stage_fix(h, Q.WT, Q.HT, Q.K2b, Q.MT, Q.R) ? 1 : 0);
        // a column tile's row blocks share blockIdx % 8 (same XCD)
        hipLaunchKernelGGL(kOneTile[a2][form], dim3(8 * Q.R * ((Q.C + 7) / 8)), dim3(64 * Q.WT), lds1[form], s, Q, n, Y, xB, xD);
    }
    return hipGetLastError();
}

// The one-launch reverse sweep of the chain engine (rnde_bchainmw.h SWEEP) leaves its verdict in h_mw_bchk behind the sweep; looked at after the
// next stream synchronisation.  true: a meeting timed out or the workgroups did not share an XCD -- the sweep's outputs are invalid, the handle
// goes back to one launch per reversed attempt.
bool bsweep_failed(rnde_node* h, hipStream_t s) {
    if (!h->pending_bsweep) return false;
    h->pending_bsweep = false;
    const MeetVerdict v = meet_verdict(h->h_mw_bchk, h->bsweep_nt, h->bsweep_global);      // the sweep's own geometry, recorded at its launch (h->B may already belong to the next forward)
    if (v == MEET_OK) return false;
    fprintf(stderr, "[rnde] chain engine: one-launch reverse sweep abandoned (%s); one launch per reversed attempt for the next %d solves\n",
            v == MEET_TIMED_OUT ? "a meeting timed out" : "workgroups pinned by block index landed on different XCDs", h->mw_retry_after);
    h->mw_bsweep = -1; h->mw_clean = 0; ++h->persist_fallbacks;
    h->mw_meet.clear_abort(s);
    h->h_mw_bchk[0] = 0;
    return true;
}

// After a synchronisation point: did a persistent launch time out, or did a column tile's workgroups land on different
// XCDs (then their slab hand-off through L2 would not be coherent)?  Either way the persistent kernels are disabled for
// this handle and the caller redoes the solve with the multi-launch kernels.
// (two halves so that the two small copies ride on a synchronisation the caller performs anyway)
void persist_check_enqueue(rnde_node* h, int grid, hipStream_t s) {
    if (h->persist != 1) return;
    h->h_pchk[0] = 1;   // stays 1 ("failed") if a copy cannot even be enqueued
    if (hipMemcpyAsync(h->h_pchk, h->pabort, 8, hipMemcpyDeviceToHost, s) != hipSuccess) return;
    (void)hipMemcpyAsync(h->h_pchk + 2, h->pxcc, (size_t)grid * 4, hipMemcpyDeviceToHost, s);
}
bool persist_check_result(rnde_node* h, int C, int R, hipStream_t s) {   // call after the stream has been synchronised
    if (h->persist != 1) return false;
    bool bad = h->h_pchk[0] != 0;
    for (int ct = 0; ct < C && !bad; ++ct)
        for (int rb = 1; rb < R; ++rb) if (h->h_pchk[2 + rb * C + ct] != h->h_pchk[2 + ct]) { bad = true; break; }
    if (bad) {
        fprintf(stderr, "[rnde] persistent attempt kernel suspended (%s); using the multi-launch kernels for the next %d solves\n",
                h->h_pchk[0] ? "hand-off timed out" : "column tile spans XCDs", h->persist_retry_after);
        h->persist = -1; h->persist_clean = 0; ++h->persist_fallbacks;
        hipMemsetAsync(h->pabort, 0, 8, s);
    }
    return bad;
}
static bool persist_failed(rnde_node* h, int grid, int C, int R, hipStream_t s) {
    if (h->persist != 1) return false;
    persist_check_enqueue(h, grid, s);
    if (hipStreamSynchronize(s) != hipSuccess) return true;
    return persist_check_result(h, C, R, s);
}

// ---- one dispatch for the three engines (stage, one-wave chain, multi-wave chain): the forward solve, rnde_debug_attempt and rnde_bench_attempt* ----
struct EngineParams { StepParams P; StageParams SQ; ChainParams CQ; MwParams MQ; };      // the engine's own blocks are filled, the others stay empty
static EngineParams engine_params(rnde_node* h, const StepParams& P, const float* p_dev) {
    EngineParams E{};
    E.P = P;
    if (h->engine != 3) E.SQ = make_stage_params(h, P, p_dev);
    else { E.CQ = make_chain_params(h, P); if (h->mw) E.MQ = make_mw_params(h, P); }
    return E;
}
static hipError_t launch_attempt(rnde_node* h, const EngineParams& E, int n, hipStream_t s) {
    if (h->engine == 3 && h->mw) return launch_mw<MW_STEP>(h, E.MQ, n, s);
    if (h->engine == 3) return launch_chain<CM_STEP>(h, E.CQ, n, nullptr, s);
    return stage_attempt(h, E.SQ, n, s);
}
// controller state after n attempts to ctl_final, the end state to u_out (may be null)
static hipError_t launch_finish(rnde_node* h, EngineParams& E, int n, float* u_out, hipStream_t s) {
    if (h->engine == 3 && h->mw) { E.MQ.u_out = u_out; return launch_mw<MW_FINISH>(h, E.MQ, n, s); }
    if (h->engine == 3) return launch_chain<CM_FINISH>(h, E.CQ, n, u_out, s);
    hipLaunchKernelGGL(rnde_stage_finish_kernel, dim3(256), dim3(256), 0, s, E.SQ, n, u_out);
    return hipGetLastError();
}
// the two halves of the initial-step rule: f(u0, t0) into f0 with the norms of u0 and f0, then f(u1, t0 + dt0) with the norm of f1 - f0
static hipError_t launch_init(rnde_node* h, const EngineParams& E, int half, hipStream_t s) {
    if (h->engine == 3 && h->mw) return half ? launch_mw<MW_INIT_B>(h, E.MQ, 0, s) : launch_mw<MW_INIT_A>(h, E.MQ, 0, s);
    if (h->engine == 3) return half ? launch_chain<CM_INIT_B>(h, E.CQ, 0, nullptr, s) : launch_chain<CM_INIT_A>(h, E.CQ, 0, nullptr, s);
    const hipError_t e = half ? launch_stage<SM_I3>(h, E.SQ, 0, 0, s) : launch_stage<SM_I1>(h, E.SQ, 0, 0, s);
    return e != hipSuccess ? e : (half ? launch_stage<SM_I4>(h, E.SQ, 0, 0, s) : launch_stage<SM_I2>(h, E.SQ, 0, 0, s));
}
// weights in the engine's layout in front of an untaped call
static rnde_status pack_untaped(rnde_node* h, const float* p_dev, hipStream_t s) { return h->engine == 3 ? chain_pack(h, p_dev, s) : stage_pack_weights(h, p_dev, s); }

#ifdef RNDE_DIAG
#include "rnde_diag.h"      // (tools/build_diag.sh) cycle-stamp reports of the forward: RNDE_DIAG_SOLVE, RNDE_DIAG_FWD, rnde_bench_attempt*
#endif

// controller state, the first n step records and the initial-step record on their way to the host (stage engine: contiguous in the mailbox, with
// the persistent kernels' health words)
static rnde_status fetch_log(rnde_node* h, int n, hipStream_t s) {
    if (h->mbox) { HIPCHK(h, hipMemcpyAsync(h->h_mbox, h->mbox, h->mbox_meta_off + (size_t)n * sizeof(StepMeta), hipMemcpyDeviceToHost, s)); return RNDE_OK; }
    HIPCHK(h, hipMemcpyAsync(h->h_ctl, h->ctl_final, sizeof(StepState), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(h->h_meta, h->meta, (size_t)n * sizeof(StepMeta), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(h->h_init, h->initrec, sizeof(InitRec), hipMemcpyDeviceToHost, s));
    return RNDE_OK;
}
// The host waits for the copies behind a solve.  Fused training step (after_solve): for the copies only; what the hook queues runs while the host
// wakes up.  A solve that needs another chunk, or is redone, calls the hook again: it only overwrites its outputs.
static rnde_status wait_for_host(rnde_node* h, hipStream_t s) {
    if (h->after_solve) {
        HIPCHK(h, hipEventRecord(h->ev_host, s));
        const rnde_status hs = h->after_solve(s);
        if (hs != RNDE_OK) return hs;
        HIPCHK(h, hipEventSynchronize(h->ev_host));
    } else HIPCHK(h, hipStreamSynchronize(s));
    return RNDE_OK;
}
// Behind that wait: did a one-launch kernel give up?  RNDE_ERR_HIP: one of the previous asynchronous backward call did (or may have), whose gradients
// cannot be trusted; RNDE_INTERNAL_RETRY: a persistent kernel of this solve did, the handle fell back and the solve is to be redone.
static rnde_status previous_backward_ok(rnde_node* h, hipStream_t s) {
    if (bsweep_failed(h, s)) { h->err = "the one-launch reverse sweep of the previous asynchronous backward call was abandoned: the gradients of that step are invalid (one launch per reversed attempt now in use)"; return RNDE_ERR_HIP; }
    if (!persist_check_result(h, h->Bpad / 16, h->sR, s)) return RNDE_OK;
    if (h->pending_bwd) {   // the failure may belong to the asynchronous reverse pass before this forward: its outputs cannot be trusted
        h->pending_bwd = false;
        h->err = "a persistent kernel abandoned its hand-off during or after the previous asynchronous reverse pass: the gradients of that step are invalid (multi-launch kernels now in use)";
        return RNDE_ERR_HIP;
    }
    return RNDE_INTERNAL_RETRY;
}

struct FwdCall {      // one forward solve: the caller's arguments; what forward_prepare made of them (cap: max_attempts; the one-launch stage solve applies, its start-up and finish run inside it)
    const float *x_dev, *p_dev; int B; float t0, t1; float* u_out_dev; const float* saveat_host; int n_saveat; float* sv_out_dev; int keep_tape; hipStream_t s;
    EngineParams E; int cap; bool stage_one_launch, solve_fold;
};
// Validation, the tape's copies, the parameter blocks, the pack launch and the launches of the initial-step rule.
static rnde_status forward_prepare(rnde_node* h, FwdCall& c) {
    hipStream_t s = c.s;
    const int B = c.B, keep_tape = c.keep_tape, n_saveat = c.n_saveat;
    if (n_saveat > 0) {
        if (h->rk_tab == 2) { h->err = "saveat: this Runge-Kutta table carries no dense output (DOP853)"; return RNDE_ERR_BAD_ARG; }
        if (!saveat_valid(c.saveat_host, n_saveat, c.t0, c.t1)) { h->err = "saveat must be increasing and inside [t0, t1]"; return RNDE_ERR_BAD_ARG; }
        HIPCHK(h, h->sv_t_dev.reserve((size_t)n_saveat));
        h->saveat.assign(c.saveat_host, c.saveat_host + n_saveat);
        HIPCHK(h, hipMemcpyAsync(h->sv_t_dev, h->saveat.data(), (size_t)n_saveat * 4, hipMemcpyHostToDevice, s));
    } else h->saveat.clear();
    if (B < 1 || B > h->cfg.max_batch || !(c.t1 > c.t0)) { h->err = "bad B or tspan"; return RNDE_ERR_BAD_ARG; }
    // the coupled controller all-reduces per-workgroup partial arrays element by element: every rank must hold the same number of columns
    if (h->couple && (long long)B * h->couple_world != h->couple_batch) {
        h->err = "coupled controller: equal shards only (B * world must equal the global batch given to rnde_node_set_coupling)";
        return RNDE_ERR_BAD_ARG;
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->have_tape = false; h->rev_packed = false; h->x3_packed = false; h->x3_fwd = false;
    const float* x_dev = c.x_dev;
    const float* x_caller = nullptr;
    if (keep_tape) {
        rnde_status st = ensure_arena(h, h->cfg.max_attempts);
        if (st != RNDE_OK) return st;
        // the tape owns copies of x and p (the caller may free or overwrite its buffers before backward)
        if (B % h->BT) HIPCHK(h, hipMemsetAsync(h->xcopy, 0, (size_t)h->D * (((B + h->BT - 1) / h->BT) * h->BT) * 4, s));
        if (h->engine != 2) {   // (stage engine: both copies are part of the one pack launch below)
            HIPCHK(h, hipMemcpyAsync(h->xcopy, x_dev, (size_t)h->D * B * 4, hipMemcpyDeviceToDevice, s));
            HIPCHK(h, hipMemcpyAsync(h->pcopy, c.p_dev, (size_t)h->P * 4, hipMemcpyDeviceToDevice, s));
        } else x_caller = x_dev;
        x_dev = h->xcopy;
    }
    StepParams P = make_params(h, x_dev, B, c.t0, c.t1, keep_tape ? 1 : 0);
    P.sv_t = n_saveat > 0 ? h->sv_t_dev : nullptr; P.nsave = n_saveat; P.sv_out = c.sv_out_dev;
    if (h->n_replay > 0) {
        HIPCHK(h, h->replay_dev.reserve((size_t)h->n_replay * 2));
        HIPCHK(h, hipMemcpyAsync(h->replay_dev, h->replay_host, (size_t)h->n_replay * 8, hipMemcpyHostToDevice, s));
        P.replay = h->replay_dev; P.n_replay = h->n_replay;
    }
    h->B = B; h->Bpad = P.Bpad; h->nwg = P.nwg; h->t0 = c.t0; h->t1 = c.t1;
    const float* const p_tape = keep_tape ? h->pcopy : c.p_dev;
    rnde_status st = RNDE_OK;
    if (h->engine == 2 && keep_tape) st = stage_pack_all(h, c.p_dev, s, x_caller, (long long)h->D * B);   // forward + reverse packs of both engines' layouts and the tape's copy of p: one launch
    else if (h->engine == 3) st = chain_pack(h, p_tape, s);
    if (st != RNDE_OK) return st;
    EngineParams& E = c.E;
    c.stage_one_launch = c.solve_fold = false;
    c.cap = h->cfg.max_attempts;
    if (h->engine == 3 && h->mw && keep_tape) st = ensure_mw_slab(h, 2 + (long long)(h->rk_S - 1) * std::max(4, h->predicted), s);
    if (h->engine == 2 && !keep_tape) st = stage_pack_weights(h, c.p_dev, s);
    if (st != RNDE_OK) return st;
    E = engine_params(h, P, p_tape);
    if (h->engine == 2) {
        StageParams& SQ = E.SQ;
        if (stage_epart_reduce(h, SQ)) SQ.F.esum = (const double*)(h->errpart + 6 * (size_t)h->nwg_max + 256);      // (inside errpart's allocation, 8-byte aligned)
        // the one-launch solve runs the initial-step rule and the copy-out of the final state inside its own launch; RNDE_SOLVE_FOLD=0, read per
        // call, keeps the four start-up launches and the finish launch around it (a redo after a time-out takes them too: persist != 1 then)
        c.stage_one_launch = h->persist == 1 && h->stage_solve && h->s_meet.xch && SQ.C <= 32 && n_saveat == 0 && h->n_replay == 0 && !h->couple &&
                             stage_fix(h, SQ.WT, SQ.HT, SQ.K2b, SQ.MT, SQ.R);
        if (c.stage_one_launch) { const char* e = getenv("RNDE_SOLVE_FOLD"); c.solve_fold = !(e && e[0] == '0'); }
    }
    if (!c.solve_fold) {      // (coupled controller: the partial norms summed over the ranks behind each half)
        HIPCHK(h, launch_init(h, E, 0, s));
        if ((st = couple_sum(h, P.initpart, 2LL * P.nwg, s)) != RNDE_OK) return st;            // norms of u0 and f0
        HIPCHK(h, launch_init(h, E, 1, s));
        if ((st = couple_sum(h, P.initpart + 2LL * P.nwg, P.nwg, s)) != RNDE_OK) return st;     // norm of f1 - f0
    }
    h->tev_fwd = false;
    if (h->timing) HIPCHK(h, hipEventRecord(h->tev[0], s));
    return RNDE_OK;
}

// The three forms of the solve, one signature: RNDE_OK = solved (the controller state, the step records and the initial-step record are on the
// host), RNDE_INTERNAL_RETRY = redo the whole call, anything else = the error.

// Chain engine, multi-wave kernels, every workgroup resident (<= 256 column tiles): the WHOLE adaptive solve is one launch (attempt loop,
// controller and the once-per-attempt meeting of the workgroups inside the kernel).  <= 32 tiles: the workgroups are pinned to one XCD
// and meet through its L2; more (B > 512, the throughput case): they spread over the chip and meet through agent-scope entries.
static bool mw_one_launch(const rnde_node* h, const StepParams& P) { return h->engine == 3 && h->mw && h->mw_solve > 0 && !h->couple && P.Bpad / 16 <= kMwMeetMax; }
static rnde_status solve_mw_one_launch(rnde_node* h, FwdCall& c) {
    hipStream_t s = c.s;
    MwParams& MQ = c.E.MQ;
    const int n_limit = c.keep_tape ? mw_taped_attempt_limit(c.cap, h->predicted) : c.cap;
    if (c.keep_tape) { const rnde_status st = ensure_mw_slab(h, 2 + (long long)(h->rk_S - 1) * n_limit, s); if (st != RNDE_OK) return st; MQ.slab = h->mw_slab; }
    MQ.n_limit = n_limit;
    MQ.meet = h->mw_meet.begin(c.E.P.Bpad / 16, true, s);
    HIPCHK(h, h->mw_meet.err);
    MQ.u_out = c.u_out_dev; MQ.xcc = h->mw_meet.xcc; MQ.xcd_slot = h->mw_meet.slot;
    HIPCHK(h, launch_mw<MW_SOLVE>(h, MQ, 0, s));
    if (h->timing) { HIPCHK(h, hipEventRecord(h->tev[1], s)); h->tev_fwd = true; }
    rnde_status st = fetch_log(h, c.cap, s);
    if (st != RNDE_OK) return st;
    HIPCHK(h, h->mw_meet.queue_check(MQ.meet, s));
    st = wait_for_host(h, s);
    if (st == RNDE_OK) st = previous_backward_ok(h, s);
    if (st != RNDE_OK) return st;
    const MeetVerdict verdict = meet_verdict(h->mw_meet.chk, MQ.meet.n, MQ.meet.global != 0);
    if (verdict != MEET_OK) {      // a meeting timed out, or the workgroups did not share an XCD: this handle goes back to one launch per attempt for the next mw_retry_after solves
        fprintf(stderr, "[rnde] chain engine: one-launch solve abandoned (%s); one launch per attempted step for the next %d solves\n",
                verdict == MEET_TIMED_OUT ? "a meeting timed out" : "workgroups pinned by block index landed on different XCDs", h->mw_retry_after);
        h->mw_solve = -1; h->mw_clean = 0; ++h->persist_fallbacks;
        h->mw_meet.clear_abort(s);
        return RNDE_INTERNAL_RETRY;
    }
    if (!h->h_ctl->done && h->h_ctl->n_att >= n_limit && n_limit < c.cap) { h->predicted = c.cap; return RNDE_INTERNAL_RETRY; }
    h->pending_bwd = false;
    ++h->one_launch_solves;
    return RNDE_OK;
}

// Stage engine, headline geometry, all workgroups resident at once (<= 32 column tiles): the WHOLE adaptive solve is one launch
// (rnde_stage_solve.h: weights, uprev and k1 stay in registers across attempts, the error norm meets through agent-scope granules).
static rnde_status solve_stage_one_launch(rnde_node* h, FwdCall& c) {
    hipStream_t s = c.s;
    const StageParams& SQ = c.E.SQ;
    PersistSync Y{h->tslab, h->pabort, h->pxcc, h->persist_spins};
    HIPCHK(h, slab_prepare(h, SQ.Bpad16, s));
    const Meet SM = h->s_meet.begin(SQ.F.nwg, false, s);      // (the granules and the epoch; the abort word is Y's)
    HIPCHK(h, h->s_meet.err);
    const int x3 = h->x3_fwd ? 1 : 0;      // (the weights were split by this forward's pack launch: x3_pack)
    SolveSync Z{SM.xch, SM.epoch, c.cap, h->x3B, h->x3D, c.solve_fold ? c.u_out_dev : nullptr, c.solve_fold ? 1 : 0};
#ifdef RNDE_DIAG
    const StageParams SD = diag_solve_params(h, SQ, s);      // (RNDE_DIAG_SOLVE: with a buffer for the cycle stamps)
#else
    const StageParams& SD = SQ;
#endif
    HIPCHK(h, rnde_launch_stage_solve(&SD, &Y, &Z, h->act2, x3, s));
    if (h->timing) { HIPCHK(h, hipEventRecord(h->tev[1], s)); h->tev_fwd = true; }
    if (!c.solve_fold) HIPCHK(h, launch_finish(h, c.E, -1, c.u_out_dev, s));
    const int cnt = stage_speculative_records(c.cap, h->predicted);
    rnde_status st = fetch_log(h, cnt, s);
    if (st == RNDE_OK) st = wait_for_host(h, s);
    if (st != RNDE_OK) return st;
#ifdef RNDE_DIAG
    diag_solve_report(h, SQ);
#endif
    if ((st = previous_backward_ok(h, s)) != RNDE_OK) return st;
    h->pending_bwd = false;
    if (h->h_ctl->n_att > cnt) {
        HIPCHK(h, hipMemcpyAsync(h->h_meta + cnt, h->meta + cnt, (size_t)(h->h_ctl->n_att - cnt) * sizeof(StepMeta), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
    }
    if (!h->h_ctl->done) { h->err = "max_attempts reached"; h->n_att = h->h_ctl->n_att; return RNDE_ERR_MAX_ATTEMPTS; }
    ++h->one_launch_solves;
    return RNDE_OK;
}

// Every engine: the attempts enqueued in chunks, one launch (stage engine without its persistent kernel: seven) per attempt, the controller state
// looked at once per chunk.
static rnde_status solve_chunked(rnde_node* h, FwdCall& c) {
    hipStream_t s = c.s;
    EngineParams& E = c.E;
    const StepParams& P = E.P;
    const bool mw_taped = h->engine == 3 && h->mw && c.keep_tape;
    int launched = 0;
    for (int chunk = first_chunk(h->couple != nullptr, h->predicted);; chunk = later_chunk(h->couple != nullptr)) {
        rnde_status st = RNDE_OK;
        if (mw_taped) {   // room in the activation slab for this chunk's evaluations (a regrowth keeps the taped ones)
            st = ensure_mw_slab(h, 2 + (long long)(h->rk_S - 1) * std::min(c.cap, launched + chunk), s);
            if (st != RNDE_OK) return st;
            E.MQ.slab = h->mw_slab;
        }
        for (int i = 0; i < chunk && launched < c.cap; ++i) {
#ifdef RNDE_DIAG
            if (diag_fwd_wants(h, launched)) HIPCHK(h, launch_attempt(h, diag_fwd_params(h, E, s), launched, s)); else      // (RNDE_DIAG_FWD: cycle stamps of THIS attempt of a real solve)
#endif
            HIPCHK(h, launch_attempt(h, E, launched, s));
            if ((st = couple_sum(h, P.errpart + (size_t)(launched & 1) * 3 * P.nwg, 3LL * P.nwg, s)) != RNDE_OK) return st;
            if (h->engine == 2 && E.SQ.F.esum) { hipLaunchKernelGGL(rnde_epart_reduce_kernel, dim3(1), dim3(64), 0, s, E.SQ.F, launched, (double*)E.SQ.F.esum); HIPCHK(h, hipGetLastError()); }
            ++launched;
        }
        if (h->timing && !h->tev_fwd) { HIPCHK(h, hipEventRecord(h->tev[1], s)); h->tev_fwd = true; }   // (first chunk: normally the whole solve)
        HIPCHK(h, launch_finish(h, E, launched, c.u_out_dev, s));
        // one synchronisation per chunk: controller state, the persistent kernels' health words, and (speculatively: the solve
        // usually ends in the first chunk) the step metadata and the initial-step record the epilogue needs
        if ((st = fetch_log(h, launched, s)) != RNDE_OK || (st = wait_for_host(h, s)) != RNDE_OK) return st;
#ifdef RNDE_DIAG
        diag_fwd_report(h);
#endif
        if (h->couple && rnde_comm_health(h->couple) != RNDE_OK) { h->err = std::string("coupled controller: ") + rnde_comm_last_error(h->couple); return RNDE_ERR_HIP; }
        st = previous_backward_ok(h, s);
        if (st == RNDE_INTERNAL_RETRY && h->couple) {   // a redo on this rank alone would leave the ranks' all-reduce sequences out of step
            h->err = "coupled controller: a persistent kernel abandoned its hand-off; the ranks are out of step -- use cfg.persist = -1 (7-launch kernels) with rnde_node_set_coupling where other work shares the GPU";
            return RNDE_ERR_HIP;
        }
        if (st != RNDE_OK) return st;
        h->pending_bwd = false;
        if (h->h_ctl->done) return RNDE_OK;
        if (launched >= c.cap) { h->err = "max_attempts reached"; h->n_att = h->h_ctl->n_att; return RNDE_ERR_MAX_ATTEMPTS; }
    }
}

// Attempt count and prediction, the two retry windows, NFE, the saved values, the controller's status.
static rnde_status forward_epilogue(rnde_node* h, const FwdCall& c, int64_t* nfe_out, float* saveval_host, int32_t* n_saveval_out) {
    h->n_att = h->h_ctl->n_att;
    h->predicted = h->n_att + 1;
    // a hand-off time-out (a co-tenant held CUs for a second, e.g. another process's kernels) must not halve the speed for good:
    // after `persist_retry_after` clean multi-launch solves the one-launch kernels get another chance; each new failure doubles the wait
    if (h->engine == 3 && (h->mw_solve == -1 || h->mw_bsweep == -1) && ++h->mw_clean >= h->mw_retry_after) {      // the same for the chain engine's one-launch kernels
        if (h->mw_solve == -1) h->mw_solve = 1;
        if (h->mw_bsweep == -1) h->mw_bsweep = 1;
        h->mw_retry_after = next_retry_window(h->mw_retry_after);
        h->mw_meet.slot = (h->mw_meet.slot + 1) & 7;                                           // (and another XCD: the one it was pinned to may be the contended one)
    }
    if (h->persist == -1 && h->engine == 2 && h->cfg.persist >= 0 && ++h->persist_clean >= h->persist_retry_after) {
        h->persist = 1; h->persist_retry_after = next_retry_window(h->persist_retry_after);
        h->tslab_Bpad = -1;                          // slabs are refilled with the empty pattern before the next persistent launch
    }
    if (nfe_out) *nfe_out = solve_nfe(h->rk_S, h->n_att);
    h->sv_index.assign(h->n_att, -1);
    h->n_saveval = gather_saved_values(h->h_meta, h->n_att, F_ACCEPT, h->cfg.regularize, h->cfg.cb_save_start != 0, h->sv_index.data(), saveval_host);
    if (n_saveval_out) *n_saveval_out = h->n_saveval;
    if (const SolveVerdict v = solve_verdict(h->h_ctl->status); v.st != RNDE_OK) { h->err = v.msg; return v.st; }
    h->have_tape = c.keep_tape != 0;
    return RNDE_OK;
}

static rnde_status forward_core(rnde_node* h, FwdCall& c, int64_t* nfe_out, float* saveval_host, int32_t* n_saveval_out) {
    rnde_status st = forward_prepare(h, c);
    if (st == RNDE_OK) st = mw_one_launch(h, c.E.P) ? solve_mw_one_launch(h, c) : (c.stage_one_launch ? solve_stage_one_launch(h, c) : solve_chunked(h, c));
    return st != RNDE_OK ? st : forward_epilogue(h, c, nfe_out, saveval_host, n_saveval_out);
}

rnde_status forward_impl(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1,
                                float* u_out_dev, const float* saveat_host, int32_t n_saveat, float* sv_out_dev,
                                int64_t* nfe_out, float* saveval_host, int32_t* n_saveval_out, int32_t keep_tape, void* stream) {
    if (!h) return RNDE_ERR_BAD_ARG;
    if (h->engine == 4) return node_tiled_forward(h, x_dev, p_dev, B, t0, t1, u_out_dev, saveat_host, n_saveat, sv_out_dev, nfe_out, saveval_host, n_saveval_out, keep_tape, stream);
    FwdCall c{x_dev, p_dev, B, t0, t1, u_out_dev, saveat_host, n_saveat, sv_out_dev, keep_tape, (hipStream_t)stream, {}, 0, false, false};
    // a solve may ask to be redone for two independent reasons (the record slab has to grow; a one-launch kernel gave up and the handle fell back):
    // both can happen back to back, each at most once per cause -- anything beyond that is an error, not a status the caller should ever see
    rnde_status st = RNDE_INTERNAL_RETRY;
    for (int tries = 0; tries < 4 && st == RNDE_INTERNAL_RETRY; ++tries) st = forward_core(h, c, nfe_out, saveval_host, n_saveval_out);
    if (st == RNDE_INTERNAL_RETRY) { h->err = "the forward solve asked to be redone four times in a row (one-launch fallbacks and slab growth): giving up"; st = RNDE_ERR_HIP; }
    return st;
}

extern "C" rnde_status rnde_node_forward(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B, float t0,
                                         float t1, float* u_out_dev, int64_t* nfe_out, float* saveval_host,
                                         int32_t* n_saveval_out, int32_t keep_tape, void* stream) {
    return forward_impl(h, x_dev, p_dev, B, t0, t1, u_out_dev, nullptr, 0, nullptr, nfe_out, saveval_host, n_saveval_out, keep_tape, stream);
}

extern "C" rnde_status rnde_node_forward_replay(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B, float t0,
                                                float t1, const float* steps_host, int32_t n_steps, float* u_out_dev,
                                                int64_t* nfe_out, float* saveval_host, int32_t* n_saveval_out,
                                                int32_t keep_tape, void* stream) {
    if (!h || !steps_host || n_steps < 1) return RNDE_ERR_BAD_ARG;
    if (n_steps > h->cfg.max_attempts) { h->err = "replay: more steps than max_attempts"; return RNDE_ERR_BAD_ARG; }
    h->replay_host = steps_host; h->n_replay = n_steps;
    const rnde_status st = forward_impl(h, x_dev, p_dev, B, t0, t1, u_out_dev, nullptr, 0, nullptr, nfe_out, saveval_host, n_saveval_out, keep_tape, stream);
    h->replay_host = nullptr; h->n_replay = 0;
    return st;
}

extern "C" rnde_status rnde_node_forward_saveat(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B, float t0,
                                                float t1, const float* saveat_host, int32_t n_saveat, float* u_saved_dev,
                                                int64_t* nfe_out, float* saveval_host, int32_t* n_saveval_out,
                                                int32_t keep_tape, void* stream) {
    if (!h || !saveat_host || n_saveat < 1 || !u_saved_dev) return RNDE_ERR_BAD_ARG;
    // every engine's solve reads the replay state of the handle, a saving solve included; rnde_node_forward_replay sets it for its own call and
    // clears it, so no saving call ever meets it -- except the one behind rnde_debug_arm_replay (the parity instrument for saved points)
    const bool armed = !h->replay_armed.empty();
    if (armed) { h->replay_host = h->replay_armed.data(); h->n_replay = (int)(h->replay_armed.size() / 2); }
    const rnde_status st = forward_impl(h, x_dev, p_dev, B, t0, t1, nullptr, saveat_host, n_saveat, u_saved_dev, nfe_out, saveval_host, n_saveval_out, keep_tape, stream);
    if (armed) { h->replay_host = nullptr; h->n_replay = 0; h->replay_armed.clear(); }
    return st;
}

extern "C" rnde_status rnde_debug_arm_replay(rnde_node* h, const float* steps_host, int32_t n_steps) {
    if (!h || n_steps < 0 || (n_steps > 0 && !steps_host)) return RNDE_ERR_BAD_ARG;
    if (n_steps > h->cfg.max_attempts) { h->err = "replay: more steps than max_attempts"; return RNDE_ERR_BAD_ARG; }
    h->replay_armed.assign(steps_host, steps_host + 2 * (size_t)n_steps);
    return RNDE_OK;
}

// save_everystep = true (reference src/models/neural_ode.jl:10-11: return_multiple = save_everystep || saveat): the state after every ACCEPTED step.
// Which times those are is known only after the solve, so the call runs it twice -- once untaped for the step sequence, once with the accepted
// step ends (and t0, if asked) as save times: the value saved at a step's end is u_new itself, no interpolation (dense_points, rnde_stage.h),
// and the second run repeats the first bit for bit (save times do not enter the controller).  A call shape for small problems: no reference
// experiment uses it (every multi-output call site passes saveat); the backward call afterwards is the saveat one.
extern "C" rnde_status rnde_node_forward_everystep(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B, float t0, float t1, int32_t save_start,
                                                   float* sol_out_dev, int32_t capacity, float* t_host_out, int32_t* n_out, int64_t* nfe_out,
                                                   float* saveval_host, int32_t* n_saveval_out, int32_t keep_tape, void* stream) {
    if (!h || !n_out || !sol_out_dev || capacity < 1) return RNDE_ERR_BAD_ARG;
    if (rnde_node_tiled_saveat_capacity(h) == 0)      // (a tiled handle without a saveat capacity: rnde_node_tiled_reserve_saveat switches saving on)
        RNDE_TILED_REFUSE(h, "rnde_node_forward_everystep is not served (the end state only; save_everystep runs on the engines of rnde_node_create)");
    rnde_status st = forward_impl(h, x_dev, p_dev, B, t0, t1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, stream);
    if (st != RNDE_OK) return st;
    const std::vector<float> times = step_end_times(h->h_meta, h->n_att, F_ACCEPT, t0, t1, save_start != 0);
    *n_out = (int32_t)times.size();
    if ((int)times.size() > capacity) { h->err = "rnde_node_forward_everystep: more accepted steps than the output has room for"; return RNDE_ERR_BAD_ARG; }
    if (t_host_out) memcpy(t_host_out, times.data(), times.size() * sizeof(float));
    st = forward_impl(h, x_dev, p_dev, B, t0, t1, nullptr, times.data(), (int32_t)times.size(), sol_out_dev, nfe_out, saveval_host, n_saveval_out, keep_tape, stream);
    if (st != RNDE_OK) return st;
    // "the value at a step's end is u_new itself, no interpolation" holds only if the second solve (another kernel path: it saves) took exactly the steps
    // the first one took -- the same arithmetic, so it must; checked, not assumed (round-4 review)
    const std::vector<float> again = step_end_times(h->h_meta, h->n_att, F_ACCEPT, t0, t1, save_start != 0);
    if (again.size() > times.size() || !std::equal(again.begin(), again.end(), times.begin())) { h->err = "rnde_node_forward_everystep: the saving solve did not retrace the steps of the first one"; return RNDE_ERR_HIP; }
    if (again.size() != times.size()) { h->err = "rnde_node_forward_everystep: the saving solve took fewer accepted steps than the first one"; return RNDE_ERR_HIP; }
    return RNDE_OK;
}

extern "C" rnde_status rnde_node_steps(rnde_node* h, float* steps_host, int32_t capacity, int32_t* n_out) {
    if (!h) return RNDE_ERR_BAD_ARG;
    const int n = std::min(capacity, h->n_att);
    export_step_log(h->h_meta, n, F_ACCEPT, steps_host);
    if (n_out) *n_out = h->n_att;
    return RNDE_OK;
}

extern "C" rnde_status rnde_node_attempts_ext(rnde_node* h, float* out_host, int32_t capacity, int32_t* n_out) {
    if (!h || !n_out) return RNDE_ERR_BAD_ARG;
    *n_out = h->n_att;
    if (out_host) {
        if (capacity < h->n_att) { h->err = "rnde_node_attempts_ext: capacity below the attempt count"; return RNDE_ERR_BAD_ARG; }
        for (int i = 0; i < h->n_att; ++i) {
            const StepMeta& m = h->h_meta[i];
            float* o = out_host + 6 * (size_t)i;
            o[0] = m.t; o[1] = m.dt; o[2] = m.dtp_in; o[3] = m.eest; o[4] = (m.flags & F_ACCEPT) ? 1.f : 0.f; o[5] = m.q;
        }
    }
    return RNDE_OK;
}

extern "C" rnde_status rnde_node_set_timing(rnde_node* h, int32_t on) {
    if (!h) return RNDE_ERR_BAD_ARG;
    if (on) for (auto& e : h->tev) HIPCHK(h, e.create());
    h->timing = on ? 1 : 0; h->tev_fwd = h->tev_bwd = false;
    return RNDE_OK;
}
extern "C" rnde_status rnde_node_timing(rnde_node* h, float* fwd_attempts_ms, float* rev_sweep_ms, float* rev_rest_ms) {
    if (h && h->engine == 4) return node_tiled_timing(h, fwd_attempts_ms, rev_sweep_ms, rev_rest_ms);      // (its events are always recorded: the solve, the reverse sweep, the tile reduction)
    if (!h || !h->timing) return RNDE_ERR_BAD_ARG;
    float a = -1.f, b = -1.f, c = -1.f;
    if (h->tev_fwd) { HIPCHK(h, hipEventSynchronize(h->tev[1])); HIPCHK(h, hipEventElapsedTime(&a, h->tev[0], h->tev[1])); }
    if (h->tev_bwd) {
        HIPCHK(h, hipEventSynchronize(h->tev[4]));
        HIPCHK(h, hipEventElapsedTime(&b, h->tev[2], h->tev[3])); HIPCHK(h, hipEventElapsedTime(&c, h->tev[3], h->tev[4]));
    }
    if (fwd_attempts_ms) *fwd_attempts_ms = a;
    if (rev_sweep_ms) *rev_sweep_ms = b;
    if (rev_rest_ms) *rev_rest_ms = c;
    return RNDE_OK;
}
extern "C" int32_t rnde_node_last_attempts(const rnde_node* h) { return h ? h->n_att : 0; }
extern "C" int32_t rnde_node_fallback_count(const rnde_node* h) { return h ? h->persist_fallbacks : 0; }

extern "C" int32_t rnde_node_one_launch_solves(const rnde_node* h) { return h ? h->one_launch_solves : 0; }
extern "C" void rnde_node_tail_folds(const rnde_node* h, int64_t counts[4]) { for (int i = 0; i < 4; ++i) counts[i] = h ? (int64_t)h->tail_folds[i] : 0; }
extern "C" rnde_status rnde_node_set_matrix_mode(rnde_node* h, int32_t mode) {
    if (!h) return RNDE_ERR_BAD_ARG;
    if (mode != RNDE_MATRIX_F32 && mode != RNDE_MATRIX_BF16X3) { h->err = "matrix mode: 0 (fp32-input MFMA) or 1 (bf16x3 on the matrix cores)"; return RNDE_ERR_BAD_ARG; }
    if (mode == RNDE_MATRIX_BF16X3) RNDE_TILED_REFUSE(h, "rnde_node_set_matrix_mode(h, 1) is not served (its layer products are the fp32-input MFMA, mode 0; bf16x3 serves the MNIST form on the stage engine)");
    h->x3 = (mode == RNDE_MATRIX_BF16X3 && h->x3B && h->x3D) ? 1 : 0;
    return RNDE_OK;
}
extern "C" int32_t rnde_node_matrix_mode(const rnde_node* h) { return (h && h->x3 && h->x3B && h->x3D) ? RNDE_MATRIX_BF16X3 : RNDE_MATRIX_F32; }
extern "C" int32_t rnde_node_launches_per_attempt(const rnde_node* h) {
    if (!h) return 0;
    return (h->engine == 2 && h->persist != 1) ? 7 : 1;
}

extern "C" rnde_status rnde_node_release_tape(rnde_node* h) {
    if (!h) return RNDE_ERR_BAD_ARG;
    h->have_tape = false;
    return RNDE_OK;
}

// ---- host-pointer variants ------------------------------------------------------------------
extern "C" rnde_status rnde_node_forward_host(rnde_node* h, const float* x, const float* p, int32_t B, float t0, float t1,
                                              float* u_out, int64_t* nfe_out, float* saveval, int32_t* n_saveval_out,
                                              int32_t keep_tape) {
    if (!h) return RNDE_ERR_BAD_ARG;
    DevBuf<float> xd, pd, ud;
    const size_t nb = (size_t)h->D * B * 4;
    HIPCHK(h, xd.alloc(nb / 4)); HIPCHK(h, ud.alloc(nb / 4)); HIPCHK(h, pd.alloc((size_t)h->P));
    HIPCHK(h, hipMemcpy(xd, x, nb, hipMemcpyHostToDevice)); HIPCHK(h, hipMemcpy(pd, p, (size_t)h->P * 4, hipMemcpyHostToDevice));
    rnde_status st = rnde_node_forward(h, xd, pd, B, t0, t1, ud, nfe_out, saveval, n_saveval_out, keep_tape, nullptr);
    if (st == RNDE_OK || st == RNDE_ERR_MAX_ATTEMPTS) hipMemcpy(u_out, ud, nb, hipMemcpyDeviceToHost);
    return st;
}

// ---- kernel-level entry points ----------------------------------------------------------------
extern "C" rnde_status rnde_debug_feval(rnde_node* h, const float* u_dev, const float* p_dev, int32_t B, float t,
                                        float* out_dev, void* stream) {
    if (!h || B < 1 || B > h->cfg.max_batch) return RNDE_ERR_BAD_ARG;
    if (h->engine == 4) return node_tiled_feval(h, u_dev, p_dev, B, t, out_dev, stream);
    hipStream_t s = (hipStream_t)stream;
    StepParams P = make_params(h, u_dev, B, 0.f, 1.f, 0);
    P.forced = 1; P.forced_t = t; P.dbg_out = out_dev;
    if (h->engine != 2 && h->engine != 3) { h->err = "rnde_debug_feval: unknown engine"; return RNDE_ERR_BAD_ARG; }
    const rnde_status st = pack_untaped(h, p_dev, s);
    if (st != RNDE_OK) return st;
    const EngineParams E = engine_params(h, P, p_dev);
    if (h->engine == 3 && h->mw) HIPCHK(h, launch_mw<MW_FEVAL>(h, E.MQ, 0, s));
    else if (h->engine == 3) HIPCHK(h, launch_chain<CM_FEVAL>(h, E.CQ, 0, nullptr, s));
    else {
        HIPCHK(h, launch_stage<SM_FEVAL1>(h, E.SQ, 0, 0, s));
        HIPCHK(h, launch_stage<SM_FEVAL2>(h, E.SQ, 0, 0, s));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    return RNDE_OK;
}

// The element-wise device functions, one at a time (include/rnde.h: rnde_debug_elementwise; rnde_probe.h).  The functor calls the functions of
// rnde_device.h with a run-time selector, as the generic kernels do.
static_assert(EW_TANH_FAST == RNDE_EW_TANH_FAST && EW_TANH_FAST2_X == RNDE_EW_TANH_FAST2_X && EW_TANH_FAST2_Y == RNDE_EW_TANH_FAST2_Y &&
              EW_PRE_FWD == RNDE_EW_PRE_FWD && EW_PRE_BWD == RNDE_EW_PRE_BWD && EW_ACT_FWD == RNDE_EW_ACT_FWD && EW_ACT_DY == RNDE_EW_ACT_DY &&
              EW_ACT_D2Y == RNDE_EW_ACT_D2Y && EW_TANH_F == RNDE_EW_TANH_F && EW_SIGMOID_F == RNDE_EW_SIGMOID_F &&
              EW_FF_SOFTPLUS == RNDE_EW_FF_SOFTPLUS, "rnde_probe.h restates rnde_elementwise_fn");
struct EwDevice {
    int fn, code;
    __device__ float operator()(float a, float b) const {
        switch (fn) {
            case EW_TANH_FAST: return tanh_fast(a);
            case EW_TANH_FAST2_X: return tanh_fast2(f32x2{a, b}).x;
            case EW_TANH_FAST2_Y: return tanh_fast2(f32x2{b, a}).y;
            case EW_PRE_FWD: return pre_fwd(code, a);
            case EW_PRE_BWD: return pre_bwd(code, a, b);
            case EW_ACT_FWD: return act_fwd(code, a);
            case EW_ACT_DY: return act_dy(code, a);
            default: return act_d2y(code, a);
        }
    }
};
extern "C" rnde_status rnde_debug_elementwise(int32_t fn, int32_t code, const float* in_dev, const float* in2_dev, int64_t n, float* out_dev,
                                              void* stream) {
    const bool two = fn == EW_TANH_FAST2_X || fn == EW_TANH_FAST2_Y || fn == EW_PRE_BWD;
    const int code_max = (fn == EW_PRE_FWD || fn == EW_PRE_BWD) ? RNDE_PRE_CUBE : ((fn == EW_ACT_FWD || fn == EW_ACT_DY || fn == EW_ACT_D2Y) ? RNDE_ACT_ELU : 0);
    if (fn < EW_TANH_FAST || fn > EW_FF_SOFTPLUS) { rnde_set_create_error("rnde_debug_elementwise: unknown function selector"); return RNDE_ERR_BAD_ARG; }
    if (code < 0 || code > code_max) { rnde_set_create_error("rnde_debug_elementwise: code out of range for this function"); return RNDE_ERR_BAD_ARG; }
    if (n < 0) { rnde_set_create_error("rnde_debug_elementwise: negative n"); return RNDE_ERR_BAD_ARG; }
    if (n == 0) return RNDE_OK;
    if (!in_dev || !out_dev || (two && !in2_dev)) { rnde_set_create_error("rnde_debug_elementwise: null operand"); return RNDE_ERR_BAD_ARG; }
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if (fn == EW_TANH_F || fn == EW_SIGMOID_F) e = elementwise_latent(fn, in_dev, (long long)n, out_dev, s);
    else if (fn == EW_FF_SOFTPLUS) e = elementwise_ffjord(in_dev, (long long)n, out_dev, s);
    else e = elementwise_launch(EwDevice{fn, code}, in_dev, two ? in2_dev : nullptr, (long long)n, out_dev, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { rnde_set_create_error(std::string("rnde_debug_elementwise: HIP: ") + hipGetErrorString(e)); return RNDE_ERR_HIP; }
    return RNDE_OK;
}

extern "C" rnde_status rnde_debug_attempt(rnde_node* h, const float* uprev_dev, const float* k1_dev, const float* p_dev,
                                          int32_t B, float t, float dt, float* k_out_dev, float* unew_out_dev,
                                          float* eest_out, void* stream) {
    if (!h || B < 1 || B > h->cfg.max_batch) return RNDE_ERR_BAD_ARG;
    RNDE_TILED_REFUSE(h, "rnde_debug_attempt is not served (its solve is one launch with no single-attempt entry; rnde_node_forward_replay runs a given attempt sequence)");
    hipStream_t s = (hipStream_t)stream;
    h->have_tape = false;
    StepParams P = make_params(h, uprev_dev, B, 0.f, 1.f, 0);
    P.forced = 1; P.forced_t = t; P.forced_dt = dt;
    const int ntiles = P.Bpad / 16, nks = h->NKD;      // (chain engine: the fragment-order arrays)
    // k1 goes to the f0 buffer: in fragment order (chain engine), or with column stride D as the caller holds it (stage engine)
    if (h->engine == 3) {
        const rnde_status st = pack_untaped(h, p_dev, s);
        if (st != RNDE_OK) return st;
        HIPCHK(h, chain_convert(k1_dev, h->f0, h->D, B, ntiles, nks, 0, s));
    } else {
        HIPCHK(h, hipMemsetAsync(h->f0, 0, (size_t)h->D * P.Bpad * 4, s));
        HIPCHK(h, hipMemcpyAsync(h->f0, k1_dev, (size_t)h->D * B * 4, hipMemcpyDeviceToDevice, s));
        const rnde_status st = pack_untaped(h, p_dev, s);
        if (st != RNDE_OK) return st;
    }
    EngineParams E = engine_params(h, P, p_dev);
    HIPCHK(h, launch_attempt(h, E, 0, s));
    HIPCHK(h, launch_finish(h, E, 1, nullptr, s));
    HIPCHK(h, hipMemcpyAsync(h->h_ctl, h->ctl_final, sizeof(StepState), hipMemcpyDeviceToHost, s));
    // record 0 of the arena (no tape: live == -1 -> rec 0): k2 .. k_S and unew
    if (h->engine == 3) {
        const ChainRec CL{(long long)ntiles * nks * 64, h->rk_S};
        for (int sidx = 2; sidx <= h->rk_S; ++sidx)      // (k_out: rk_S - 1 arrays)
            HIPCHK(h, chain_convert(h->arena + CL.k(sidx), k_out_dev + (size_t)(sidx - 2) * h->D * B, h->D, B, ntiles, nks, 1, s));
        HIPCHK(h, chain_convert(h->arena + CL.unew(), unew_out_dev, h->D, B, ntiles, nks, 1, s));
    } else {
        const RecLayout L{(long long)h->D * P.Bpad, (long long)h->H * P.Bpad};
        for (int sidx = 2; sidx <= 7; ++sidx)
            HIPCHK(h, hipMemcpyAsync(k_out_dev + (size_t)(sidx - 2) * h->D * B, h->arena + L.k(sidx), (size_t)h->D * B * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(h, hipMemcpyAsync(unew_out_dev, h->arena + L.unew(), (size_t)h->D * B * 4, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    if (h->engine == 2 && persist_failed(h, h->sR * (P.Bpad / 16), P.Bpad / 16, h->sR, s)) { h->err = "persistent attempt kernel abandoned its hand-off; call again (multi-launch kernels now in use)"; return RNDE_ERR_HIP; }
    if (eest_out) *eest_out = h->h_ctl->last_eest;
    return RNDE_OK;
}

static rnde_status bench_attempt_impl(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B, int32_t iters, int32_t taped,
                                      float* mean_us_out, void* stream) {
    if (!h || B < 1 || B > h->cfg.max_batch || iters < 1) return RNDE_ERR_BAD_ARG;
    RNDE_TILED_REFUSE(h, "rnde_bench_attempt* are not served (there is no per-attempt launch to time; rnde_node_timing reports the one-launch solve and the reverse sweep)");
    hipStream_t s = (hipStream_t)stream;
    h->have_tape = false;
    if (taped > 1) { const rnde_status sa = ensure_arena(h, std::min<long long>(taped, h->cfg.max_attempts)); if (sa != RNDE_OK) return sa; }
    StepParams P = make_params(h, x_dev, B, 0.f, 1.f, taped ? 1 : 0);   // taped: the variant a training step runs (record 0 of the arena)
    P.forced = 1; P.forced_t = 0.f; P.forced_dt = 0.05f;
    rnde_status st = pack_untaped(h, p_dev, s);
    if (st != RNDE_OK) return st;
    if (h->engine == 3 && h->mw && taped) { st = ensure_mw_slab(h, 8, s); if (st != RNDE_OK) return st; }
    EngineParams E = engine_params(h, P, p_dev);
    HIPCHK(h, launch_init(h, E, 0, s));      // k1 = f(x, 0) into f0
    for (int i = 0; i < 3; ++i) HIPCHK(h, launch_attempt(h, E, 0, s));
    Event e0, e1;
    HIPCHK(h, e0.create()); HIPCHK(h, e1.create());
    HIPCHK(h, hipEventRecord(e0, s));
    const auto host_t0 = std::chrono::steady_clock::now();
    // taped > 1 (stage engine): every attempt writes ANOTHER record of the arena, `taped` of them in turn -- what a solve does (31 records
    // of 21.7 MB at B = 512: the tape leaves the chip); taped == 1 rewrites record 0, which then lives in the Infinity Cache
    const int cyc = (taped > 1 && h->engine == 2) ? (int)std::min<long long>(taped, (long long)h->arena.cap() / h->rec_stride) : 1;
    for (int i = 0; i < iters; ++i) {
        E.SQ.F.rec_shift = i % cyc;
        HIPCHK(h, launch_attempt(h, E, 0, s));
    }
    const double host_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - host_t0).count();
    if (getenv("RNDE_TRACE_HOST")) fprintf(stderr, "[rnde] host enqueue: %.2f us per attempt (%d launches each)\n", host_us / iters, h->engine == 2 ? 7 : 1);
    HIPCHK(h, hipEventRecord(e1, s));
    HIPCHK(h, hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
    if (mean_us_out) *mean_us_out = ms * 1000.f / iters;
#ifdef RNDE_DIAG
    diag_bench_report(h, E, s);      // phase stamps of one more attempt
#endif
    return RNDE_OK;
}
extern "C" rnde_status rnde_bench_attempt(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B, int32_t iters,
                                          float* mean_us_out, void* stream) {
    return bench_attempt_impl(h, x_dev, p_dev, B, iters, 0, mean_us_out, stream);
}
extern "C" rnde_status rnde_bench_attempt_taped(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B, int32_t iters,
                                                float* mean_us_out, void* stream) {
    return bench_attempt_impl(h, x_dev, p_dev, B, iters, 1, mean_us_out, stream);
}
extern "C" rnde_status rnde_bench_attempt_cold_tape(rnde_node* h, const float* x_dev, const float* p_dev, int32_t B, int32_t iters,
                                                    int32_t records, float* mean_us_out, void* stream) {
    if (records < 2) return RNDE_ERR_BAD_ARG;
    return bench_attempt_impl(h, x_dev, p_dev, B, iters, records, mean_us_out, stream);
}
