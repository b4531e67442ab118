// rnde_diag.h -- the diagnostic build's (-DRNDE_DIAG, tools/build_diag.sh) cycle-stamp reports of the forward host path: the kernels stamp clock
// values into StepParams::dbg_out, the functions here arm that buffer and decode it onto stderr.  Included by rnde.hip alone, under
// #ifdef RNDE_DIAG and behind its launch helpers (EngineParams, launch_attempt): the default build never sees this file.
#pragma once

// ---- RNDE_DIAG_SOLVE: the one-launch stage solve, workgroup 0, every attempt (tools/diag_solve.py) ----
static StageParams diag_solve_params(rnde_node* h, const StageParams& SQ, hipStream_t s) {
    StageParams SD = SQ;
    if (getenv("RNDE_DIAG_SOLVE")) {
        h->diag_buf.reset();
        (void)h->diag_buf.alloc(4096);
        hipMemsetAsync(h->diag_buf, 0, 16384, s);
        SD.F.dbg_out = h->diag_buf;
    }
    return SD;
}
static void diag_solve_report(rnde_node* h, const StageParams& SQ) {
    if (!(getenv("RNDE_DIAG_SOLVE") && h->diag_buf)) return;
    static unsigned long long hst[1024];
    hipMemcpy(hst, h->diag_buf, 8192, hipMemcpyDeviceToHost);
    int na = 0; while (na < 119 && hst[(na + 1) * 8]) ++na;      // attempts with a successor
    double acc[7] = {0}; int cnt = 0;
    for (int a = 2; a + 1 < na; ++a, ++cnt) {
        const unsigned long long* q = hst + a * 8;
        acc[0] += (double)(q[1] - q[0]); acc[1] += (double)(q[2] - q[1]); acc[2] += (double)(q[3] - q[2]); acc[3] += (double)(q[4] - q[3]);
        acc[4] += (double)(q[5] - q[4]); acc[5] += (double)(q[6] - q[5]); acc[6] += (double)(q[8] - q[0]);
    }
    static unsigned long long arr[512];
    hipMemcpy(arr, (char*)h->diag_buf.get() + 8192, 4096, hipMemcpyDeviceToHost);
    {   // arrival spread and exchange latency of the meeting of attempt 10, all workgroups (100 MHz wall clock: 10 ns units)
        std::vector<long long> a, o; const int nw = SQ.C * SQ.R;
        for (int i = 0; i < nw && i < 256; ++i) if (arr[2 * i]) { a.push_back((long long)arr[2 * i]); o.push_back((long long)arr[2 * i + 1]); }
        if (a.size() > 4) {
            std::vector<long long> sa = a; std::sort(sa.begin(), sa.end());
            const long long last = sa.back(), first = sa.front();
            std::vector<long long> so = o; std::sort(so.begin(), so.end());
            fprintf(stderr, "meeting of attempt 10, %zu workgroups (x10 ns): arrivals after the first: median %lld, 90%% %lld, last %lld | out after the LAST arrival: first %lld, median %lld, last %lld\n",
                    a.size(), sa[sa.size() / 2] - first, sa[sa.size() * 9 / 10] - first, last - first, so.front() - last, so[so.size() / 2] - last, so.back() - last);
            int late[7] = {0}; for (size_t i = 0; i < a.size(); ++i) if (a[i] - first > (last - first) * 3 / 4) ++late[(i / SQ.C) % 7];
            fprintf(stderr, "  latest quarter of the spread by row block: %d %d %d %d %d %d %d\n", late[0], late[1], late[2], late[3], late[4], late[5], late[6]);
        }
    }
    if (cnt) fprintf(stderr, "one-launch solve, workgroup 0, mean over %d attempts (cycles): controller %.0f | START %.0f | stages 1-6 %.0f | reduce + barrier %.0f | "
                             "meeting %.0f | barrier %.0f | attempt %.0f\n", cnt, acc[0] / cnt, acc[1] / cnt, acc[2] / cnt, acc[3] / cnt, acc[4] / cnt, acc[5] / cnt, acc[6] / cnt);
}

// ---- RNDE_DIAG_FWD=n: attempt n of a real solve on the stage engine (the chunked loop) ----
static bool diag_fwd_wants(const rnde_node* h, int n) {
    static const int diag_n = getenv("RNDE_DIAG_FWD") ? atoi(getenv("RNDE_DIAG_FWD")) : -1;
    return h->engine == 2 && n == diag_n;
}
static EngineParams diag_fwd_params(rnde_node* h, const EngineParams& E, hipStream_t s) {
    (void)h->diag_buf.reserve(2048);
    hipMemsetAsync(h->diag_buf, 0, 8192, s);
    EngineParams D = E;
    D.SQ.F.dbg_out = h->diag_buf;
    return D;
}
static void diag_fwd_report(rnde_node* h) {
    if (!(h->engine == 2 && getenv("RNDE_DIAG_FWD") && h->diag_buf)) return;
    unsigned long long hst[64] = {0};
    hipMemcpy(hst, h->diag_buf, sizeof(hst), hipMemcpyDeviceToHost);
    if (!hst[34]) return;
    fprintf(stderr, "attempt %s of a real solve (workgroup 0 thread 0, cycles): controller %lld startC %lld startD %lld |", getenv("RNDE_DIAG_FWD"), (long long)(hst[1]-hst[0]), (long long)(hst[2]-hst[1]), (long long)(hst[3]-hst[2]));
    for (int st_ = 0; st_ < 6; ++st_) fprintf(stderr, " poll %lld", (long long)(hst[4 + 5 * st_] - hst[3 + 5 * st_]));
    fprintf(stderr, " | total %lld  (entry -> all loads issued %lld, -> controller state here %lld)\n", (long long)(hst[34]-hst[0]), (long long)(hst[35]-hst[0]), (long long)(hst[36]-hst[35]));
}

// ---- rnde_bench_attempt*: phase stamps of the LAST f evaluation of one more launch (workgroup 0), in shader cycles relative to stamp 0 of wave 0 ----
static void diag_bench_report(rnde_node* h, EngineParams E, hipStream_t s) {
    DevBuf<unsigned long long> d; unsigned long long hst[512] = {0};
    (void)d.alloc(512); hipMemset(d, 0, sizeof(hst));
    E.MQ.F.dbg_out = E.CQ.F.dbg_out = E.SQ.F.dbg_out = (float*)d.get();
    launch_attempt(h, E, 0, s);
    hipStreamSynchronize(s);
    hipMemcpy(hst, d, sizeof(hst), hipMemcpyDeviceToHost);
    if (h->engine == 3 && h->mw) {
        fprintf(stderr, "mw chain stamps (cycles): LDS fill %lld, controller %lld, state load %lld |", (long long)(hst[1]-hst[0]), (long long)(hst[2]-hst[1]), (long long)(hst[3]-hst[2]));
        for (int i = 4; i <= 9; ++i) fprintf(stderr, " eval%d %lld", i - 3, (long long)(hst[i]-hst[i-1]));
        fprintf(stderr, " | tail %lld total %lld\n  first eval: input->L0 %lld", (long long)(hst[10]-hst[9]), (long long)(hst[10]-hst[0]), (long long)(hst[16]-hst[3]));
        for (int l = 0; l < h->mg.n_layers; ++l) fprintf(stderr, " L%d %lld", l, (long long)(hst[17+l]-hst[16+l]));
        fprintf(stderr, "\n");
    } else if (h->engine == 3) {
        fprintf(stderr, "chain stamps (cycles): fill %lld ctl %lld loads %lld |", (long long)(hst[1]-hst[0]), (long long)(hst[2]-hst[1]), (long long)(hst[3]-hst[2]));
        for (int i = 4; i <= 9; ++i) fprintf(stderr, " st%d %lld", i - 3, (long long)(hst[i]-hst[i-1]));
        fprintf(stderr, " | tail %lld total %lld\n", (long long)(hst[10]-hst[9]), (long long)(hst[10]-hst[0]));
        for (int l = 0; l < h->cg.n_layers; ++l) fprintf(stderr, "  layer %d: bias %lld mm %lld act %lld (gap to next %lld)\n", l, (long long)(hst[17+4*l]-hst[16+4*l]), (long long)(hst[18+4*l]-hst[17+4*l]), (long long)(hst[19+4*l]-hst[18+4*l]), l + 1 < h->cg.n_layers ? (long long)(hst[20+4*l]-hst[19+4*l]) : 0LL);
    } else if (h->persist == 1) {
        fprintf(stderr, "persistent attempt (workgroup 0 thread 0, cycles): prologue(weights) %lld ctl %lld startC %lld startD %lld\n", 0LL, (long long)(hst[1]-hst[0]), (long long)(hst[2]-hst[1]), (long long)(hst[3]-hst[2]));
        for (int st = 1; st <= 6; ++st) { const unsigned long long* q = hst + 4 + 5 * (st - 1); const unsigned long long prev = st == 1 ? hst[3] : hst[8 + 5 * (st - 2)];
            if (st < 6) fprintf(stderr, "  stage %d: poll %lld A %lld B %lld C %lld D+put %lld\n", st, (long long)(q[0]-prev), (long long)(q[1]-q[0]), (long long)(q[2]-q[1]), (long long)(q[3]-q[2]), (long long)(q[4]-q[3]));
            else fprintf(stderr, "  stage %d: poll %lld A %lld B %lld C+err %lld | total %lld cycles\n", st, (long long)(q[0]-prev), (long long)(q[1]-q[0]), (long long)(q[2]-q[1]), (long long)(hst[34]-q[2]), (long long)(hst[34]-hst[0])); }
        fprintf(stderr, "per wave, relative to wave 0's poll-done of the stage: poll-done | barrier A in, out | B done | C done (before the barrier of D) | after it | put done\n");
        for (int st = 1; st <= 5; ++st) for (int w = 0; w < 7; ++w) { const unsigned long long* q = hst + 64 + ((st - 1) * 8 + w) * 8; const long long z = (long long)hst[64 + (st - 1) * 64];
            fprintf(stderr, "  stage %d wave %d: %6lld | %6lld %6lld | %6lld | %6lld | %6lld | %6lld\n", st, w, (long long)q[0]-z, (long long)q[1]-z, (long long)q[2]-z, (long long)q[3]-z, (long long)q[4]-z, (long long)q[5]-z, (long long)q[6]-z); }
    } else {
        fprintf(stderr, "stamps (cycles since wave0 stamp0); column-owner: start sync1 gemm1 sync2 reduce sync3 gemm2 tanh | stage: start scalars A sync B C sync D\n");
        for (int w = 0; w < 8; ++w) { fprintf(stderr, "wave %d:", w); for (int i = 0; i < 8; ++i) fprintf(stderr, " %7lld", (long long)(hst[w * 8 + i] - hst[0])); fprintf(stderr, "\n"); }
    }
}
