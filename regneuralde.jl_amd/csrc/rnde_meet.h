// rnde_meet.h -- "the meeting": how the workgroups of a one-launch solve or sweep sum a few numbers once per attempted step, device and host
// side (DESIGN.md 4.0 has the protocol in full).  Granules are 8 bytes {float value, uint tag}, laid out [sequence number][row][workgroup].  At
// meeting `seq` every workgroup writes one granule per value (ONE 8-byte store: the data is its own validity), wave 0 polls everybody's until
// each carries meet_tag(epoch, seq) and sums the values in double in the order sum_partials forms them (lane l adds entries l, l + 64, ..., then
// the wave reduction), so a one-launch solve is bit-identical to one launch per attempt.  Nothing is cleared inside a launch; every spin is
// bounded: a poll that runs out, or sees the abort word raised, raises the abort word and the kernel returns; the host reads the word back.
// Two forms: agent scope (Meet::global = 1: relaxed agent-scope atomics, any placement) and one XCD (global = 0, at most kMeetXcdCus
// workgroups: a plain store, written through to the XCD's L2, and an L1-bypassing buffer load).  The latter is valid only when all
// participants share one L2: 8 x n workgroups are launched, every eighth works and records its XCC id, and the host checks behind the launch
// that the ids agree (meet_verdict) -- a solve whose workgroups were split is thrown away.
#pragma once
#include "rnde_alloc.h"
#include "rnde_device.h"

namespace rnde {

constexpr int kMeetSpinMax = 4000000;        // bound of every poll of meet_exchange (~1 s)
constexpr unsigned kMeetRows = 8192u;        // sequence numbers one epoch's tags tell apart
constexpr unsigned kMeetEpochs = 500000u;    // epochs before the tags start over (kMeetEpochs * kMeetRows < 2^32)
constexpr int kMeetXcdCus = 32;              // CUs of one XCD: the one-XCD form holds one workgroup on each

struct Meet {
    unsigned long long* xch;     // [sequence number][rows per sequence number][n] granules
    unsigned* abort_word;        // a meeting timed out
    unsigned epoch;
    int n;                       // workgroups that meet (all of them resident)
    int global;                  // 1: agent scope, any placement; 0: one XCD
};

// The tag of row `row` in epoch `epoch` (never 0, a cleared granule).  Rows are INDEXED by the sequence number, so only tags of one row ever
// meet, they differ in the epoch alone, and epoch * kMeetRows differs for any two epochs below kMeetEpochs whatever the row: a stale granule
// never passes for a fresh one, also past kMeetRows attempts.  No engine needs a bound on max_attempts for the tags' sake (the bounds some
// have are kept as they are).  When the epoch wraps the host clears the array (MeetRes::begin).
__host__ __device__ __forceinline__ constexpr unsigned meet_tag(unsigned epoch, int row) { return epoch * kMeetRows + (unsigned)row + 1u; }

// {value, tag} as one granule.  NaNs are canonicalised, so that a granule is a function of (value as a number, tag) alone.
__device__ __forceinline__ unsigned long long meet_pack(float value, unsigned tag) {
    if (value != value) value = __uint_as_float(0x7FC00000u);
    return ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(value);
}
__device__ __forceinline__ bool meet_tagged(unsigned long long e, unsigned tag) { return (unsigned)(e >> 32) == tag; }
__device__ __forceinline__ float meet_value(unsigned long long e) { return __uint_as_float((unsigned)(e & 0xFFFFFFFFull)); }

// A poll that has not succeeded, `spins` polls in.  meet_spent: the bound is passed, or (looked at whenever spins & check_mask is 0) somebody
// else has given up.  meet_give_up raises the abort word.  (Two pieces: as one bool function the callers' code comes out different.)
__device__ __forceinline__ bool meet_spent(unsigned* abort_word, int spins, int max_spins, int check_mask) {
    return spins > max_spins || ((spins & check_mask) == 0 && __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u);
}
__device__ __forceinline__ void meet_give_up(unsigned* abort_word, int lane) { if (lane == 0) __hip_atomic_store(abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Meeting `seq` of NV values, ROWS rows per sequence number (NV <= ROWS), either form.  Called by wave 0 of workgroup `me`; `mine` valid in
// lane 0.  Polls 64 workgroups at a time.  false: timed out / aborted.
typedef unsigned meet_u32x2 __attribute__((ext_vector_type(2)));
template <int ROWS, int NV>
__device__ __forceinline__ bool meet_exchange(const Meet& Q, int seq, const float (&mine)[NV], double (&out)[NV], int me, int lane) {
    static_assert(NV <= ROWS, "a meeting has at most ROWS values");
    const unsigned tag = meet_tag(Q.epoch, seq);
    unsigned long long* base = Q.xch + (size_t)seq * ROWS * Q.n;
    if (lane == 0) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const unsigned long long e = meet_pack(mine[v], tag);
            if (Q.global) __hip_atomic_store(base + (size_t)v * Q.n + me, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else base[(size_t)v * Q.n + me] = e;
        }
    }
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        double sv = 0.0;
        for (int b0 = 0; b0 < Q.n; b0 += 64) {
            const int i = b0 + lane;
            unsigned long long e = 0;
            bool ok = i >= Q.n;
            int spins = 0;
            while (true) {
                if (!ok) {
                    if (Q.global) e = __hip_atomic_load(base + (size_t)v * Q.n + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else {
                        __asm__ volatile("" ::: "memory");      // (the buffer load is a plain read to the optimiser: keep it inside the spin loop)
                        const meet_u32x2 q = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(((size_t)v * Q.n + i) * 8), 0, 16);   // aux 16 = sc1: misses L1
                        e = ((unsigned long long)q.y << 32) | q.x;
                    }
                    ok = meet_tagged(e, tag);
                }
                if (__all(ok)) break;
                if (meet_spent(Q.abort_word, ++spins, kMeetSpinMax, 1023)) {
                    meet_give_up(Q.abort_word, lane);
                    return false;
                }
            }
            if (i < Q.n) sv += (double)meet_value(e);
        }
        out[v] = wave_sum_d(sv);
    }
    return true;
}

// The same meeting in the stage solve's shape (rnde_stage_solve.h): agent scope only, three rows of a fixed 256 granules, `nval` (1 or 3) in
// use, four loads in flight per lane, the abort word looked at every 256 spins, a run-time spin bound.  The fields come loose, by reference
// (read where they are used): that kernel's parameter blocks keep their layout and its instruction stream is the parent's, line for line.
// (One set of polling loads at a time: keeping a second set in flight makes an attempt 0.3 us SLOWER -- the extra reads of the same lines
// on the memory side delay the stores they are waiting for; a back-off between polls, s_sleep 4 / 8 / 16, does not help either: 23.37 /
// 23.46 / 23.60 us against 23.34.)
typedef __attribute__((address_space(1))) unsigned long long meet_gu64;
__device__ __forceinline__ bool meet_exchange_256(unsigned long long* const& xch, const unsigned& epoch, unsigned* const& abort_word, const int& max_spins, int seq, int n, int me,
                                                  int nval, const float (&mine)[3], double (&out)[3], int lane) {
    const unsigned tag = meet_tag(epoch, seq);
    meet_gu64* base = (meet_gu64*)xch + (size_t)seq * 3 * 256;
    if (lane == 0) {
#pragma unroll
        for (int v = 0; v < 3; ++v)
            if (v < nval) __hip_atomic_store(base + (size_t)v * 256 + me, meet_pack(mine[v], tag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    out[0] = out[1] = out[2] = 0.0;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        if (v >= nval) break;
        unsigned long long e[4] = {0, 0, 0, 0};
        bool ok[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) ok[q] = lane + 64 * q >= n;
        int spins = 0;
        while (true) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (!ok[q]) {
                    e[q] = __hip_atomic_load(base + (size_t)v * 256 + lane + 64 * q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    ok[q] = meet_tagged(e[q], tag);
                }
            }
            if (__all(ok[0] && ok[1] && ok[2] && ok[3])) break;
            if (meet_spent(abort_word, ++spins, max_spins, 255)) {
                meet_give_up(abort_word, lane);
                return false;
            }
        }
        double s = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (lane + 64 * q < n) s += (double)meet_value(e[q]);
        out[v] = wave_sum_d(s);
    }
    return true;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
// What the host reads back behind a launch: chk[0] = the abort word, chk[2 + i] = the XCC id workgroup i recorded.
enum MeetVerdict { MEET_OK = 0, MEET_TIMED_OUT = 1, MEET_SPLIT_XCD = 2 };
inline bool meet_split(const unsigned* chk, int n, bool global) {      // (the agent-scope form does not depend on the placement)
    for (int i = 1; i < n && !global; ++i)
        if (chk[2 + i] != chk[2]) return true;
    return false;
}
inline MeetVerdict meet_verdict(const unsigned* chk, int n, bool global) { return chk[0] != 0u ? MEET_TIMED_OUT : (meet_split(chk, n, global) ? MEET_SPLIT_XCD : MEET_OK); }
// The next launch's epoch; true when the tags start over (the granules must be cleared before that launch).
inline bool meet_next_epoch(unsigned& epoch) { if (++epoch < kMeetEpochs) return false; epoch = 1; return true; }

// A handle's meeting place; slot: the XCD its one-XCD launches work on (blockIdx % 8 == slot; handles take turns: two streams, two XCDs).
struct MeetRes {
    // (owners, rnde_alloc.h: counted, and released with the handle that holds the MeetRes)
    Buf<unsigned long long, DevPlain> xch;      // max_rows sequence numbers x rows_per_seq x max_wg granules
    Buf<unsigned, DevPlain> xcc, abort_word;
    PinBuf<unsigned> chk;            // pinned: [2 + max_wg]
    unsigned epoch = 0; int slot = 0;
    hipError_t err = hipSuccess;     // of the last begin

    // xch and the epoch alone (the stage solve: the rest is PersistSync's).  Neither create goes through the RNDE_POISON fill of
    // rnde_alloc.h, on purpose (the DevPlain policy): these words are protocol state, a tag or an abort word that reads as anything but
    // "not yet" ends or hangs a meeting.  Both zero EVERYTHING they allocate -- the granules, the XCC ids (the host compares the first n of
    // them behind a one-XCD launch; a workgroup writes its own before anything else), the abort word and the pinned check words.
    hipError_t create_granules(size_t max_rows, int rows_per_seq, int max_wg) {
        const hipError_t e = xch.alloc(max_rows * rows_per_seq * max_wg);
        return e == hipSuccess ? hipMemset(xch, 0, xch.cap() * 8) : e;
    }
    hipError_t create(size_t max_rows, int rows_per_seq, int max_wg) {
        static std::atomic<int> next_slot{0};
        slot = next_slot.fetch_add(1) & 7;
        hipError_t e = create_granules(max_rows, rows_per_seq, max_wg);
        if (e == hipSuccess) e = xcc.alloc((size_t)max_wg);
        if (e == hipSuccess) e = abort_word.alloc(4);
        if (e == hipSuccess) e = chk.alloc((size_t)max_wg + 2);
        if (e == hipSuccess) e = hipMemset(xcc, 0, (size_t)max_wg * 4);
        if (e == hipSuccess) e = hipMemset(abort_word, 0, 16);
        if (e == hipSuccess) for (int i = 0; i < max_wg + 2; ++i) chk[i] = 0u;
        return e;
    }
    // The parameter block of the next launch's meetings of n workgroups; allow_local: the one-XCD form while they fit one.
    Meet begin(int n, bool allow_local, hipStream_t s) {
        err = meet_next_epoch(epoch) ? hipMemsetAsync(xch, 0, xch.cap() * 8, s) : hipSuccess;
        return Meet{xch, abort_word, epoch, n, (allow_local && n <= kMeetXcdCus) ? 0 : 1};
    }
    static int grid(const Meet& m) { return m.global ? m.n : 8 * m.n; }      // one XCD: every eighth workgroup works
    // Behind the launch: the abort word (abort_too; the SDE solve reports a time-out in its own status) and (one XCD) the ids -> dst.
    hipError_t queue_check(const Meet& m, hipStream_t s, unsigned* dst = nullptr, bool abort_too = true) {
        if (!dst) dst = chk;
        hipError_t e = abort_too ? hipMemcpyAsync(dst, abort_word, 4, hipMemcpyDeviceToHost, s) : hipSuccess;
        if (e == hipSuccess && !m.global) e = hipMemcpyAsync(dst + 2, xcc, (size_t)m.n * 4, hipMemcpyDeviceToHost, s);
        return e;
    }
    hipError_t clear_abort(hipStream_t s) { return hipMemsetAsync(abort_word, 0, 16, s); }
};

}  // namespace rnde
