// rnde_solve_sync.h -- parameter block of the one-launch solve kernel (rnde_stage_solve.h), shared with the host code in rnde.hip (which only
// launches that kernel through its translation unit's launcher).
#pragma once

namespace rnde {

struct SolveSync {
    unsigned long long* xch;   // [n_limit + kSolveInitRows][3][256] granules {float value, uint tag}
    unsigned epoch;            // of the tags (rnde_meet.h)
    int n_limit;               // attempts this launch may run (n_limit + kSolveInitRows < kMeetRows); rows n_limit, n_limit + 1: the two meetings of the start-up
    // X3 kernels (rnde_x3.h): the weights split into three bf16 planes, [tile][k-step < 4][plane < 3][64 lanes] fragments of 16 bytes
    const void* x3B;           // layer 2: tile = row tile (49)
    const void* x3D;           // layer 1: tile = hidden tile * 7 + row block
    float* u_out;              // the final state, caller layout, stored from registers when the kernel returns (null: no store)
    int fold;                  // 1: the kernel runs the initial-step rule itself in front of the attempt loop (else the SM_I1 .. SM_I4 launches have run)
};
constexpr int kSolveInitRows = 2;      // granule rows behind the attempts' for the start-up's two meetings (||u0||, ||f0||; ||f1 - f0||)
constexpr int kSlabBufs = 5;           // hand-off buffers: three the attempts cycle through (exchange % 3), two for the start-up's two exchanges

}  // namespace rnde
