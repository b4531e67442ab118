// rnde_tile_meet.h -- tile_meet: how the tiles of a one-launch solve on the tile layout (rnde_ffjordt.h: four waves per 16 batch columns) meet
// once per attempt, over rnde_meet.h's meet_exchange, and tile_place: which tile a workgroup of such a launch is.  Used by the tile driver
// (rnde_tile_driver.h).
#pragma once
#include "rnde_ffjordt.h"      // kFtThreads; rnde_meet.h

namespace rnde {

// The placement prologue of a launch whose tiles meet (MeetRes::grid): false for a block that is no tile, otherwise the block's tile index
// in *tile.  Agent scope: every block is a tile.  One XCD: every eighth block, the ones of the slot, is a tile (the others return at once),
// and leaves the XCD it runs on in xcc[tile] for the host's check.  (The index is formed from blockIdx alone, with no sentinel value: the
// compiler then knows its range, and the 64-bit offsets formed from it stay 32 x 32 multiplies.)
__device__ __forceinline__ bool tile_place(const Meet& M, int xcd_slot, unsigned* xcc, int* tile) {
    if (!M.global && (int)(blockIdx.x & 7) != xcd_slot) return false;
    *tile = !M.global ? (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    if (!M.global && threadIdx.x == 0) xcc[*tile] = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 15;
    return true;
}

// Publish this tile's three partials (wave 0), collect everybody's sums in tile order; false when the meeting timed out (every thread).
__device__ __forceinline__ bool tile_meet(const Meet& M, float* red, int seq, float a, float b, float c, double (&out)[3], int tile, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    a = wave_sum_f(a); b = wave_sum_f(b); c = wave_sum_f(c);
    if (lane == 0) { red[wave] = a; red[4 + wave] = b; red[8 + wave] = c; }
    __syncthreads();
    double* RD = (double*)(red + 64);
    if (wave == 0) {
        const float mine[3] = {((red[0] + red[1]) + red[2]) + red[3], ((red[4] + red[5]) + red[6]) + red[7], ((red[8] + red[9]) + red[10]) + red[11]};
        double o[3];
        const bool ok = meet_exchange<3, 3>(M, seq, mine, o, tile, lane);
        if (lane == 0) { RD[0] = o[0]; RD[1] = o[1]; RD[2] = o[2]; red[70] = ok ? 1.f : 0.f; }
    }
    __syncthreads();
    const bool ok = red[70] != 0.f;
    out[0] = RD[0]; out[1] = RD[1]; out[2] = RD[2];
    __syncthreads();
    return ok;
}

}  // namespace rnde
