// rnde_tile_meet.h -- tile_meet: how the tiles of a one-launch solve on the tile layout (rnde_ffjordt.h: four waves per 16 batch columns) meet
// once per attempt, over rnde_meet.h's meet_exchange.  Shared by the tile driver of TrackedFFJORD (rnde_ffjord_tile.h) and the tiled engine of
// TrackedNeuralODE (rnde_node_tile.h).
#pragma once
#include "rnde_ffjordt.h"      // kFtThreads; rnde_meet.h

namespace rnde {

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
