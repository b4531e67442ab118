// rnde_alloc.h -- the library's device allocator.  Every translation unit that allocates device memory includes this header (through
// rnde_node.h: rnde.hip, rnde_reverse.hip, rnde_node_tile.hip; directly: rnde_ffjord.hip, rnde_sde.hip, rnde_latent.hip,
// rnde_comm.hip), BEHIND the HIP runtime header and ahead of its first hipMalloc: the macro below routes that name here.
//
// RNDE_POISON=1 fills fresh memory with 0xFF bytes (NaN as float, -1 as an integer): a read of something that was never written then
// shows up as NaN in the results instead of depending on what the allocator hands back (a debugging aid, off by default;
// tests/test_gpu_memory_independence.py and tests/test_gpu_edge.py run every engine under it, docs/memory_audit.md says who writes each
// buffer before who reads it).  The variable is read per allocation (allocations are rare), so a test can switch it per handle.
// Two counters say how much was filled since the library was loaded (rnde_debug_poison_allocs / _bytes, include/rnde.h): a test that
// creates a handle under the variable asserts that they grew, so a translation unit that leaves this wrapper again is noticed.
//
// The fill is a hipMemset, which is ordered on the null stream and does not block the host for device memory.  A handle driven from a
// non-blocking stream of its own (the ranks of the coupled controller; any caller's stream) uses a buffer it has just grown -- an upload, the
// first kernel -- while that fill may still be queued, and the fill then lands on top of what was written (seen as NaN in tspan-bar and the
// first layer's p-bar of a coupled Dense-chain solve whose reverse buffers are allocated by the first backward).  So the wrapper waits for
// the device behind the fill: an allocation is handed out poisoned, never about to be.  Only under the variable; nothing is added otherwise.
//
// Outside on purpose: MeetRes::create (rnde_meet.h) -- its words are protocol state and it zeroes every one of them itself -- and pinned
// host memory (hipHostMalloc), which the host fills before the device sees it.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>

// (inline variables at global scope: one instance for the whole library, whatever a translation unit calls its copy of namespace rnde)
inline std::atomic<long long> rnde_g_poison_allocs{0}, rnde_g_poison_bytes{0};

static inline hipError_t rnde_malloc(void** p, size_t bytes) {
    const hipError_t e = (hipMalloc)(p, bytes);
    const bool poison = getenv("RNDE_POISON") != nullptr;
    if (e == hipSuccess && poison && bytes && hipMemset(*p, 0xFF, bytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess) {
        rnde_g_poison_allocs.fetch_add(1, std::memory_order_relaxed);
        rnde_g_poison_bytes.fetch_add((long long)bytes, std::memory_order_relaxed);
    }
    return e;
}
#define hipMalloc(p, n) rnde_malloc((void**)(p), (n))
