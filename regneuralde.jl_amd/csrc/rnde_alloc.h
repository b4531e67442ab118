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
// Outside the fill on purpose: MeetRes::create (rnde_meet.h) -- its words are protocol state and it zeroes every one of them itself (the
// DevPlain policy below) -- and pinned host memory (hipHostMalloc), which the host fills before the device sees it.
//
// Live counters.  Every device allocation, poisoned or not, counts rnde_g_live_allocs / _bytes up and its release (hipFree is routed here
// too) counts them down; a pointer-to-size map under a mutex remembers the size (allocations are rare).  A handle that is created, run and
// destroyed must leave both where they were (rnde_debug_live_allocs / _bytes, tests/test_gpu_handle_lifetime.py).  Pinned memory is not counted.
//
// Owners.  Buf<T, A> owns one block of cap() elements of T from the allocator policy A (two static functions, get and put) and releases it in
// its destructor; it converts to T*, so it is handed to a parameter block or a launch like the raw pointer it replaces.  DevBuf<T> is device
// memory through rnde_malloc, PinBuf<T> pinned host memory; Event and Stream own a hipEvent_t (created on first use) and a hipStream_t.  A
// handle's allocated members are owners, a member that points into another allocation stays a raw pointer and nothing is freed through
// it (docs/memory_audit.md, "who owns what"); a handle declares its stream and events ahead of its buffers, so that the buffers go first.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <unordered_map>

// (inline variables at global scope: one instance for the whole library, whatever a translation unit calls its copy of namespace rnde)
inline std::atomic<long long> rnde_g_poison_allocs{0}, rnde_g_poison_bytes{0};
inline std::atomic<long long> rnde_g_live_allocs{0}, rnde_g_live_bytes{0};
inline std::mutex rnde_g_live_mutex;
inline std::unordered_map<void*, size_t>& rnde_live_sizes() {      // (never destroyed: a handle may be released while the process exits)
    static auto* const m = new std::unordered_map<void*, size_t>();
    return *m;
}

static inline hipError_t rnde_malloc_plain(void** p, size_t bytes) {      // counted, not filled
    const hipError_t e = (hipMalloc)(p, bytes);
    if (e == hipSuccess && *p) {
        std::lock_guard<std::mutex> g(rnde_g_live_mutex);
        rnde_live_sizes()[*p] = bytes;
        rnde_g_live_allocs.fetch_add(1, std::memory_order_relaxed);
        rnde_g_live_bytes.fetch_add((long long)bytes, std::memory_order_relaxed);
    }
    return e;
}
static inline hipError_t rnde_malloc(void** p, size_t bytes) {
    const hipError_t e = rnde_malloc_plain(p, bytes);
    const bool poison = getenv("RNDE_POISON") != nullptr;
    if (e == hipSuccess && poison && bytes && hipMemset(*p, 0xFF, bytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess) {
        rnde_g_poison_allocs.fetch_add(1, std::memory_order_relaxed);
        rnde_g_poison_bytes.fetch_add((long long)bytes, std::memory_order_relaxed);
    }
    return e;
}
static inline hipError_t rnde_free(void* p) {
    if (p) {
        std::lock_guard<std::mutex> g(rnde_g_live_mutex);
        const auto it = rnde_live_sizes().find(p);
        if (it != rnde_live_sizes().end()) {
            rnde_g_live_allocs.fetch_sub(1, std::memory_order_relaxed);
            rnde_g_live_bytes.fetch_sub((long long)it->second, std::memory_order_relaxed);
            rnde_live_sizes().erase(it);
        }
    }
    return (hipFree)(p);
}
#define hipMalloc(p, n) rnde_malloc((void**)(p), (n))
#define hipFree(p) rnde_free((void*)(p))

struct DevAlloc   { static hipError_t get(void** p, size_t bytes) { return rnde_malloc(p, bytes); }       static void put(void* p) { (void)rnde_free(p); } };
struct DevPlain   { static hipError_t get(void** p, size_t bytes) { return rnde_malloc_plain(p, bytes); } static void put(void* p) { (void)rnde_free(p); } };
struct PinAlloc   { static hipError_t get(void** p, size_t bytes) { return hipHostMalloc(p, bytes); }     static void put(void* p) { (void)hipHostFree(p); } };

template <class T, class A>
class Buf {
    T* p_ = nullptr; size_t cap_ = 0;
public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Buf& operator=(Buf&& o) noexcept { if (this != std::addressof(o)) { reset(); swap(o); } return *this; }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { reset(); }
    hipError_t alloc(size_t n) {      // (the owner is empty)
        void* q = nullptr;
        const hipError_t e = A::get(&q, n * sizeof(T));
        if (e == hipSuccess) { p_ = static_cast<T*>(q); cap_ = n; }
        return e;
    }
    hipError_t reserve(size_t n) {      // room for n elements; growing discards the contents, a failure leaves the owner empty
        if (cap_ >= n) return hipSuccess;
        reset();
        return alloc(n);
    }
    void reset() { if (p_) A::put(p_); p_ = nullptr; cap_ = 0; }
    T* get() const { return p_; }
    size_t cap() const { return cap_; }
    void swap(Buf& o) { T* p = p_; p_ = o.p_; o.p_ = p; const size_t c = cap_; cap_ = o.cap_; o.cap_ = c; }
    operator T*() const { return p_; }
};
template <class T> using DevBuf = Buf<T, DevAlloc>;
template <class T> using PinBuf = Buf<T, PinAlloc>;

struct Event {      // created on first use
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};
