// The owning buffer of csrc/rnde_alloc.h (Buf<T, A>) over a host allocator policy, checked by a program of its own
// (tests/test_alloc_host.py compiles it with the address and undefined-behaviour sanitizers and runs it; no GPU is touched): malloc / free, a
// count of live blocks and of releases, and a switch that makes the n-th request fail.  Prints one line per failed check; exit status 0 when
// there is none.  The sanitizer's leak check at exit is part of the test.
#include "rnde_alloc.h"

#include <cstdio>
#include <cstring>
#include <utility>

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

struct TestAlloc {
    static int live, puts, requests, fail_at;      // fail_at: the request (counted from 1) that is refused; 0 = none
    static hipError_t get(void** p, size_t bytes) {
        if (++requests == fail_at) { *p = nullptr; return hipErrorOutOfMemory; }
        *p = std::malloc(bytes ? bytes : 1);
        std::memset(*p, 0xA5, bytes);
        ++live;
        return hipSuccess;
    }
    static void put(void* p) { std::free(p); --live; ++puts; }
    static void start(int fail = 0) { puts = 0; requests = 0; fail_at = fail; }
};
int TestAlloc::live = 0, TestAlloc::puts = 0, TestAlloc::requests = 0, TestAlloc::fail_at = 0;

template <class T> using TBuf = Buf<T, TestAlloc>;

struct Handle {      // several owners, as a handle has them
    TBuf<float> a, b;
    TBuf<double> c;
    TBuf<int> d;
};

int main() {
    // alloc, then the destructor
    TestAlloc::start();
    {
        TBuf<float> b;
        CHECK(b.get() == nullptr && b.cap() == 0);
        CHECK(b.alloc(10) == hipSuccess && b.get() != nullptr && b.cap() == 10 && TestAlloc::live == 1);
        float* p = b;      // (the implicit conversion)
        CHECK(p == b.get());
        p[9] = 1.f;        // (the whole capacity is there: the sanitizer watches)
    }
    CHECK(TestAlloc::live == 0 && TestAlloc::puts == 1);

    // reserve below the capacity is a no-op, above it releases exactly once
    TestAlloc::start();
    {
        TBuf<double> b;
        CHECK(b.reserve(8) == hipSuccess && b.cap() == 8);
        double* p = b.get();
        CHECK(b.reserve(8) == hipSuccess && b.reserve(3) == hipSuccess && b.reserve(0) == hipSuccess);
        CHECK(b.get() == p && b.cap() == 8 && TestAlloc::puts == 0 && TestAlloc::requests == 1);
        CHECK(b.reserve(9) == hipSuccess && b.cap() == 9 && TestAlloc::puts == 1 && TestAlloc::live == 1);
        b.get()[8] = 1.0;
    }
    CHECK(TestAlloc::live == 0 && TestAlloc::puts == 2);

    // a failed reserve or alloc leaves the owner empty, and a later reserve succeeds
    TestAlloc::start(2);
    {
        TBuf<int> b;
        CHECK(b.alloc(4) == hipSuccess);
        CHECK(b.reserve(100) == hipErrorOutOfMemory);      // (the second request)
        CHECK(b.get() == nullptr && b.cap() == 0 && TestAlloc::live == 0 && TestAlloc::puts == 1);
        CHECK(b.reserve(100) == hipSuccess && b.cap() == 100 && TestAlloc::live == 1);
        b.get()[99] = 1;
    }
    CHECK(TestAlloc::live == 0);
    TestAlloc::start(1);
    {
        TBuf<int> b;
        CHECK(b.alloc(4) == hipErrorOutOfMemory && b.get() == nullptr && b.cap() == 0 && TestAlloc::live == 0);
        CHECK(b.reserve(4) == hipSuccess && b.cap() == 4);
    }
    CHECK(TestAlloc::live == 0 && TestAlloc::puts == 1);

    // move construction and move assignment: the source is left empty, the target's old block is freed once
    TestAlloc::start();
    {
        TBuf<float> a;
        CHECK(a.alloc(5) == hipSuccess);
        float* pa = a.get();
        TBuf<float> b(std::move(a));
        CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == pa && b.cap() == 5 && TestAlloc::puts == 0);
        TBuf<float> c;
        CHECK(c.alloc(7) == hipSuccess);
        c = std::move(b);
        CHECK(b.get() == nullptr && b.cap() == 0 && c.get() == pa && c.cap() == 5 && TestAlloc::puts == 1 && TestAlloc::live == 1);
        TBuf<float>& same = c;
        c = std::move(same);      // (onto itself: nothing happens)
        CHECK(c.get() == pa && c.cap() == 5 && TestAlloc::puts == 1);
    }
    CHECK(TestAlloc::live == 0 && TestAlloc::puts == 2);

    // swap exchanges pointer and capacity; reset twice is harmless
    TestAlloc::start();
    {
        TBuf<int> a, b;
        CHECK(a.alloc(2) == hipSuccess && b.alloc(3) == hipSuccess);
        int *pa = a.get(), *pb = b.get();
        a.swap(b);
        CHECK(a.get() == pb && a.cap() == 3 && b.get() == pa && b.cap() == 2 && TestAlloc::puts == 0);
        TBuf<int> none;
        a.swap(none);      // (with an empty owner: the grow-and-keep pattern's last step)
        CHECK(a.get() == nullptr && a.cap() == 0 && none.get() == pb && none.cap() == 3);
        b.reset();
        CHECK(b.get() == nullptr && b.cap() == 0 && TestAlloc::puts == 1);
        b.reset();
        CHECK(TestAlloc::puts == 1 && TestAlloc::live == 1);
    }
    CHECK(TestAlloc::live == 0 && TestAlloc::puts == 2);

    // a struct of several owners destroyed half-filled, as after a failed create
    TestAlloc::start(3);
    {
        Handle* h = new Handle();
        bool ok = h->a.alloc(16) == hipSuccess && h->b.alloc(1) == hipSuccess && h->c.alloc(4) == hipSuccess && h->d.alloc(4) == hipSuccess;
        CHECK(!ok && TestAlloc::requests == 3 && TestAlloc::live == 2);      // (the chain stops at the third request)
        CHECK(h->c.get() == nullptr && h->d.get() == nullptr);
        delete h;
    }
    CHECK(TestAlloc::live == 0 && TestAlloc::puts == 2);

    if (!failures) std::printf("alloc host checks passed\n");
    return failures ? 1 : 0;
}
