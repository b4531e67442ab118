// Host part of csrc/rnde_meet.h, checked by a program of its own (tests/test_meet_host.py compiles and runs it; no GPU is touched):
// the verdict over the check words, the tags, the epoch bump.  Prints one line per failed check; exit status 0 when there is none.
#include "rnde_meet.h"

#include <cstdio>
#include <vector>

using namespace rnde;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static std::vector<unsigned> words(unsigned abort_word, int n, unsigned id) {      // chk[0] = abort word, chk[2 + i] = XCC id of workgroup i
    std::vector<unsigned> c(2 + n, id);
    c[0] = abort_word; c[1] = 0u;
    return c;
}

int main() {
    // ---- meet_verdict ----
    for (int n : {1, 2, 32, 256})
        for (bool global : {false, true}) {
            std::vector<unsigned> c = words(0u, n, 5u);
            CHECK(meet_verdict(c.data(), n, global) == MEET_OK);                      // equal ids
            c[0] = 1u;
            CHECK(meet_verdict(c.data(), n, global) == MEET_TIMED_OUT);               // abort word set, ids equal
            if (n > 1) { c[2 + n - 1] = 6u; CHECK(meet_verdict(c.data(), n, global) == MEET_TIMED_OUT); }      // ... whatever the ids are
        }
    for (int n : {2, 32})
        for (int who = 0; who < n; ++who) {      // one differing id, wherever it sits
            std::vector<unsigned> c = words(0u, n, 3u);
            c[2 + who] = 4u;
            CHECK(meet_verdict(c.data(), n, false) == MEET_SPLIT_XCD);
            CHECK(meet_split(c.data(), n, false));
            CHECK(meet_verdict(c.data(), n, true) == MEET_OK);                        // agent scope: the placement does not matter
            CHECK(!meet_split(c.data(), n, true));
        }
    {   // ids past n are not looked at
        std::vector<unsigned> c = words(0u, 32, 3u);
        c[2 + 20] = 9u;
        CHECK(meet_verdict(c.data(), 20, false) == MEET_OK);
        CHECK(meet_verdict(c.data(), 21, false) == MEET_SPLIT_XCD);
    }

    // ---- meet_tag ----
    // injective over (epoch, row), row < kMeetRows: row and epoch can be read back from the tag, and no tag is 0 (a cleared granule)
    for (unsigned epoch : {1u, 2u, 77u, kMeetEpochs - 2u, kMeetEpochs - 1u})
        for (unsigned row = 0; row < kMeetRows; ++row) {
            const unsigned t = meet_tag(epoch, (int)row);
            CHECK(t != 0u);
            CHECK((t - 1u) / kMeetRows == epoch && (t - 1u) % kMeetRows == row);
            if (failures) return 1;
        }
    CHECK((unsigned long long)(kMeetEpochs - 1u) * kMeetRows + kMeetRows <= 0xFFFFFFFFull);      // the largest tag fits 32 bits
    // two epochs, one row: the tags differ for ANY row, also at and beyond kMeetRows (rows are indexed by the sequence number, so only
    // tags of one row ever meet)
    const unsigned epochs[] = {1u, 2u, 3u, 1000u, 1001u, kMeetEpochs / 2u, kMeetEpochs - 2u, kMeetEpochs - 1u};
    for (int row : {0, 1, 4095, 8191, 8192, 8193, 20000, 1 << 20, 0x7FFFFFFF})
        for (unsigned e1 : epochs)
            for (unsigned e2 : epochs)
                if (e1 != e2) CHECK(meet_tag(e1, row) != meet_tag(e2, row));

    // ---- the epoch bump ----
    {
        unsigned epoch = 0;
        CHECK(!meet_next_epoch(epoch) && epoch == 1u);                 // a fresh handle's first launch
        epoch = kMeetEpochs - 2u;                                      // 499 998
        CHECK(!meet_next_epoch(epoch) && epoch == kMeetEpochs - 1u);   // -> 499 999, no wrap
        CHECK(meet_next_epoch(epoch) && epoch == 1u);                  // the next call: epoch 1, "wrapped"
        CHECK(!meet_next_epoch(epoch) && epoch == 2u);
    }
    static_assert(kMeetEpochs == 500000u && kMeetRows == 8192u && kMeetXcdCus == 32, "the constants the engines were tuned and tested with");

    if (!failures) std::printf("meet host checks passed\n");
    return failures ? 1 : 0;
}
