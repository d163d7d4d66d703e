// RankBarrier / rank_phase (edsparser_amd/csrc/rank_barrier.hpp) on CPU threads.  The order of the threads is forced
// with the barrier's own state, not with sleeps; a hang is caught by the subprocess timeout of the Python driver
// (tests/test_vcf_multi_cpu.py).
#include "rank_barrier.hpp"

#include <atomic>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <thread>

using edsx::RankBarrier;

static int failures = 0;
#define CHECK(c)                                                                     \
    do {                                                                             \
        if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); failures++; } \
    } while (0)

// Three ranks pass barrier 1.  Rank 0 fails in the phase right behind it and arrives at barrier 2 with its failure while
// rank 1 has not yet looked at the result of barrier 1.  Rank 1 must still see barrier 1 as clean (and so go on to
// barrier 2 instead of leaving early); all three then leave at barrier 2 with rank 0's text.
static void late_reader()
{
    RankBarrier bar(3);
    bool b1[3] = {true, true, true}, b2[3] = {false, false, false};
    const std::string boom = "rank 0: boom";
    std::thread t0([&] {
        b1[0] = bar.arrive(0, nullptr);
        b2[0] = bar.arrive(0, &boom);
    });
    std::thread t2([&] {
        b1[2] = bar.arrive(2, nullptr);
        b2[2] = bar.arrive(2, nullptr);
    });
    std::thread t1([&] {
        const bool r1 = bar.arrive(1, nullptr);
        while (!bar.failed()) std::this_thread::yield();      // rank 0 is now waiting in barrier 2 with its failure
        b1[1] = r1;                                           // ... and only now does rank 1 act on barrier 1
        b2[1] = bar.arrive(1, nullptr);
    });
    t0.join(); t1.join(); t2.join();
    for (int r = 0; r < 3; r++) { CHECK(!b1[r]); CHECK(b2[r]); }
    CHECK(bar.message() == boom);
    CHECK(bar.failed_rank() == 0);
}

// The same through rank_phase, the loop every rank thread of multi_gpu.hip / vcf_multi.hip runs: rank 2 throws in
// phase 2; every rank leaves at barrier 2, no body of phase 3 runs, the exception itself stays with rank 2.
static void phases()
{
    RankBarrier bar(3);
    int left_at[3] = {0, 0, 0};
    std::atomic<int> phase3_bodies{0};
    std::string fails[3];
    std::exception_ptr err[3];
    auto rank = [&](int r) {
        for (int p = 1; p <= 4; p++) {
            const bool ok = edsx::rank_phase(bar, r, fails[r], [&] {
                if (p == 2 && r == 2) throw std::runtime_error("rank 2 failed in phase 2");
                if (p == 3) phase3_bodies++;
            }, &err[r]);
            if (!ok) { left_at[r] = p; return; }
        }
    };
    std::thread a([&] { rank(0); }), b([&] { rank(1); }), c([&] { rank(2); });
    a.join(); b.join(); c.join();
    for (int r = 0; r < 3; r++) CHECK(left_at[r] == 2);
    CHECK(phase3_bodies == 0);
    CHECK(bar.message() == "rank 2 failed in phase 2");
    CHECK(bar.failed_rank() == 2);
    CHECK(err[2] != nullptr && err[0] == nullptr && err[1] == nullptr);
    bar.reset();
    CHECK(!bar.failed() && bar.message().empty());
    // after reset the barrier is clean again
    bool r[3] = {true, true, true};
    std::thread x([&] { r[0] = bar.arrive(0, nullptr); }), y([&] { r[1] = bar.arrive(1, nullptr); }), z([&] { r[2] = bar.arrive(2, nullptr); });
    x.join(); y.join(); z.join();
    CHECK(!r[0] && !r[1] && !r[2]);
}

int main()
{
    for (int i = 0; i < 50; i++) late_reader();
    for (int i = 0; i < 50; i++) phases();
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("rank barrier ok\n");
    return 0;
}
