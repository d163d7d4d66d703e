// rank_barrier.hpp — barrier of the rank threads of one process (multi_gpu.hip), carrying the first failure to every
// rank.  Plain C++17: no HIP, so that a CPU test can drive it (tests/cpp/test_rank_barrier.cpp).
//
// A rank that fails leaves right after the barrier that reports it; every other rank must leave at the SAME barrier,
// or the ones that go on wait for it in the next barrier or collective for ever.  So the failure state a rank acts on
// is the one of the barrier it has just passed: arrive() returns it, snapshotted under the lock when the generation
// flips.  Reading it later (failed()) could already see a failure that a faster rank hit in the NEXT phase.
#pragma once

#include <condition_variable>
#include <exception>
#include <mutex>
#include <string>

namespace edsx {

class RankBarrier {
public:
    explicit RankBarrier(int n) : n_(n) {}
    // returns when all n have arrived: true when some rank had failed by the time the last one arrived
    bool arrive(int rank, const std::string* failure)
    {
        std::unique_lock<std::mutex> lk(mu_);
        if (failure && (!failed_ || rank < failed_rank_)) { failed_ = true; msg_ = *failure; failed_rank_ = rank; }
        const unsigned long g = gen_;
        if (++count_ == n_) { count_ = 0; gen_failed_ = failed_; gen_++; cv_.notify_all(); }
        else cv_.wait(lk, [&] { return gen_ != g; });
        // (gen_failed_ cannot change before this rank has returned: the next flip needs this rank's next arrival)
        return gen_failed_;
    }
    bool failed() const { std::lock_guard<std::mutex> g(mu_); return failed_; }
    std::string message() const { std::lock_guard<std::mutex> g(mu_); return msg_; }
    int failed_rank() const { std::lock_guard<std::mutex> g(mu_); return failed_rank_; }
    void reset() { std::lock_guard<std::mutex> g(mu_); failed_ = gen_failed_ = false; msg_.clear(); failed_rank_ = -1; }
private:
    int n_, count_ = 0; unsigned long gen_ = 0;
    bool failed_ = false, gen_failed_ = false; std::string msg_; int failed_rank_ = -1;
    mutable std::mutex mu_; std::condition_variable cv_;
};

// One phase of a rank thread: the body runs unless this rank has failed before; then every rank waits for the others.
// false: some rank has failed, leave (every rank gets false at the same barrier).  `error`, if given, keeps the
// exception itself, so that the caller can rethrow the failing rank's error with its type.
template <class F> bool rank_phase(RankBarrier& bar, int rank, std::string& fail, F&& body, std::exception_ptr* error = nullptr)
{
    if (fail.empty()) {
        try { body(); } catch (const std::exception& ex) {
            fail = ex.what();
            if (fail.empty()) fail = "unknown failure";
            if (error) *error = std::current_exception();
        }
    }
    return !bar.arrive(rank, fail.empty() ? nullptr : &fail);
}

} // namespace edsx
