// kernel_times.hpp — device time per kernel (edsx_set_timing / edsx_get_timing) for every pipeline but the MSA one, whose
// timers live inside the benchmark's timed region and are its own (msa_device.hip).
//
//   KernelTimes   the accumulator a pipeline keeps: total milliseconds and launches per name, in order of first use
//   TimedRuns     the scope of one call: event pairs around its launches on one stream, read after a synchronisation
#pragma once

#include "dev_util.hpp"

#include <deque>
#include <vector>

namespace edsx {

class KernelTimes {
public:
    void set(bool on) { on_ = on; acc_.clear(); }
    bool on() const { return on_; }
    void add(const char* name, float ms)
    {
        for (auto& a : acc_) if (std::string(a.name) == name) { a.total_ms += ms; a.count++; return; }
        acc_.push_back({name, ms, 1});
    }
    int get(const char** names, float* ms, int* counts, int cap) const
    {
        int n = 0;
        for (const auto& a : acc_) {
            if (n >= cap) break;
            names[n] = a.name; ms[n] = a.total_ms; counts[n] = a.count; n++;
        }
        return n;
    }

private:
    struct Acc { const char* name; float total_ms; int count; };
    bool on_ = false;
    std::vector<Acc> acc_;
};

class TimedRuns {
public:
    // times may be null: then only runs with a bucket are timed
    TimedRuns(hipStream_t st, KernelTimes* times) : st_(st), times_(times && times->on() ? times : nullptr) {}

    // launch(), between two events when timing is on; no event is made or recorded when it is off
    template <class F> void run(const char* name, F&& launch)
    {
        if (times_) record(name, nullptr, launch); else launch();
    }
    // always between two events: *bucket grows by the time at harvest(), whether timing is on or not
    template <class F> void run(const char* name, F&& launch, double* bucket) { record(name, bucket, launch); }

    // after a stream synchronisation: the times of the runs since the last harvest go where they belong
    void harvest()
    {
        for (auto& t : timed_) {
            const float ms = t.ev.ms();
            if (t.bucket) *t.bucket += ms;
            if (times_) times_->add(t.name, ms);
        }
        timed_.clear();
    }

private:
    struct Timed { const char* name; double* bucket; EventPair ev; Timed(const char* n, double* b) : name(n), bucket(b) {} };
    template <class F> void record(const char* name, double* bucket, F&& launch)
    {
        timed_.emplace_back(name, bucket);
        EDSX_HIP(hipEventRecord(timed_.back().ev.a, st_));
        launch();
        EDSX_HIP(hipEventRecord(timed_.back().ev.b, st_));
    }
    hipStream_t st_;
    KernelTimes* times_;
    std::deque<Timed> timed_;
};

} // namespace edsx
