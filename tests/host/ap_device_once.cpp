// Stand-alone host check of ap_once_per_device (airpose_amd/csrc/ap_device.h).  It makes no HIP call, so it runs without a GPU;
// tests/test_ap_device.py builds it under ThreadSanitizer and runs it.  Exit status 0 = every check held.
//
// THREADS threads race through every one of the AP_MAX_DEVICES slots of a fresh, zero-initialised ApDeviceOnce, ROUNDS times over,
// with a counting stand-in for f.  Held, per round and slot:
//   * f ran at least once (and at most once per thread);
//   * a thread that has seen the call succeed never runs f again, and once every thread has seen that, nobody does;
//   * an f that fails on its first FAILS calls has each failure returned to the caller that ran it (not swallowed, not cached),
//     is retried, and is cached from its first success on;
//   * what f wrote before it returned is visible to every thread that sees the flag set (the acquire / release pair).
#include "../../airpose_amd/csrc/ap_device.h"

#include <cstdio>
#include <thread>
#include <vector>

namespace {
constexpr int THREADS = 8, ROUNDS = 1000, FAILS = 5;

struct Slots {
    ApDeviceOnce once;                                       // static storage: zero-initialised, as in the launchers
    std::atomic<int> runs[AP_MAX_DEVICES];                   // calls of f
    std::atomic<int> payload[AP_MAX_DEVICES];                // what a successful f leaves behind
};
Slots g_ok[ROUNDS], g_retry[ROUNDS];
std::atomic<int> g_errors{0};

void expect(bool ok, const char* what, int round, int dev) {
    if (ok) return;
    if (g_errors.fetch_add(1) < 10) std::fprintf(stderr, "FAILED round %d slot %d: %s\n", round, dev, what);
}

// sense-reversing spin barrier (C++17 has none)
std::atomic<int> g_waiting{0}, g_phase{0};
void barrier() {
    const int phase = g_phase.load(std::memory_order_acquire);
    if (g_waiting.fetch_add(1, std::memory_order_acq_rel) == THREADS - 1) {
        g_waiting.store(0, std::memory_order_relaxed);
        g_phase.store(phase + 1, std::memory_order_release);
    } else {
        while (g_phase.load(std::memory_order_acquire) == phase) std::this_thread::yield();
    }
}

// one thread's walk over the slots of one round; fails: how many first calls of f (over all threads) report an error
void walk(Slots& s, int round, int tid, int fails) {
    for (int i = 0; i < AP_MAX_DEVICES; ++i) {
        const int dev = (i + tid * 5) % AP_MAX_DEVICES;      // the threads start on different slots and cross each other
        bool seen_success = false;
        int my_runs = 0, my_failed_runs = 0, my_errors = 0;
        auto f = [&]() -> hipError_t {
            expect(!seen_success, "f ran after this thread had seen a success", round, dev);
            ++my_runs;
            if (s.runs[dev].fetch_add(1, std::memory_order_relaxed) < fails) { ++my_failed_runs; return hipErrorUnknown; }
            s.payload[dev].store(dev + 1, std::memory_order_relaxed);
            return hipSuccess;
        };
        for (int call = 0; call < fails + 4; ++call) {
            const hipError_t e = ap_once_per_device(s.once, dev, f);
            if (e != hipSuccess) { ++my_errors; continue; }
            seen_success = true;
            expect(s.payload[dev].load(std::memory_order_relaxed) == dev + 1, "the flag was visible before what f wrote", round, dev);
        }
        expect(seen_success, "no success within fails + 4 calls", round, dev);
        expect(my_errors == my_failed_runs, "an error was returned without running f, or a failure of f was swallowed", round, dev);
        expect(my_runs <= my_failed_runs + 1, "one thread ran f successfully more than once", round, dev);
    }
}

void thread_main(int tid) {
    for (int mode = 0; mode < 2; ++mode) {
        Slots* all = mode ? g_retry : g_ok;
        const int fails = mode ? FAILS : 0;
        for (int r = 0; r < ROUNDS; ++r) {
            barrier();                                       // all threads enter the round together: the first calls do race
            walk(all[r], r, tid, fails);
            barrier();
            if (tid == 0) {
                for (int d = 0; d < AP_MAX_DEVICES; ++d) {
                    const int n = all[r].runs[d].load(std::memory_order_relaxed);
                    expect(n >= fails + 1, "f did not run (often enough to succeed)", r, d);
                    expect(n <= fails + THREADS, "f ran more often than once per thread after its failures", r, d);
                }
            }
            for (int d = 0; d < AP_MAX_DEVICES; ++d) {       // cached for good: f (which would complain) is not called
                const hipError_t e = ap_once_per_device(all[r].once, d, [&]() -> hipError_t {
                    expect(false, "f ran in a round that was over", r, d);
                    return hipErrorUnknown;
                });
                expect(e == hipSuccess, "a cached success was not returned", r, d);
            }
        }
    }
}
}  // namespace

int main() {
    std::vector<std::thread> threads;
    for (int t = 0; t < THREADS; ++t) threads.emplace_back(thread_main, t);
    for (auto& t : threads) t.join();
    long races = 0;                                          // slots in which more than one thread ran f: the allowed double run did occur
    for (int r = 0; r < ROUNDS; ++r)
        for (int d = 0; d < AP_MAX_DEVICES; ++d) races += g_ok[r].runs[d].load() > 1;
    const int errors = g_errors.load();
    std::printf("ap_once_per_device: %d threads x %d slots x %d rounds x 2 modes, %ld slots run by more than one thread, %d errors\n",
                THREADS, AP_MAX_DEVICES, ROUNDS, races, errors);
    return errors ? 1 : 0;
}
