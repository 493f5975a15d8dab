#pragma once
// The host threads of the batched entries (api_batch.cpp, api_mle_batch.cpp).  Plain C++, no HIP: shared with the stand-alone
// driver of the verification's host side (tests/c_driver/sumcheck_verify_host.cpp), which times the replay alone on them.
#include <stddef.h>

#include <atomic>
#include <thread>
#include <vector>

// Host threads for the per-table work of a batched entry (a table's rounds of a radix pass, a proof's replay): up to 8, each with
// at least 4 tables (one table's k <= 10 rounds are a SHA3 challenge per round plus O(2^k) scalar field work, of the order of a
// thread start).  Not tuned yet: the 16 x 2^20 batch is bound by these rounds, so the count is the first thing to
// sweep.
inline unsigned host_threads(size_t count) {
    const unsigned hw = std::thread::hardware_concurrency();
    size_t t = count / 4;
    if (t > 8) t = 8;
    if (hw && t > hw) t = hw;
    return t < 1 ? 1 : (unsigned)t;
}

template <class F>
void parallel_for(size_t count, F &&fn) {
    const unsigned nt = host_threads(count);
    if (nt <= 1) {
        for (size_t j = 0; j < count; j++) fn(j);
        return;
    }
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t j; (j = next.fetch_add(1)) < count;) fn(j);
    };
    std::vector<std::thread> th;
    th.reserve(nt - 1);
    for (unsigned t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
}
