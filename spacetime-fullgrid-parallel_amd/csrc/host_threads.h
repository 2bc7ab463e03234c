// The host threads of libstk's set-up routines (mesh_refine.hip, sample.hip): how many, a
// fork-join over them, and the share of n items that ends before thread k.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <thread>
#include <vector>

namespace {

inline int host_threads(int64_t items)
{
    int T = (int)std::thread::hardware_concurrency();
    if (const char *env = getenv("STK_HOST_THREADS")) T = atoi(env);
    T = std::max(1, std::min(T, 32));
    if (items < 16384) T = 1;
    return T;
}

template <class F>
void on_threads(int T, F body)
{
    if (T == 1) {
        body(0);
        return;
    }
    std::vector<std::thread> pool;
    for (int k = 0; k < T; ++k) pool.emplace_back(body, k);
    for (auto &th : pool) th.join();
}

inline int64_t share(int64_t n, int T, int k) { return n * k / T; }

}  // namespace
