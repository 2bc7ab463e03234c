// csrc/dev_arrays.h without a GPU: the three seam functions are defined here over malloc,
// with a table of live pointers, call counters and two switches ("fail the k-th malloc",
// "fail the k-th copy").  Built with -fsanitize=address,undefined as an ordinary program
// (tests/test_dev_arrays_host.py); prints "dev_arrays_host ok" and returns 0 when every
// check holds, otherwise names the line of the first one that does not and returns 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "dev_arrays.h"

namespace {

std::set<void *> g_live;
int g_mallocs = 0, g_copies = 0, g_frees = 0;
int g_fail_malloc = 0, g_fail_copy = 0;  // 1-based position of the call that fails, 0: none
int g_bad_frees = 0;                     // frees of a pointer that is not live (twice, or never allocated)
bool g_failed = false;                   // did the seam fail a call since the flag was last cleared?
size_t g_last_bytes = 0;

void reset(int fail_malloc = 0, int fail_copy = 0)
{
    g_mallocs = g_copies = g_frees = g_bad_frees = 0;
    g_fail_malloc = fail_malloc, g_fail_copy = fail_copy;
    g_failed = false;
}

}  // namespace

void *stk_dev_malloc(size_t bytes)
{
    g_last_bytes = bytes;
    if (++g_mallocs == g_fail_malloc) {
        g_failed = true;
        return nullptr;
    }
    void *p = std::malloc(bytes);
    g_live.insert(p);
    return p;
}

void stk_dev_free(void *p)
{
    ++g_frees;
    if (g_live.erase(p) != 1) {
        ++g_bad_frees;
        return;
    }
    std::free(p);
}

bool stk_dev_copy_in(void *dst, const void *src, size_t bytes)
{
    if (++g_copies == g_fail_copy) {
        g_failed = true;
        return false;
    }
    std::memcpy(dst, src, bytes);
    return true;
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

// a call returns null exactly when the seam failed inside it; a failed call keeps nothing
#define STEP(ptr)                                   \
    do {                                            \
        CHECK(((ptr) == nullptr) == g_failed);      \
        if (g_failed) CHECK(g_live.size() == live); \
        g_failed = false;                           \
        live = g_live.size();                       \
    } while (0)

namespace {

// alloc / upload / adopt / release in one scope: 6 mallocs, 3 copies when nothing fails
int mixed_sequence()
{
    const int32_t ints[7] = {3, 1, 4, 1, 5, 9, 2};
    const double doubles[3] = {0.5, -2.0, 8.25};
    const std::vector<float> floats = {1.0f, 2.0f, 3.0f, 4.0f, 5.0f};
    {
        stk_dev_arrays a;
        size_t live = g_live.size();
        CHECK(live == 0);
        double *p1 = a.alloc<double>(10);
        STEP(p1);
        if (p1) p1[9] = 1.0;
        int32_t *p2 = a.upload(ints, 7);
        STEP(p2);
        if (p2) CHECK(std::memcmp(p2, ints, sizeof(ints)) == 0);
        void *ext = stk_dev_malloc(32);  // an array that came from elsewhere
        STEP(ext);
        if (ext) a.adopt(ext);
        double *p3 = a.upload(doubles, 3);
        STEP(p3);
        if (p3) CHECK(p3[2] == 8.25);
        a.release(p1);  // (null when its malloc failed: nothing to do)
        CHECK(g_live.size() == live - (p1 ? 1 : 0) && g_live.count(p1) == 0);
        live = g_live.size();
        char *p4 = a.alloc<char>(0);
        STEP(p4);
        float *p5 = a.upload(floats);
        STEP(p5);
        if (p5) CHECK(p5[4] == 5.0f);
        a.release(nullptr);
        CHECK(g_live.size() == live && a.ptrs.size() == live);
    }
    CHECK(g_live.empty());     // everything that did get allocated is freed at scope exit,
    CHECK(g_bad_frees == 0);   // nothing twice, and nothing that was never allocated
    return 0;
}

int upload_with_a_failing_copy()
{
    const double src[4] = {1, 2, 3, 4};
    reset(0, 1);
    stk_dev_arrays a;
    CHECK(a.upload(src, 4) == nullptr);
    CHECK(g_mallocs == 1 && g_frees == 1 && g_live.empty() && a.ptrs.empty());  // freed at once, not at scope exit
    CHECK(a.upload(src, 4) != nullptr && g_live.size() == 1);                   // and the owner stays usable
    return 0;
}

int take_moves_every_pointer()
{
    reset();
    {
        stk_dev_arrays b;
        CHECK(b.alloc<int>(2) && b.alloc<int>(3));
        {
            stk_dev_arrays a;
            CHECK(a.alloc<double>(1) && a.alloc<double>(2) && a.alloc<double>(3));
            const std::vector<void *> held = a.ptrs;
            b.take(std::move(a));
            CHECK(a.ptrs.empty() && b.ptrs.size() == 5);
            for (void *p : held) CHECK(std::find(b.ptrs.begin(), b.ptrs.end(), p) != b.ptrs.end());
        }
        CHECK(g_frees == 0 && g_live.size() == 5);  // the owner that was emptied frees nothing
    }
    CHECK(g_frees == 5 && g_live.empty() && g_bad_frees == 0);
    return 0;
}

int move_construction_moves_every_pointer()
{
    reset();
    {
        stk_dev_arrays a;
        CHECK(a.alloc<double>(4) && a.alloc<char>(5));
        const std::vector<void *> held = a.ptrs;
        {
            stk_dev_arrays b(std::move(a));
            CHECK(a.ptrs.empty() && b.ptrs == held);
        }
        CHECK(g_frees == 2 && g_live.empty());
    }
    CHECK(g_frees == 2 && g_bad_frees == 0);  // the moved-from owner frees nothing
    return 0;
}

int empty_arrays_have_one_element()
{
    reset();
    stk_dev_arrays a;
    double *p = a.alloc<double>(0);
    CHECK(p != nullptr && g_last_bytes == sizeof(double));
    p[0] = 1.0;  // (the sanitizer watches the write)
    const int32_t *none = nullptr;
    int32_t *q = a.upload(none, 0);
    CHECK(q != nullptr && g_last_bytes == sizeof(int32_t) && g_copies == 0);
    q[0] = 7;
    int32_t *r = a.upload(std::vector<int32_t>());
    CHECK(r != nullptr && r != q && g_live.size() == 3);
    return 0;
}

int release_of_null_does_nothing()
{
    reset();
    stk_dev_arrays a;
    CHECK(a.alloc<int>(1) != nullptr);
    a.release(nullptr);
    CHECK(g_frees == 0 && g_bad_frees == 0 && a.ptrs.size() == 1 && g_live.size() == 1);
    return 0;
}

}  // namespace

int main()
{
    reset();
    if (mixed_sequence()) return 1;
    const int n_mallocs = g_mallocs, n_copies = g_copies;
    if (n_mallocs != 6 || n_copies != 3 || g_frees != 6) {
        std::fprintf(stderr, "the clean sequence made %d mallocs, %d copies, %d frees\n", n_mallocs, n_copies, g_frees);
        return 1;
    }
    for (int k = 1; k <= n_mallocs; ++k) {
        reset(k, 0);
        if (mixed_sequence()) return std::fprintf(stderr, "  (with malloc %d failing)\n", k), 1;
        if (g_mallocs != n_mallocs) return std::fprintf(stderr, "malloc %d never came\n", k), 1;
    }
    for (int k = 1; k <= n_copies; ++k) {
        reset(0, k);
        if (mixed_sequence()) return std::fprintf(stderr, "  (with copy %d failing)\n", k), 1;
        if (g_copies != n_copies) return std::fprintf(stderr, "copy %d never came\n", k), 1;
    }
    if (upload_with_a_failing_copy() || take_moves_every_pointer() || move_construction_moves_every_pointer() ||
        empty_arrays_have_one_element() || release_of_null_does_nothing())
        return 1;
    if (!g_live.empty() || g_bad_frees != 0) return std::fprintf(stderr, "arrays left behind\n"), 1;
    std::printf("dev_arrays_host ok\n");
    return 0;
}
