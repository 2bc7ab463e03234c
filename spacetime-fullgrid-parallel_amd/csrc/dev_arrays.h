// The one owner of a plan's device arrays.  A plan embeds one stk_dev_arrays and
// allocates through it; `delete plan` then frees the device memory, and nothing else
// does.  Plans keep their raw T * members (kernel arguments stay plain pointers).
// Short-lived device arrays use a local stk_dev_arrays on the stack.
// Not thread-safe: callers that share one owner between threads lock around adopt().
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

// The seam to the device (common.hip, over hipMalloc / hipFree / hipMemcpy).
void *stk_dev_malloc(size_t bytes);  // null on failure; the HIP reason goes to stk_set_error
void stk_dev_free(void *p);
bool stk_dev_copy_in(void *dst, const void *src, size_t bytes);  // host to device, synchronous

struct stk_dev_arrays {
    std::vector<void *> ptrs;

    stk_dev_arrays() = default;
    stk_dev_arrays(const stk_dev_arrays &) = delete;
    stk_dev_arrays &operator=(const stk_dev_arrays &) = delete;
    stk_dev_arrays(stk_dev_arrays &&other) noexcept { ptrs.swap(other.ptrs); }
    ~stk_dev_arrays()
    {
        for (void *p : ptrs) stk_dev_free(p);
    }

    // n elements, uninitialised (one element for n == 0); null on failure
    template <class T>
    T *alloc(size_t n)
    {
        ptrs.push_back(nullptr);  // the place first: nothing can fail between the allocation and its entry
        void *p = stk_dev_malloc((n ? n : 1) * sizeof(T));
        if (p)
            ptrs.back() = p;
        else
            ptrs.pop_back();
        return static_cast<T *>(p);
    }

    // a device copy of src[0..n); null, with nothing kept, if the allocation or the copy fails
    template <class T>
    T *upload(const T *src, size_t n)
    {
        T *p = alloc<T>(n);
        if (p && n && !stk_dev_copy_in(p, src, n * sizeof(T))) release(p), p = nullptr;
        return p;
    }
    template <class T>
    T *upload(const std::vector<T> &host)
    {
        return upload(host.data(), host.size());
    }

    void adopt(void *p) { ptrs.push_back(p); }

    // everything `other` owns becomes this owner's
    void take(stk_dev_arrays &&other)
    {
        ptrs.insert(ptrs.end(), other.ptrs.begin(), other.ptrs.end());
        other.ptrs.clear();
    }

    // frees p now and forgets it (null: nothing to do); the grow-on-demand buffers use it
    void release(void *p)
    {
        if (!p) return;
        auto it = std::find(ptrs.begin(), ptrs.end(), p);
        if (it != ptrs.end()) ptrs.erase(it);
        stk_dev_free(p);
    }
};
