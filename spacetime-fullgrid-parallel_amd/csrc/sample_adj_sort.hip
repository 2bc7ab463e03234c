// The grouping step of stk_sample_pairs_adjoint (sample.hip, include/stk.h "the adjoint of
// paired sampling"): a STABLE sort of (destination key, term) records by key, so that the
// terms of one slab entry end up next to each other in the order they were written --
// ascending point index.  rocPRIM's radix sort (header-only, ships with ROCm; stable by
// its contract) on the low `key_bits` bits of the 64-bit keys.  A translation unit of its
// own: the templates take long to compile and nothing else needs them.
#include <cstring>  // rocPRIM's headers use memcpy without including it

#include <rocprim/rocprim.hpp>

#include "sample_adj_sort.h"

namespace {

hipError_t sort_call(void *temp, size_t &bytes, uint64_t *const keys[2], double *const vals[2], unsigned int n,
                     unsigned int key_bits, hipStream_t st, int *result)
{
    rocprim::double_buffer<uint64_t> k(keys[0], keys[1]);
    rocprim::double_buffer<double> v(vals[0], vals[1]);
    const hipError_t e = rocprim::radix_sort_pairs(temp, bytes, k, v, n, 0u, key_bits, st, false);
    if (result) *result = k.current() == keys[0] ? 0 : 1;
    return e;
}

}  // namespace

// Bytes of scratch a sort of n records needs, whatever the number of key bits.  Asks
// rocPRIM, which looks at the current device to pick its configuration.
int stk_adj_sort_temp_bytes(int64_t n, size_t *bytes)
{
    STK_REQUIRE(bytes && n >= 0 && n < ((int64_t)1 << 31), "stk_adj_sort_temp_bytes: n=%lld", (long long)n);
    uint64_t *const keys[2] = {nullptr, nullptr};
    double *const vals[2] = {nullptr, nullptr};
    size_t need = 0;
    STK_HIP(sort_call(nullptr, need, keys, vals, (unsigned int)n, 64u, nullptr, nullptr));
    *bytes = need;
    return 0;
}

// Sorts the n records (keys[0], vals[0]) by the low key_bits bits of the key, stably;
// (keys[1], vals[1]) are the second halves of the two double buffers.  *result names the
// half that holds the sorted records.  Enqueues on `st`; allocates nothing.
int stk_adj_sort(hipStream_t st, void *temp, size_t temp_bytes, uint64_t *const keys[2], double *const vals[2],
                 int64_t n, int key_bits, int *result)
{
    STK_REQUIRE(temp && result && n > 0 && n < ((int64_t)1 << 31) && key_bits >= 1 && key_bits <= 64,
                "stk_adj_sort: n=%lld key_bits=%d", (long long)n, key_bits);
    size_t bytes = temp_bytes;
    STK_HIP(sort_call(temp, bytes, keys, vals, (unsigned int)n, (unsigned int)key_bits, st, result));
    return 0;
}
