// The grouping step of stk_sample_pairs_adjoint (sample_adj_sort.hip), called by sample.hip:
// a stable sort of n < 2^31 (key, term) records by the low key_bits bits of the key, in
// caller-provided double buffers and scratch; *result = the half that holds the outcome.
#pragma once
#include "stk_common.h"

int stk_adj_sort_temp_bytes(int64_t n, size_t *bytes);
int stk_adj_sort(hipStream_t st, void *temp, size_t temp_bytes, uint64_t *const keys[2], double *const vals[2],
                 int64_t n, int key_bits, int *result);
