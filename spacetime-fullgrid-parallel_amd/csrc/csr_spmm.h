// Internal form of stk_csr_spmm (kron.hip) for callers inside the library.
#pragma once
#include <cstdint>

// y = alpha * A(t) x + beta * z on the first `cols` columns of a slab (n_loc <= cols <= ld):
// columns n_loc .. cols - 1 are written as zero, columns cols .. ld - 1 are neither read nor
// written -- the multigrid's slab may be a column range of a wider one whose other columns
// another stream is working on (mg.hip).  cols = ld is stk_csr_spmm.
int stk_csr_spmm_cols(void *stream, int32_t rows, int32_t n_loc, int32_t ld, int32_t cols, const int32_t *indptr,
                      const int32_t *indices, const double *vals_a, double ca, const double *vals_m, const double *cm,
                      const double *x, double alpha, double beta, const double *z, double *y);
