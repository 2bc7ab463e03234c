/* stk.h -- C ABI of libstk, the MI355X (gfx950) hot path of the space-time
 * Kronecker solver.
 *
 * The reference (Jannertje/spacetime-fullgrid-parallel) has no FFI: its
 * boundary is the duck-typed Python protocol LinearOperatorMPI / KronVectorMPI
 * (reference source/mpi_kron.py:13-36, source/mpi_vector.py:41-122).  Every
 * entry point below names the reference method whose arithmetic it replaces;
 * the Python classes in spacetime-fullgrid-parallel_amd/source/ bind them with
 * ctypes and keep the reference's class names and call signatures.
 *
 * Conventions
 *  - extern "C", int status return (0 = ok, nonzero = error; text from
 *    stk_last_error()).  No exceptions cross the ABI.
 *  - All array arguments are DEVICE pointers unless the name ends in _host.
 *    The caller owns every buffer.  float64 values, int32 indices
 *    (reference source/mpi_shared_mem.py:46-48).
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 *    work is enqueued asynchronously on it; nothing synchronises.
 *  - One caller thread per process, one process per GPU.
 *
 * Vector layout ("space-major"): the local slab of a KronVectorMPI, which the
 * reference stores as X_loc[t][i] (mpi_vector.py:62-71), lives on the device
 * as x[i * ld + t], i in [0, M), t in [0, n_loc), ld >= n_loc.  Entries
 * t in [n_loc, ld) are padding and are kept zero by every kernel.  A time
 * column is therefore contiguous: a CSR gather of neighbour j fetches n_loc
 * consecutive doubles.  Ghost time rows t = -1 and t = n_loc (the reference's
 * X_loc_bdr[0], X_loc_bdr[-1], mpi_vector.py:148-175) are separate contiguous
 * arrays of length M.
 */
#ifndef STK_H
#define STK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library ------------------------------------------------------------ */
const char *stk_last_error(void);
int stk_version(void);
/* Device properties the host side sizes launches with (CUs, wavefront). */
int stk_device_info(int32_t *n_cu, int32_t *wave_size, int64_t *hbm_bytes);
/* Process-wide tuning keys, settable from any thread.  Returns non-zero, with
 * stk_last_error naming the key, for an unknown key or a value outside the key's
 * range.  Launch keys act on the next launch; plan keys are read when a plan is
 * created and hold for its lifetime.  "Bit-identical" means results never depend
 * on the key; "rounding" means the last bits may change.
 *   ell_wg_per_cu        (launch, 0..16, default 0) persistent workgroups per CU
 *                        of stk_kron_ell_apply; 0 = 2 for K >= 12, else 3; never
 *                        more than fit 160 KiB of LDS.  Bit-identical.
 *   ell_force_wide       (launch, 0..1, default 0) 64-bit addressing in the
 *                        sliced-ELL Kronecker kernels on small slabs (tests).
 *                        Bit-identical.
 *   rows_force_wide      (launch, 0..1, default 0) the same for the ELL row engine
 *                        (stk_mg_*, stk_ell_rows_*).  Bit-identical.
 *   pack_rows            (plan, 1..2, default 2) matrix rows per slot row of the
 *                        packed form of stk_kron_plan_create.  Bit-identical.
 *   pack_multi_lanes     (launch, 0..2, default 1) stk_kron_pack_apply_multi:
 *                        1 = a lane group per term on long slabs, turns on short
 *                        ones; 2 = lane groups wherever two slot rows fit a
 *                        workgroup (at most 256 lanes per slot row); 0 = turns
 *                        always.  Bit-identical.
 *   pack_check_steps     (launch, 0..1, default 0) stk_kron_pack_apply_multi_steps
 *                        checks the stated time steps against the factors (one
 *                        stream synchronisation per call; tests).  No effect on
 *                        results that pass the check.
 *   mg_strip_mb          (launch, 0..1048576, default 250) working set in MB of a
 *                        strip of the strip-wise Gauss-Seidel sweeps; 0 = off.
 *                        Bit-identical.
 *   mg_strip_width       (launch, 0..1024, default 2) least strip width in units
 *                        of (sweeps x groups) bands; 0 = as thin as possible
 *                        (tests).  Bit-identical.
 *   mg_strips_used       (counter) launches that came from a strip table: 0
 *                        resets it, n > 0 fails unless at least n happened.
 *   mg_zero_start        (launch, 0..1, default 1) 1 = the first sweep of a level
 *                        visit does not read the zero start vector; 0 = zero it in
 *                        memory.  Bit-identical.
 *   mg_gs_diag_free      (plan, 0..2, default 1) row form of the Gauss-Seidel
 *                        copies of stk_mg_create_from_csr (see there).  Rounding.
 *   mg_fuse_restrict     (launch, 0..1, default 1) restricted residual as
 *                        (R A) u - R f for plans that follow it (see
 *                        stk_mg_set_option).  Rounding.
 *   mg_restrict_one_pass (launch, 0..2, default 1) (R A) u - R f as one pass:
 *                        1 = for matrices with per-slice coefficients, 2 = for
 *                        every plan, 0 = never.  Bit-identical.
 *   mg_fuse_coarse       (launch, 0..1, default 1) the coarse end of the V-cycle
 *                        as one fused launch.  Bit-identical.
 *   mg_coarse_lds        (launch, 0..1, default 1) the fused coarse end keeps its
 *                        level vectors in LDS.  Bit-identical.
 *   mg_coarse_uniform    (launch, 0..2, default 1) the LDS form on uniform ELL
 *                        copies; 0 = on the levels' own copies; 2 = 512 threads
 *                        throughout.  Bit-identical. */
int stk_set_tuning(const char *key, int32_t value);

/* ---- time slices of a slab (BlockDiagMPI._matvec with different operators per
 *      slice, mpi_kron.py:126-131: every distinct operator gets the slices it owns
 *      as one slab) --------------------------------------------------------------
 * gather:  y[i*ld_y + k] = x[i*ld_x + cols[k]], k < n_cols; the padding columns
 *          n_cols .. ld_y-1 of y are written as zero.
 * scatter: y[i*ld_y + cols[k]] = x[i*ld_x + k], k < n_cols; other columns of y
 *          are left alone.  cols: device int32; the caller guarantees that they
 *          are valid, distinct columns of the wider slab. */
int stk_slab_gather_columns(void *stream, int32_t M, int32_t n_cols,
                            const int32_t *cols, const double *x, int32_t ld_x,
                            double *y, int32_t ld_y);
int stk_slab_scatter_columns(void *stream, int32_t M, int32_t n_cols,
                             const int32_t *cols, const double *x, int32_t ld_x,
                             double *y, int32_t ld_y);

/* ---- slab storage for hosts that own no device allocator (KronVectorMPI.__init__
 *      / reset, mpi_vector.py:62-71; scatter / gather, :124-138) ------------------
 * stk_slab_alloc: a zeroed slab of M rows with leading dimension *ld =
 * stk_slab_ld(n_loc) (n_loc rounded up to even: time pairs are 16-byte aligned).
 * upload / download move the reference's time-major host block X_loc[t][i],
 * (n_loc, M) C order, to / from the space-major slab (a transpose on the device
 * through a staging buffer; padding columns are written as zero).  These two
 * calls block until the transfer is complete. */
int stk_slab_ld(int32_t n_loc);
int stk_slab_alloc(int32_t M, int32_t n_loc, int32_t *ld, double **slab);
int stk_slab_free(double *slab);
int stk_slab_upload(void *stream, int32_t M, int32_t n_loc, int32_t ld,
                    const double *x_host, double *slab);
int stk_slab_download(void *stream, int32_t M, int32_t n_loc, int32_t ld,
                      const double *slab, double *x_host);
/* dst[c * ld_dst + r] = src[r * ld_src + c] for r < rows, c < cols (device to
 * device, tiled through LDS); the columns rows .. zero_to-1 of dst are written
 * as zero (0: none).  Time-major block <-> slab, and the block transposes of
 * KronVectorMPI.permute (mpi_vector.py:212-240). */
int stk_transpose(void *stream, int32_t rows, int32_t cols, const double *src,
                  int64_t ld_src, double *dst, int64_t ld_dst, int32_t zero_to);
/* The two time rows a slab sends to its neighbour ranks in communicate_bdr
 * (mpi_vector.py:148-167): first[j * stride_first] = x[j][0], last[j *
 * stride_last] = x[j][n_loc-1], both from one pass over the slab's lines.
 * Stride 1: contiguous send buffers; stride 2: every other double of an
 * interleaved ghost buffer gh[j] = (lo, hi) (stk_kron_pack_apply), e.g. the
 * neighbour's own buffer mapped into this process.  Either pointer may be NULL. */
int stk_halo_pack(void *stream, int32_t M, int32_t n_loc, int32_t ld,
                  const double *x, double *first, int32_t stride_first,
                  double *last, int32_t stride_last);
/* out[k * ld_out + j] = x[j][t_idx[k]], k < n_rows: the time rows communicate_dofs
 * sends (mpi_vector.py:189-203), all from one pass over the slab.  t_idx: device
 * int32, valid local time indices. */
/* stk_halo_pack, and per spatial dof the four entries the boundary steps of a Kronecker
 * apply read once the halo is there (stk_kron_pack_boundary_apply), from the same two
 * lines of the row: records[4*j .. 4*j+3] = (x[j][0], x[j][1], x[j][n_loc-2], x[j][n_loc-1]);
 * first / last may be NULL. */
int stk_halo_pack_records(void *stream, int32_t M, int32_t n_loc, int32_t ld,
                          const double *x, double *first, int32_t stride_first,
                          double *last, int32_t stride_last, double *records);
int stk_slab_extract_time_rows(void *stream, int32_t M, int32_t n_rows,
                               const int32_t *t_idx, const double *x, int32_t ld,
                               double *out, int64_t ld_out);
/* dst[r * ld_dst + c] = src[r * ld_src + c], r < rows, c < cols: a block of rows
 * moved to another leading dimension (the pieces of the all-to-all transposes of
 * KronVectorMPI.permute and of the distributed wavelet transform). */
int stk_copy_block(void *stream, int64_t rows, int32_t cols, const double *src,
                   int64_t ld_src, double *dst, int64_t ld_dst);
/* y[i * ld + t] = u_t[t] * u_x[i]: the right-hand side u0_t kron u0_x of
 * heateq_mpi.py:189-191 formed on the device.  All ld columns of every row are
 * written, those from n_loc on as +0.0 (any ld >= n_loc, odd ones included). */
int stk_outer(void *stream, int32_t M, int32_t n_loc, int32_t ld,
              const double *u_t, const double *u_x, double *y);

/* ---- communication of the time-slab decomposition for hosts without
 *      torch.distributed: the reference's mpi4py call sites on
 *      RCCL over xGMI, one process per GPU --------------------------------------
 * RCCL is loaded at run time (librccl.so.1); nothing else in the library needs it.
 * Rank 0 obtains a unique id and the HOST distributes its STK_COMM_ID_BYTES bytes
 * to the other ranks (by whatever launched them: MPI, a file, a socket); every
 * rank then calls stk_comm_create on the device it computes on.  All calls are
 * enqueued on `stream`; buffers are device pointers of float64.
 *   stk_comm_allreduce_sum  KronVectorMPI.dot's allreduce (mpi_vector.py:209), in place
 *   stk_comm_halo_exchange  communicate_bdr (mpi_vector.py:140-187): send_first goes to
 *                           rank-1 (its X_loc_bdr[-1]), send_last to rank+1 (its
 *                           X_loc_bdr[0]); recv_lo / recv_hi receive the neighbours' rows
 *                           (M doubles each); pointers of a side without a neighbour are
 *                           ignored.  Feed it from stk_halo_pack.
 *   stk_comm_exchange       a batch of sends and receives as ONE group (communicate_dofs,
 *                           mpi_vector.py:189-203; the tiles of permute, :224-239);
 *                           messages between a pair of ranks match in posting order. */
#define STK_COMM_ID_BYTES 128
typedef struct stk_comm stk_comm;
typedef struct {
    void *buf;     /* device, float64 */
    int64_t count; /* doubles */
    int32_t peer;  /* rank */
} stk_comm_msg;
int stk_comm_unique_id(void *id_host);
int stk_comm_create(int32_t rank, int32_t size, const void *id_host, stk_comm **out);
int stk_comm_destroy(stk_comm *comm);
int stk_comm_allreduce_sum(stk_comm *comm, void *stream, double *values, int32_t n);
int stk_comm_halo_exchange(stk_comm *comm, void *stream, int32_t M,
                           const double *send_first, const double *send_last,
                           double *recv_lo, double *recv_hi);
int stk_comm_exchange(stk_comm *comm, void *stream, int32_t n_send,
                      const stk_comm_msg *sends_host, int32_t n_recv,
                      const stk_comm_msg *recvs_host);

/* ---- plan construction on the device (the set-up of MultiGrid.__init__,
 *      multigrid.py:130-166, that the reference does with SciPy on the host) --------
 * stk_ell_from_csr: the sliced-ELL copy (stk_ell_rows) of a CSR matrix resident on
 * the device.  ELL row `pos` is CSR row order[pos] (order NULL: pos); K slots per
 * row, unused ones = (pad_col, 0); pad_col < 0: the row's first kept column, or
 * the row itself if it keeps none.  strip_diag: the diagonal entry goes to dia_a /
 * dia_m only (Gauss-Seidel copies, diag_free); otherwise it stays among the slots
 * and dia_a / dia_m (either may be NULL) still receive it.  grp (or NULL): keep
 * only the entries whose column lies in an EARLIER dependency group than the row,
 * grp[col] < grp[row] (the zero-start copies of the first sweep of a level visit).
 * *overflow (device int32, zeroed by the caller) receives the longest kept row if
 * one has more than K entries; such a row holds its first K kept entries, every
 * other row is complete.  A row without a diagonal entry gives dia_a = dia_m = 0.
 * n_pos = 0 returns 0 and touches nothing.
 * stk_csr_galerkin: C = R A P for CSR matrices on the device, one row of C per
 * thread, every sum accumulated in the order SciPy's (R @ A) @ P accumulates it and
 * with separately rounded products and sums -- C is bit for bit the reference's
 * Galerkin matrix.  Row i: row_counts[i] entries at out_indices / out_data
 * [i*cap ...], columns ascending, the slots from row_counts[i] on untouched;
 * 1 <= cap <= 64.  An entry whose sum is exactly zero is not emitted (csr_matmat's
 * rule), but a row is held by the columns its products TOUCH -- those whose sum
 * cancels, and those reached only through an entry of R A that cancelled,
 * included: *overflow (device int32, zeroed by the caller) receives the largest
 * such count over the rows where it exceeds cap, and 65 where a row of R A or of
 * R A P touches more than 64 columns; a row that overflows leaves its count and
 * its slots unwritten (the caller forms the product on the host then).  P = NULL
 * (all three arrays): C = R A alone, the product the restricted residual uses.
 * stk_gs_depth_step: one relaxation of the depth of every row in the dependency
 * DAG of a Gauss-Seidel sweep in dof order (forward: row i waits for its
 * neighbours j < i; backward: j > i), depth_out[i] = max depth_in[j] + 1;
 * *changed (device int32) is set when any depth moved.  The host repeats it from
 * depth = 0 until nothing changes; rows of equal depth are the groups mg.hip
 * launches together (source/multigrid.py gauss_seidel_schedule). */
int stk_ell_from_csr(void *stream, int32_t n_pos, int32_t K, const int32_t *order,
                     const int32_t *indptr, const int32_t *indices,
                     const double *vals_a, const double *vals_m, int32_t strip_diag,
                     const int32_t *grp, int32_t pad_col, int32_t *idx_out,
                     double *va_out, double *vm_out, double *dia_a, double *dia_m,
                     int32_t *overflow);
int stk_gs_depth_step(void *stream, int32_t n, const int32_t *indptr,
                      const int32_t *indices, int32_t backward,
                      const int32_t *depth_in, int32_t *depth_out, int32_t *changed);
int stk_csr_galerkin(void *stream, int32_t nc, const int32_t *r_indptr,
                     const int32_t *r_indices, const double *r_data,
                     const int32_t *a_indptr, const int32_t *a_indices,
                     const double *a_data, const int32_t *p_indptr,
                     const int32_t *p_indices, const double *p_data, int32_t cap,
                     int32_t *row_counts, int32_t *out_indices, double *out_data,
                     int32_t *overflow);

/* ---- BLAS-1 on flat arrays (KronVectorMPI arithmetic, mpi_vector.py:84-122,
 *      and dot, mpi_vector.py:205-210, local part) -------------------------- */
/* y = a * x + b * y   (b == 0 ignores the old y; x == y allowed) */
int stk_axpby(void *stream, int64_t n, double a, const double *x, double b,
              double *y);
/* z = a * x + b * y   (three-operand form, z may alias x or y) */
int stk_axpbyz(void *stream, int64_t n, double a, const double *x, double b,
               const double *y, double *z);
/* out[0] = sum x[k] * y[k] (n = 0: +0.0, x and y may be NULL).  Deterministic
 * two-stage reduction; `work` holds at least stk_dot_work_size() doubles, of
 * which the first min(ceil((n / 2 + 1) / 256), 2048) are written; x and y are
 * 16-byte aligned. */
int64_t stk_dot_work_size(void);
int stk_dot(void *stream, int64_t n, const double *x, const double *y,
            double *work, double *out);
/* KronVectorMPI.dot (mpi_vector.py:205-210) with a value that does NOT depend on
 * the number of ranks.  The reference (and stk_dot + a scalar all-reduce) adds the
 * products slab by slab, so the last digits of every r.Pr of a solve move with
 * the partition of the time axis (the reference against itself on 8 ranks:
 * 4.6e-11 in the history).  stk_slab_dot sums the products of every TIME STEP over
 * the spatial index in one fixed shape that depends on M alone (csrc/blas1.hip:
 * blocks of 256 rows, 8 interleaved fused-multiply-add chains per block, pairwise
 * tree, fixed tree over the blocks) and writes them to out_steps[t_begin + t], t <
 * n_loc; the other entries of out_steps[0 .. N) are written as zero.  The caller
 * all-reduces the N values (adding zeros is exact in any order) and adds them in
 * increasing t (stk_sum_steps, host): bit for bit the same number on 1, 2, 4 or 8
 * ranks.  x, y: slabs (M rows of ld doubles, time fastest, padding ignored);
 * work: stk_slab_dot_work_size(M, n_loc) device doubles, 16-byte aligned. */
int64_t stk_slab_dot_work_size(int32_t M, int32_t n_loc);
int stk_slab_dot(void *stream, int32_t M, int32_t n_loc, int32_t ld,
                 const double *x, const double *y, double *work, int32_t N,
                 int32_t t_begin, double *out_steps);
double stk_sum_steps(const double *steps_host, int32_t N);
/* ---- time-slab partition (DofDistributionMPI, mpi_vector.py:5-38) ---------
 * Rank p owns the time rows [displs[p], displs[p] + counts[p]): N / size rows
 * each, the N % size extra rows go to the last ranks.  Any output pointer may
 * be NULL; counts / displs hold `size` entries. */
int stk_partition(int32_t N, int32_t size, int32_t rank, int32_t *t_begin,
                  int32_t *t_end, int32_t *counts, int32_t *displs);

/* ---- preconditioned CG (PCG, linalg.py:6-42) ------------------------------
 * Solves T w = b on this rank's slab (n = M*ld doubles, padding zero) with the
 * reference's recurrence and stopping rule: stop when r.Pr < eps^2, at most
 * kmax-1 iterations, return immediately if b = 0 or the initial r.Pr is small.
 * The operators are callbacks (they launch on `stream`; T may communicate);
 * `allreduce` sums host doubles over the ranks (NULL on one rank).  `w` holds
 * the initial guess on entry.  `work`: stk_pcg_work_size(n) device doubles.
 * history (host, kmax entries or NULL) receives r.Pr after the initial
 * residual and after every iteration; *iters the iteration count.  kmax < 1 is
 * refused (there would be no room for the initial r.Pr). */
typedef int (*stk_operator_fn)(void *ctx, void *stream, const double *x,
                               double *y);
typedef int (*stk_allreduce_fn)(void *ctx, double *values, int32_t n);
int64_t stk_pcg_work_size(int64_t n);
int stk_pcg_solve(void *stream, int64_t n, stk_operator_fn T, void *T_ctx,
                  stk_operator_fn P, void *P_ctx, stk_allreduce_fn allreduce,
                  void *allreduce_ctx, const double *b, double *w, double eps,
                  int32_t kmax, double *work, double *history, int32_t *iters);
/* The same loop on slabs (M rows of ld doubles, this rank's time steps [t_begin,
 * t_begin + n_loc) of N) with stk_slab_dot for the inner products: `allreduce` is
 * then called with the N per-step sums, and history / iterate are bit for bit
 * those of a one-rank run, whatever the number of ranks (given operators that
 * have that property, as the Kronecker and multigrid applies of this library do).
 * work: stk_pcg_slab_work_size(M, n_loc, ld, N) device doubles. */
int64_t stk_pcg_slab_work_size(int32_t M, int32_t n_loc, int32_t ld, int32_t N);
int stk_pcg_solve_slab(void *stream, int32_t M, int32_t n_loc, int32_t ld,
                       int32_t N, int32_t t_begin, stk_operator_fn T, void *T_ctx,
                       stk_operator_fn P, void *P_ctx, stk_allreduce_fn allreduce,
                       void *allreduce_ctx, const double *b, double *w, double eps,
                       int32_t kmax, double *work, double *history,
                       int32_t *iters);

/* ---- per-operation device-time counters (LinearOperatorMPI.num_applies /
 *      time_applies, mpi_kron.py:23-36, for hosts without the Python classes) -----
 * While enabled, every apply entry point brackets what it enqueues with two
 * HIP events on its stream.  stk_timing_get waits for the recorded events and
 * returns the number of calls and the summed device seconds of one class:
 * "kron" (stk_kron_*_apply), "space" (stk_csr_spmm, stk_ell_spmm), "time"
 * (stk_time_*_apply), "wavelet", "multigrid" (stk_mg_apply, stk_mg_smooth),
 * "blas1" (stk_axpby(z), stk_dot).  Classes nest where entry points do (the
 * BLAS-1 calls of stk_pcg_solve are counted as blas1).  Applies enqueued on
 * DIFFERENT streams are each timed on their own stream: where they overlap (the two
 * K applies inside S run side by side), the seconds of a class add up to more than
 * the wall time they took.  Communication time is the caller's. */
int stk_timing_enable(int32_t on);
int stk_timing_reset(void);
int stk_timing_get(const char *op_class, int64_t *calls, double *seconds);

/* ---- Lanczos estimate of the extreme eigenvalues of P A (Lanczos,
 *      lanczos.py:87-159; Sturm-sequence bisection bisec / pol, :20-85) ---------
 * The reference's recurrence on device vectors of n doubles: `w` holds the start
 * vector on entry (it is overwritten); A and P are callbacks as in
 * stk_pcg_solve.  Stops when lambda_max and lambda_min both moved by less than
 * `tol` relative (reference default 1e-4; bisection tolerance 1e-6), after at
 * most max_iterations steps (*converged = 0 then), or at a breakdown (invariant
 * Krylov space).  alpha_host / beta_host (max_iterations / max_iterations - 1
 * host doubles, or NULL) receive the recurrence coefficients.  work:
 * stk_lanczos_work_size(n) device doubles. */
int64_t stk_lanczos_work_size(int64_t n);
int stk_lanczos(void *stream, int64_t n, stk_operator_fn A, void *A_ctx,
                stk_operator_fn P, void *P_ctx, stk_allreduce_fn allreduce,
                void *allreduce_ctx, double *w, int32_t max_iterations,
                double tol, double tol_bisec, double *work, double *alpha_host,
                double *beta_host, double *lmax, double *lmin,
                int32_t *iterations, int32_t *converged);
/* On slabs, inner products through stk_slab_dot (see stk_pcg_solve_slab). */
int64_t stk_lanczos_slab_work_size(int32_t M, int32_t n_loc, int32_t ld, int32_t N);
int stk_lanczos_slab(void *stream, int32_t M, int32_t n_loc, int32_t ld, int32_t N,
                     int32_t t_begin, stk_operator_fn A, void *A_ctx,
                     stk_operator_fn P, void *P_ctx, stk_allreduce_fn allreduce,
                     void *allreduce_ctx, double *w, int32_t max_iterations,
                     double tol, double tol_bisec, double *work,
                     double *alpha_host, double *beta_host, double *lmax,
                     double *lmin, int32_t *iterations, int32_t *converged);

/* ---- sum of Kronecker terms  y = beta*y + sum_k (T_k kron X_k) x_k --------
 * Replaces TridiagKronMatMPI._matvec (mpi_kron.py:214-219), i.e.
 * TridiagKronIdentityMPI (:186-201) followed by IdentityKronMatMPI (:143-150),
 * and the accumulation loop of SumMPI._matvec (:77-90), in one pass.
 * All X_k share one sparsity pattern; their values differ per term.
 *
 * Sliced-ELL form.  Every row owns K slots (K <= 16): ell_idx[pos*K + e] /
 * ell_vals[pos*K + e]; unused slots hold the row's own column and the value 0.
 * Rows are listed in processing order (a mesh-tile or RCM order keeps the
 * gathers of one XCD inside its L2; the result does not depend on it), row pos
 * writes output row row_ids[pos] (row_ids == NULL: pos itself).  Entries
 * beyond K of longer rows are kept in an overflow CSR indexed by pos (NULL if
 * none).  Requires ld even and 16-byte aligned x, y. */
typedef struct {
    int32_t M, K;
    const int32_t *ell_idx;     /* M*K */
    const int32_t *row_ids;     /* M or NULL */
    const int32_t *ovf_indptr;  /* M+1 or NULL */
    const int32_t *ovf_indices;
} stk_ell_pattern;

typedef struct {
    /* 3*n_loc coefficients [sub | diag | super]: output time row t takes
     * sub[t]*z[t-1] + diag[t]*z[t] + super[t]*z[t+1].  NULL = identity. */
    const double *tri;
    const double *ell_vals; /* M*K values of X_k */
    const double *ovf_vals; /* overflow values or NULL */
    const double *x;        /* input vector, M x ld */
    const double *x_lo;     /* ghost time row t = -1 (length M) or NULL */
    const double *x_hi;     /* ghost time row t = n_loc (length M) or NULL */
} stk_kron_ell_term;

/* Tuning key "ell_wg_per_cu" (stk_set_tuning).  K must be one of 5, 7, 9, 12,
 * 16; at most 3 terms.
 * Terms with ghost rows (x_lo / x_hi) are handled as two launches: the
 * slab-local part, then stk_kron_ell_ghost_apply (with a copy of the old
 * boundary entries of y in between when beta != 0).  Every entry of y is
 * rounded as on one rank, wherever the time axis is cut. */
int stk_kron_ell_apply(void *stream, const stk_ell_pattern *pattern_host,
                       int32_t n_loc, int32_t ld, int32_t n_terms,
                       const stk_kron_ell_term *terms_host, double beta,
                       double *y);

/* The first and last local time step of the same operator once the ghost time
 * rows are there: "first/last rows after the halo arrived" of
 * TridiagKronIdentityMPI._matvec (mpi_kron.py:186-201, :199-200).  A caller that
 * overlaps the halo exchange with compute calls stk_kron_ell_apply with x_lo =
 * x_hi = NULL and beta = 0 while the exchange is in flight and this function
 * once it has completed.  The two steps are RECOMPUTED from x, x_lo and x_hi in
 * the order of operations of the main kernel,
 *   y[:, t] = sum_k fma(sup_k[t], z_k[t+1], fma(sub_k[t], z_k[t-1], dia_k[t] z_k[t])),
 * and overwrite what the ghost-less call left there: the result is bit for bit
 * the one-rank apply of the same rows, whatever the partition of the time axis
 * (a share ADDED afterwards, as in rounds 1-5, puts the neighbour's term last in
 * the sum and differs from the one-rank result in the last bits). */
int stk_kron_ell_ghost_apply(void *stream, const stk_ell_pattern *pattern_host,
                             int32_t n_loc, int32_t ld, int32_t n_terms,
                             const stk_kron_ell_term *terms_host, double *y);

/* The same operator with the matrix stream PACKED and the ghost time steps
 * fused into the one pass (the fast path of the metric's operator,
 * SumMPI([TridiagKronMatMPI, TridiagKronMatMPI])._matvec, mpi_kron.py:77-90,
 * with the halo of TridiagKronIdentityMPI._matvec, :186-201).
 * slots[pos*K + e] = code << col_bits | column; `code` indexes the dictionary of
 * distinct value tuples of the union pattern: matrix m has the value
 * dict[m*n_codes + code] in that slot.  Unused slots hold the row's own column
 * and a code whose values are all zero.  Exact: the dictionary holds the
 * doubles themselves.  Every term reads the same x; term k multiplies with
 * matrix t[k].mat.  `ghosts` (NULL on a slab without neighbours) holds the
 * ghost time steps interleaved: ghosts[2*j] = x[j, t = -1] (X_loc_bdr[0],
 * mpi_vector.py:148-175), ghosts[2*j + 1] = x[j, t = n_loc] (X_loc_bdr[-1]);
 * a side without a neighbour is zero-filled.  K one of 5, 7, 9, 12, 16; at most
 * 3 terms; n_loc <= 1020 (one lane per pair of time steps and the ghost lane in a
 * workgroup of 512), and less where n_terms * rows_per_unit * (n_loc + 3) sums, the
 * dictionary and the time factors exceed 64 KiB of LDS for a single slot row (the
 * call is refused: with a dictionary of 16 codes from 1017 steps on for two terms,
 * 676 for three, and with row pairs 810 and 537); slabs of any size (64-bit
 * addressing).  The stores of y and the loads of the slot stream are non-temporal. */
typedef struct {
    int32_t M, K;
    int32_t col_bits; /* 2^col_bits >= M */
    int32_t n_codes;  /* <= 2^(32 - col_bits) */
    int32_t n_mats;
    int32_t rows_per_unit;  /* 1, or 2 = row pairs (below) */
    int32_t n_units;        /* slot rows: M when rows_per_unit = 1 */
    const uint32_t *slots;  /* n_units*K */
    const int32_t *row_ids; /* n_units*rows_per_unit; NULL (index order) only when rows_per_unit = 1 */
    const double *dict;     /* n_mats*n_codes*rows_per_unit */
    const double *vals;     /* NULL, or explicit values (no dictionary; rows_per_unit = 2 only):
                               n_units*K*rows_per_unit*n_mats, the slot words are then bare columns */
} stk_pack_pattern;
/* Explicit values: matrices whose entries do not repeat (an unstructured mesh;
 * the reference takes any CSR, mpi_kron.py:135-150) have no dictionary, but their
 * rows still share COLUMNS.  vals[((u*K + s)*2 + j)*n_mats + m] is the entry of
 * matrix m in row j of slot row u at the column of slot s (zero where that row
 * has none): 36 bytes per slot for two matrices instead of 20 in the one-row
 * plain form (stk_kron_ell_apply), 10 gathers for two rows instead of 14, every
 * row's space-factor sum accumulated in the same order.  A call on such a pattern
 * must use ALL its matrices, term k naming matrix k (n_terms = n_mats): the
 * caller keeps one value array per combination of matrices it applies. */
/* Row pairs (rows_per_unit = 2): slot row u serves the matrix rows
 * row_ids[2u] and row_ids[2u + 1] (-1: none); its K slots (K one of 8, 10, 12)
 * list the UNION of their columns in ascending order, and matrix m has the
 * values dict[(m*n_codes + code)*2 + j] for row j of the pair (zero where that
 * row has no entry in the column).  Two neighbouring vertices of a P1
 * triangulation share 4 of their 7 columns, so a pair costs 10 gathers
 * instead of 14; every row's sum is still accumulated in ascending column
 * order, so the results are bit-identical with rows_per_unit = 1. */

typedef struct {
    const double *tri; /* as in stk_kron_ell_term */
    int32_t mat;       /* which matrix of the pattern */
} stk_kron_pack_term;

/* Host helper of the planners (no device work): groups rows that follow each
 * other in the processing order into units of up to rp rows whose union of
 * columns has at most K_out entries (greedily, left to right).  cols / codes:
 * [M][K], the real entries of position p in the first counts[p] slots, columns
 * ascending; own[p]: matrix row at position p.  Outputs sized for M units:
 * ucols [units][K_out], ucodes [units][K_out][rp] (zero_code = "no entry"),
 * urows [units][rp] (-1 = none).  stk_pack_unit_slots: K_out of the instantiated
 * kernels for rows of K slots (0: none). */
int32_t stk_pack_unit_slots(int32_t K, int32_t rp);
/* Host helper: a processing order in which rows that can share a slot row follow
 * each other, for patterns whose given order lacks that (unstructured meshes).
 * Behind every not yet placed row of the given order goes ONE not yet placed
 * neighbour (a column of the row) whose union of columns with it fits K_out
 * slots -- the nearest in the given order, at most `window` positions away.
 * counts / cols / own as in stk_pack_group_rows; perm[q] = position in the given
 * order of the row at position q of the new order. */
int stk_pack_match_order(int32_t M, int32_t K, const int32_t *counts,
                         const int32_t *cols, const int32_t *own, int32_t K_out,
                         int32_t window, int32_t *perm);
int stk_pack_group_rows(int32_t M, int32_t K, const int32_t *counts,
                        const int32_t *cols, const int32_t *codes,
                        const int32_t *own, int32_t zero_code, int32_t rp,
                        int32_t K_out, int32_t *n_units, int32_t *ucols,
                        int32_t *ucodes, int32_t *urows);

int stk_kron_pack_apply(void *stream, const stk_pack_pattern *pattern_host,
                        int32_t n_loc, int32_t ld, int32_t n_terms,
                        const stk_kron_pack_term *terms_host, const double *x,
                        const double *ghosts, double beta, double *y);

/* The first and last local time step after stk_kron_pack_apply ran with ghosts =
 * NULL and beta = 0 while the halo exchange was in flight (the reference overlaps
 * the exchange with the rows that do not need it, mpi_kron.py:193-200,
 * mpi_vector.py:177-179).  Both steps are recomputed from x and the received rows
 * in the one-pass kernel's order of operations and OVERWRITE y[i][0] and
 * y[i][n_loc-1]: pass + this call, the one-pass form with `ghosts`, and the
 * one-rank apply agree bit for bit (tests: torch.equal).  x: the slab the pass
 * read; x_lo / x_hi: the received rows as they arrive (contiguous, length M; NULL
 * on a side without a neighbour).  One lane per slot row and side on the packed
 * stream. */
int stk_kron_pack_ghost_apply(void *stream, const stk_pack_pattern *pattern_host,
                              int32_t n_loc, int32_t ld, int32_t n_terms,
                              const stk_kron_pack_term *terms_host, const double *x,
                              const double *x_lo, const double *x_hi, double *y);

/* The same two steps from COMPACT operands, one lane per slot row for both sides:
 * records[4*j .. 4*j+3] = (x[j][0], x[j][1], x[j][n_loc-2], x[j][n_loc-1]) as stk_halo_pack_records
 * leaves them (32-byte aligned), ghosts[2*j], ghosts[2*j+1] = (x_lo[j], x_hi[j]) as
 * stk_interleave_ghosts does (a side without a neighbour: zeros, and has_lo / has_hi = 0:
 * its step is not rewritten).  Three 16-byte loads per slot from two lines where
 * stk_kron_pack_ghost_apply gathers six times 8 bytes from the slab: 1.5-2 x faster, the
 * same doubles (tests: torch.equal).  Pass with ghosts = NULL and beta = 0 first, as above. */
int stk_kron_pack_boundary_apply(void *stream, const stk_pack_pattern *pattern_host,
                                 int32_t n_loc, int32_t ld, int32_t n_terms,
                                 const stk_kron_pack_term *terms_host,
                                 const double *records, const double *ghosts,
                                 int32_t has_lo, int32_t has_hi, double *y);

/* The same packed stream with an input slab PER TERM: y = beta*y + sum_k (T_k kron
 * X_k) xs[k] -- the last stage of the Schur complement S = B^T K B + G of
 * heateq_mpi.py:166-181 once K is applied to two right-hand sides instead of four
 * times: (I kron M_x) v1 + (I kron A_x) v2 + (G_t kron M_x) x, i.e. three
 * TridiagKronMatMPI / IdentityKronMatMPI applies and the sum of SumMPI._matvec
 * (mpi_kron.py:77-90, 135-150, 214-219) in one pass.  Every slot row gets a LANE
 * GROUP PER TERM (csrc/kron_pack_multi.hip): a lane gathers K columns of ITS
 * term's slab for one pair of time steps, the sums of all lanes meet in LDS, and
 * the first lane group applies the time factors and adds the terms in term order.
 * A lane whose term's time factor never multiplies its pair of time steps does
 * not gather (G_t has the single entry (0, 0)).  No ghost time steps: a term whose
 * factor couples to the neighbour ranks' rows takes stk_kron_pack_apply.  The
 * pattern must have a dictionary; xs_host: n_terms device pointers (host array),
 * 2 or 3 terms.  Every row's sums are those of stk_kron_pack_apply, term by term,
 * bit for bit.  (Slot rows that would need more than 256 lanes -- fewer than two
 * of them per workgroup of 512 -- and tuning key "pack_multi_lanes" = 0: the terms
 * take turns in one lane, round 4's form.) */
int stk_kron_pack_apply_multi(void *stream, const stk_pack_pattern *pattern_host,
                              int32_t n_loc, int32_t ld, int32_t n_terms,
                              const stk_kron_pack_term *terms_host,
                              const double *const *xs_host, double beta, double *y);
/* ... with the caller's knowledge of the time factors (host arrays of n_terms
 * entries, or both NULL): term k's factor has no non-zero entry in a COLUMN
 * outside the local time steps [t_begin_host[k], t_end_host[k]) -- it reads
 * xs[k] at those steps only -- so term k gets lanes for those pairs of steps only
 * and a workgroup holds more slot rows of the others (G_t: [0, 1); an identity or
 * a full tridiagonal factor: [0, n_loc)).  Term 0's lanes also write y and always
 * cover every step.  A range that leaves out a column the factor does reach gives
 * a wrong result: the library cannot see the factors' entries from the host. */
int stk_kron_pack_apply_multi_steps(void *stream, const stk_pack_pattern *pattern_host,
                                    int32_t n_loc, int32_t ld, int32_t n_terms,
                                    const stk_kron_pack_term *terms_host,
                                    const double *const *xs_host,
                                    const int32_t *t_begin_host,
                                    const int32_t *t_end_host, double beta, double *y);

/* ---- plan construction from CSR (no Python needed) ---------------------------
 * Everything the three forms above stream is derived here, on the host side of
 * the library, from the CSR matrices a caller of the reference holds
 * (mpi_shared_mem.py:46-48; TridiagKronMatMPI keeps references to them,
 * mpi_kron.py:209-210): union pattern of the n_mats matrices, K = the smallest
 * instantiated slot count that holds the longest row (overflow CSR beyond 16),
 * rows listed in `row_order_host` (a permutation of 0..M-1, e.g. a mesh-tile or
 * RCM order; NULL = index order), the dictionary of distinct value tuples and
 * the packed slot words when the tuples fit.  All arrays are HOST pointers;
 * the plan owns its device copies.  stk_kron_plan_apply runs
 *   y = beta*y + sum_k (T_k kron X_{t[k].mat}) x
 * on the fastest form the plan has; x_lo / x_hi are the ghost time rows
 * (device, length M, or NULL) and ghost_work 2*M device doubles of scratch,
 * needed when either is given. */
typedef struct stk_kron_plan stk_kron_plan;
int stk_kron_plan_create(int32_t M, int32_t n_mats,
                         const int32_t *const *indptr_host,
                         const int32_t *const *indices_host,
                         const double *const *data_host,
                         const int32_t *row_order_host, stk_kron_plan **out);
int stk_kron_plan_destroy(stk_kron_plan *plan);
/* Any output may be NULL.  K: slots per row of the sliced-ELL copy; packed = 1
 * if the dictionary form was built; rows_per_unit = 2 if a row-pair form was
 * built as well -- stk_kron_plan_apply uses it for slabs of 8 time steps and
 * more, the one-row form below (tuning key "pack_rows" = 1: no pairs in plans
 * created afterwards).  packed = 0 with rows_per_unit = 2: matrices without a
 * dictionary whose rows still share columns -- pairs with explicit values
 * (stk_pack_pattern.vals), the plain sliced-ELL form below 24 time steps. */
int stk_kron_plan_info(const stk_kron_plan *plan, int32_t *K, int32_t *n_codes,
                       int32_t *packed, int64_t *nnz_union,
                       int32_t *rows_per_unit);
int stk_kron_plan_apply(stk_kron_plan *plan, void *stream, int32_t n_loc,
                        int32_t ld, int32_t n_terms,
                        const stk_kron_pack_term *terms_host, const double *x,
                        const double *x_lo, const double *x_hi,
                        double *ghost_work, double beta, double *y);

/* After stk_kron_plan_apply ran with x_lo = x_hi = NULL and beta = 0 while the halo
 * exchange was in flight (mpi_kron.py:193-200): the first / last local time step
 * recomputed with the two received rows, as stk_kron_pack_ghost_apply /
 * stk_kron_ell_ghost_apply do.  x: the slab the apply read. */
int stk_kron_plan_ghost_apply(stk_kron_plan *plan, void *stream, int32_t n_loc,
                              int32_t ld, int32_t n_terms,
                              const stk_kron_pack_term *terms_host, const double *x,
                              const double *x_lo, const double *x_hi, double *y);

/* The same two steps from the compact records stk_halo_pack_records left (4*M doubles) and
 * the received rows (interleaved into ghost_work, 2*M doubles): stk_kron_pack_boundary_apply
 * on the plan's packed form, 2-3 x faster than the slab form above and the same doubles.
 * records = NULL, or a plan without a packed stream: the slab form (needs x). */
int stk_kron_plan_boundary_apply(stk_kron_plan *plan, void *stream, int32_t n_loc,
                                 int32_t ld, int32_t n_terms,
                                 const stk_kron_pack_term *terms_host, const double *x,
                                 const double *records, const double *x_lo,
                                 const double *x_hi, double *ghost_work, double *y);

/* ghosts[2*j] = lo[j], ghosts[2*j + 1] = hi[j] (a NULL side is written as
 * zero): brings the two received time rows into the layout above. */
int stk_interleave_ghosts(void *stream, int32_t M, const double *lo,
                          const double *hi, double *ghosts);

/* ---- (I_t kron A) for a general, possibly rectangular CSR A ---------------
 * y = alpha * A x + beta * z  on `rows` x n_loc outputs (IdentityKronMatMPI,
 * mpi_kron.py:143-150; residual / restriction / prolongation steps of
 * MultiGrid.MGM, multigrid.py:174-180).  The entries of A may depend on the
 * time slice: a(t) = ca * vals_a + cm[t] * vals_m (vals_m, cm may be NULL).
 * z may be NULL (treated as 0) or alias y. */
int stk_csr_spmm(void *stream, int32_t rows, int32_t n_loc, int32_t ld,
                 const int32_t *indptr, const int32_t *indices,
                 const double *vals_a, double ca, const double *vals_m,
                 const double *cm, const double *x, double alpha, double beta,
                 const double *z, double *y);

/* The same on a sliced-ELL copy (fast path; slot count K one of 2, 4, 5, 6, 7,
 * 9, 12, 16, 20; padding slots: any valid column, value 0).  ELL row `pos`
 * produces output row row_ids[pos]; dia_a / dia_m hold the diagonal entry of
 * that row (Gauss-Seidel only).  diag_free (Gauss-Seidel copies): the slots hold
 * the OFF-diagonal entries only and a row is updated as
 *     u_i = (f_i - sum_{j != i} a_ij u_j) / a_ii
 * -- the form of PETSc's MatSOR, which the reference calls (multigrid.py:116-127);
 * one gather less per row than u_i += (f_i - sum_j a_ij u_j) / a_ii with the
 * diagonal among the slots (diag_free = 0), equal up to rounding. */
typedef struct {
    int32_t n_pos;  /* ELL rows */
    int32_t n_rows; /* rows of the output slab */
    int32_t K;
    const int32_t *idx;     /* n_pos*K columns */
    const double *va, *vm;  /* n_pos*K values; vm may be NULL */
    const int32_t *row_ids; /* n_pos or NULL */
    const double *dia_a, *dia_m; /* n_pos each or NULL */
    int32_t diag_free;
} stk_ell_rows;

/* y = alpha * A(t) x + beta * z; x has x_rows rows, y and z have ell->n_rows.
 * ld must be even, n_loc at most 1024, the slabs 16-byte aligned.  A call writes the columns
 * 0 .. 2*ceil(n_loc/2) - 1 of the listed rows of y and nothing else: the padding column of an
 * odd n_loc is written as +0.0 whatever x and z hold there (their padding is read with its
 * pair and discarded), and the columns from there to ld -- the slab as a column range of a
 * wider one -- are neither read nor written.  A refused call writes nothing. */
int stk_ell_spmm(void *stream, const stk_ell_rows *ell_host, int32_t n_loc,
                 int32_t ld, int32_t x_rows, double ca, const double *cm,
                 const double *x, double alpha, double beta, const double *z,
                 double *y);

/* ---- direct inverse of a space matrix (InvLinOp, linop.py:18-26; precond =
 *      'direct', heateq_mpi.py:155-157) ----------------------------------------
 * x = A^-1 b for all time steps of a slab from the factors Pr A Pc = L U of
 * scipy.sparse.linalg.splu (SuperLU), which stays on the host at set-up as in the
 * reference (`self.inv = splu(mat)`); what `self.inv.solve` does per apply -- row
 * permutation, two triangular solves, column permutation -- runs on the device,
 * level-scheduled: wide levels of the elimination tree one launch each, runs of
 * narrow levels inside one workgroup (csrc/sptrsv.hip).  L and U: CSR on the host
 * (sorted columns; L unit lower triangular, its diagonal stored or not, U upper with its
 * diagonal), perm_r / perm_c: SuperLU.perm_r / perm_c (NULL = identity).  The sums
 * of a row have one shape whatever the slab length: the result does not depend on the
 * partition of the time axis.  work: M * ld device doubles; b may be x. */
typedef struct stk_lu stk_lu;
int stk_lu_create(int32_t n, const int32_t *L_indptr, const int32_t *L_indices,
                  const double *L_data, const int32_t *U_indptr,
                  const int32_t *U_indices, const double *U_data,
                  const int32_t *perm_r, const int32_t *perm_c, stk_lu **out);
int stk_lu_destroy(stk_lu *lu);
/* Any output may be NULL: dependency levels of the two solves, kernel launches
 * per stk_lu_solve. */
int stk_lu_info(const stk_lu *lu, int32_t *levels_L, int32_t *levels_U,
                int32_t *launches);
int stk_lu_solve(stk_lu *lu, void *stream, int32_t n_loc, int32_t ld,
                 const double *b, double *x, double *work);
/* The top of the elimination tree as a dense block (optional).  The narrow levels are
 * the separators near the root: a few thousand rows, one dependent row after the other
 * (770 of the 802 levels of A_x at J_space = 6 hold 2 578 of its 16 129 rows).  The plan
 * names them -- S = the rows from the first narrow level of L on, ascending
 * (stk_lu_top_rows; n_top = 0: no such block, or U's rows of S reach outside S) -- and a
 * caller that hands over the two blocks L[S, S] and U[S, S] as dense matrices (n_top x
 * n_top, row-major, DEVICE; the plan copies them) whose DIAGONAL BLOCKS of `block` rows
 * are replaced by their inverses turns every solve into
 *   head levels, d_S = (Pr b)_S - L[S, H] y_H, per block k ascending: y_k = inv(L_kk) (d_k - L[k, <k] y_<k);
 *   per block k descending: z_k = inv(U_kk) (y_k - U[k, >k] z_>k), head levels
 * with one launch per block.  block = n_top: the explicit inverses of the whole blocks
 * (two launches per solve, five to ten times the rounding error of substitution); 256
 * keeps the accuracy of substitution.  The inverted blocks are read WITH their diagonal:
 * inv(L_kk) carries its ones whether or not L stores its unit diagonal.  Without the call
 * the plan walks every level (a run of narrow levels in one workgroup). */
int stk_lu_top_rows(const stk_lu *lu, int32_t *n_top, int32_t *rows_host);
int stk_lu_set_top_inverse(stk_lu *lu, const double *L_blocks_dev,
                           const double *U_blocks_dev, int32_t block);

/* ---- (A_t kron I) for a small sparse time matrix ---------------------------
 * y[., t] = (add_identity ? x[., t] : 0) + sum_e val[e] * src(col[e]) over the
 * CSR row t of the LOCAL rows of the time matrix; col < n_loc addresses the
 * local slab, col >= n_loc addresses row (col - n_loc) of `recv`, a
 * (n_recv x M) array of time rows fetched from other ranks
 * (SparseKronIdentityMPI._matvec, mpi_kron.py:285-317;
 * TridiagKronIdentityMPI._matvec, :186-201). */
int stk_time_csr_apply(void *stream, int32_t M, int32_t n_loc, int32_t ld,
                       const int32_t *t_indptr, const int32_t *t_cols,
                       const double *t_vals, const double *x,
                       const double *recv, int32_t add_identity, double *y);

/* ---- (T kron I) for a dense, possibly rectangular time factor --------------
 * y[i, r] = sum_c T[r*n_in + c] * x[i*ld_in + c] for r < n_out; columns
 * n_out..ld_out-1 of y are set to zero.  The time side of the serial KronLinOp
 * (linop.py:6-15: mat_time.dot(X)) when the factor is not square -- the trial
 * and test spaces in time of heateq.py:37-51 differ -- or is given as a
 * LinearOperator; x and y are slabs with their own row strides. */
int stk_time_dense_apply(void *stream, int32_t M, int32_t n_in, int32_t ld_in,
                         int32_t n_out, int32_t ld_out, const double *T,
                         const double *x, double *y);

/* ---- test-space slabs: the time side of B, B^T and K on Y ---------------------
 * The test space of the serial driver is discontinuous P1 in time (heateq.py:37-51):
 * two dofs per time element, 2e + a.  Its time factors are rectangular, 2(N-1) x N,
 * and every one of them -- B1_t, B2_t (heateq.py:45-48), their transposes (:52-54),
 * the mass inverse of Y (:57-63) -- is one 2 x 2 block per element.  A rank that owns
 * the nodes [t_begin, t_end) holds the elements [max(t_begin-1, 0), min(t_end, N-1));
 * its test-space slab is y[i*ld_y + 2*e_loc + a] with ld_y = 2*n_el (no padding: an
 * element is one aligned 16-byte pair).  With t_begin > 0 the first element is a copy
 * of the lower neighbour's last one, computed by both ranks with the same
 * instructions; inner products skip it.  `first_node` is the local node index of the
 * first held element's first node: -1 (the ghost row below the slab; t_begin > 0) or 0.
 * blocks: 4*n_el device doubles per term, blk[4*e_loc + 2*a + b], 16-byte aligned.
 *
 * These entry points are the TIME side; the space factors are applied by the caller
 * with the row engine (one stk_ell_spmm pass per matrix).  They replace the time
 * factor of KronLinOp (linop.py:6-15) for B = B1_t kron M_x + B2_t kron A_x
 * (heateq.py:45-54), for B^T (:52-54, :93-102: f = B^T K g + u0) and for the time
 * factor of K = Minv_Y kron Kinv_x (:57-63) in the Y' estimator (:154-155).
 *
 * forward:   z_host[k] = X_k x on the node slab (M x ld_z, n_loc local nodes),
 *            zg_host[k] = X_k applied to the interleaved ghost pair (M x 2; needed when
 *            an element reaches the node -1 or the node n_loc; else NULL).  With z0, z1 the
 *            two nodes of element e,
 *              acc_a = 0; for k ascending: acc_a = fma(blk_k[e][a][1], z1_k, fma(blk_k[e][a][0], z0_k, acc_a));
 *              y_{e,a} = beta == 0 ? acc_a : fma(beta, y_{e,a}, acc_a)     (non-temporal stores)
 * transpose: w_host[k] = X_k^T y on the test-space slab (M x 2*n_el).  Node n adds the
 *            element n-1 (where it is the second node), then the element n (the first):
 *              acc = 0; for k ascending, for e in (n-1, n) that exist, a = 0, 1:
 *                acc = fma(blk_k[e][a][n-e], w_k[e,a], acc);
 *              x_n = beta == 0 ? acc : fma(beta, x_n, acc); the padding column of x is zero.
 *            Both elements of every local node are held (the overlap): no exchange.
 * block mix: y_{e,a} = fma(blk[e][a][1], x_{e,1}, blk[e][a][0] * x_{e,0}) on a test-space
 *            slab; y may be x.
 * The order of the sums depends on the element alone: results do not depend on the
 * number of ranks.  At most STK_ELEM_MAX_TERMS terms. */
#define STK_ELEM_MAX_TERMS 3
int stk_elem_time_apply(void *stream, int32_t M, int32_t n_el, int32_t n_loc,
                        int32_t ld_z, int32_t first_node, int32_t n_terms,
                        const double *const *z_host, const double *const *zg_host,
                        const double *const *blocks_host, double beta, double *y);
int stk_elem_time_apply_t(void *stream, int32_t M, int32_t n_el, int32_t n_loc,
                          int32_t ld_x, int32_t first_node, int32_t n_terms,
                          const double *const *w_host,
                          const double *const *blocks_host, double beta, double *x);
int stk_elem_block_mix(void *stream, int32_t M, int32_t n_el, const double *blocks,
                       const double *x, double *y);

/* The same two maps FUSED with their space factors, in one pass over a packed slot
 * stream (stk_pack_pattern with a dictionary, rows_per_unit 1 or 2; csrc/kron_pack_elem.hip):
 *   forward:    y_{e,a} = sum_k sum_b blk_k[e][a][b] (X_{t[k].mat} x)_{node(e)+b}
 *   transpose:  x_n = sum_k (element n-1, then n) sum_a blk_k[e][a][n-e] (X_{t[k].mat} y)_{e,a}
 * (the space factors themselves are not transposed: symmetric matrices, as M_x and A_x).
 * The walk and the gathers are those of stk_kron_pack_apply -- persistent workgroups on
 * XCD-interleaved row groups, one lane per 16-byte pair, forward with the ghost lane on
 * the interleaved `ghosts` (needed when an element reaches the node -1 or n_loc, else
 * NULL) -- the space sums stay in LDS, and the time stage writes one 16-byte pair per
 * element (forward) or per two nodes (transpose) with non-temporal stores.  Every row's
 * space sums accumulate in ascending column order from zero; the time stage adds its
 * products in the order written down above for the composed forms, which give the same
 * doubles.  t[k].tri is ignored.  Exactly 2 terms (B = B1 + B2, heateq.py:52-53); x (y_in)
 * must not alias y (x_out); slabs 16-byte aligned, ld even.
 * Slab length: a workgroup keeps all 8*n_el block doubles, the dictionary and, per slot
 * row it serves, 2 * rows_per_unit sums per node (forward) or per test-space column
 * (transpose) in LDS, and a slot row needs at most 512 lanes.  The host function
 * stk_kron_pack_elem_lds_bytes returns the bytes for ONE slot row at a time (host; reads
 * K, n_codes and rows_per_unit of the pattern only), -1 where the lanes do not suffice;
 * the fused calls serve a slab iff that is within 65536 -- with row pairs about 680
 * nodes forward and 500 elements transposed -- and fail otherwise: the caller takes the
 * composed forms above (ElementKronMatMPI asks first). */
int64_t stk_kron_pack_elem_lds_bytes(const stk_pack_pattern *pattern_host, int32_t n_el,
                                     int32_t n_loc, int32_t transposed);
int stk_kron_pack_elem_apply(void *stream, const stk_pack_pattern *pattern_host,
                             int32_t n_el, int32_t n_loc, int32_t ld,
                             int32_t first_node, int32_t n_terms,
                             const stk_kron_pack_term *terms_host,
                             const double *const *blocks_host, const double *x,
                             const double *ghosts, double beta, double *y);
int stk_kron_pack_elem_apply_t(void *stream, const stk_pack_pattern *pattern_host,
                               int32_t n_el, int32_t n_loc, int32_t ld,
                               int32_t first_node, int32_t n_terms,
                               const stk_kron_pack_term *terms_host,
                               const double *const *blocks_host, const double *y_in,
                               double beta, double *x_out);

/* ---- wavelet transform in time, whole time axis on this GPU ---------------
 * y = (W_t kron I) x or (W_t^T kron I) x in the interleaved numbering, all
 * J levels in one pass (WaveletTransformOp._matmat / _rmatmat,
 * wavelets.py:106-134; same operator as the composite of
 * wavelets.py:172-198 on one rank).  Requires n_loc == 2^J + 1, 0 <= J <= 11,
 * ld >= n_loc; x == y is allowed.  Padding (columns n_loc .. ld - 1): padding of y
 * is zero provided padding of x is zero; the data columns never read it.  (With
 * 1 <= J <= 7, ld == n_loc + 1 and both pointers 16-byte aligned, whole rows move
 * as they are and y's padding column is x's; in every other case y's padding is
 * written as zero whatever x holds there.) */
int stk_wavelet_apply(void *stream, int32_t M, int32_t J, int32_t ld,
                      int32_t transposed, const double *x, double *y);

/* ---- multigrid V-cycles with Gauss-Seidel smoothing ------------------------
 * MultiGrid._matvec / MGM (multigrid.py:168-193), PETScSMoother / Smoother
 * (multigrid.py:83-127), batched over the n_loc time slices. */
typedef struct {
    int32_t n; /* dofs on this level */
    const int32_t *indptr, *indices;
    const double *vals_a, *vals_m; /* a(t) = ca*vals_a + cm[t]*vals_m */
    const int32_t *diag;           /* CSR position of the diagonal of row i */
    /* Gauss-Seidel dependency schedule: rows grouped into DAG levels; rows of
     * one group are mutually independent.  *_ptr_host has n_groups+1 entries
     * (host memory), *_rows is a device array of row indices. */
    int32_t n_fwd;
    const int32_t *fwd_ptr_host;
    const int32_t *fwd_rows;
    int32_t n_bwd;
    const int32_t *bwd_ptr_host;
    const int32_t *bwd_rows;
    /* prolongation from the next coarser level (n x n_coarse) and its
     * transpose; NULL on level 0 */
    const int32_t *p_indptr, *p_indices;
    const double *p_vals;
    const int32_t *r_indptr, *r_indices;
    const double *r_vals;
    /* Optional sliced-ELL copies (host structs, copied by stk_mg_create); when
     * present the V-cycle runs on them.  ell_a: the level matrix in a
     * locality order, for the residual.  ell_fwd / ell_bwd: the level matrix
     * with its rows listed group by group of the forward / backward
     * Gauss-Seidel schedule; *_pos_host[g] .. [g+1] is the position range of
     * group g (n_fwd+1 / n_bwd+1 entries).  ell_p / ell_r: the transfers.
     * ell_ra (optional): the product R * (level matrix) on the coarse rows
     * (va = R*vals_a, vm = R*vals_m): the restricted residual is then formed
     * as (R A) u - R f without writing the fine residual. */
    const stk_ell_rows *ell_a, *ell_fwd, *ell_bwd, *ell_p, *ell_r;
    const int32_t *fwd_pos_host, *bwd_pos_host;
    const stk_ell_rows *ell_ra;
    /* ell_fwd0 (optional): n_fwd matrices, one per group of the forward
     * schedule, for the first sweep of a level visit, which starts from u = 0:
     * group g keeps only the entries whose column lies in a group < g (the
     * other products are exact zeros), unused slots point at a row of group 0.
     * With it the plan neither zeroes u before that sweep nor gathers the
     * zeros. */
    const stk_ell_rows *ell_fwd0;
    /* Optional (0 / NULL if absent): the rows of ell_fwd / ell_bwd are listed in
     * an order that follows the geometry; *_tile_row_host[pos] is the index of
     * the tile row (0 .. n_tile_rows-1, ascending inside every group) position
     * pos lies in, and rows in tile row r only couple to tile rows r-1 .. r+1.
     * With it a sweep on a large level runs strip by strip -- all groups on one
     * strip of tile rows before the next strip, each group shifted by one tile
     * row against the previous one so that the order of updates is unchanged --
     * and the strip's vectors stay in the Infinity Cache between the group
     * passes. */
    int32_t n_tile_rows;
    const int32_t *fwd_tile_row_host, *bwd_tile_row_host;
    /* Optional (NULL if absent): ell_fwd / ell_bwd once more in the OTHER row form
     * (stk_ell_rows.diag_free), same rows in the same order: what the sweeps the
     * plan options "fast_until_cycle" / "fast_parts" name run on. */
    const stk_ell_rows *ell_fwd_alt, *ell_bwd_alt;
} stk_mg_level;

typedef struct stk_mg stk_mg;

/* coarse_inv: n_kinds dense (n0 x n0) inverses of the level-0 matrix, row
 * major, one per distinct time-slice coefficient (device).  max_ld bounds the
 * ld of later applies (workspace is allocated here). */
int stk_mg_create(int32_t n_levels, const stk_mg_level *levels_host,
                  int32_t smoothsteps, int32_t vcycles, int32_t n_kinds,
                  const double *coarse_inv, int32_t max_ld, stk_mg **out);
int stk_mg_destroy(stk_mg *mg);
/* Per-plan choices that regroup the reference's arithmetic (results change in
 * the last bits only; the solve's r.Pr history is sensitive to them, DESIGN.md
 * section 5).  "fuse_restrict": 1 = the restricted residual as (R A) u - R f from
 * the precomputed product R A (no fine-level residual is written), 0 = the
 * reference's R (A u - f) (multigrid.py:174-175), -1 = follow the process-wide
 * tuning key "mg_fuse_restrict" (default 1).  "strip_pct": the strips of the
 * strip-wise smoothing of THIS plan as a percentage of the tuning key
 * "mg_strip_mb" (results do not depend on it): plans whose applies run two at a
 * time share the caches and want smaller strips, a plan that runs alone larger
 * ones.
 * Where the reference's forms are used (the history's gap to the CPU path is owned
 * by the LAST V-cycle's restricted residual and post-smoothing on the FINEST level:
 * DESIGN.md section 5): "fuse_restrict_min_level" / "_max_level" (default 0 / no
 * bound): the fused form only on levels inside the window, the two steps outside;
 * "fast_until_cycle" (default 0): the V-cycles with a smaller index take the fast
 * forms throughout -- the alternative sweep copies of levels that have them
 * (stk_mg_level.ell_fwd_alt / ell_bwd_alt), the fused restricted residual on every
 * level; "fast_parts": in the later V-cycles bit 0 lets the pre-smoothing and bit 1
 * the restricted residual take the fast forms as well (the post-smoothing never
 * does). */
int stk_mg_set_option(stk_mg *plan, const char *key, int32_t value);
/* u = MG(f): `vcycles` V-cycles from u = 0.  cm/kind: per-time-slice mass
 * coefficient and coarse-inverse index (device, n_loc) or NULL.  u need not be
 * initialised.  With an even ld the columns 0 .. 2*ceil(n_loc/2) - 1 of u are written (the
 * padding column of an odd n_loc as +0.0, whatever f holds there) and the columns behind
 * them -- the slab as a column range of a wider one -- are neither read nor written, in f
 * or in u.  With an odd ld (the flat kernels, which know no pairs) every column of u from
 * n_loc to ld - 1 is written as +0.0, as by stk_csr_spmm. */
int stk_mg_apply(stk_mg *mg, void *stream, int32_t n_loc, int32_t ld,
                 double ca, const double *cm, const int32_t *kind,
                 const double *f, double *u);
/* Member matrices for the coarse end of a plan with a second matrix (cm != NULL):
 * by default time slice t runs on ca * A_l + cm[t] * M_l on every level l, the two
 * Galerkin chains combined per slice.  The reference builds one hierarchy per
 * wavelet level from the ASSEMBLED matrix 2^j M + alpha A (heateq_mpi.py:97-98,
 * 147-153; Galerkin products multigrid.py:142-145): its coarse matrices carry the
 * rounding of that one chain, and the difference to the combination grows fourfold
 * per level down (1e-16 at the top, 1e-12 on level 0 of a ten-level hierarchy) --
 * on the smallest levels it owns most of the gap between the two r.Pr histories
 * (profiles/r06_history_by_coarse_level_J7_J10.json).  With member matrices the
 * levels 1 .. stk_mg_coarse_levels(plan) -- the levels of the fused coarse kernel --
 * read, for slice t, the entries of matrix kind[t] itself (kind as in stk_mg_apply:
 * the index of the slice's coarse inverse).  One call per level with the n_kinds
 * matrices of that level as CSR on the host (sorted columns; a NULL indptr for a
 * kind no slice names); members take effect once every level 1..coarse_levels has
 * them.  Entries outside the plan's pattern are ignored.  Every given matrix needs its
 * diagonal entries; a call that is refused for a missing one leaves the plan, and members
 * already in use, as they were. */
int stk_mg_coarse_levels(const stk_mg *plan);
int stk_mg_set_member_matrices(stk_mg *plan, int32_t level, int32_t n_kinds,
                               const int32_t *const *indptr_host,
                               const int32_t *const *indices_host,
                               const double *const *data_host);
/* `its` forward (backward = 0) or backward Gauss-Seidel sweeps on one level
 * (exposed for tests; multigrid.py:116-127). */
int stk_mg_smooth(stk_mg *mg, void *stream, int32_t level, int32_t n_loc,
                  int32_t ld, double ca, const double *cm, int32_t its,
                  int32_t backward, const double *f, double *u);

/* The same plan built inside the library from what a caller of the reference
 * holds when it constructs MultiGrid(mat, hierarchy) (multigrid.py:130-166): the
 * finest-level matrix A (and optionally a second matrix M on the same rows, for
 * families a(t) = ca*A + cm[t]*M, heateq_mpi.py:97-98) and the n_levels - 1
 * prolongation matrices, P[j] from level j to level j + 1 (multigrid.py:39-60),
 * all as HOST CSR.  Computes the Galerkin products R A P (multigrid.py:142-145;
 * same accumulation order as SciPy's csr_matmat, rounding-noise entries dropped),
 * the Gauss-Seidel dependency schedules, every sliced-ELL copy, the bands of the
 * strip-wise smoothing (verified on the pattern) and the exact inverses of the
 * coarsest matrices: kind 0 = A_0, kind 1 + k = ca*A_0 + cms[k]*M_0.
 * coords (optional, HOST): coordinates of the finest-level dofs, row-major
 * (n x dim), level l = the first n_l of them -- only used for cache-friendly row
 * orders and bands; NULL = index order / breadth-first bands.
 * The level matrices must be structurally symmetric (a_ij stored iff a_ji is; the values
 * may differ): the sweeps run the rows of equal depth in the dependency DAG side by side,
 * and a row that reads a row of its own group which does not read it back would race with
 * that row's update.  stk_mg_create_from_csr refuses a finest-level pattern (A united with
 * M) that is not; Galerkin products of such a matrix with R = P^T are so again and are not
 * checked, nor are the levels handed to stk_mg_create.
 * The Gauss-Seidel copies follow the tuning key "mg_gs_diag_free" AS IT STANDS WHEN
 * THE PLAN IS BUILT: 1 (default) = diagonal-free rows, u_i = (f_i - sum_{j != i}
 * a_ij u_j) / a_ii; 0 = the diagonal among the slots and the reference's update
 * u_i += (f_i - row_i u) / a_ii (multigrid.py:89-97); 2 = the latter on the finest
 * level, which also gets the diagonal-free copies as its alternative form, the
 * former below.  Key 2 together with stk_mg_set_option(plan,
 * "fuse_restrict_max_level", n_levels - 2), ("fast_until_cycle", vcycles - 1) and
 * ("fast_parts", 1) is the arithmetic the mirrored driver runs by default (r.Pr
 * histories within 1e-10 of the CPU path for 4 % of the solve); key 0 with
 * ("fuse_restrict", 0) has the reference's forms everywhere.
 * With coordinates, the bands of the strip-wise sweeps hold several mesh rows (6
 * for a family, 1 for a single matrix): inside a thicker band a stage walks mesh
 * tiles instead of the level's full width (a family's P apply 2 % faster on slabs of
 * 17 time steps and more, bit-identical).
 * The host work runs on the threads of the library (STK_HOST_THREADS overrides
 * their number). */
typedef struct {
    int32_t n_rows, n_cols;
    const int32_t *indptr, *indices;
    const double *data;
} stk_csr_host;

/* The exact solve on level 0 (multigrid.py:161-165, 169-171) is a dense inverse
 * here.  By default the library inverts the coarsest matrices itself (Gauss-Jordan
 * with partial pivoting); a caller whose other code path inverts them with its own
 * factorisation -- the Python planner of this repository takes numpy.linalg.inv,
 * i.e. LAPACK -- hands that routine over, and plans created from then on carry ITS
 * inverse: the two planners' V-cycles are then equal bit for bit, not to 1e-13.
 * fn(n, a, inv, user): a and inv are n x n, row-major, HOST; returns 0 on success.
 * fn = NULL restores the built-in inverse.  Called on the thread that calls
 * stk_mg_create_from_csr.  The hook and the tuning key "mg_gs_diag_free" are
 * process-wide; a plan construction reads both once, under a mutex, when it starts,
 * so a setter on another thread takes effect for constructions that start later and
 * never half way through one.  A caller that wants a hook for ONE construction while
 * other threads build plans must serialise those constructions itself. */
typedef int (*stk_dense_inverse_fn)(int32_t n, const double *a, double *inv,
                                    void *user);
int stk_mg_set_coarse_inverse(stk_dense_inverse_fn fn, void *user);

int stk_mg_create_from_csr(int32_t n_levels, const stk_csr_host *A_fine,
                           const stk_csr_host *M_fine,
                           const stk_csr_host *P_host,
                           const double *coords_host, int32_t dim,
                           int32_t smoothsteps, int32_t vcycles, double ca,
                           int32_t n_cms, const double *cms_host,
                           int32_t max_ld, stk_mg **out);

/* ---- problem set-up: P1 assembly on the host threads of the library ----------
 * Mass M and stiffness A of a triangulation, restricted to its free dofs, explicit
 * zeros dropped: what the reference gets from NGSolve's BilForm(...).assemble()
 * and source/ngsolve_helper.py:38-45 (heateq_mpi.py:91-96).  HOST arrays:
 * points [nv][2], cells [nc][3] (vertex numbers), boundary [nv] (1 = Dirichlet
 * vertex).  Every row sums the contributions of the triangles around its vertex in
 * ascending triangle number, without fused multiply-adds: the result depends on
 * the mesh alone, not on the number of threads.  Stiffness entries below zero_rel
 * times the largest one are rounding noise of exact zeros and are dropped.
 * The result is read with stk_p1_result_sizes / _copy (which = 0: A, 1: M; CSR with
 * int32 indices, as mpi_shared_mem.py:46-48) and released with stk_p1_result_free. */
typedef struct stk_p1_result stk_p1_result;
int stk_p1_assemble_2d(int64_t nv, int64_t nc, const double *points,
                       const int64_t *cells, const uint8_t *boundary,
                       double zero_rel, stk_p1_result **out);
int stk_p1_result_sizes(const stk_p1_result *r, int32_t *n_free, int64_t *nnz_a,
                        int64_t *nnz_m);
int stk_p1_result_copy(const stk_p1_result *r, int32_t which, int32_t *indptr,
                       int32_t *indices, double *data);
int stk_p1_result_free(stk_p1_result *r);

/* ---- problem set-up: one uniform refinement of a triangulation ---------------
 * What the reference takes from Netgen (source/problem.py:7-41: mesh.Refine())
 * together with NGSolve's parent-vertex table (source/multigrid.py:20-21,
 * GetParentVertices): every triangle cut into four, the midpoints appended to the
 * vertices in the order (colour of the bisected edge, y, x) -- the hierarchical
 * numbering the prolongations and the dof-order sweeps are built on.  HOST arrays:
 * points [nv][2], tris [nt][3], tri_colors [nt][3] (colour of the edge opposite
 * each local vertex; the two triangles of an edge must agree).  Written: the
 * n_new <= capacity new vertices (new_points [.][2], new_parents [.][2] = the ends
 * of the bisected edge, smaller number first, new_colors [.]), and the 4 nt children
 * with their edge colours, child b of triangle t at row b * nt + t.  Integer work
 * and one halving per coordinate on the host threads of the library: the result
 * does not depend on their number. */
int stk_tri_refine(int64_t nv, int64_t nt, const double *points,
                   const int64_t *tris, const int64_t *tri_colors,
                   int64_t capacity, double *new_points, int64_t *new_parents,
                   int64_t *new_colors, int64_t *child_tris,
                   int64_t *child_colors, int64_t *n_new);

/* ---- problem set-up: load vector of a triangulation --------------------------
 * int f phi_i over the mesh with an nq-point rule given in barycentric
 * coordinates (rule_points [nq][3], rule_weights [nq], weights summing to 1):
 * what the reference gets from LinearForm(u0 * v * dx).assemble()
 * (heateq_mpi.py:102-103).  Two calls around the CALLER's evaluation of f:
 * stk_p1_load_points_2d writes the coordinates of the quadrature points
 * (qx, qy [nt][nq]: l0 p0 + l1 p1 + l2 p2, summed from the left);
 * stk_p1_load_sum_2d takes f [nt][nq] at those points and writes vec [nv] (ALL
 * vertices; the caller keeps the free ones): the share of triangle t in the entry
 * of its local vertex a is (sum_q (f_q w_q) l_qa) * |T|, q ascending, and an entry
 * sums its shares in ascending (t, a) -- no fused multiply-adds, the result depends
 * on the mesh alone, not on the number of host threads. */
int stk_p1_load_points_2d(int64_t nv, int64_t nt, const double *points,
                          const int64_t *tris, int32_t nq,
                          const double *rule_points, double *qx, double *qy);
int stk_p1_load_sum_2d(int64_t nv, int64_t nt, const double *points,
                       const int64_t *tris, int32_t nq,
                       const double *rule_weights, const double *rule_points,
                       const double *f, double *vec);

/* ---- space-time load vectors: int g(t_k, .) phi_i on the device ------------------
 * A right-hand side g(t, x) that is no short separable sum needs one spatial load
 * vector per time quadrature point, hundreds per problem; the two host calls above
 * serve the single one of u0.  The plan is built once per mesh from HOST arrays:
 * points [nv][d], cells [nc][d + 1] (d = 2 or 3), free_vertices [n_free] = the vertex
 * of every slab row, and optionally row_order [n_free], a permutation of the rows
 * in which the gather pass visits them (stk_tile_order's; a performance hint, results
 * never depend on it; null = ascending).  It uploads them, computes |T| per cell by
 * the expression of stk_p1_load_sum_2d (tetrahedra: the cofactor expansion of
 * source/assembly.py; csrc/p1_mesh.h holds the one definition that the load vectors, the
 * error norms and the sampler use) and builds for every free dof the list of its (cell, local
 * vertex) incidences in ascending order.  max_k = the most time points one
 * stk_load_columns call takes (1..STK_LOAD_MAX_K): the plan owns max_k * (d + 1) * nc
 * doubles of workspace, so one plan serves one stream at a time.
 *
 * The rule is the caller's, per call, as HOST arrays in barycentric coordinates:
 * rule_points [nq][d + 1], rule_weights [nq], 1 <= nq <= STK_LOAD_MAX_NQ.
 * stk_load_points writes the DEVICE array q_points [d][nc][nq]: coordinate k of
 * point q of cell t is l_q0 p0[k] + l_q1 p1[k] + ..., summed from the left -- the
 * doubles of stk_p1_load_points_2d.
 * stk_load_columns takes the DEVICE array f [n_k][nc][nq] (f at those points for n_k
 * time points), HOST coefficients coef [n_k][2], and out_pair = the 16-byte aligned
 * address of columns (2e, 2e + 1) of row 0 of a test-space slab with leading
 * dimension ld (even), and writes for every free dof i and a = 0, 1
 *     out_pair[i ld + a] (+)= sum_k coef[k][a] L_k[i],   k ascending, the first
 *                              product starting the sum,
 * where L_k is the vector stk_p1_load_sum_2d documents: the share of cell t in the
 * entry of its local vertex a' is (sum_q (f_q w_q) l_qa') |T|, q ascending from 0.0,
 * and an entry sums its shares in ascending (t, a') from 0.0.  accumulate = 0
 * overwrites the pair, 1 adds the sum to what is there (old + sum).  Nothing else of
 * the slab is touched.  No fused multiply-adds anywhere: bit for bit the doubles of
 * the host routines combined on the host, whatever the launch shape. */
#define STK_LOAD_MAX_NQ 16
#define STK_LOAD_MAX_K 16
typedef struct stk_load_plan stk_load_plan;
int stk_load_plan_create(int32_t d, int64_t nv, int64_t nc, const double *points,
                         const int64_t *cells, int64_t n_free,
                         const int64_t *free_vertices, const int32_t *row_order,
                         int32_t max_k, stk_load_plan **out);
int stk_load_plan_destroy(stk_load_plan *plan);
int stk_load_points(void *stream, const stk_load_plan *plan, int32_t nq,
                    const double *rule_points, double *q_points);
int stk_load_columns(void *stream, const stk_load_plan *plan, int32_t nq,
                     const double *rule_weights, const double *rule_points,
                     int32_t n_k, const double *f, const double *coef,
                     int32_t accumulate, int32_t ld, double *out_pair);

/* ---- sampling the trial space: u_h(t_k, x_p) on the device ------------------------
 * The evaluation operator of the trial space (continuous P1 in time on a uniform
 * mesh, P1 on a simplicial mesh in space): points anywhere in the mesh, times anywhere
 * in [0, T], read from a slab of nodal values where it lies.  Three steps.
 *
 * The PLAN is built once per mesh from the HOST arrays stk_load_plan_create takes:
 * points [nv][d], cells [nc][d + 1] (d = 2 or 3), free_vertices [n_free] = the vertex
 * of every slab row.  It uploads the mesh, the map vertex -> slab row (-1 for a
 * boundary vertex, whose value is 0) and a BUCKET GRID for point location, which
 * stk_sample_grid_build makes on the host threads of the library (no GPU touched; the
 * result does not depend on their number): with extent = the longest side of the
 * bounding box [lo, hi] and widen = 1e-12 extent, the box [lo - widen, hi + widen] is
 * cut into bins[k] = round(nc^(1/d)) equal bins per axis,
 *     bin of x along k = floor((x - (lo[k] - widen)) * inv_width[k]), clamped to
 *                        0 .. bins[k] - 1;    bin index = (iz bins[1] + iy) bins[0] + ix,
 * and every cell is listed, in ascending cell order, in every bin between the bins of
 * the two corners of its bounding box widened by `widen`.  Nothing assumes nested or
 * congruent cells.  _sizes reports bins [3], the shifted corner lo [3], inv_width [3]
 * (axes beyond d: 1, 0, 0), widen and the number of list entries; _copy writes
 * bin_ptr [bins + 1] and bin_cells [entries] (CSR).
 *
 * stk_sample_locate takes DEVICE coordinates x [d][n_p] and writes cell [n_p] (int32,
 * -1 = outside the mesh) and lam [n_p][d + 1].  One lane per point; the candidates are
 * the cells of the point's bin (a point outside the box falls into an edge bin).
 * Barycentric coordinates of a candidate with vertices p0 .. pd, e_r = p_r - p0,
 * q = x - p0: triangles l1 = (q x e2) / (e1 x e2), l2 = (e1 x q) / (e1 x e2) with
 * a x b = a0 b1 - a1 b0; tetrahedra l1 = q . (e2 x e3) / det, l2 = q . (e3 x e1) / det,
 * l3 = q . (e1 x e2) / det, det = e1 . (e2 x e3), dot products summed from the left;
 * l0 = ((1 - l1) - l2) [- l3].  No fused multiply-adds.  The chosen cell has the largest
 * min_a l_a, the lowest index among equals; the point is inside iff that minimum is
 * >= -1e-12.  lam holds the chosen candidate's coordinates also for an outside point
 * (NaN if its bin is empty).
 *
 * stk_sample_eval takes the located points, a slab (M = n_free rows, n_loc valid
 * columns, leading dimension ld) and n_k requests as HOST arrays columns [n_k][2]
 * (local columns c0, c1 of the slab; -1 = "not on this rank") and weights [n_k][2],
 * and writes the DEVICE array out [n_k][ld_out >= n_p] (64-bit addressing):
 *     out[k][p] = p0 + p1,   p_a = w_a (((l0 u[v0][c_a] + l1 u[v1][c_a]) + l2 u[v2][c_a])
 *                                       [+ l3 u[v3][c_a]]),
 * v_a the slab rows of the cell's vertices; every product and every sum is rounded on
 * its own; a boundary vertex contributes the value 0; a term whose column is -1 is
 * exactly 0.0 and its rows are not read; an outside point gives NaN.  Only the named
 * columns are read (never the padding of an odd n_loc).  With the two columns of a
 * request owned by different ranks, each rank's out holds one of the two terms and 0.0
 * for the other: their sum over the ranks is the one-rank double.  Requests are served in
 * launches of at most 96 distinct columns each (one launch for a slab of up to 96 time
 * steps, whatever n_k).  The plan owns the request tables of a call in flight: one plan
 * serves one stream at a time.  No atomics.
 *
 * PAIRED REQUESTS AND DERIVATIVES.  stk_sample_pairs serves a list (t_p, x_p) -- a
 * trajectory, a set of tracers -- without the (n_k, n_p) block it is the diagonal of, and
 * returns, per point, any of u_h, its time derivative and its gradient.  It takes what
 * stk_sample_locate wrote (cell [n_p], lam [n_p][d + 1]), t [n_p] DEVICE doubles, the
 * element length h and number N >= 2 of nodes of the time mesh, the first node t_begin of
 * this slab (n_loc valid columns, leading dimension ld, M = n_free rows), and `fields`,
 * a mask: 1 = u, 2 = dt, 4 = grad.  out [n_rows][ld_out >= n_p] (64-bit addressing) holds
 * the requested rows only, in the fixed order u, dt, grad_0 .. grad_(d-1).  Per point:
 *     e = min(floor(t / h), N - 2),  s = t / h - e,  (w_0, w_1) = (1 - s, s)
 * (the right-hand derivative at an interior node, the left-hand one at T); the nodes
 * e, e + 1 are the local columns c_a = e + a - t_begin, and one outside [0, n_loc) is
 * "not on this rank";
 *     S(k, c) = ((k_0 u[v_0][c] + k_1 u[v_1][c]) + k_2 u[v_2][c]) [+ k_3 u[v_3][c]],
 *     u      = w_0 S(lam, c_0) + w_1 S(lam, c_1),
 *     dt     = (-(S(lam, c_0) / h)) + S(lam, c_1) / h,
 *     grad_j = w_0 S(G_j, c_0) + w_1 S(G_j, c_1),   G_j[a] = d_j l_a of the located cell,
 * every product, quotient and sum rounded on its own, a boundary vertex contributing the
 * value 0.  A term whose column is absent is exactly 0.0 and its entries are not read; the
 * padding column of an odd n_loc is never read.  Every requested field is NaN where
 * cell < 0, where t is NaN and where t is outside [0, (N - 1) h]: the times are checked on
 * the device, the call does not synchronise.  With the two columns of a point on different
 * ranks each rank's out holds one term and 0.0 for the other; the sum over the ranks is
 * the one-rank double.  One lane per point, no LDS, no atomics; n_p = 0 launches nothing;
 * the plan is only read, so the call may share it with a stk_sample_eval in flight.
 *
 * The gradients of the barycentric coordinates are EVALUATED IN THE KERNEL, per point,
 * from the vertices of the located cell by the expressions stk_sample_locate uses (the
 * plan holds no table of them; its construction is unchanged): with e_r = p_r - p_0,
 *     triangles   det = e1[0] e2[1] - e1[1] e2[0],
 *                 grad l_1 = (e2[1] / det, (-e2[0]) / det),
 *                 grad l_2 = ((-e1[1]) / det, e1[0] / det);
 *     tetrahedra  det = e1 . (e2 x e3), summed from the left,
 *                 grad l_1 = (e2 x e3) / det, grad l_2 = (e3 x e1) / det,
 *                 grad l_3 = (e1 x e2) / det, every component a difference of two products;
 *     grad l_0 = ((0 - grad l_1) - grad l_2) [- grad l_3],
 * each quotient rounded once.  stk_sample_grad_coeffs writes the same doubles per located
 * point, out [d][n_p][d + 1] (DEVICE; out[j][p][a] = d_j l_a, NaN for cell < 0): row j,
 * passed to stk_sample_eval as `lam`, gives the (n_k, n_p) block of grad_j, and
 * stk_sample_eval with the weights (-1 / h, 1 / h) gives the block of dt.
 *
 * THE ADJOINT OF PAIRED SAMPLING.  stk_sample_pairs_adjoint applies E^T: numbers w_p given
 * at the pairs (t_p, x_p) become the functional v -> sum_p w_p v_h(t_p, x_p) (field 1 = u),
 * sum_p w_p d/dt v_h (field 2 = dt) or sum_p w_p . grad v_h (field 4 = grad) on the trial
 * space, written into a slab -- the right-hand side of a solve that uses measurements.  It
 * takes what stk_sample_pairs takes (cell, lam, t, h, N, t_begin, M, n_loc, ld; the slab is
 * now the OUTPUT), DEVICE weights w [n_w][ld_w >= n_p] (n_w = 1 for u and dt, n_w = d for
 * grad), `field` (exactly one of 1, 2, 4), `accumulate` (0 or 1), a DEVICE byte array
 * used [n_p] and a DEVICE workspace of stk_sample_pairs_adjoint_work_size(n_p, d, &bytes)
 * bytes on a 256-byte boundary (the size query asks the sort for its scratch, which looks
 * at the current device).  The call allocates nothing and does not synchronise.
 *
 * Point p is USED when cell >= 0, t is not NaN and 0 <= t <= (N - 1) h, decided on the
 * device; used[p] = 1 then, else 0, and an unused point contributes nothing (its weight and
 * coordinates are not looked at: a NaN there poisons nothing).  For a used point e, s and
 * (w_0, w_1) = (1 - s, s) are those of stk_sample_pairs and G_j[b] = d_j l_b the doubles of
 * stk_sample_grad_coeffs.  Its terms, for a = 0, 1 and local vertex b = 0 .. d:
 *     u      (w[p] w_a) lam[p][b]
 *     dt     (-(w[p] / h)) lam[p][b] for a = 0,   (w[p] / h) lam[p][b] for a = 1
 *     grad   w_a q_b,   q_b = ((w[0][p] G_0[b] + w[1][p] G_1[b]) [+ w[2][p] G_2[b]])
 * every product, quotient and sum rounded on its own (no fused multiply-adds).  The term
 * goes to the local column e + a - t_begin if that lies in [0, n_loc) and to the slab row
 * of vertex v_b if that vertex is free; any other term is dropped.
 *
 * An entry's terms are taken in ascending p (for one p: a, then b) and cut into chunks of
 * STK_SAMPLE_ADJ_CHUNK consecutive terms; each chunk is summed from the left starting with
 * its first term, and the chunk sums are added from the left in chunk order (for up to
 * STK_SAMPLE_ADJ_CHUNK terms: the plain sum from the left).  accumulate = 0: every entry of
 * the n_loc valid columns becomes that sum, +0.0 where no term lands; accumulate = 1:
 * old + sum at the entries with terms, the others untouched.  The padding column of an odd
 * n_loc is never written.  No float atomics: one lane per point stores its 2 (d + 1)
 * (64-bit destination, term) records, a stable sort groups them by destination and keeps
 * ascending p, and one pass sums every run by the rule above -- so a slab entry does not
 * depend on the launch shape, nor on the number of ranks: every rank is given ALL pairs and
 * builds the entries of the columns it owns, without communication.  n_p = 0 is the zero
 * fill alone.  One call indexes 2 (d + 1) n_p < 2^31 records; more is refused (return 2,
 * also by the size query): split the list and accumulate. */
#define STK_SAMPLE_ADJ_CHUNK 512
typedef struct stk_sample_grid stk_sample_grid;
typedef struct stk_sample_plan stk_sample_plan;
int stk_sample_grid_build(int32_t d, int64_t nv, int64_t nc, const double *points,
                          const int64_t *cells, stk_sample_grid **out);
int stk_sample_grid_sizes(const stk_sample_grid *grid, int32_t *bins, double *lo,
                          double *inv_width, double *widen, int64_t *n_entries);
int stk_sample_grid_copy(const stk_sample_grid *grid, int32_t *bin_ptr,
                         int32_t *bin_cells);
int stk_sample_grid_free(stk_sample_grid *grid);
int stk_sample_plan_create(int32_t d, int64_t nv, int64_t nc, const double *points,
                           const int64_t *cells, int64_t n_free,
                           const int64_t *free_vertices, stk_sample_plan **out);
int stk_sample_plan_destroy(stk_sample_plan *plan);
int stk_sample_locate(void *stream, const stk_sample_plan *plan, int64_t n_p,
                      const double *x, int32_t *cell, double *lam);
int stk_sample_eval(void *stream, stk_sample_plan *plan, int64_t n_p,
                    const int32_t *cell, const double *lam, int32_t M, int32_t n_loc,
                    int32_t ld, const double *slab, int32_t n_k, const int32_t *columns,
                    const double *weights, int64_t ld_out, double *out);
int stk_sample_pairs(void *stream, const stk_sample_plan *plan, int64_t n_p,
                     const int32_t *cell, const double *lam, const double *t, double h,
                     int32_t N, int32_t t_begin, int32_t M, int32_t n_loc, int32_t ld,
                     const double *slab, int32_t fields, int64_t ld_out, double *out);
int stk_sample_grad_coeffs(void *stream, const stk_sample_plan *plan, int64_t n_p,
                           const int32_t *cell, double *out);
int stk_sample_pairs_adjoint_work_size(int64_t n_p, int32_t d, int64_t *bytes);
int stk_sample_pairs_adjoint(void *stream, const stk_sample_plan *plan, int64_t n_p,
                             const int32_t *cell, const double *lam, const double *t,
                             double h, int32_t N, int32_t t_begin, int32_t M, int32_t n_loc,
                             int32_t ld, double *slab, const double *w, int64_t ld_w,
                             int32_t field, int32_t accumulate, unsigned char *used,
                             void *work, int64_t work_bytes);

/* ---- space-time error norms: || u - u_h || by quadrature on the device --------------
 * The error of a trial-space vector (continuous P1 in time on a uniform mesh, P1 on a
 * simplicial mesh in space) against a function the caller evaluates at quadrature points:
 * its square in L2 and in the H1 seminorm of the mesh, integrated over ONE time element
 * per call, without downloading the slab and without an interpolant standing in for u.
 *
 * The PLAN is built once per mesh from the HOST arrays stk_load_plan_create and
 * stk_sample_plan_create take, with their checks: points [nv][d], cells [nc][d + 1]
 * (d = 2 or 3), free_vertices [n_free] = the vertex of every slab row.  Nothing assumes
 * that the cells cover anything.  It uploads the cells (int32) and the map vertex -> slab
 * row (-1 for a boundary vertex, whose value is 0), and computes per cell |T| and the
 * gradients of the barycentric coordinates [nc][d + 1][d] by the simplex routine of
 * csrc/p1_mesh.h that stk_load_plan_create and the sampler call: with e_r = p_r - p_0,
 *     triangles   det = e1[0] e2[1] - e1[1] e2[0],
 *                 grad l_1 = (e2[1] / det, -e2[0] / det),  grad l_2 = (-e1[1] / det, e1[0] / det);
 *     tetrahedra  det = (e1[0] C_00 + e1[1] C_10) + e1[2] C_20 with the cofactors
 *                 (C_0a, C_1a, C_2a) = e2 x e3, e3 x e1, e1 x e2 for a = 0, 1, 2, each
 *                 component a difference of two products,
 *                 grad l_(a+1)[j] = C_ja / det;
 *     grad l_0[j] = -((grad l_1[j] + grad l_2[j]) [+ grad l_3[j]]),
 * each quotient rounded once.  The plan owns 4 ceil(nc / 256) doubles of workspace for
 * the tile partials of a call in flight: one plan serves one stream at a time.
 *
 * The rule is the caller's, per call, as for the load vectors: HOST arrays rule_points
 * [nq][d + 1] (barycentric) and rule_weights [nq], 1 <= nq <= STK_ERR_MAX_NQ.
 * stk_err_points writes the DEVICE array q_points [d][nc][nq] with the kernel of
 * stk_load_points (csrc/p1_mesh.h) -- the same doubles.
 *
 * stk_err_element takes, for the n_k (1..STK_ERR_MAX_K) time points of one time element,
 * HOST arrays w_lo, w_hi, c [n_k] and DEVICE arrays f [n_k][nc][nq] (the exact solution at
 * the quadrature points) and gf [n_k][d][nc][nq] (its gradient; NULL = no H1 part), and
 * the nodal values at the two ends of the element: u_lo / u_hi point at row 0 of the
 * lower / upper time node, consecutive rows stride_lo / stride_hi doubles apart (a slab
 * column: ld; a contiguous row such as a ghost row: 1).  One lane per cell, a workgroup
 * per tile of 256 consecutive cells.  Per cell with vertices a = 0 .. d, every product
 * and every sum rounded on its own (no fused multiply-adds):
 *     U_a  = w_lo[k] lo_a + w_hi[k] hi_a       (0.0 for a boundary vertex; no row is read)
 *     uh_q = ((l_q0 U_0 + l_q1 U_1) + l_q2 U_2) [+ l_q3 U_3]
 *     E_k  = sum_q ((f_q - uh_q)^2) w_q,    R_k = sum_q (f_q^2) w_q      q ascending from 0.0
 *     G_j  = ((U_0 grad l_0[j] + U_1 grad l_1[j]) + U_2 grad l_2[j]) [+ U_3 grad l_3[j]]
 *     EG_k = sum_j [sum_q ((gf_qj - G_j)^2) w_q],  RG_k the same with G_j = 0,
 *            the inner sum first from 0.0, j ascending from 0.0
 *     the cell's four numbers:  sum_k c[k] (X_k |T|),  k ascending, the first product
 *            starting the sum,  X = E, EG, R, RG.
 * The sum over the cells has one shape, fixed by nc: tile i is cells [256 i, 256 i + 256)
 * whatever the grid; its 256 lanes (absent cells: 0.0) are added in the tree
 * x[i] += x[i + s], s = 128, 64, .., 1; the tile partials are added by one workgroup in the
 * same tree over the tile index, s = P / 2, .., 1 with P the power of two at or above the
 * number of tiles (an absent partner adds nothing).  No atomics.  The result is the
 * DEVICE array out4 = (err_L2^2, err_H1^2, ref_L2^2, ref_H1^2): the integrals of
 * (u - u_h)^2, |grad (u - u_h)|^2, u^2, |grad u|^2 over the element when c[k] carries the
 * time rule's weights; entries 1 and 3 are 0.0 without gf.  Offsets into f and gf are
 * 64-bit; lanes beyond nc read nothing.  A null pointer (gf excepted), n_k or nq out of
 * range or a stride below 1 is refused with out4 untouched.  The plan checks indices, not
 * geometry (as the load plan): a degenerate cell (det = 0) has |T| = 0 and gradients that
 * are inf or NaN, which reach the H1 sums unannounced. */
#define STK_ERR_MAX_NQ 16
#define STK_ERR_MAX_K 16
typedef struct stk_err_plan stk_err_plan;
int stk_err_plan_create(int32_t d, int64_t nv, int64_t nc, const double *points,
                        const int64_t *cells, int64_t n_free,
                        const int64_t *free_vertices, stk_err_plan **out);
int stk_err_plan_destroy(stk_err_plan *plan);
int stk_err_points(void *stream, const stk_err_plan *plan, int32_t nq,
                   const double *rule_points, double *q_points);
int stk_err_element(void *stream, stk_err_plan *plan, int32_t nq,
                    const double *rule_weights, const double *rule_points, int32_t n_k,
                    const double *w_lo, const double *w_hi, const double *c,
                    const double *f, const double *gf, const double *u_lo,
                    int64_t stride_lo, const double *u_hi, int64_t stride_hi,
                    double *out4);

/* ---- history maps: peak, dose, rates and threshold times of every row in one scan ----
 * A row is a function of time that is piecewise linear between the nodes t_k = (double)k h:
 * a spatial dof of a trial-space slab, or a point the sampler evaluated at the nodes.
 * stk_history_scan reduces every row along time into a STATE of STK_HISTORY_STATE = 9
 * doubles, state [9][M] (DEVICE, row-major, in/out):
 *     0 peak, 1 t_peak, 2 dose, 3 time_above, 4 t_first, 5 t_last, 6 max_rate, 7 min_rate,
 *     8 last (the value at the last node seen).
 * u[i*row_stride + c*col_stride] is row i at node k_first + c, c < n_cols.  With fresh != 0
 * column 0 INITIALISES the state (it is not read):
 *     peak = last = v,  t_peak = (double)k h,  dose = time_above = 0.0,
 *     t_first = t_last = (double)k h if v > threshold, else NaN,
 *     max_rate = -inf,  min_rate = +inf.
 * Every further column k, with a = last, b = its value, e = k - 1, in this order and every
 * operation rounded on its own (no fused multiply-adds):
 *     if b > peak:  peak = b, t_peak = (double)k h        (strict: the earliest node wins a tie)
 *     dose = dose + (a + b) * (0.5 * h)
 *     rate = (b - a) / h;  max_rate, min_rate by strict comparisons
 *     a > threshold and b > threshold:  time_above += h,  t_last = (double)k h
 *     only b > threshold:  x = (threshold - a) / (b - a),  time_above += h * (1.0 - x),
 *                          t_first = ((double)e + x) * h if it is still NaN,  t_last = (double)k h
 *     only a > threshold:  x = (threshold - a) / (b - a),  time_above += h * x,
 *                          t_last = ((double)e + x) * h
 *     last = b.
 * No division happens unless a and b lie on different sides of the threshold.  Because
 * `last` is carried, a scan of [k0, k1) followed by one of [k1, k2) with fresh = 0 gives the
 * doubles of one scan of [k0, k2): the result depends neither on how the columns are cut
 * (ranks, chunks) nor on the launch shape.
 *
 * Exactly two layouts are served:
 *   slab        col_stride == 1, row_stride = ld >= n_cols: time contiguous (a slab of this
 *               library).  A workgroup streams the run of its rows through LDS and one lane
 *               walks one row; columns c >= n_cols are never read.  u need only be 8-byte
 *               aligned (base + 8 skip for a scan that starts at column skip).
 *   time-major  row_stride == 1, col_stride >= M: the (n_k, n_p) block of stk_sample_eval.
 *               One lane per row, coalesced loads, no LDS.
 * All offsets are 64-bit; no atomics; nothing is allocated and nothing synchronises.
 * n_cols == 0 with fresh == 0 leaves the state untouched.  Refused (non-zero, the text of
 * stk_last_error names the argument, state untouched): a null u or state, M < 0, n_cols < 0,
 * fresh with n_cols == 0, k_first < 0, h not finite or <= 0, a NaN threshold (+-inf are
 * allowed: never / always above), a stride pair that is neither layout.
 *
 * stk_history_tile sets the tile of the slab form for the launches that follow, process-wide
 * (measurement and tests; results never depend on it): `rows` per workgroup -- 64, 128, 256
 * or 512 -- and the LDS a workgroup may take in KiB, 1..64, which sets the columns per chunk
 * (at least one); 0 for either = the default.  Anything else is refused. */
#define STK_HISTORY_STATE 9
int stk_history_tile(int32_t rows, int32_t lds_kib);
int stk_history_scan(void *stream, int64_t M, int32_t n_cols, const double *u,
                     int64_t row_stride, int64_t col_stride, int64_t k_first, double h,
                     double threshold, int32_t fresh, double *state);

/* ---- time curves: heat content, norms, outflow, peak and hot zone per time node ----------
 * The reductions over SPACE of a trial-space slab, one number per time node: the complement
 * of the history maps, from one pass over the cells, without downloading the slab.
 *
 * The PLAN is built once per mesh from the HOST arrays of stk_err_plan_create, with its
 * checks; it stores per cell |T| and grad lambda_a (the expressions given there), a mask of
 * boundary faces, and owns the workspace of the tile partials (at most 8 MiB, or one column
 * of partials where that is more): one plan serves one stream at a time.
 *
 * stk_curves_boundary_faces (HOST only, touches no GPU, serial): bit a of mask[t] is set iff
 * the face of cell t opposite its vertex a belongs to no other cell of `cells` [nc][d + 1].
 * The face keys (the other d vertices, ascending) are sorted with the slot as the last key, a
 * total order: no hash, nothing that could vary from run to run.
 *
 * stk_curves_eval reads slab[i * row_stride + c], c < n_cols, i < M = n_free (the caller
 * offsets the pointer for a column range; 8-byte alignment is all it needs) and writes the
 * DEVICE array out[q * ld_out + c], q < stk_curves_rows(d) = 7 + 3 d:
 *     STK_CURVES_HEAT, _L2, _H1, _OUTFLOW, _MEASURE, _MOMENT + j (j < d), then
 *     STK_CURVES_PEAK(d), _PEAK_ROW(d) (an exact double), _BOX_LO(d) + j, _BOX_HI(d) + j.
 * Per cell with vertices a = 0 .. d, U_a its nodal values (0.0 for a boundary vertex, no row
 * is read), g_a = grad lambda_a, every product, quotient and sum rounded on its own:
 *     S = ((U_0 + U_1) + U_2) [+ U_3],   Q = ((U_0 U_0 + U_1 U_1) + U_2 U_2) [+ U_3 U_3]
 *     heat     (|T| S) / (d + 1)
 *     l2_sq    (|T| (S S + Q)) / ((d + 1)(d + 2))
 *     G_j = ((U_0 g_0j + U_1 g_1j) + U_2 g_2j) [+ U_3 g_3j]
 *     h1_sq    |T| ((G_0 G_0 + G_1 G_1) [+ G_2 G_2])
 *     outflow  (d |T|) F,  F = 0.0, then for a ascending with bit a of the face mask set
 *              F = F + ((G_0 g_a0 + G_1 g_a1) [+ G_2 g_a2])       (n_a |F_a| = -d |T| g_a)
 * The zone {u_h > threshold}: vertex a is above iff U_a > threshold, strictly.  The vertices
 * are put in the order q_0 .. q_d, those above in ascending a and then the others in ascending
 * a, with values W; n are above.  C_ab = q_a + s (q_b - q_a), s = (W_a - threshold) /
 * (W_a - W_b), a above and b not, so the denominator is positive.  The pieces:
 *     d = 2  n = 1: X = (q_0, C_01, C_02): X0 X1 X2;  n = 2: X = (q_0, q_1, C_12, C_02): X0 X1
 *            X2 and X0 X2 X3
 *     d = 3  n = 1: X = (q_0, C_01, C_02, C_03): X0 X1 X2 X3;  n = 2: X = (q_0, C_02, C_03, q_1,
 *            C_12, C_13), n = 3: X = (q_0, q_1, q_2, C_03, C_13, C_23): X0 X1 X2 X3, X1 X2 X3 X4
 *            and X2 X3 X4 X5
 *     n = d + 1: the cell with its own |T| and its own vertices in their order; n = 0: nothing.
 * A piece has the measure m = |det| / d! of its edge vectors X_r - X_first (the expressions of
 * |T|) and adds m to the measure, from 0.0 in the order above, and (m (sum of its vertices,
 * from the left)) / (d + 1) to moment j.  Every term is >= 0: no "cell minus corner".  The
 * box is the min / max over the X of the case; an empty one leaves as NaN.
 * The peak is the largest u over the slab rows and the lowest row that has it; a NaN value
 * takes no part, and a column of nothing else gives (-inf, M).
 * The sums over the mesh have the ONE shape of stk_err_element, fixed by nc: tile i is cells
 * [256 i, 256 i + 256), its 256 lanes (absent cells: 0.0) are added in the tree x[i] + x[i + s],
 * s = 128, .., 1, and the tile partials in the same tree with P the power of two at or above
 * the number of tiles (an absent partner adds nothing).  No atomics.  Column c's numbers
 * depend neither on the columns that share its call, nor on stk_curves_tile (the columns a
 * workgroup takes in turn, 1..32, 0 = the default 8), nor on stk_curves_batch (the bytes of
 * partials per column batch, up to the default 8 MiB, 0 = the default), nor on alignment.
 * threshold = +inf: never above (measure and moment 0.0, the box NaN); -inf: every vertex
 * above, boundary vertices included; NaN is refused.  Refused with `out` untouched and the
 * argument named in stk_last_error: a null pointer, n_cols < 1, M != n_free, row_stride or
 * ld_out below n_cols, a NaN threshold; stk_curves_tile and stk_curves_batch refuse values
 * outside their ranges.
 * Out of scope: time windows other than whole nodes, several thresholds per call,
 * sub-regions of the mesh, values between nodes, test-space vectors. */
#define STK_CURVES_HEAT 0
#define STK_CURVES_L2 1
#define STK_CURVES_H1 2
#define STK_CURVES_OUTFLOW 3
#define STK_CURVES_MEASURE 4
#define STK_CURVES_MOMENT 5
#define STK_CURVES_PEAK(d) (5 + (d))
#define STK_CURVES_PEAK_ROW(d) (6 + (d))
#define STK_CURVES_BOX_LO(d) (7 + (d))
#define STK_CURVES_BOX_HI(d) (7 + 2 * (d))
typedef struct stk_curves_plan stk_curves_plan;
int stk_curves_rows(int32_t d);
int stk_curves_boundary_faces(int32_t d, int64_t nc, const int64_t *cells, uint8_t *mask);
int stk_curves_plan_create(int32_t d, int64_t nv, int64_t nc, const double *points,
                           const int64_t *cells, int64_t n_free,
                           const int64_t *free_vertices, stk_curves_plan **out);
int stk_curves_plan_destroy(stk_curves_plan *plan);
int stk_curves_eval(void *stream, stk_curves_plan *plan, int64_t M, int32_t n_cols,
                    const double *slab, int64_t row_stride, double threshold,
                    int64_t ld_out, double *out);
int stk_curves_tile(int32_t cols);
int stk_curves_batch(int64_t bytes);

/* ---- isotherms: the level-set segments and triangles of every time node ---------------------
 * The cut of the time curves' zone itself: per column of a trial-space slab the pieces of
 * {u_h = threshold} -- segments for d = 2, triangles for d = 3 -- exact for the P1 function.
 * They are the faces of the zone pieces above that lie on the level set and carry the doubles
 * that enter box_lo and box_hi.  On a stk_curves_plan; the plan's workspace is not used.
 *
 * Everything is the time curves' rule, every product, quotient and sum rounded on its own:
 * U_a (0.0 for a boundary vertex, no row is read), above iff U_a > threshold strictly, the
 * order q_0 .. q_d with values W, n of them above, C_ab = q_a + s (q_b - q_a), s =
 * (W_a - threshold) / (W_a - W_b).  The pieces of a cell, in this order:
 *     d = 2  n = 1: segment (C_01, C_02);  n = 2: segment (C_12, C_02)
 *     d = 3  n = 1: triangle (C_01, C_02, C_03);  n = 2: triangles (C_02, C_03, C_12), then
 *            (C_03, C_12, C_13);  n = 3: triangle (C_03, C_13, C_23)
 *     n = 0 or d + 1: none.
 * A vertex AT the threshold is not above (a cut on its edge has s == 1.0 and is that vertex); a
 * NaN value is not above, and coordinates computed from it are whatever IEEE gives; threshold
 * = +-inf gives no piece at all; a NaN threshold is refused.  The orientation of a piece is
 * not promised: the record carries the gradient.
 *
 * A piece is one RECORD of stk_iso_width(d) = d d + d + 1 doubles: the vertices X[r][j] at
 * r d + j; G_j = ((U_0 g_0j + U_1 g_1j) + U_2 g_2j) [+ U_3 g_3j] at d d + j, g the plan's
 * gradients in the cell's own vertex order (the expression of h1_sq); the cell index at
 * d d + d, an exact double.  The records are ordered by column, then by cell in the mesh's
 * order, then as in the table.  No square root is taken: lengths and areas are the caller's.
 *
 * The result has no fixed length, so there are two calls, and the scan between them is the
 * caller's.  Tile t is the cells [256 t, 256 t + 256), n_tiles = ceil(nc / 256).
 * stk_iso_count writes counts[c * n_tiles + t], the pieces of tile t in column c.
 * stk_iso_fill takes the counts and first[c * n_tiles + t], the index of that tile's first
 * record (the caller's exclusive prefix of the counts, in whatever table it assembles), and
 * writes piece i = first[c][t] + (its rank in the tile) to out[i * W ..] iff 0 <= i < n_out;
 * nothing else of `out` is touched, so tables that do not belong together cannot make it
 * write out of bounds.  A (column, tile) with counts == 0 is skipped before a slab row is
 * read; otherwise the lanes' counts are recomputed, the table only opens the gate.
 * No atomics: a lane's rank comes from ballots over its wavefront and the four wavefront
 * totals.  A column's records depend neither on the columns that share its call, nor on
 * stk_iso_tile (the columns a workgroup takes in turn, 1..32, 0 = the default 16), nor on
 * alignment beyond 8 bytes (the caller offsets the pointers for a column range).
 * Refused with the outputs untouched and the argument named in stk_last_error: a null
 * pointer, n_cols < 1, M != n_free, row_stride below n_cols, a NaN threshold, n_out < 0;
 * stk_iso_tile refuses values outside its range.
 * Out of scope: times between nodes, several thresholds per call, joining the pieces into
 * polylines or surfaces, orientation, sub-regions of the mesh, test-space vectors. */
int stk_iso_width(int32_t d);
int stk_iso_count(void *stream, stk_curves_plan *plan, int64_t M, int32_t n_cols,
                  const double *slab, int64_t row_stride, double threshold, int64_t *counts);
int stk_iso_fill(void *stream, stk_curves_plan *plan, int64_t M, int32_t n_cols,
                 const double *slab, int64_t row_stride, double threshold,
                 const int64_t *counts, const int64_t *first, int64_t n_out, double *out);
int stk_iso_tile(int32_t cols);

/* ---- solidification maps: gradient, cooling rate and front speed per cell ----------------
 * What happens at the freezing front of a trial-space slab, per CELL: when the mean of the
 * cell last dropped to or below a threshold, how fast it was cooling and what grad u_h was at
 * that moment, how often that happened, and the largest |grad u_h|^2 it ever saw.  grad u_h is
 * constant per cell, so the history maps (rows are dofs or points) cannot see it; mean and
 * gradient of a cell are linear in time per element, so all of it is ONE scan over the
 * cells' rows with a carried state, without downloading the slab.
 *
 * The PLAN is built once per mesh from the HOST arrays of stk_curves_plan_create, with its
 * checks; it puts the cells in an order of its own, and stores per cell grad lambda_a (the
 * doubles of stk_err_plan_create), per tile of 256 consecutive cells of that order the
 * ascending list of the distinct slab rows its cells touch, and per cell the d + 1 positions
 * in that list.  A cell's numbers are its own, so the order changes no double; the state is
 * indexed by the caller's cells.  It owns no workspace: one plan serves any number of streams.
 *
 * stk_solid_cell_order (HOST only, touches no GPU, serial): order[i] = the cell in place i
 * along the Z-curve of the centroids, so that 256 consecutive cells are a compact patch that
 * shares its rows (in the order meshes come in after refinement, 256 consecutive cells can
 * share none).  The key of a cell: per axis j the 16 bits trunc((c_j - lo_j) / (hi_j - lo_j) *
 * 65535), c = ((p_0 + p_1) + p_2 [+ p_3]) / (d + 1) its centroid and [lo, hi] the box of all
 * points (0 on an axis of no extent), bit b of axis j at bit d b + j; the cells are sorted by
 * (key, cell): a total order, no hash, the same on every run.  stk_solid_order(1) makes plans
 * created from then on take the cells as given, stk_solid_order(0) restores the default:
 * measurement and tests; results never depend on it.
 *
 * stk_solid_tile_rows (HOST only, touches no GPU, serial): for tile i = cells [256 i,
 * 256 i + 256) of `cells` [nc][d + 1], tile_rows[tile_ptr[i] .. tile_ptr[i + 1]) is the
 * ascending list of the distinct values row_of[v] >= 0 over the vertices v of its cells
 * (row_of [nv]: the slab row of a vertex, -1 on the boundary), and cell_pos[(d + 1) t + a] the
 * position of row_of[cells[t][a]] in the list of t's tile, 0xFFFF for a boundary vertex (a
 * list has at most 256 (d + 1) <= 1024 entries).  tile_ptr has n_tiles + 1 entries, tile_rows
 * room for (d + 1) nc.  Sort and unique per tile: no hash, nothing that could vary from run
 * to run.
 *
 * stk_solid_scan reads slab[i * row_stride + c], c < n_cols, i < M = n_free, row i at the
 * node k_first + c (the caller offsets the pointer for a column range; 8-byte alignment is
 * all it needs), and updates the DEVICE array state[q * nc + t], q < STK_SOLID_ROWS(d) =
 * 6 + 2 d, row-major, in/out:
 *     STK_SOLID_T_SOLID, _COOLING_RATE, _N_SOLID, _MAX_GRAD_SQ, _T_MAX_GRAD, _LAST_MEAN,
 *     STK_SOLID_GRAD_SOLID + j, STK_SOLID_LAST_GRAD(d) + j  (j < d).
 * Cell t has vertices a = 0 .. d, g_a = grad lambda_a, U_a(k) the slab value of vertex a at
 * node k and 0.0 for a boundary vertex (no row is read); every product, quotient and sum is
 * rounded on its own, no fused multiply-add:
 *     m   = (((U_0 + U_1) + U_2) [+ U_3]) / (double)(d + 1)              the cell mean
 *     G_j = ((U_0 g_0j + U_1 g_1j) + U_2 g_2j) [+ U_3 g_3j]              j < d
 *     Q   = (G_0 G_0 + G_1 G_1) [+ G_2 G_2]
 * With fresh != 0 the first column k initialises the state: t_solid = cooling_rate =
 * grad_solid[j] = NaN, n_solid = 0.0, max_grad_sq = Q, t_max_grad = (double)k h, last_mean = m,
 * last_grad = G.  Every further column k, with e = k - 1, a = last_mean, b = m, in this order:
 *     if Q > max_grad_sq:  max_grad_sq = Q, t_max_grad = (double)k h     (strict: the earliest
 *                                                                          node wins)
 *     if a > threshold and b <= threshold:          (the rule of the history maps: AT the
 *                                                    threshold is not above)
 *         x = (threshold - a) / (b - a)
 *         t_solid       = ((double)e + x) * h
 *         cooling_rate  = (a - b) / h
 *         grad_solid[j] = last_grad[j] + x * (G_j - last_grad[j])
 *         n_solid       = n_solid + 1.0
 *     last_mean = b, last_grad = G
 * No division happens without a crossing.  NaN data makes no crossing (both comparisons are
 * false) and a NaN Q never replaces max_grad_sq.  threshold = +-inf is allowed, NaN refused.
 * |grad u_h|^2 is a convex quadratic in t on every time element, so its maximum over [0, T]
 * sits at a node: max_grad_sq is the EXACT maximum, not a nodal approximation.
 * last_mean and last_grad are carried: a scan of [k0, k1) followed by one of [k1, k2) with
 * fresh = 0 gives the doubles of one scan of [k0, k2).  The result depends neither on ranks,
 * nor on column chunks, nor on the launch shape (stk_solid_tile), nor on the alignment of the
 * slab.  The square root of Q and the front speed cooling_rate / |grad_solid| are NOT taken
 * here: the table is a matter of + - * / only, as every bit-for-bit contract of this library.
 * Refused with the state untouched and the argument named in stk_last_error: a null pointer,
 * M != n_free, n_cols < 0, fresh with n_cols == 0, k_first < 0, h not finite or <= 0, a NaN
 * threshold, row_stride < n_cols.  n_cols == 0 with fresh == 0 leaves the state untouched.
 * No atomics, nothing allocated per call, nothing synchronises.
 * stk_solid_tile(cols, lds_kib): measurement and tests; results never depend on it.  cols =
 * the columns of a chunk (1..128, fewer where the image of the longest tile list would exceed
 * 64 KiB; 0 = from the budget), lds_kib = the LDS budget of a workgroup (1..64, 0 = the
 * default 16; a chunk is at least one column whatever the budget).  Values outside are refused.
 * Out of scope: per-cell thresholds, several thresholds per call, upward crossings, time
 * windows other than whole nodes, a parallel merge of per-rank states, test-space vectors. */
#define STK_SOLID_ROWS(d) (6 + 2 * (d))
#define STK_SOLID_T_SOLID 0
#define STK_SOLID_COOLING_RATE 1
#define STK_SOLID_N_SOLID 2
#define STK_SOLID_MAX_GRAD_SQ 3
#define STK_SOLID_T_MAX_GRAD 4
#define STK_SOLID_LAST_MEAN 5
#define STK_SOLID_GRAD_SOLID 6
#define STK_SOLID_LAST_GRAD(d) (6 + (d))
typedef struct stk_solid_plan stk_solid_plan;
int stk_solid_rows(int32_t d);
int stk_solid_cell_order(int32_t d, int64_t nv, int64_t nc, const double *points,
                         const int64_t *cells, int32_t *order);
int stk_solid_order(int32_t caller_order);
int stk_solid_tile_rows(int32_t d, int64_t nv, int64_t nc, const int64_t *cells,
                        const int32_t *row_of, int32_t *tile_ptr, int32_t *tile_rows,
                        uint16_t *cell_pos);
int stk_solid_plan_create(int32_t d, int64_t nv, int64_t nc, const double *points,
                          const int64_t *cells, int64_t n_free,
                          const int64_t *free_vertices, stk_solid_plan **out);
int stk_solid_plan_destroy(stk_solid_plan *plan);
int stk_solid_scan(void *stream, stk_solid_plan *plan, int64_t M, int32_t n_cols,
                   const double *slab, int64_t row_stride, int64_t k_first, double h,
                   double threshold, int32_t fresh, double *state);
int stk_solid_tile(int32_t cols, int32_t lds_kib);

/* ---- level transfer: a coarse trial-space slab prolonged to a finer discretisation ------
 * The first engine that connects two discretisations: the trial-space vector of a coarser
 * space mesh (one red refinement fewer, its vertices a prefix of the finer mesh's) and of a
 * coarser time mesh (N_f - 1 = 2^a (N_c - 1) elements, a >= 0) as the vector of the finer
 * trial space that represents the SAME function -- P1 in space, piecewise linear in time.
 * All arithmetic is rounded term by term (no fused multiply-adds).
 *
 * SPACE, one level.  A plan holds parents [M_fine][2] (int32): per free row of the fine level
 * the free rows of the coarse level it interpolates, -1 for a parent on the boundary (value
 * 0).  With uc the coarse slab and q a coarse time node:
 *     parents[i] = (p, p):   s_i(q) = uc[p, q]                   a copy, no arithmetic
 *     otherwise:             s_i(q) = (A + B) * 0.5              A, B = the parents' values,
 *                                                                0.0 for an absent one
 *                                                                (both absent, the pair
 *                                                                (-1, -1): 0.0)
 * TIME, a levels in one shot.  The fine node k = k_first + c has q = k >> a and
 * rem = k & (2^a - 1):
 *     rem == 0:   out[i, c] = s_i(q)                             column q + 1 is NOT read
 *     otherwise:  w1 = rem / 2^a,  w0 = 1.0 - w1  (both exact),
 *                 out[i, c] = w0 * s_i(q) + w1 * s_i(q + 1)      two rounded products, one
 *                                                                rounded sum
 * (A chain of half-steps in time would round differently: time goes in one shot.  Several
 * space levels are chained by the caller: a = 0 on the coarse time mesh for all but the
 * last level, which carries all of the time refinement and writes the big slab once.)
 *
 * Layouts: both slabs are this library's, time contiguous -- uc[j*ldc + (q - qc_first)] for
 * q - qc_first < n_cc, out[i*ld + c] for c < n_cols; columns c >= n_cols of out (the pad of
 * an odd n_loc) are never written.  out and uc need only be 8-byte aligned (a rank's window
 * may start at an odd column).  All offsets are 64-bit; no atomics; nothing is allocated and
 * nothing synchronises.  NaN and +-inf in uc give what the rules give.
 *
 * stk_transfer_plan_create checks every index -- in [-1, M_coarse); (-1, -1), the vertex
 * between two boundary vertices, not in a row i < M_coarse: in the hierarchical numbering those
 * are the coarse level's own vertices, which copy and need a row to copy; M_coarse = 0 is
 * allowed -- and uploads the table to the current device: after that the
 * kernel reads no row outside [0, M_coarse), whatever it is given.  stk_transfer_prolong
 * refuses (non-zero, stk_last_error names the argument, out untouched): a null plan, uc or
 * out, a outside [0, STK_TRANSFER_MAX_A], negative sizes or node numbers, ldc < n_cc,
 * ld < n_cols, and a coarse window [qc_first, qc_first + n_cc) that does not cover every
 * column the rules read -- q of the first and of the last fine column, and q + 1 of the
 * last one only if its rem != 0.  n_cols == 0 or M_fine == 0 is a no-op.
 *
 * stk_transfer_tile sets the launch form for the calls that follow, process-wide
 * (measurement and tests; results never depend on it): `rows` of the fine level per
 * workgroup -- 64, 128 or 256 -- and the LDS a workgroup may take in KiB, 1..64, which
 * sets the fine columns per chunk (at least one); 0 for either = the default.  Anything
 * else is refused and changes nothing. */
#define STK_TRANSFER_MAX_A 8
typedef struct stk_transfer_plan stk_transfer_plan;
int stk_transfer_plan_create(int64_t M_fine, int64_t M_coarse, const int32_t *parents,
                             stk_transfer_plan **out);
int stk_transfer_plan_destroy(stk_transfer_plan *plan);
int stk_transfer_tile(int32_t rows, int32_t lds_kib);
int stk_transfer_prolong(void *stream, const stk_transfer_plan *plan, int32_t a,
                         const double *uc, int64_t ldc, int64_t qc_first, int32_t n_cc,
                         double *out, int64_t ld, int64_t k_first, int32_t n_cols);

/* ---- restriction P^T: the adjoint of the level transfer -------------------------------
 * With P the prolongation above (one space level `parents`, a time levels), the functional
 * f on the FINE trial space as the functional P^T f on the coarse one: (P^T f) . v = f . (P v).
 * Residuals, duality-based indicators, and the coarse right-hand side of a functional that
 * exists only as a fine vector.  Every operation is rounded on its own (no fused
 * multiply-adds) and every sum has ONE order -- a gather over a transposed table, never an
 * atomic scatter.
 *
 * SPACE.  The entries of the coarse row j, in ascending fine row i: (i, 1.0) where
 * parents[i] = (j, j); (i, 0.5) where one of the two differing parents is j; a -1 parent
 * contributes to nobody.  g_j(k) = the left fold of w * f_i(k) over these entries, the first
 * term starting the sum (no 0.0 + in front); a coarse row without entries gives 0.0.
 * TIME, a levels in one shot, n_fine nodes with (n_fine - 1) % 2^a == 0.  out_j(q) = the left
 * fold over k = max(0, ((q - 1) << a) + 1) .. min(n_fine - 1, ((q + 1) << a) - 1), ascending,
 * of w(k) * g_j(k), the first term starting the sum:
 *     k == q << a:  w = 1.0
 *     below it:     w = rem / 2^a,        rem = k - ((q - 1) << a)      (prolong's w1)
 *     above it:     w = 1.0 - rem / 2^a,  rem = k - (q << a)            (prolong's w0)
 * For a = 0 out = g; with an identity table g = f: both stages are then exact copies, so
 * "space with a = 0, then time only" gives the doubles of the fused call.  Several space
 * levels are chained by the caller: the first call acts on the fine slab and carries all of
 * a, the later ones use a = 0 on the coarse columns.
 *
 * stk_transfer_children (host threads, no GPU, deterministic: a stable counting sort) writes
 * the transposed table as CSR per coarse row: ptr [M_coarse + 1] and ptr[M_coarse] entries,
 * at most 2 M_fine -- the caller provides that many --, an entry being
 *     (fine row << 1) | h,     h = 1 where the weight is 0.5, 0 where it is 1.0,
 * a non-negative int32; hence M_fine <= STK_RESTRICT_MAX_M_FINE = 2^30, anything above is
 * refused.  It makes the index checks of stk_transfer_plan_create (one routine serves both).
 * stk_restrict_plan_create builds that table and uploads it to the current device; the
 * kernel then reads no row outside [0, M_fine), whatever it is given.
 *
 * stk_transfer_restrict computes the coarse columns [q_first, q_first + n_qc) into
 * out[j*ldc + (q - q_first)] from the fine window [k_first, k_first + n_cols) at
 * f[i*ld + (k - k_first)]; columns >= n_qc of out are never written; 8-byte alignment
 * suffices; 64-bit offsets, no atomics, nothing allocated, nothing synchronises.
 * stk_transfer_restrict_time is the time stage alone over M rows (g = f); it needs no
 * table.  Both refuse (non-zero, stk_last_error names the argument, out untouched): a null
 * plan, f or out, a outside [0, STK_TRANSFER_MAX_A], negative sizes or node numbers,
 * ld < n_cols, ldc < n_qc, (n_fine - 1) % 2^a != 0, a q beyond (n_fine - 1) >> a, and a fine
 * window that does not cover every column the stencils read after clipping to
 * [0, n_fine - 1].  n_qc == 0 or M_coarse == 0 is a no-op; M_fine == 0 with M_coarse > 0
 * writes 0.0.
 *
 * stk_restrict_tile sets the launch form for the calls that follow, process-wide
 * (measurement and tests; results never depend on it): `rows` of the coarse level per
 * workgroup, 1..256, and the LDS a workgroup may take in KiB, 1..64; 0 for either = the
 * default.  Columns are cut into chunks of whole stencils that fit; where `rows` stencils
 * do not fit, fewer rows are taken, and one row of one stencil (at most 4 088 bytes) is
 * always allowed.  Anything else is refused and changes nothing. */
#define STK_RESTRICT_MAX_M_FINE 1073741824
typedef struct stk_restrict_plan stk_restrict_plan;
int stk_transfer_children(int64_t M_fine, int64_t M_coarse, const int32_t *parents,
                          int64_t *ptr, int32_t *entries);
int stk_restrict_plan_create(int64_t M_fine, int64_t M_coarse, const int32_t *parents,
                             stk_restrict_plan **out);
int stk_restrict_plan_destroy(stk_restrict_plan *plan);
int stk_restrict_tile(int32_t rows, int32_t lds_kib);
int stk_transfer_restrict(void *stream, const stk_restrict_plan *plan, int32_t a,
                          const double *f, int64_t ld, int64_t k_first, int32_t n_cols,
                          int64_t n_fine, double *out, int64_t ldc, int64_t q_first,
                          int32_t n_qc);
int stk_transfer_restrict_time(void *stream, int64_t M, int32_t a, const double *f,
                               int64_t ld, int64_t k_first, int32_t n_cols, int64_t n_fine,
                               double *out, int64_t ldc, int64_t q_first, int32_t n_qc);

/* ---- plan construction on the host threads: processing order and union pattern ---
 * stk_tile_order: the mesh-tile order of n dofs with coordinates coords [n][d]
 * (d = 2 or 3): the bounding box cut into cubes of edge `side` from the corner `lo`
 * (the caller's choice: source/assembly.py takes about 2 048 dofs per tile), tiles
 * visited lexicographically with the last axis slowest and the dofs of a tile
 * likewise; ties by index.  A performance hint for the gather kernels
 * (stk_kron_*_apply's row_ids): results never depend on it.
 * stk_csr_union_count / _fill: one CSR pattern holding the patterns of n_mats
 * matrices of n rows (each with strictly ascending columns per row), and every
 * matrix's values on it, zeros where it has no entry -- what SumMPI's terms
 * (mpi_kron.py:186-200) become for a fused pass.  _count writes out_indptr [n + 1];
 * the caller allocates out_indices and out_data[k] of out_indptr[n] entries;
 * _fill writes them. */
int stk_tile_order(int64_t n, int32_t d, const double *coords, const double *lo,
                   double side, int32_t *order);
int stk_csr_union_count(int64_t n, int32_t n_mats, const int32_t *const *indptr,
                        const int32_t *const *indices, int32_t *out_indptr);
int stk_csr_union_fill(int64_t n, int32_t n_mats, const int32_t *const *indptr,
                       const int32_t *const *indices, const double *const *data,
                       const int32_t *out_indptr, int32_t *out_indices,
                       double *const *out_data);

#ifdef __cplusplus
}
#endif
#endif /* STK_H */
