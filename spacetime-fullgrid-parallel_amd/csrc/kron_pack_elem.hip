// Element-block Kronecker sums between the node slab and the test-space slab on the PACKED
// slot stream (include/stk.h "test-space slabs", fused forms):
//
//   stk_kron_pack_elem_apply    y_{e,a} = sum_k sum_b blk_k[e][a][b] (X_k x)_{node(e)+b}
//   stk_kron_pack_elem_apply_t  x_n     = sum_k (element n-1, then n) sum_a blk_k[e][a][n-e] (X_k y)_{e,a}
//
// B = B1_t kron M_x + B2_t kron A_x of the serial driver (reference heateq.py:45-54) and its
// transpose, on time slabs, in ONE pass over the plan's slot stream: the walk and the gathers
// are those of kron_pack_kernel (csrc/kron_pack.hip: persistent workgroups on XCD-interleaved
// row groups, one lane per 16-byte pair, all K gathers of a lane back to back, the next group's
// slot words prefetched into registers, the ghost lane on the interleaved ghost array), the
// space-factor sums of a slot row meet in LDS, and only the time stage is new: it reads the
// per-element 2 x 2 blocks (in LDS) instead of three diagonals and writes one 16-byte pair per
// element (forward) or per pair of nodes (transpose) with non-temporal stores.
//
// Every space sum is accumulated in ascending column order from zero with fused multiply-adds
// (as in kron_pack_kernel and in the row engine), and the time stage adds its products in the
// order stk.h writes down for stk_elem_time_apply / _t: the composed path (one stk_ell_spmm
// pass per matrix, then csrc/kron_elem.hip) gives the same doubles.
#include "stk_common.h"

namespace {

constexpr int BS = 512;
constexpr int NT = 2;  // B and B^T have two terms; other sums take the composed path

struct ElemArgs {
    const uint32_t *slots;   // [n_units][K]
    const int32_t *row_ids;  // [n_units][RP] (-1: no row) or NULL (RP = 1, index order)
    const double *dict[NT];  // [n_codes][RP] values of term k's matrix per code
    const double *blk[NT];   // [n_el][2][2]
    const double *x;         // forward: node slab (ld); transpose: test-space slab (2 n_el)
    const double *gh;        // forward: [M][2] interleaved ghost rows or NULL
    double *y;               // forward: test-space slab; transpose: node slab (ld)
    double beta;
    int32_t n_units, n_loc, ld, n_el, first_node;
    int32_t W, R;            // lanes per slot row, slot rows per group
    int32_t ngroups, chunk;  // groups in total / per XCD
    int32_t col_bits, n_codes;
};

typedef double stk_v2d __attribute__((ext_vector_type(2)));

__device__ inline double2 load2(const char *p) { return *reinterpret_cast<const double2 *>(p); }

__device__ inline void store2_nt(double *dst, double v0, double v1)
{
    stk_v2d out;
    out.x = v0, out.y = v1;
    __builtin_nontemporal_store(out, reinterpret_cast<stk_v2d *>(dst));
}

// TRANSPOSED = false: lanes 0 .. P-1 of a slot row own the pairs of nodes (2p, 2p+1), lane P
// the two ghost rows; the space sums land in s_w[k][row][q], q = node + 1 (0: the ghost row
// below, n_loc + 1: the one above); lane p then writes the elements p and p + W.
// TRANSPOSED = true: lane p owns element p (its pair in the test-space slab); the sums land in
// s_w[k][row][2e + a]; lane p < P then writes the nodes 2p and 2p+1.
template <int K, int NPF, int RP, bool TRANSPOSED>
__global__ __launch_bounds__(BS, (K >= 12 || RP > 1) ? 4 : 6) void kron_pack_elem_kernel(const ElemArgs a)
{
    constexpr int KS = (K + 3) & ~3;  // LDS stride of a row's slots (16-byte vectors)
    extern __shared__ double sm[];
    const int W = a.W, R = a.R;
    const int SW = TRANSPOSED ? 2 * a.n_el + 2 : a.n_loc + 3;
    uint32_t *s_slot = reinterpret_cast<uint32_t *>(sm);            // [R][KS]
    int32_t *s_row = reinterpret_cast<int32_t *>(s_slot + R * KS);  // [R][RP]
    double *s_blk = reinterpret_cast<double *>(s_row + ((R * RP + 3) & ~3));  // [NT][4][n_el]
    double *s_dict = s_blk + NT * 4 * a.n_el;                        // [n_codes][RP][NT]
    double *s_w = s_dict + a.n_codes * RP * NT;                      // [NT][R * RP][SW]

    const int tid = threadIdx.x;
    const int r = tid / W;
    const int p = tid - r * W;
    const bool in_row = r < R;
    const int P = (a.n_loc + 1) / 2;
    const bool ghost_lane = !TRANSPOSED && p == P;
    // a lane without an element (transpose) or without ghost rows (forward) gathers nothing
    const bool gathers = TRANSPOSED ? p < a.n_el : !(ghost_lane && a.gh == nullptr);
    const int t0 = 2 * p;
    // what distinguishes the lanes of a row: where their 16 bytes of a column start
    const char *base_lane = ghost_lane ? reinterpret_cast<const char *>(a.gh)
                                       : reinterpret_cast<const char *>(a.x) + (size_t)t0 * 8;
    const uint32_t stride_lane = ghost_lane ? 16u : (uint32_t)(TRANSPOSED ? 2 * a.n_el : a.ld) * 8u;
    const uint32_t col_mask = (1u << a.col_bits) - 1u;
    // where a lane leaves its two sums in s_w
    const int wq0 = TRANSPOSED ? t0 : (ghost_lane ? 0 : t0 + 1);
    const int wdq = (!TRANSPOSED && ghost_lane) ? a.n_loc + 1 : 1;
    const bool wr1 = TRANSPOSED || ghost_lane || t0 + 1 < a.n_loc;  // a padding step is not a node

    for (int i = tid; i < a.n_codes * RP * NT; i += BS) {
        const int c = i / NT, k = i - c * NT;  // c = code * RP + row of the pair
        s_dict[i] = a.dict[k][c];
    }
    // the blocks component by component, s_blk[(k * 4 + c) * n_el + e], c = 2 a + b: lanes that
    // work on consecutive elements read consecutive doubles
    for (int i = tid; i < NT * 4 * a.n_el; i += BS) {
        const int k = i / (4 * a.n_el), rem = i - k * 4 * a.n_el;
        const int c = rem / a.n_el, e = rem - c * a.n_el;
        s_blk[i] = a.blk[k][4 * e + c];
    }

    // groups of this workgroup: interleaved with the other workgroups of its XCD
    const int xcd = blockIdx.x & 7;
    const int step = gridDim.x >> 3;
    const int gend = min((xcd + 1) * a.chunk, a.ngroups);
    int g = xcd * a.chunk + (int)(blockIdx.x >> 3);

    uint32_t pslot[NPF];
    int32_t prow = 0;
#pragma unroll
    for (int q = 0; q < NPF; ++q) pslot[q] = 0;
    auto fetch = [&](int gq) {
        const int rows = min(R, a.n_units - gq * R);
        const uint32_t *src = a.slots + (size_t)gq * R * K;
#pragma unroll
        for (int q = 0; q < NPF; ++q) {
            const int i = tid + q * BS;
            if (i < rows * K) pslot[q] = __builtin_nontemporal_load(src + i);
        }
        if (tid < rows * RP) prow = a.row_ids ? a.row_ids[(size_t)gq * R * RP + tid] : gq * R + tid;
    };
    if (g < gend) fetch(g);

    for (; g < gend; g += step) {
        const int rows = min(R, a.n_units - g * R);
        // ---- publish this group's entries ----------------------------------
#pragma unroll
        for (int q = 0; q < NPF; ++q) {
            const int i = tid + q * BS;
            if (i < rows * K) s_slot[i + (i / K) * (KS - K)] = pslot[q];
        }
        if (tid < rows * RP) s_row[tid] = prow;
        __syncthreads();
        if (g + step < gend) fetch(g + step);  // in flight behind the gathers

        const bool active = in_row && r < rows;
        int32_t yrow[RP];
#pragma unroll
        for (int j = 0; j < RP; ++j) yrow[j] = active ? s_row[r * RP + j] : -1;

        if (active && gathers) {
            double acc0[RP][NT], acc1[RP][NT];
#pragma unroll
            for (int j = 0; j < RP; ++j)
#pragma unroll
                for (int k = 0; k < NT; ++k) acc0[j][k] = acc1[j][k] = 0.0;
            int ro = r * KS;
            double2 xv[K];
            {
                uint32_t sl[KS];
                const uint4 *so = reinterpret_cast<const uint4 *>(s_slot + ro);
#pragma unroll
                for (int u = 0; u < KS / 4; ++u) {
                    const uint4 v = so[u];
                    sl[4 * u] = v.x, sl[4 * u + 1] = v.y, sl[4 * u + 2] = v.z, sl[4 * u + 3] = v.w;
                }
#pragma unroll
                for (int u = 0; u < K; ++u) xv[u] = load2(base_lane + (size_t)(sl[u] & col_mask) * stride_lane);
            }
            // the slot words are read a second time for their codes rather than kept in
            // registers across the gathers (kron_pack_kernel: 8 VGPRs less while the loads fly)
            asm volatile("" : "+v"(ro));
            uint32_t sl[KS];
            const uint4 *so = reinterpret_cast<const uint4 *>(s_slot + ro);
#pragma unroll
            for (int u = 0; u < KS / 4; ++u) {
                const uint4 v = so[u];
                sl[4 * u] = v.x, sl[4 * u + 1] = v.y, sl[4 * u + 2] = v.z, sl[4 * u + 3] = v.w;
            }
#pragma unroll
            for (int u = 0; u < K; ++u) {
                const double *dv = s_dict + (sl[u] >> a.col_bits) * (RP * NT);
#pragma unroll
                for (int j = 0; j < RP; ++j, dv += NT) {
                    const double2 vv = *reinterpret_cast<const double2 *>(dv);  // NT = 2
                    acc0[j][0] = fma(vv.x, xv[u].x, acc0[j][0]);
                    acc1[j][0] = fma(vv.x, xv[u].y, acc1[j][0]);
                    acc0[j][1] = fma(vv.y, xv[u].x, acc0[j][1]);
                    acc1[j][1] = fma(vv.y, xv[u].y, acc1[j][1]);
                }
            }
#pragma unroll
            for (int j = 0; j < RP; ++j) {
                double *w = s_w + (r * RP + j) * SW + wq0;
#pragma unroll
                for (int k = 0; k < NT; ++k, w += R * RP * SW) {
                    w[0] = acc0[j][k];
                    if (wr1) w[wdq] = acc1[j][k];
                }
            }
        }
        __syncthreads();

        // ---- time stage: the element blocks on the sums in LDS, store -----------------
        if (active) {
#pragma unroll
            for (int j = 0; j < RP; ++j) {
                if (RP > 1 && yrow[j] < 0) continue;  // a slot row that serves one matrix row only
                const double *w0 = s_w + (r * RP + j) * SW;
                if constexpr (!TRANSPOSED) {
                    double *dst_row = a.y + (size_t)(uint32_t)yrow[j] * ((size_t)2 * a.n_el);
                    // elements p and p + W: the lanes of a row store one contiguous run per turn
                    for (int e = p; e < a.n_el; e += W) {
                        const int q0 = a.first_node + e + 1;
                        double v0 = 0.0, v1 = 0.0;
#pragma unroll
                        for (int k = 0; k < NT; ++k) {
                            const double *w = w0 + k * R * RP * SW;
                            const double *b = s_blk + k * 4 * a.n_el + e;
                            const double z0 = w[q0], z1 = w[q0 + 1];
                            v0 = fma(b[a.n_el], z1, fma(b[0], z0, v0));
                            v1 = fma(b[3 * a.n_el], z1, fma(b[2 * a.n_el], z0, v1));
                        }
                        double *dst = dst_row + 2 * e;
                        if (a.beta != 0.0) {
                            const double2 old = *reinterpret_cast<const double2 *>(dst);
                            v0 = fma(a.beta, old.x, v0);
                            v1 = fma(a.beta, old.y, v1);
                        }
                        store2_nt(dst, v0, v1);
                    }
                } else if (p < P) {
                    double out[2] = {0.0, 0.0};
                    for (int n = t0; n < min(t0 + 2, a.n_loc); ++n) {
                        const int e_left = n - a.first_node - 1, e_right = e_left + 1;
                        double acc = 0.0;
#pragma unroll
                        for (int k = 0; k < NT; ++k) {
                            const double *w = w0 + k * R * RP * SW;
                            // (a range shorter than the slab: the nodes behind it have no element)
                            if (e_left >= 0 && e_left < a.n_el) {  // this node is the element's second one
                                const double *b = s_blk + k * 4 * a.n_el + e_left;
                                acc = fma(b[3 * a.n_el], w[2 * e_left + 1], fma(b[a.n_el], w[2 * e_left], acc));
                            }
                            if (e_right < a.n_el) {  // ... its first one
                                const double *b = s_blk + k * 4 * a.n_el + e_right;
                                acc = fma(b[2 * a.n_el], w[2 * e_right + 1], fma(b[0], w[2 * e_right], acc));
                            }
                        }
                        out[n - t0] = acc;
                    }
                    double *dst = a.y + (size_t)(uint32_t)yrow[j] * (size_t)a.ld + t0;
                    if (a.beta != 0.0) {
                        const double2 old = *reinterpret_cast<const double2 *>(dst);
                        out[0] = fma(a.beta, old.x, out[0]);
                        if (t0 + 1 < a.n_loc) out[1] = fma(a.beta, old.y, out[1]);  // the padding column stays zero
                    }
                    store2_nt(dst, out[0], out[1]);
                }
            }
        }
        // s_w is rewritten after the next group's first barrier, s_slot / s_row before it:
        // every wave has passed the barrier above, i.e. finished its gathers and read its rows
    }
}

// LDS of a workgroup that serves R slot rows at a time: the slot words and row numbers of the
// group, ALL element blocks of the slab, the dictionary, and the space sums of the group's rows
size_t elem_lds_bytes(int K, int RP, int n_codes, int n_el, int n_loc, bool transposed, int R)
{
    const int KS = (K + 3) & ~3;
    const int SW = transposed ? 2 * n_el + 2 : n_loc + 3;
    return sizeof(double) * ((size_t)NT * R * RP * SW + (size_t)n_codes * RP * NT + (size_t)NT * 4 * n_el) +
           sizeof(uint32_t) * ((size_t)R * KS + (size_t)((R * RP + 3) & ~3)) + 32;
}

int elem_lanes(int n_el, int n_loc, bool transposed)
{
    const int P = (n_loc + 1) / 2;
    return transposed ? (n_el > P ? n_el : P) : P + 1;
}

template <int K, int RP, bool TRANSPOSED>
int launch_npf(hipStream_t st, const ElemArgs &a, unsigned grid, size_t lds)
{
    const int npf = (a.R * K + BS - 1) / BS;
    if (npf <= 1)
        hipLaunchKernelGGL((kron_pack_elem_kernel<K, 1, RP, TRANSPOSED>), dim3(grid), dim3(BS), lds, st, a);
    else if (npf <= 2)
        hipLaunchKernelGGL((kron_pack_elem_kernel<K, 2, RP, TRANSPOSED>), dim3(grid), dim3(BS), lds, st, a);
    else
        hipLaunchKernelGGL((kron_pack_elem_kernel<K, 4, RP, TRANSPOSED>), dim3(grid), dim3(BS), lds, st, a);
    STK_LAUNCH_CHECK();
    return 0;
}

template <int RP, bool TRANSPOSED>
int launch(hipStream_t st, ElemArgs a, int K, const char *who)
{
    a.W = elem_lanes(a.n_el, a.n_loc, TRANSPOSED);
    STK_REQUIRE(a.W <= BS, "%s: a slab of %d nodes and %d elements needs %d lanes per row (at most %d)", who, a.n_loc,
                a.n_el, a.W, BS);
    a.R = BS / a.W;
    if (a.R * K > 4 * BS) a.R = 4 * BS / K;  // at most 4 prefetched words per thread
    auto lds_of = [&](int R) { return elem_lds_bytes(K, RP, a.n_codes, a.n_el, a.n_loc, TRANSPOSED, R); };
    while (a.R > 1 && lds_of(a.R) > 64 * 1024) --a.R;
    const size_t lds = lds_of(a.R);
    STK_REQUIRE(lds <= 64 * 1024, "%s: %zu bytes of LDS per workgroup for one slot row (stk_kron_pack_elem_lds_bytes)", who, lds);
    a.ngroups = (a.n_units + a.R - 1) / a.R;
    a.chunk = (a.ngroups + 7) / 8;
    const int n_cu = stk_cu_count();
    int per_cu = (K >= 12 || RP > 1) ? 2 : 3;
    const int by_lds = (int)(160 * 1024 / (lds + 256));
    if (per_cu > by_lds) per_cu = by_lds > 0 ? by_lds : 1;
    int per_xcd = (n_cu / 8) * per_cu;
    if (per_xcd > a.chunk) per_xcd = a.chunk;
    if (per_xcd < 1) per_xcd = 1;
    const unsigned grid = (unsigned)per_xcd * 8;
#define STK_ELEM_CASE(KK) \
    case KK:              \
        return launch_npf<KK, RP, TRANSPOSED>(st, a, grid, lds);
    if constexpr (RP == 1) {
        switch (K) {
            STK_ELEM_CASE(5)
            STK_ELEM_CASE(7)
            STK_ELEM_CASE(9)
            STK_ELEM_CASE(12)
            STK_ELEM_CASE(16)
        }
        stk_set_error("%s: K=%d is not one of 5, 7, 9, 12, 16", who, K);
    } else {
        switch (K) {
            STK_ELEM_CASE(8)
            STK_ELEM_CASE(10)
            STK_ELEM_CASE(12)
        }
        stk_set_error("%s: K=%d is not one of 8, 10, 12 (row pairs)", who, K);
    }
#undef STK_ELEM_CASE
    return 2;
}

template <bool TRANSPOSED>
int elem_apply(const char *who, void *stream, const stk_pack_pattern *pat, int32_t n_el, int32_t n_loc, int32_t ld,
               int32_t first_node, int32_t n_terms, const stk_kron_pack_term *t, const double *const *blocks_host,
               const double *x, const double *ghosts, double beta, double *y)
{
    const stk_timed timed_(STK_OP_KRON, stream);
    STK_REQUIRE(pat && t && blocks_host && x && y, "%s: null pointer", who);
    STK_REQUIRE(n_terms == NT, "%s: %d terms (the fused form has %d; other sums take the composed path)", who, n_terms, NT);
    STK_REQUIRE(pat->M > 0 && pat->slots && pat->dict && !pat->vals,
                "%s: the pattern must have a dictionary (explicit values take the composed path)", who);
    STK_REQUIRE(pat->rows_per_unit == 1 || pat->rows_per_unit == 2, "%s: rows_per_unit=%d is not 1 or 2", who,
                pat->rows_per_unit);
    STK_REQUIRE(pat->n_units > 0 && (int64_t)pat->n_units * pat->rows_per_unit >= pat->M &&
                    (pat->rows_per_unit == 1 ? pat->n_units == pat->M : pat->row_ids != nullptr),
                "%s: %d slot rows of %d matrix rows each do not cover M=%d", who, pat->n_units, pat->rows_per_unit, pat->M);
    STK_REQUIRE(pat->col_bits >= 1 && pat->col_bits <= 31 && ((int64_t)1 << pat->col_bits) >= pat->M,
                "%s: col_bits=%d cannot address %d columns", who, pat->col_bits, pat->M);
    STK_REQUIRE(pat->n_codes >= 1 && (int64_t)pat->n_codes <= ((int64_t)1 << (32 - pat->col_bits)),
                "%s: %d codes do not fit %d bits", who, pat->n_codes, 32 - pat->col_bits);
    STK_REQUIRE(n_loc > 0 && n_el > 0 && ld >= n_loc && (ld & 1) == 0, "%s: bad sizes n_loc=%d n_el=%d ld=%d (ld must be even)",
                who, n_loc, n_el, ld);
    STK_REQUIRE((first_node == 0 || first_node == -1) && first_node + n_el <= n_loc,
                "%s: elements from node %d, %d of them, on %d local nodes", who, first_node, n_el, n_loc);
    const bool reads_ghosts = first_node < 0 || first_node + n_el == n_loc;
    STK_REQUIRE(TRANSPOSED || !reads_ghosts || ghosts, "%s: an element reaches a ghost row and there is no ghost pair", who);
    STK_REQUIRE(x != y, "%s: input aliases output", who);
    STK_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)ghosts) & 15) == 0, "%s: x, y and ghosts must be 16-byte aligned", who);
    ElemArgs a;
    a.slots = pat->slots, a.row_ids = pat->row_ids;
    for (int k = 0; k < NT; ++k) {
        STK_REQUIRE(t[k].mat >= 0 && t[k].mat < pat->n_mats && blocks_host[k], "%s: term %d: matrix %d of %d, or no blocks",
                    who, k, t[k].mat, pat->n_mats);
        a.dict[k] = pat->dict + (size_t)t[k].mat * pat->n_codes * pat->rows_per_unit;
        a.blk[k] = blocks_host[k];
    }
    a.x = x, a.gh = TRANSPOSED ? nullptr : ghosts, a.y = y, a.beta = beta;
    a.n_units = pat->n_units, a.n_loc = n_loc, a.ld = ld, a.n_el = n_el, a.first_node = first_node;
    a.col_bits = pat->col_bits, a.n_codes = pat->n_codes;
    hipStream_t st = stk_stream(stream);
    return pat->rows_per_unit == 2 ? launch<2, TRANSPOSED>(st, a, pat->K, who) : launch<1, TRANSPOSED>(st, a, pat->K, who);
}

}  // namespace

extern "C" int64_t stk_kron_pack_elem_lds_bytes(const stk_pack_pattern *pat, int32_t n_el, int32_t n_loc,
                                                int32_t transposed)
{
    if (!pat || n_el < 1 || n_loc < 1 || pat->n_codes < 1 || (pat->rows_per_unit != 1 && pat->rows_per_unit != 2))
        return -1;
    if (elem_lanes(n_el, n_loc, transposed != 0) > BS) return -1;
    return (int64_t)elem_lds_bytes(pat->K, pat->rows_per_unit, pat->n_codes, n_el, n_loc, transposed != 0, 1);
}

extern "C" int stk_kron_pack_elem_apply(void *stream, const stk_pack_pattern *pat, int32_t n_el, int32_t n_loc,
                                        int32_t ld, int32_t first_node, int32_t n_terms, const stk_kron_pack_term *t,
                                        const double *const *blocks_host, const double *x, const double *ghosts,
                                        double beta, double *y)
{
    return elem_apply<false>("stk_kron_pack_elem_apply", stream, pat, n_el, n_loc, ld, first_node, n_terms, t,
                             blocks_host, x, ghosts, beta, y);
}

extern "C" int stk_kron_pack_elem_apply_t(void *stream, const stk_pack_pattern *pat, int32_t n_el, int32_t n_loc,
                                          int32_t ld, int32_t first_node, int32_t n_terms,
                                          const stk_kron_pack_term *t, const double *const *blocks_host,
                                          const double *y_in, double beta, double *x_out)
{
    return elem_apply<true>("stk_kron_pack_elem_apply_t", stream, pat, n_el, n_loc, ld, first_node, n_terms, t,
                            blocks_host, y_in, nullptr, beta, x_out);
}
