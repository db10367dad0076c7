// amg.hip — smoothed-aggregation multigrid for matrices on a dxo_csr pattern (dxo_amg_*), the preconditioner DXO_PC_AMG of
// dxo_krylov_gmres / dxo_krylov_cg.
//
// Symbolic phase (dxo_amg_create, host C++ once per pattern): the node graph of the block pattern, aggregates in three passes in
// ascending node order, and per level the block patterns of P (node -> the aggregates of its neighbours), of A P, of the coarse matrix
// P^T A P as a dxo_csr without a mesh, and the transposed incidence of P. Every level keeps the block size of the fine matrix.
//
// Numeric phase (dxo_amg_setup, every time the values change): per level the block-Jacobi inverses (the kernel of
// dxo_csr_block_jacobi), rho = |Dinv A|_inf by one pass over the matrix and a max-reduction, omega = (4/3) / rho kept on the device,
// P = T - omega Dinv A T (one thread per block of P), A P (one thread per block: the neighbours j of its node in ascending order, the
// block of P in row j found by search), P^T (A P) (one thread per coarse block: the blocks of P in its column in ascending fine-node
// order, the block of A P in that row found by search). The source blocks of a sum are not stored as lists: they are found in the
// same fixed ascending order from the patterns, which keeps the tables at the size of the patterns themselves. The coarsest matrix is
// expanded to dense [A | I] and inverted by Gauss-Jordan with partial pivoting, one launch per pivot, out of place between two
// buffers (every workgroup finds the pivot of the step itself, so a step needs no grid-wide wait). No atomics: a setup is
// bit-reproducible. The host waits once, at the end, for one flag word.
//
// Apply (dxo_amg_cycle): per level x = omega Dinv r (amg_first_step), then x <- x + omega Dinv (r - A x) with A x by the row_product of
// krylov_internal.h, which csr_spmv is made of too (LW lanes own a node, fixed xor-butterfly), and the update in the epilogue,
// t = r - A x by the same kernel, r_c = P^T t gathered through the
// transposed incidence in ascending fine-node order, x += P x_c, the same sweeps again; the coarsest level is one dense product.
//
// With a near-null space (dxo_amg_create_nns: B [n_rows][k], the rigid-body modes of dxo_rigid_body_modes, k = 3 for bs 2 and 6 for
// bs 3) the tentative prolongator is not an identity per node: at creation, as soon as a level has its aggregates, amg_tentative
// orthonormalises the rows of B of every aggregate (ascending node order; Gram-Schmidt in column order with a second pass; a lane group owns an aggregate, column
// products by the xor-butterfly), keeps the Q factors as the blocks of T ([n_nodes][bs_l][k]) and the R factors as the B of the next
// level. A column that keeps no more than rank_tol of its norm is dead: its Q column and its row of the next B are zero, so it stays out
// on every coarser level and its coarse diagonal entry, exactly zero, becomes 1. Every coarse level then has block size k; the kernels
// of P, A P, P^T A P, restriction and prolongation take <BSR, BSC> (rows of the level, rows of the next), and the levels of block
// size 6 invert their diagonal blocks by the kernel and the invert_block of the others (there: Gauss-Jordan with partial pivoting in
// registers, rows exchanged by compare-and-select).
// T and B depend on B_0, the aggregates and the constraints alone: dxo_amg_setup does not touch them.
//
// The relaxation (dxo_amg_set_smoother; the default is what is described above). rho from the power iteration: amg_power_init writes
// the fixed start vector, amg_power_step forms w = Dinv (A (s v)) by row_product together with the workgroup's partial of
// |w|^2, and the one-workgroup amg_power_norm adds the partials in a fixed order and leaves s = 1 / |w| on the device for the next step;
// after the last step it stores rho = safety |w|, omega = (4/3) / rho and the level's Chebyshev pairs. The vectors are xa and xb of the
// level, free during a setup; the setup still waits once, at its end. Chebyshev smoothing: amg_first_step with the first c2 (the step
// from x = 0, no SpMV, d = x) and amg_cheby_sweep (d = c1 d + c2 Dinv (r - A x), x_out = x + d; d in place, x between xa and xb as the Jacobi sweeps) with
// the pairs (c1, c2) read from the device like omega; the post-smoothing is the same polynomial started from the corrected x.
//
// Strength of connection (dxo_amg_create_soc with theta > 0). Block (i, j) is strong when |A_ij|_F^2 >= theta^2 |A_ii|_F |A_jj|_F or
// the same holds for (j, i): amg_diag_norm writes |A_ii|_F per node, amg_strength (a lane group per node, a lane per block, the
// transposed block found by search) one byte per block; both square entries scaled by a power of two, so the mask does not depend on
// the scale of the matrix (see there). Creation then interleaves with the numeric phase level by level: the mask of
// level l comes to the host, the aggregates are made on the strong graph, P gets the pattern (strong graph) x (aggregates) while A P
// and P^T A P keep the full graph, and the numeric kernels of level l give the matrix of level l + 1 for the next mask (one wait per
// level, at creation only; the relaxation is the default one there). The masks are frozen: dxo_amg_setup reuses them. The
// prolongator is smoothed with the filtered matrix A^F (weak blocks added onto the diagonal block of their row, never stored):
// amg_lump forms the lumped diagonal blocks and their inverses dinv_f (a block that fails the test of invert_block: the inverse of
// A_ii, counted; a node without a strong neighbour: zero, its row of P is its row of T), amg_rho / amg_power_step estimate the rho_F
// of Dinv_F A^F given the mask, omega_F = (4/3) / rho_F, and amg_build_p skips the weak blocks (all three through amg_filtered_block).
// The sweeps keep A, Dinv and rho.
//
// The K-cycle (dxo_amg_set_cycle with DXO_AMG_CYCLE_K). The cycle is a recursion over the cycle body B_l of a level (pre-smoothing,
// restriction, the solve of the next level, prolongation, post-smoothing: amg_body). The V-cycle solves the next level by its body, once.
// The K-cycle solves every intermediate level l (1 <= l <= levels - 2) by two GCR steps preconditioned with B_l (amg_solve_level):
// c1 = B_l(r), v1 = A_l c1 (the SpMV of krylov.hip), the partials of (v1, v1) and (v1, r) in one pass (amg_k_dots, a fixed grid per
// level), a one-workgroup kernel that adds them in a fixed order and leaves a1 / rho1 on the device (amg_k_scalar),
// r1 = r - (a1 / rho1) v1 (amg_k_residual), c2 = B_l(r1), v2 = A_l c2, the partials of (v2, v2), (v2, v1), (v2, r1), the two
// coefficients of x with their guards (rho1 == 0: x = 0; rho2 not finite or <= 1e-14 (v2, v2): x = (a1 / rho1) c1) and
// x = co1 c1 + co2 c2 (amg_k_combine). Both steps always run: no host read, no skipped launch, so an apply stays capture-safe and
// bit-reproducible. The two calls of B_l share xa, xb, t, d of the level and everything below it, so B_l writes its result straight
// into c1 (then c2) of the level's K vectors, which nothing else touches. Level 0 runs B_0 alone: the Krylov method is its acceleration.
//
// Single precision (dxo_amg_set_precision with DXO_AMG_PRECISION_FP32). The numeric phase above stays double to its end; a setup then
// casts the values, Dinv and P of every level but the coarsest to float (amg_narrow, one launch per array, before the one wait; a
// finite entry that overflows raises flag[2]). The kernels of the cycle take their scalar as a template parameter, and so does
// row_product: the float cycle is the launch sequence of the V-cycle on the copies (level_view picks the arrays), with float
// vectors and v_fma_f32 in the same order. omega and the Chebyshev pairs are read as double and narrowed in the kernel, and the dense
// inverse of the coarsest level stays double (amg_dense_apply widens its right-hand side). r and z stay double: one amg_narrow of r
// on entry (12 B per row, repaid by the 2 nu + 1 kernels of level 0 that then read 4 B of r per row instead of 8), and the last
// post-sweep of level 0 writes z in double (its TO). The K-cycle stays double: the two settings exclude each other.
//
// A given first transfer (dxo_amg_create_transfer; quadratic elements). The prolongator of level 0 is a nodal interpolation the caller
// hands over, P = W (x) I_bs without the constrained dofs, instead of a smoothed aggregation: level 1 is then the degree-1 space on the
// same cells. Its blocks are diagonal, so they are kept as p_diag [p_blocks][bs] (filled on the host at creation from W and the two
// constraint masks; frozen), the symbolic tables come from transfer_tables on the given rows of P, and the numeric phase of level 0
// is the block inverses, rho and omega for its sweeps, then amg_build_ap_w / amg_build_c_w (the kernels of A P and P^T (A P) with a
// column and a row scaling in place of the block products): no amg_build_p, no mask kernels. Level 1 is a finest level in all but
// where its matrix comes from: its mask is the constraints of the nodes coarse_to_fine, nodes with every dof constrained join no
// aggregate, its B is the rows of the zeroed B_0 at those nodes (amg_gather_b), and strength of connection starts there. The cycle
// of level 0 restricts and prolongs with amg_restrict_w / amg_prolong_w, one thread per dof (8 or 4 bytes of P per dof and block where
// the block form reads bs^2 values; consecutive lanes read consecutive entries of the vectors).
//
// Host side. Run-time shapes reach the templates through one dispatcher (with_int and with_bs of krylov_internal.h, with_pairs here,
// and their named lists: with_level, with_pair, with_square, with_nns_pair), so a kernel's argument list is written once. amg_build allocates the device scalars
// of every level once, before the level loop, and walks read pattern -> [strength mask] -> aggregates -> transfer tables -> coarse
// level -> [T and B] -> [numeric phase] per level, the bracketed stages on the hierarchies that have them.
#include "krylov_internal.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#ifndef DXO_AMG_BLOCK
#define DXO_AMG_BLOCK 256
#endif

namespace {

constexpr int64_t AMG_MAX_DENSE = 4096;
constexpr int AMG_MAX_DEGREE = 8;
constexpr int AMG_CHEB_STRIDE = 2 * AMG_MAX_DEGREE;

struct amg_level {
    const dxo_csr* A = nullptr;        // pattern (level 0: the caller's, coarser: own)
    dxo_csr* own = nullptr;
    int bs = 0, bsc = 0;               // block size of this level and of the next (equal without a near-null space)
    int64_t n_nodes = 0, n_rows = 0, nnzb = 0;
    int lw = 8;                        // lanes per node of the sweeps
    const double* values = nullptr;    // level 0: the pointer of the last setup
    double* dinv = nullptr;            // [n_nodes][bs][bs]
    uint8_t* mask = nullptr;           // [n_rows] 1: the dof's row of T is zero
    // transfer to the next level (absent on the coarsest)
    int64_t n_agg = 0, p_blocks = 0, ap_blocks = 0, c_blocks = 0;
    int32_t* agg = nullptr;            // [n_nodes]
    int64_t* p_ptr = nullptr;          // [n_nodes + 1]
    int32_t *p_col = nullptr, *p_row = nullptr;
    double* p_val = nullptr;           // [p_blocks][bs][bs]
    int64_t *pt_ptr = nullptr, *pt_blk = nullptr;     // column a of P: its blocks, ascending fine node
    int64_t* ap_ptr = nullptr;
    int32_t *ap_col = nullptr, *ap_row = nullptr;
    double* ap_val = nullptr;
    int64_t* c_bptr = nullptr;         // [n_agg + 1] first block of a coarse node
    int32_t* c_row = nullptr;          // [c_blocks] coarse node of a block
    // vectors [n_rows]
    double *r = nullptr, *xa = nullptr, *xb = nullptr, *t = nullptr;
    double* d = nullptr;               // the Chebyshev direction (absent on the coarsest)
    // the K-cycle (dxo_amg_set_cycle; intermediate levels only): [n_rows] each, the partials [3][knb] and the coefficients
    double *kc1 = nullptr, *kv1 = nullptr, *kc2 = nullptr, *kv2 = nullptr, *kr1 = nullptr;
    double *kpart = nullptr, *kco = nullptr;
    int knb = 0;                       // workgroups of amg_k_dots on this level = partials per product
    // near-null space path only
    double* b_val = nullptr;           // [n_rows][k] B of this level
    double* t_val = nullptr;           // [n_nodes][bs][k] blocks of T (absent on the coarsest)
    int64_t* agg_ptr = nullptr;        // [n_agg + 1] the nodes of an aggregate ...
    int32_t* agg_node = nullptr;       // ... ascending
    uint8_t* dead_a = nullptr;         // [n_agg] dead columns of an aggregate
    int tl = 8;                        // lanes per aggregate of amg_tentative
    int64_t dead = 0;                  // dead columns of T (host, after creation)
    // strength of connection only (absent on the coarsest level)
    uint8_t* strong = nullptr;         // [nnzb] 1: a strong block, in the order of the block pattern; frozen at creation
    double* diag_f = nullptr;          // [n_nodes][bs][bs] the diagonal blocks of the filtered matrix
    double* dinv_f = nullptr;          // [n_nodes][bs][bs] their inverses (A_ii's after a failed test; zero: the node is not smoothed)
    uint8_t* unlumped = nullptr;       // [n_nodes] 1: the lumped block failed the test
    int64_t n_strong = 0;              // strong blocks (host)
    // single precision (dxo_amg_set_precision): the copies a setup casts (absent on the coarsest level) and the cycle's vectors
    float *values32 = nullptr, *dinv32 = nullptr, *p_val32 = nullptr;
    float *r32 = nullptr, *xa32 = nullptr, *xb32 = nullptr, *t32 = nullptr, *d32 = nullptr;
    // a given nodal transfer (dxo_amg_create_transfer; level 0 only): P = W (x) I_bs without the constrained dofs, kept as the
    // diagonals of its blocks. p_val, agg and the near-null-space and strength arrays of the level are absent then
    double* p_diag = nullptr;          // [p_blocks][bs], frozen at creation
    float* p_diag32 = nullptr;
    int32_t* ctf = nullptr;            // [n_agg] the node of this level a node of the next one is
};

// what the cycle reads and writes on a level, in the scalar T of the cycle
template <class T>
struct level_view;

template <>
struct level_view<double> {
    const double *values, *dinv, *p_val, *p_diag;
    double *r, *xa, *xb, *t, *d;
    explicit level_view(const amg_level& v)
        : values(v.values), dinv(v.dinv), p_val(v.p_val), p_diag(v.p_diag), r(v.r), xa(v.xa), xb(v.xb), t(v.t), d(v.d) {}
};

template <>
struct level_view<float> {
    const float *values, *dinv, *p_val, *p_diag;
    float *r, *xa, *xb, *t, *d;
    explicit level_view(const amg_level& v)
        : values(v.values32), dinv(v.dinv32), p_val(v.p_val32), p_diag(v.p_diag32), r(v.r32), xa(v.xa32), xb(v.xb32), t(v.t32), d(v.d32) {}
};

}  // namespace

struct dxo_amg {
    int device = 0, bs = 0, sweeps = 1;
    std::vector<amg_level> L;
    std::vector<void*> allocs;         // everything hipMalloc'ed here
    double* omega = nullptr;           // [levels]
    double* part = nullptr;            // partial maxima of the rho pass
    int64_t part_cap = 0;
    int* flag = nullptr;               // [0] singular diagonal block, [1] zero pivot, [2] 1 + the first level a cast overflowed on
    double* dense[2] = {nullptr, nullptr};   // [nc][2 nc] each: [W | B], B ends as the inverse
    int64_t nc = 0;                    // rows of the coarsest level
    bool ready = false;
    double build_ms = 0.0, complexity = 1.0;
    int k = 0;                         // columns of the near-null space; 0: none (an identity per node)
    // the relaxation (dxo_amg_set_smoother)
    int smooth_kind = DXO_AMG_SMOOTH_JACOBI, degree = 1, rho_kind = DXO_AMG_RHO_INF_NORM, rho_iters = 10;
    double lower = 0.1, safety = 1.1;
    double* rho = nullptr;             // [levels] the estimate omega was made from
    double* cheb = nullptr;            // [levels][AMG_CHEB_STRIDE] the pairs (c1, c2) of the Chebyshev steps
    double* scal = nullptr;            // power iteration: [0] 1 / |w|, the scale of the next step, [1] |w|
    // strength of connection (dxo_amg_create_soc with theta > 0)
    double theta = 0.0;
    double* omega_f = nullptr;         // [levels] omega of the filtered prolongator smoothing
    double* rho_f = nullptr;           // [levels] the estimate of Dinv_F A^F it was made from
    double* cheb_f = nullptr;          // [AMG_CHEB_STRIDE] where amg_power_norm leaves the pairs of rho_F: not used
    int cycle = DXO_AMG_CYCLE_V;       // dxo_amg_set_cycle
    int precision = DXO_AMG_PRECISION_FP64;      // dxo_amg_set_precision
    int64_t fp32_bytes = 0;            // of the single-precision copies and vectors; 0: never allocated
};

namespace {

// ---- device helpers
// position of v in the ascending run col[lo, hi), or -1
__device__ __forceinline__ int64_t amg_find(const int32_t* __restrict__ col, int64_t lo, int64_t hi, int32_t v) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t c = col[mid];
        if (c < v) lo = mid + 1;
        else if (c > v) hi = mid;
        else return mid;
    }
    return -1;
}

// block k of a node's row in the matrix the prolongator is smoothed with. Without a mask (strong == nullptr) that is A: the stored
// block. With one it is the filtered matrix A^F: false for a weak block (skip it), and the diagonal block (`diagonal`, looked at only
// with a mask) is the lumped one, diag_f[node] with leading dimension BS
template <int BS>
__device__ __forceinline__ bool amg_filtered_block(const NodeRow<BS>& R, int k, int64_t node, bool diagonal, const double* __restrict__ values,
                                                   const uint8_t* __restrict__ strong, const double* __restrict__ diag_f, const double*& ab,
                                                   int64_t& ld) {
    ab = values + R.r0 + (int64_t)k * BS;
    ld = R.len;
    if (strong) {
        if (!strong[R.r0 / (BS * BS) + k]) return false;
        if (diagonal) {
            ab = diag_f + node * BS * BS;
            ld = BS;
        }
    }
    return true;
}

// ---- numeric phase
// part[block] = max over the block's nodes of the absolute row sums of Dinv A; with `strong`, of Dinv_F A^F (dinv is then dinv_f)
template <int BS, int LW>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_rho(int64_t n_nodes, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                         const double* __restrict__ values, const double* __restrict__ dinv,
                                                         const uint8_t* __restrict__ strong, const double* __restrict__ diag_f,
                                                         double* __restrict__ part) {
    __shared__ double lds[DXO_AMG_BLOCK / 64];
    constexpr int NPB = DXO_AMG_BLOCK / LW;
    const int64_t node = (int64_t)blockIdx.x * NPB + threadIdx.x / LW;
    const int lane = threadIdx.x % LW;
    double acc[BS];
#pragma unroll
    for (int i = 0; i < BS; ++i) acc[i] = 0.0;
    if (node < n_nodes) {
        const NodeRow<BS> R(row_ptr, node);
        double D[BS][BS];
#pragma unroll
        for (int i = 0; i < BS; ++i)
#pragma unroll
            for (int j = 0; j < BS; ++j) D[i][j] = dinv[node * BS * BS + i * BS + j];
        for (int k = lane; k < R.nnb; k += LW) {
            const double* ab;
            int64_t ld;
            if (!amg_filtered_block<BS>(R, k, node, strong && col[R.r0 + (int64_t)k * BS] == node * BS, values, strong, diag_f, ab, ld)) continue;
            double a[BS][BS];
#pragma unroll
            for (int i = 0; i < BS; ++i)
#pragma unroll
                for (int j = 0; j < BS; ++j) a[i][j] = ab[i * ld + j];
#pragma unroll
            for (int i = 0; i < BS; ++i)
#pragma unroll
                for (int j = 0; j < BS; ++j) {
                    double s = 0.0;
#pragma unroll
                    for (int q = 0; q < BS; ++q) s = fma(D[i][q], a[q][j], s);
                    acc[i] += fabs(s);
                }
        }
    }
#pragma unroll
    for (int off = LW / 2; off > 0; off >>= 1)
#pragma unroll
        for (int i = 0; i < BS; ++i) acc[i] += __shfl_xor(acc[i], off, LW);
    double m = 0.0;
#pragma unroll
    for (int i = 0; i < BS; ++i) m = fmax(m, acc[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < DXO_AMG_BLOCK / 64; ++k) m = fmax(m, lds[k]);
        part[blockIdx.x] = m;
    }
}

// one workgroup: rho = max(part), omega = (4/3) / rho
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_omega(const double* __restrict__ part, int64_t n, double* __restrict__ omega,
                                                           double* __restrict__ rho) {
    __shared__ double lds[DXO_AMG_BLOCK / 64];
    double m = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += DXO_AMG_BLOCK) m = fmax(m, part[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < DXO_AMG_BLOCK / 64; ++k) m = fmax(m, lds[k]);
        rho[0] = m;
        omega[0] = m > 0.0 ? (4.0 / 3.0) / m : 0.0;
    }
}

// ---- rho by power iteration on Dinv A, and the Chebyshev coefficients
// the sum of s over the workgroup, on every thread: the xor-butterfly of a wave, then the waves in ascending order
__device__ __forceinline__ double amg_block_sum(double s, double* lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = lds[0];
    for (int k = 1; k < DXO_AMG_BLOCK / 64; ++k) t += lds[k];
    return t;
}

// the start vector, the same on every level and exact in fp64: v[i] = 0.5 + ((uint32)(i * 2654435761) >> 8) * 2^-24, and the
// workgroup's partial of |v|^2
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_power_init(int64_t n_rows, double* __restrict__ v, double* __restrict__ part) {
    __shared__ double lds[DXO_AMG_BLOCK / 64];
    const int64_t row = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    double q = 0.0;
    if (row < n_rows) {
        const double x = 0.5 + (double)(((uint32_t)row * 2654435761u) >> 8) * 0x1p-24;
        v[row] = x;
        q = x * x;
    }
    q = amg_block_sum(q, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = q;
}

// w = Dinv (A (s v)) with s = scal[0] by row_product, and the workgroup's partial of |w|^2; with `strong`, w = Dinv_F (A^F (s v))
template <int BS, int LW>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_power_step(int64_t n_nodes, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                const double* __restrict__ values, const double* __restrict__ dinv,
                                                                const uint8_t* __restrict__ strong, const double* __restrict__ diag_f,
                                                                const double* __restrict__ scal, const double* __restrict__ v,
                                                                double* __restrict__ w, double* __restrict__ part) {
    __shared__ double lds[DXO_AMG_BLOCK / 64];
    constexpr int NPB = DXO_AMG_BLOCK / LW;
    const int64_t node = (int64_t)blockIdx.x * NPB + threadIdx.x / LW;
    const int lane = threadIdx.x % LW;
    double acc[BS];
    row_product<BS, LW, true>(n_nodes, node, lane, row_ptr, col, values, v, scal[0], acc,
                              [&](const NodeRow<BS>& R, int k, int64_t c, const double*& ab, int64_t& ld) {
                                  return amg_filtered_block<BS>(R, k, node, c == node * BS, values, strong, diag_f, ab, ld);
                              });
    double q = 0.0;
    if (node < n_nodes && lane == 0) {
#pragma unroll
        for (int i = 0; i < BS; ++i) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < BS; ++j) s = fma(dinv[node * BS * BS + i * BS + j], acc[j], s);
            w[node * BS + i] = s;
            q = fma(s, s, q);
        }
    }
    q = amg_block_sum(q, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = q;
}

// the pairs (c1, c2) of the steps d = c1 d + c2 Dinv (r - A x), x += d of the Chebyshev polynomial of the given degree on
// [lower rho, rho]; the first step has c1 = 0. rho == 0: no relaxation, as omega = 0
__device__ __forceinline__ void amg_cheby_table(double rho, double lower, int degree, double* __restrict__ c) {
    if (!(rho > 0.0)) {
        for (int k = 0; k < 2 * degree; ++k) c[k] = 0.0;
        return;
    }
    const double a = lower * rho, theta = 0.5 * (a + rho), delta = 0.5 * (rho - a), sigma = theta / delta;
    double r0 = 1.0 / sigma;
    c[0] = 0.0;
    c[1] = 1.0 / theta;
    for (int k = 1; k < degree; ++k) {
        const double r1 = 1.0 / (2.0 * sigma - r0);
        c[2 * k] = r1 * r0;
        c[2 * k + 1] = 2.0 * r1 / delta;
        r0 = r1;
    }
}

// one workgroup: |w| from the n partials (a thread's partials in ascending order, then amg_block_sum); scal = (1 / |w|, |w|) for
// the next step. After the last step rho = safety |w|, omega = (4/3) / rho and the Chebyshev pairs
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_power_norm(const double* __restrict__ part, int64_t n, int last, double safety, double lower,
                                                                int degree, double* __restrict__ scal, double* __restrict__ rho,
                                                                double* __restrict__ omega, double* __restrict__ cheb) {
    __shared__ double lds[DXO_AMG_BLOCK / 64];
    double q = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += DXO_AMG_BLOCK) q += part[i];
    q = amg_block_sum(q, lds);
    if (threadIdx.x != 0) return;
    const double lam = sqrt(q);
    scal[0] = lam > 0.0 ? 1.0 / lam : 0.0;
    scal[1] = lam;
    if (last) {
        const double r = safety * lam;
        rho[0] = r;
        omega[0] = r > 0.0 ? (4.0 / 3.0) / r : 0.0;
        amg_cheby_table(r, lower, degree, cheb);
    }
}

// the Chebyshev pairs from the rho of amg_omega (Chebyshev smoothing on the interval of the infinity norm)
__global__ void amg_cheby_coeffs(const double* __restrict__ rho, double lower, int degree, double* __restrict__ cheb) {
    if (threadIdx.x == 0 && blockIdx.x == 0) amg_cheby_table(rho[0], lower, degree, cheb);
}

// coarse levels: a dof whose row has no nonzero off-diagonal entry takes no part in the tentative prolongator
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_row_mask(int64_t n_rows, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                              const double* __restrict__ values, uint8_t* __restrict__ mask) {
    const int64_t row = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (row >= n_rows) return;
    bool any = false;
    for (int64_t e = row_ptr[row]; e < row_ptr[row + 1]; ++e) any = any || (col[e] != row && values[e] != 0.0);
    mask[row] = any ? 0 : 1;
}

// P = T - omega Dinv (A T), one thread per block (i, a): the neighbours j of i with aggregate a, ascending. NNS: the block of T of
// node j is t_val[j] (BSR x BSC); otherwise an identity without the masked dofs (BSR == BSC). With `strong`:
// P = T - omega_F Dinv_F (A^F T), dinv and omega being dinv_f and omega_F
template <int BSR, int BSC, bool NNS>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_build_p(int64_t p_blocks, const int32_t* __restrict__ p_row, const int32_t* __restrict__ p_col,
                                                             const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                             const double* __restrict__ values, const double* __restrict__ dinv,
                                                             const int32_t* __restrict__ agg, const uint8_t* __restrict__ mask,
                                                             const double* __restrict__ t_val, const double* __restrict__ omega,
                                                             const uint8_t* __restrict__ strong, const double* __restrict__ diag_f,
                                                             double* __restrict__ p_val) {
    static_assert(NNS || BSR == BSC, "an identity per node needs square blocks");
    const int64_t e = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (e >= p_blocks) return;
    const int64_t i = p_row[e];
    const int32_t a = p_col[e];
    const NodeRow<BSR> R(row_ptr, i);
    double acc[BSR][BSC];
#pragma unroll
    for (int r = 0; r < BSR; ++r)
#pragma unroll
        for (int c = 0; c < BSC; ++c) acc[r][c] = 0.0;
    for (int k = 0; k < R.nnb; ++k) {
        const int64_t j = col[R.r0 + (int64_t)k * BSR] / BSR;
        if (agg[j] != a) continue;
        const double* ab;
        int64_t ld;
        if (!amg_filtered_block<BSR>(R, k, i, j == i, values, strong, diag_f, ab, ld)) continue;      // A^F T (dinv is dinv_f)
        if constexpr (NNS) {
#pragma unroll
            for (int q = 0; q < BSR; ++q) {
                double tq[BSC];
#pragma unroll
                for (int c = 0; c < BSC; ++c) tq[c] = t_val[(j * BSR + q) * BSC + c];
#pragma unroll
                for (int r = 0; r < BSR; ++r) {
                    const double v = ab[r * ld + q];
#pragma unroll
                    for (int c = 0; c < BSC; ++c) acc[r][c] = fma(v, tq[c], acc[r][c]);
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < BSC; ++c) {
                if (mask[j * BSR + c]) continue;
#pragma unroll
                for (int r = 0; r < BSR; ++r) acc[r][c] += ab[r * ld + c];
            }
        }
    }
    const double om = omega[0];
    const bool own = agg[i] == a;
#pragma unroll
    for (int r = 0; r < BSR; ++r)
#pragma unroll
        for (int c = 0; c < BSC; ++c) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < BSR; ++q) s = fma(dinv[i * BSR * BSR + r * BSR + q], acc[q][c], s);
            double t;
            if constexpr (NNS) t = own ? t_val[(i * BSR + r) * BSC + c] : 0.0;
            else t = (own && r == c && !mask[i * BSR + r]) ? 1.0 : 0.0;
            p_val[e * BSR * BSC + r * BSC + c] = t - om * s;
        }
}

// (A P)(i, a) = sum over the neighbours j of i, ascending, of A_ij P_ja
template <int BSR, int BSC>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_build_ap(int64_t ap_blocks, const int32_t* __restrict__ ap_row, const int32_t* __restrict__ ap_col,
                                                              const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                              const double* __restrict__ values, const int64_t* __restrict__ p_ptr,
                                                              const int32_t* __restrict__ p_col, const double* __restrict__ p_val,
                                                              double* __restrict__ ap_val) {
    const int64_t e = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (e >= ap_blocks) return;
    const int64_t i = ap_row[e];
    const int32_t a = ap_col[e];
    const NodeRow<BSR> R(row_ptr, i);
    double acc[BSR][BSC];
#pragma unroll
    for (int r = 0; r < BSR; ++r)
#pragma unroll
        for (int c = 0; c < BSC; ++c) acc[r][c] = 0.0;
    for (int k = 0; k < R.nnb; ++k) {
        const int64_t j = col[R.r0 + (int64_t)k * BSR] / BSR;
        const int64_t f = amg_find(p_col, p_ptr[j], p_ptr[j + 1], a);
        if (f < 0) continue;
        // one row of the block of P at a time: an entry of acc still takes its terms in ascending q
#pragma unroll
        for (int q = 0; q < BSR; ++q) {
            double pq[BSC];
#pragma unroll
            for (int c = 0; c < BSC; ++c) pq[c] = p_val[f * BSR * BSC + q * BSC + c];
#pragma unroll
            for (int r = 0; r < BSR; ++r) {
                const double v = values[R.r0 + r * R.len + (int64_t)k * BSR + q];
#pragma unroll
                for (int c = 0; c < BSC; ++c) acc[r][c] = fma(v, pq[c], acc[r][c]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < BSR; ++r)
#pragma unroll
        for (int c = 0; c < BSC; ++c) ap_val[e * BSR * BSC + r * BSC + c] = acc[r][c];
}

// A_c(a, b) = sum over the blocks (i, a) of P, ascending i, of P_ia^T (A P)_ib; an exactly zero diagonal entry becomes 1
template <int BSR, int BSC>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_build_c(int64_t c_blocks, const int32_t* __restrict__ c_row, const int64_t* __restrict__ c_bptr,
                                                             const int64_t* __restrict__ c_row_ptr, const int32_t* __restrict__ c_col,
                                                             const int64_t* __restrict__ pt_ptr, const int64_t* __restrict__ pt_blk,
                                                             const int32_t* __restrict__ p_row, const double* __restrict__ p_val,
                                                             const int64_t* __restrict__ ap_ptr, const int32_t* __restrict__ ap_col,
                                                             const double* __restrict__ ap_val, double* __restrict__ c_val) {
    const int64_t g = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (g >= c_blocks) return;
    const int64_t a = c_row[g];
    const int64_t k = g - c_bptr[a];
    const NodeRow<BSC> R(c_row_ptr, a);
    const int32_t b = c_col[R.r0 + k * BSC] / BSC;
    double acc[BSC][BSC];
#pragma unroll
    for (int r = 0; r < BSC; ++r)
#pragma unroll
        for (int c = 0; c < BSC; ++c) acc[r][c] = 0.0;
    for (int64_t e = pt_ptr[a]; e < pt_ptr[a + 1]; ++e) {
        const int64_t pb = pt_blk[e];
        const int64_t i = p_row[pb];
        const int64_t f = amg_find(ap_col, ap_ptr[i], ap_ptr[i + 1], b);
        if (f < 0) continue;
#pragma unroll
        for (int q = 0; q < BSR; ++q) {
            double w[BSC];
#pragma unroll
            for (int c = 0; c < BSC; ++c) w[c] = ap_val[f * BSR * BSC + q * BSC + c];
#pragma unroll
            for (int r = 0; r < BSC; ++r) {
                const double p = p_val[pb * BSR * BSC + q * BSC + r];
#pragma unroll
                for (int c = 0; c < BSC; ++c) acc[r][c] = fma(p, w[c], acc[r][c]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < BSC; ++r)
#pragma unroll
        for (int c = 0; c < BSC; ++c) {
            double v = acc[r][c];
            if (a == b && r == c && v == 0.0) v = 1.0;
            c_val[R.r0 + r * R.len + k * BSC + c] = v;
        }
}

// ---- a given nodal transfer (dxo_amg_create_transfer): every block of P is diagonal, p_diag[block][BS], so the two products of the
// Galerkin matrix scale the columns and then the rows of the blocks of A. The patterns, the order of the sums and the search for the
// source blocks are those of amg_build_ap / amg_build_c.
// (A P)(i, a) = sum over the neighbours j of i, ascending, of A_ij diag(p_ja)
template <int BS>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_build_ap_w(int64_t ap_blocks, const int32_t* __restrict__ ap_row, const int32_t* __restrict__ ap_col,
                                                                const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                const double* __restrict__ values, const int64_t* __restrict__ p_ptr,
                                                                const int32_t* __restrict__ p_col, const double* __restrict__ p_diag,
                                                                double* __restrict__ ap_val) {
    const int64_t e = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (e >= ap_blocks) return;
    const int64_t i = ap_row[e];
    const int32_t a = ap_col[e];
    const NodeRow<BS> R(row_ptr, i);
    double acc[BS][BS];
#pragma unroll
    for (int r = 0; r < BS; ++r)
#pragma unroll
        for (int c = 0; c < BS; ++c) acc[r][c] = 0.0;
    for (int k = 0; k < R.nnb; ++k) {
        const int64_t j = col[R.r0 + (int64_t)k * BS] / BS;
        const int64_t f = amg_find(p_col, p_ptr[j], p_ptr[j + 1], a);
        if (f < 0) continue;
        double pd[BS];
#pragma unroll
        for (int c = 0; c < BS; ++c) pd[c] = p_diag[f * BS + c];
#pragma unroll
        for (int r = 0; r < BS; ++r)
#pragma unroll
            for (int c = 0; c < BS; ++c) acc[r][c] = fma(values[R.r0 + r * R.len + (int64_t)k * BS + c], pd[c], acc[r][c]);
    }
#pragma unroll
    for (int r = 0; r < BS; ++r)
#pragma unroll
        for (int c = 0; c < BS; ++c) ap_val[e * BS * BS + r * BS + c] = acc[r][c];
}

// A_c(a, b) = sum over the blocks (i, a) of P, ascending i, of diag(p_ia) (A P)_ib; an exactly zero diagonal entry becomes 1
template <int BS>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_build_c_w(int64_t c_blocks, const int32_t* __restrict__ c_row, const int64_t* __restrict__ c_bptr,
                                                               const int64_t* __restrict__ c_row_ptr, const int32_t* __restrict__ c_col,
                                                               const int64_t* __restrict__ pt_ptr, const int64_t* __restrict__ pt_blk,
                                                               const int32_t* __restrict__ p_row, const double* __restrict__ p_diag,
                                                               const int64_t* __restrict__ ap_ptr, const int32_t* __restrict__ ap_col,
                                                               const double* __restrict__ ap_val, double* __restrict__ c_val) {
    const int64_t g = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (g >= c_blocks) return;
    const int64_t a = c_row[g];
    const int64_t k = g - c_bptr[a];
    const NodeRow<BS> R(c_row_ptr, a);
    const int32_t b = c_col[R.r0 + k * BS] / BS;
    double acc[BS][BS];
#pragma unroll
    for (int r = 0; r < BS; ++r)
#pragma unroll
        for (int c = 0; c < BS; ++c) acc[r][c] = 0.0;
    for (int64_t e = pt_ptr[a]; e < pt_ptr[a + 1]; ++e) {
        const int64_t pb = pt_blk[e];
        const int64_t i = p_row[pb];
        const int64_t f = amg_find(ap_col, ap_ptr[i], ap_ptr[i + 1], b);
        if (f < 0) continue;
#pragma unroll
        for (int r = 0; r < BS; ++r) {
            const double p = p_diag[pb * BS + r];
#pragma unroll
            for (int c = 0; c < BS; ++c) acc[r][c] = fma(p, ap_val[f * BS * BS + r * BS + c], acc[r][c]);
        }
    }
#pragma unroll
    for (int r = 0; r < BS; ++r)
#pragma unroll
        for (int c = 0; c < BS; ++c) {
            double v = acc[r][c];
            if (a == b && r == c && v == 0.0) v = 1.0;
            c_val[R.r0 + r * R.len + k * BS + c] = v;
        }
}

// B of the level below a given transfer: the rows of the (already zeroed) B of this level at the nodes the coarse nodes are
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_gather_b(int64_t n_rows_c, int bs, int k, const int32_t* __restrict__ ctf,
                                                              const double* __restrict__ B, double* __restrict__ Bc) {
    const int64_t row = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (row >= n_rows_c) return;
    const int64_t src = (int64_t)ctf[row / bs] * bs + row % bs;
    for (int c = 0; c < k; ++c) Bc[row * k + c] = B[src * k + c];
}

// ---- strength of connection
// The test does not depend on the scale of the matrix: every sum of squares is formed on entries multiplied by a power of two that
// brings them near 1 (amg_pow2_down of a reference value: exact, as in invert_block), so that neither |A_ii|_F nor the two sides of
// the comparison leave the range of double where the entries themselves are inside it. Wherever the unscaled squares neither
// overflow nor underflow the mask is the one of the unscaled arithmetic bit for bit.
// 2^-e, e the exponent of m (frexp) held in +-1000 so that 2^-e is a normal number; 1 for a zero, NaN or infinite m
__device__ __forceinline__ double amg_pow2_down(double m) {
    int e = 0;
    if (m > 0.0 && m <= 1.7976931348623157e308) (void)frexp(m, &e);
    e = e > 1000 ? 1000 : (e < -1000 ? -1000 : e);
    return ldexp(1.0, -e);
}

// the sum of the squares of s a, entry by entry in row-major order
template <int BS>
__device__ __forceinline__ double amg_block_norm2(const double* __restrict__ a, int64_t ld, double s) {
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
        for (int j = 0; j < BS; ++j) {
            const double v = a[i * ld + j] * s;
            sum = fma(v, v, sum);
        }
    return sum;
}

// dn[node] = |A_ii|_F (0 without a diagonal block): the norm of 2^-e A_ii, e the exponent of its largest entry, divided by 2^-e
template <int BS>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_diag_norm(int64_t n_nodes, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                               const double* __restrict__ values, double* __restrict__ dn) {
    const int64_t node = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (node >= n_nodes) return;
    const NodeRow<BS> R(row_ptr, node);
    const int lo = block_pos<BS>(R, col, node);
    double d = 0.0;
    if (lo >= 0) {
        const double* a = values + R.r0 + (int64_t)lo * BS;
        double m = 0.0;
#pragma unroll
        for (int i = 0; i < BS; ++i)
#pragma unroll
            for (int j = 0; j < BS; ++j) m = fmax(m, fabs(a[i * R.len + j]));
        const double s = amg_pow2_down(m);
        d = sqrt(amg_block_norm2<BS>(a, R.len, s)) / s;
    }
    dn[node] = d;
}

// strong[block] = |s A_ij|_F^2 >= th2 (s |A_ii|_F) (s |A_jj|_F) with s = 2^-e, e the exponent of the larger of the two norms, or the
// same for the transposed block (found by search in row j; absent: the one-sided test). LW lanes own a node, a lane its blocks
// k = lane, lane + LW, ...; diagonal blocks are strong
template <int BS, int LW>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_strength(int64_t n_nodes, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                              const double* __restrict__ values, const double* __restrict__ dn, double th2,
                                                              uint8_t* __restrict__ strong) {
    constexpr int NPB = DXO_AMG_BLOCK / LW;
    const int64_t node = (int64_t)blockIdx.x * NPB + threadIdx.x / LW;
    const int lane = threadIdx.x % LW;
    if (node >= n_nodes) return;
    const NodeRow<BS> R(row_ptr, node);
    const int64_t b0 = R.r0 / (BS * BS);
    const double di = dn[node];
    for (int k = lane; k < R.nnb; k += LW) {
        const int64_t j = col[R.r0 + (int64_t)k * BS] / BS;
        bool st = j == node;
        if (!st) {
            const double dj = dn[j];
            const double s = amg_pow2_down(fmax(di, dj));
            const double bound = th2 * ((di * s) * (dj * s));
            st = amg_block_norm2<BS>(values + R.r0 + (int64_t)k * BS, R.len, s) >= bound;
            if (!st) {
                const NodeRow<BS> Rj(row_ptr, j);
                const int t = block_pos<BS>(Rj, col, node);      // the block (j, node)
                if (t >= 0) st = amg_block_norm2<BS>(values + Rj.r0 + (int64_t)t * BS, Rj.len, s) >= bound;
            }
        }
        strong[b0 + k] = st ? 1 : 0;
    }
}

// the lumped diagonal block A_ii + the weak blocks of the row in ascending order, and its inverse. A block that fails the test of
// invert_block takes the inverse of A_ii (dinv) and is marked; a node without a strong off-diagonal block gets a zero inverse (its
// lumped block is a near-zero row sum): it is not smoothed
template <int BS>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_lump(int64_t n_nodes, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                          const double* __restrict__ values, const uint8_t* __restrict__ strong,
                                                          const double* __restrict__ dinv, double* __restrict__ diag_f,
                                                          double* __restrict__ dinv_f, uint8_t* __restrict__ unlumped) {
    const int64_t node = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (node >= n_nodes) return;
    const NodeRow<BS> R(row_ptr, node);
    const int64_t b0 = R.r0 / (BS * BS);
    const int lo = block_pos<BS>(R, col, node);
    double a[BS][BS];
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
        for (int j = 0; j < BS; ++j) a[i][j] = lo >= 0 ? values[R.r0 + i * R.len + (int64_t)lo * BS + j] : 0.0;
    int n_strong = 0;
    for (int k = 0; k < R.nnb; ++k) {
        if (k == lo) continue;
        if (strong[b0 + k]) {
            ++n_strong;
            continue;
        }
#pragma unroll
        for (int i = 0; i < BS; ++i)
#pragma unroll
            for (int j = 0; j < BS; ++j) a[i][j] += values[R.r0 + i * R.len + (int64_t)k * BS + j];
    }
#pragma unroll
    for (int i = 0; i < BS; ++i)      // stored before the inversion, which then holds the scaled block alone
#pragma unroll
        for (int j = 0; j < BS; ++j) diag_f[node * BS * BS + i * BS + j] = a[i][j];
    double b[BS][BS];
    const bool ok = invert_block<BS>(a, b);
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
        for (int j = 0; j < BS; ++j) {
            const int64_t o = node * BS * BS + i * BS + j;
            dinv_f[o] = n_strong == 0 ? 0.0 : (ok ? b[i][j] : dinv[o]);
        }
    unlumped[node] = n_strong > 0 && !ok ? 1 : 0;
}

// ---- the near-null space, at creation
// the rows of constrained dofs of B_0 are zero
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_zero_rows(int64_t n_rows, int k, const uint8_t* __restrict__ mask, double* __restrict__ B) {
    const int64_t row = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (row >= n_rows || !mask[row]) return;
    for (int c = 0; c < k; ++c) B[row * k + c] = 0.0;
}

// LG lanes own one aggregate: its rows (BSR per node, the nodes ascending) go to the lanes in turn, row t to lane t % LG. Column j of
// the aggregate's rows of B is copied to column j of its T blocks and worked on there (a lane reads back only what it wrote itself):
// twice c = Q_{<j}^T v, v -= Q_{<j} c, R_{<j, j} += c; a column that keeps no more than tol of its norm is dead (Q column and R
// diagonal zero). Every column product is a lane's partial sum in ascending row order, then the fixed xor-butterfly over the group.
template <int LG>
__device__ __forceinline__ double amg_group_sum(double s) {
#pragma unroll
    for (int off = LG / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, LG);
    return s;
}

template <int BSR, int K, int LG>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_tentative(int64_t n_agg, const int64_t* __restrict__ agg_ptr, const int32_t* __restrict__ agg_node,
                                                               const double* __restrict__ B, double tol, double* t_val, double* __restrict__ Bn,
                                                               uint8_t* __restrict__ dead_a) {
    constexpr int APB = DXO_AMG_BLOCK / LG;
    const int64_t a = (int64_t)blockIdx.x * APB + threadIdx.x / LG;
    const int lane = threadIdx.x % LG;
    const bool valid = a < n_agg;                              // the lanes of an absent aggregate run along with no rows
    const int64_t first = valid ? agg_ptr[a] : 0;
    const int64_t m = valid ? (agg_ptr[a + 1] - first) * BSR : 0;
    int n_dead = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double s = 0.0;
        for (int64_t t = lane; t < m; t += LG) {
            const int64_t row = (int64_t)agg_node[first + t / BSR] * BSR + t % BSR;
            const double v = B[row * K + j];
            t_val[row * K + j] = v;
            s = fma(v, v, s);
        }
        const double n0 = sqrt(amg_group_sum<LG>(s));
        double racc[K];
#pragma unroll
        for (int i = 0; i < K; ++i) racc[i] = 0.0;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            double c[K];
#pragma unroll
            for (int i = 0; i < K; ++i) c[i] = 0.0;
            for (int64_t t = lane; t < m; t += LG) {
                const int64_t row = (int64_t)agg_node[first + t / BSR] * BSR + t % BSR;
                const double v = t_val[row * K + j];
#pragma unroll
                for (int i = 0; i < j; ++i) c[i] = fma(t_val[row * K + i], v, c[i]);
            }
#pragma unroll
            for (int i = 0; i < j; ++i) {
                c[i] = amg_group_sum<LG>(c[i]);
                racc[i] += c[i];
            }
            for (int64_t t = lane; t < m; t += LG) {
                const int64_t row = (int64_t)agg_node[first + t / BSR] * BSR + t % BSR;
                double v = t_val[row * K + j];
#pragma unroll
                for (int i = 0; i < j; ++i) v = fma(-c[i], t_val[row * K + i], v);
                t_val[row * K + j] = v;
            }
        }
        s = 0.0;
        for (int64_t t = lane; t < m; t += LG) {
            const int64_t row = (int64_t)agg_node[first + t / BSR] * BSR + t % BSR;
            const double v = t_val[row * K + j];
            s = fma(v, v, s);
        }
        const double nv = sqrt(amg_group_sum<LG>(s));
        const bool dead = n0 == 0.0 || !(nv > tol * n0);
        n_dead += dead ? 1 : 0;
        for (int64_t t = lane; t < m; t += LG) {
            const int64_t row = (int64_t)agg_node[first + t / BSR] * BSR + t % BSR;
            t_val[row * K + j] = dead ? 0.0 : t_val[row * K + j] / nv;
        }
        if (valid && lane == 0) {
#pragma unroll
            for (int i = 0; i < K; ++i) Bn[(a * K + i) * K + j] = i < j ? racc[i] : (i == j && !dead ? nv : 0.0);
        }
    }
    if (valid && lane == 0) dead_a[a] = (uint8_t)n_dead;
}

// B of the rigid-body modes from node coordinates x [n_nodes][G]: the G translations, then (-y, x) or (-y, x, 0), (0, -z, y), (z, 0, -x)
template <int G>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_rigid_body_modes(int64_t n_nodes, const double* __restrict__ x, double* __restrict__ B) {
    constexpr int K = G == 2 ? 3 : 6;
    const int64_t i = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (i >= n_nodes) return;
    double p[G];
#pragma unroll
    for (int d = 0; d < G; ++d) p[d] = x[i * G + d];
    double b[G][K];
#pragma unroll
    for (int d = 0; d < G; ++d)
#pragma unroll
        for (int c = 0; c < K; ++c) b[d][c] = d == c ? 1.0 : 0.0;
    if constexpr (G == 2) {
        b[0][2] = -p[1];
        b[1][2] = p[0];
    } else {
        b[0][3] = -p[1];
        b[1][3] = p[0];
        b[1][4] = -p[2];
        b[2][4] = p[1];
        b[0][5] = p[2];
        b[2][5] = -p[0];
    }
#pragma unroll
    for (int d = 0; d < G; ++d)
#pragma unroll
        for (int c = 0; c < K; ++c) B[(i * G + d) * K + c] = b[d][c];
}

// ---- the dense coarsest level. W is [n][2 n] = [A | I]
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_dense_fill(int64_t n, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                const double* __restrict__ values, double* __restrict__ W) {
    const int64_t row = blockIdx.x;
    double* w = W + row * 2 * n;
    for (int64_t c = threadIdx.x; c < 2 * n; c += DXO_AMG_BLOCK) w[c] = c == n + row ? 1.0 : 0.0;
    __syncthreads();
    for (int64_t e = row_ptr[row] + threadIdx.x; e < row_ptr[row + 1]; e += DXO_AMG_BLOCK) w[col[e]] = values[e];
}

// step k of Gauss-Jordan with partial pivoting, out of place: workgroup i forms row i of `out`. Every workgroup finds the pivot row
// (largest |in[i][k]|, i >= k, the lowest i among equals) itself.
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_dense_step(int64_t n, int64_t k, const double* __restrict__ in, double* __restrict__ out,
                                                                int* __restrict__ flag) {
    __shared__ double lv[DXO_AMG_BLOCK];
    __shared__ int64_t li[DXO_AMG_BLOCK];
    const int64_t ld = 2 * n;
    double best = -1.0;
    int64_t bi = k;
    for (int64_t i = k + threadIdx.x; i < n; i += DXO_AMG_BLOCK) {
        const double v = fabs(in[i * ld + k]);
        if (v > best) {
            best = v;
            bi = i;
        }
    }
    lv[threadIdx.x] = best;
    li[threadIdx.x] = bi;
    __syncthreads();
    for (int off = DXO_AMG_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const double v = lv[threadIdx.x + off];
            const int64_t j = li[threadIdx.x + off];
            if (v > lv[threadIdx.x] || (v == lv[threadIdx.x] && j < li[threadIdx.x])) {
                lv[threadIdx.x] = v;
                li[threadIdx.x] = j;
            }
        }
        __syncthreads();
    }
    const int64_t p = li[0];
    if (blockIdx.x == 0 && threadIdx.x == 0 && !(lv[0] > 0.0)) flag[1] = 1;
    const double piv = in[p * ld + k];
    const int64_t row = blockIdx.x;
    const double* pr = in + p * ld;
    double* o = out + row * ld;
    if (row == k) {
        for (int64_t c = threadIdx.x; c < ld; c += DXO_AMG_BLOCK) o[c] = pr[c] / piv;
    } else {
        const double* sr = in + (row == p ? k : row) * ld;
        const double f = sr[k];
        for (int64_t c = threadIdx.x; c < ld; c += DXO_AMG_BLOCK) o[c] = fma(-f, pr[c] / piv, sr[c]);
    }
}

// x = B r with B the right half of W: one wave per row. B and the sums are double under either precision of the cycle: a float r is
// widened entry by entry and the result narrowed once
template <class T>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_dense_apply(int64_t n, const double* __restrict__ W, const T* __restrict__ r,
                                                                 T* __restrict__ x) {
    const int64_t row = (int64_t)blockIdx.x * (DXO_AMG_BLOCK / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    double s = 0.0;
    if (row < n) {
        const double* b = W + row * 2 * n + n;
        for (int64_t c = lane; c < n; c += 64) s = fma(b[c], (double)r[c], s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (row < n && lane == 0) x[row] = (T)s;
}

// out = (float) in, entry by entry (grid-stride). With a flag (the copies of a setup): a finite double that leaves the range of
// float stores `mark` there unless an earlier level already has (every thread of a launch stores the same word, and the launches of
// the levels follow each other on the stream: no atomics). Underflow to zero is not an error. Without one: the right-hand side of a cycle
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_narrow(int64_t n, const double* __restrict__ in, float* __restrict__ out, int* flag, int mark) {
    const int64_t stride = (int64_t)gridDim.x * DXO_AMG_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x; i < n; i += stride) {
        const double v = in[i];
        const float f = (float)v;
        out[i] = f;
        if (flag && std::isfinite(v) && !std::isfinite(f) && flag[2] == 0) flag[2] = mark;
    }
}

// ---- the cycle
// The kernels of the cycle take the scalar T of the level's matrix, inverses, prolongator and vectors: double, or float for the
// single-precision cycle (dxo_amg_set_precision), where every fma below is v_fma_f32 in the same order. omega and the Chebyshev
// pairs stay double on the device and are narrowed here. TO, the scalar of a sweep's result, differs from T in one place: the last
// post-sweep of level 0 of the float cycle writes the caller's double z.
//
// x = scale[0] Dinv r, and d = x if d is given: the first step of a smoother from x = 0 (no SpMV). Jacobi: scale is omega; Chebyshev:
// the c2 of the first pair, and d the direction
template <int BS, class T>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_first_step(int64_t n_nodes, const T* __restrict__ dinv, const double* __restrict__ scale,
                                                                const T* __restrict__ r, T* __restrict__ d, T* __restrict__ x) {
    const int64_t node = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (node >= n_nodes) return;
    const T sc = (T)scale[0];
    T rb[BS];
#pragma unroll
    for (int j = 0; j < BS; ++j) rb[j] = r[node * BS + j];
#pragma unroll
    for (int i = 0; i < BS; ++i) {
        T s = 0.0;
#pragma unroll
        for (int j = 0; j < BS; ++j) s = fma(dinv[node * BS * BS + i * BS + j], rb[j], s);
        const T v = sc * s;
        if (d) d[node * BS + i] = v;
        x[node * BS + i] = v;
    }
}

// RESID: out = r - A x; otherwise out = x + omega Dinv (r - A x). LW lanes own a node (A x by row_product). out may be r: a node's
// entries of r are read by its own lane 0 only, before it writes.
template <int BS, int LW, bool RESID, class T, class TO>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_sweep(int64_t n_nodes, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                           const T* __restrict__ values, const T* __restrict__ dinv,
                                                           const double* __restrict__ omega, const T* r, const T* __restrict__ x,
                                                           TO* out) {
    constexpr int NPB = DXO_AMG_BLOCK / LW;
    const int64_t node = (int64_t)blockIdx.x * NPB + threadIdx.x / LW;
    const int lane = threadIdx.x % LW;
    T acc[BS];
    row_product<BS, LW>(n_nodes, node, lane, row_ptr, col, values, x, acc);
    if (node < n_nodes && lane == 0) {
        T d[BS];
#pragma unroll
        for (int i = 0; i < BS; ++i) d[i] = r[node * BS + i] - acc[i];
        if constexpr (RESID) {
#pragma unroll
            for (int i = 0; i < BS; ++i) out[node * BS + i] = (TO)d[i];
        } else {
            const T om = (T)omega[0];
#pragma unroll
            for (int i = 0; i < BS; ++i) {
                T s = 0.0;
#pragma unroll
                for (int j = 0; j < BS; ++j) s = fma(dinv[node * BS * BS + i * BS + j], d[j], s);
                out[node * BS + i] = (TO)fma(om, s, x[node * BS + i]);
            }
        }
    }
}

// d = c1 d + c2 Dinv (r - A x), out = x + d with (c1, c2) = c[0..1], A x by row_product as in amg_sweep. d is updated in place: a
// node's entries are touched by its own lane 0 only. With c1 == 0 (the first step of the post-smoothing) d is not read. out may be r,
// as in amg_sweep.
template <int BS, int LW, class T, class TO>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_cheby_sweep(int64_t n_nodes, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                 const T* __restrict__ values, const T* __restrict__ dinv,
                                                                 const double* __restrict__ c, const T* r, const T* __restrict__ x,
                                                                 T* __restrict__ d, TO* out) {
    constexpr int NPB = DXO_AMG_BLOCK / LW;
    const int64_t node = (int64_t)blockIdx.x * NPB + threadIdx.x / LW;
    const int lane = threadIdx.x % LW;
    T acc[BS];
    row_product<BS, LW>(n_nodes, node, lane, row_ptr, col, values, x, acc);
    if (node < n_nodes && lane == 0) {
        const T c1 = (T)c[0], c2 = (T)c[1];
        T res[BS];
#pragma unroll
        for (int i = 0; i < BS; ++i) res[i] = r[node * BS + i] - acc[i];
#pragma unroll
        for (int i = 0; i < BS; ++i) {
            T s = 0.0;
#pragma unroll
            for (int j = 0; j < BS; ++j) s = fma(dinv[node * BS * BS + i * BS + j], res[j], s);
            const T dn = fma(c2, s, c1 != T(0) ? c1 * d[node * BS + i] : T(0));
            d[node * BS + i] = dn;
            out[node * BS + i] = (TO)(x[node * BS + i] + dn);
        }
    }
}

// r_c[a] = sum over the blocks (i, a) of P, ascending i, of P_ia^T t_i
template <int BSR, int BSC, class T>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_restrict(int64_t n_agg, const int64_t* __restrict__ pt_ptr, const int64_t* __restrict__ pt_blk,
                                                              const int32_t* __restrict__ p_row, const T* __restrict__ p_val,
                                                              const T* __restrict__ t, T* __restrict__ rc) {
    const int64_t a = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (a >= n_agg) return;
    T acc[BSC];
#pragma unroll
    for (int c = 0; c < BSC; ++c) acc[c] = 0.0;
    for (int64_t e = pt_ptr[a]; e < pt_ptr[a + 1]; ++e) {
        const int64_t pb = pt_blk[e];
        const int64_t i = p_row[pb];
#pragma unroll
        for (int q = 0; q < BSR; ++q) {
            const T tv = t[i * BSR + q];
#pragma unroll
            for (int c = 0; c < BSC; ++c) acc[c] = fma(p_val[pb * BSR * BSC + q * BSC + c], tv, acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < BSC; ++c) rc[a * BSC + c] = acc[c];
}

// x_i += sum over the blocks of row i of P, ascending aggregate, of P_ia xc_a
template <int BSR, int BSC, class T>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_prolong(int64_t n_nodes, const int64_t* __restrict__ p_ptr, const int32_t* __restrict__ p_col,
                                                             const T* __restrict__ p_val, const T* __restrict__ xc, T* __restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (i >= n_nodes) return;
    T acc[BSR];
#pragma unroll
    for (int r = 0; r < BSR; ++r) acc[r] = 0.0;
    for (int64_t e = p_ptr[i]; e < p_ptr[i + 1]; ++e) {
        const int64_t a = p_col[e];
#pragma unroll
        for (int c = 0; c < BSC; ++c) {
            const T v = xc[a * BSC + c];
#pragma unroll
            for (int r = 0; r < BSR; ++r) acc[r] = fma(p_val[e * BSR * BSC + r * BSC + c], v, acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < BSR; ++r) x[i * BSR + r] += acc[r];
}

// The transfers of a given nodal transfer, one thread per dof: consecutive lanes read consecutive entries of p_diag, t and x, where
// a thread per node would stride them by BS.
// r_c[a][c] = sum over the blocks (i, a) of P, ascending i, of p_diag[block][c] t_i[c]
template <int BS, class T>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_restrict_w(int64_t n_rows_c, const int64_t* __restrict__ pt_ptr, const int64_t* __restrict__ pt_blk,
                                                                const int32_t* __restrict__ p_row, const T* __restrict__ p_diag,
                                                                const T* __restrict__ t, T* __restrict__ rc) {
    const int64_t g = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (g >= n_rows_c) return;
    const int64_t a = g / BS;
    const int c = (int)(g % BS);
    T acc = 0.0;
    for (int64_t e = pt_ptr[a]; e < pt_ptr[a + 1]; ++e) {
        const int64_t pb = pt_blk[e];
        acc = fma(p_diag[pb * BS + c], t[(int64_t)p_row[pb] * BS + c], acc);
    }
    rc[g] = acc;
}

// x_i[r] += sum over the blocks of row i of P, ascending coarse node, of p_diag[block][r] xc_a[r]
template <int BS, class T>
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_prolong_w(int64_t n_rows, const int64_t* __restrict__ p_ptr, const int32_t* __restrict__ p_col,
                                                               const T* __restrict__ p_diag, const T* __restrict__ xc, T* __restrict__ x) {
    const int64_t g = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x;
    if (g >= n_rows) return;
    const int64_t i = g / BS;
    const int r = (int)(g % BS);
    T acc = 0.0;
    for (int64_t e = p_ptr[i]; e < p_ptr[i + 1]; ++e) acc = fma(p_diag[e * BS + r], xc[(int64_t)p_col[e] * BS + r], acc);
    x[g] += acc;
}

// ---- the K-cycle
constexpr int AMG_K_MAX_PARTS = 1024;
enum { KCO_RHO1 = 0, KCO_A1 = 1, KCO_ALPHA1 = 2, KCO_X1 = 3, KCO_X2 = 4, KCO_COUNT = 8 };

// part[q * gridDim.x + block] = the workgroup's share of (w, w) (q = 0), (w, a) (q = 1) and, with b, (w, b) (q = 2); w is read once.
// The grid is fixed for a level and the rows are taken with its stride, so the terms a thread adds, and their order, are fixed
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_k_dots(int64_t n, const double* __restrict__ w, const double* __restrict__ a,
                                                            const double* __restrict__ b, double* __restrict__ part) {
    __shared__ double lds[3][DXO_AMG_BLOCK / 64];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const int64_t stride = (int64_t)gridDim.x * DXO_AMG_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x; i < n; i += stride) {
        const double wi = w[i];
        s0 = fma(wi, wi, s0);
        s1 = fma(wi, a[i], s1);
        if (b) s2 = fma(wi, b[i], s2);
    }
    s0 = amg_block_sum(s0, lds[0]);
    s1 = amg_block_sum(s1, lds[1]);
    s2 = amg_block_sum(s2, lds[2]);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s0;
        part[(int64_t)gridDim.x + blockIdx.x] = s1;
        part[2 * (int64_t)gridDim.x + blockIdx.x] = s2;
    }
}

// one workgroup: the sums of the partials (a thread's in ascending order, then amg_block_sum) and the coefficients of the GCR step.
// step 1: rho1 = (v1, v1), a1 = (v1, r), alpha1 = a1 / rho1 (0 with rho1 == 0). step 2: beta = (v2, v2), g = (v2, v1), a2 = (v2, r1),
// rho2 = beta - g (g / rho1) and x = X1 c1 + X2 c2: (0, 0) with rho1 == 0, (alpha1, 0) when rho2 is not finite or at most 1e-14 beta
// (the second direction depends on the first: the rule of the singular diagonal block), else X2 = a2 / rho2 and
// X1 = alpha1 - (g / rho1) X2. Only ratios of the dot products are formed, no product of two of them (that would be a fourth power
// of |r|): the coefficients are homogeneous of degree 0 in r, bit for bit, wherever the dot products themselves are finite and normal
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_k_scalar(const double* __restrict__ part, int nb, int step, double* __restrict__ co) {
    __shared__ double lds[3][DXO_AMG_BLOCK / 64];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < nb; i += DXO_AMG_BLOCK) {
        s0 += part[i];
        s1 += part[nb + i];
        s2 += part[2 * nb + i];
    }
    s0 = amg_block_sum(s0, lds[0]);
    s1 = amg_block_sum(s1, lds[1]);
    s2 = amg_block_sum(s2, lds[2]);
    if (threadIdx.x != 0) return;
    if (step == 1) {
        co[KCO_RHO1] = s0;
        co[KCO_A1] = s1;
        co[KCO_ALPHA1] = s0 == 0.0 ? 0.0 : s1 / s0;
        return;
    }
    const double rho1 = co[KCO_RHO1], alpha1 = co[KCO_ALPHA1], beta = s0, g = s1, a2 = s2;
    double x1 = 0.0, x2 = 0.0;
    if (rho1 != 0.0) {
        const double gr = g / rho1;
        const double rho2 = beta - g * gr;
        if (!std::isfinite(rho2) || rho2 <= 1e-14 * beta) {
            x1 = alpha1;
        } else {
            x2 = a2 / rho2;
            x1 = alpha1 - gr * x2;
        }
    }
    co[KCO_X1] = x1;
    co[KCO_X2] = x2;
}

// r1 = r - alpha1 v1
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_k_residual(int64_t n, const double* __restrict__ co, const double* __restrict__ r,
                                                                const double* __restrict__ v1, double* __restrict__ r1) {
    const double alpha = co[KCO_ALPHA1];
    const int64_t stride = (int64_t)gridDim.x * DXO_AMG_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x; i < n; i += stride) r1[i] = fma(-alpha, v1[i], r[i]);
}

// c1 <- X1 c1 + X2 c2 in place; a zero coefficient leaves its vector out, so that the guards give exactly 0 and exactly alpha1 c1
__global__ __launch_bounds__(DXO_AMG_BLOCK) void amg_k_combine(int64_t n, const double* __restrict__ co, double* __restrict__ c1,
                                                               const double* __restrict__ c2) {
    const double x1 = co[KCO_X1], x2 = co[KCO_X2];
    const int64_t stride = (int64_t)gridDim.x * DXO_AMG_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * DXO_AMG_BLOCK + threadIdx.x; i < n; i += stride) {
        const double t = x1 != 0.0 ? x1 * c1[i] : 0.0;
        c1[i] = x2 != 0.0 ? fma(x2, c2[i], t) : t;
    }
}

// ---- host: launch helpers
// a shape without an instantiation is a defect of this file, not of the caller: the entry points admit (1..3) and the lists below
[[noreturn]] inline void amg_no_shape(int a, int b) {
    fprintf(stderr, "amg.hip: no kernel instantiation for the shape (%d, %d)\n", a, b);
    std::abort();
}

inline dim3 amg_grid(int64_t items, int per_block = DXO_AMG_BLOCK) { return dim3((unsigned)std::max<int64_t>(1, (items + per_block - 1) / per_block)); }

// one workgroup per `per_block` items
template <class... P, class... Args>
void amg_launch(void (*kernel)(P...), int64_t items, int per_block, hipStream_t s, Args... args) {
    hipLaunchKernelGGL(kernel, amg_grid(items, per_block), dim3(DXO_AMG_BLOCK), 0, s, args...);
}

// from run-time shapes to compile-time ones (with_int and with_bs of krylov_internal.h, with_pairs here): f(constant...) for the entry
// of the list that matches, amg_no_shape for none. The lists are the instantiations of this file
constexpr auto amg_miss = [](int v) { amg_no_shape(v, v); };

constexpr int amg_pair(int bsr, int bsc) { return bsr * 8 + bsc; }

template <int... Ps, class F>
void with_pairs(int bsr, int bsc, F&& f) {
    if (!((amg_pair(bsr, bsc) == Ps && (f(int_c<Ps / 8>{}, int_c<Ps % 8>{}), true)) || ...)) amg_no_shape(bsr, bsc);
}

// (rows of the level, rows of the next): with a near-null space (2, 3) -> (3, 3) and (3, 6) -> (6, 6), square without one
template <class F>
void with_nns_pair(int bsr, int bsc, F&& f) { with_pairs<amg_pair(2, 3), amg_pair(3, 3), amg_pair(3, 6), amg_pair(6, 6)>(bsr, bsc, f); }

template <class F>
void with_square(int bsr, int bsc, F&& f) { with_pairs<amg_pair(1, 1), amg_pair(2, 2), amg_pair(3, 3)>(bsr, bsc, f); }

template <class F>
void with_pair(int bsr, int bsc, F&& f) {
    if (bsr == bsc && bsr <= 3) with_square(bsr, bsc, f);
    else with_nns_pair(bsr, bsc, f);
}

// (block size, lanes per node) of the lane-group kernels of a level
template <class F>
void with_level(const amg_level& v, F&& f) {
    with_bs(v.bs, [&](auto BS) { with_int<8, 32>(v.lw, [&](auto LW) { f(BS, LW); }, amg_miss); }, amg_miss);
}

template <bool RESID, class T, class TO>
void sweep(const amg_level& v, const double* omega, const T* r, const T* x, TO* out, hipStream_t s) {
    const level_view<T> w(v);
    with_level(v, [&](auto BS, auto LW) {
        amg_launch(amg_sweep<BS, LW, RESID, T, TO>, v.n_nodes, DXO_AMG_BLOCK / LW, s, v.n_nodes, v.A->d_row_ptr, v.A->d_col, w.values, w.dinv, omega, r, x,
                   out);
    });
}

template <class T, class TO>
void cheby_step(const amg_level& v, const double* c, const T* r, const T* x, TO* out, hipStream_t s) {
    const level_view<T> w(v);
    with_level(v, [&](auto BS, auto LW) {
        amg_launch(amg_cheby_sweep<BS, LW, T, TO>, v.n_nodes, DXO_AMG_BLOCK / LW, s, v.n_nodes, v.A->d_row_ptr, v.A->d_col, w.values, w.dinv, c, r, x, w.d,
                   out);
    });
}

int64_t rho_parts(const amg_level& v) { return std::max<int64_t>(1, (v.n_nodes + DXO_AMG_BLOCK / v.lw - 1) / (DXO_AMG_BLOCK / v.lw)); }
int64_t init_parts(const amg_level& v) { return std::max<int64_t>(1, (v.n_rows + DXO_AMG_BLOCK - 1) / DXO_AMG_BLOCK); }

// ---- host: the symbolic phase
struct HostGraph {                      // node graph of a block pattern: sorted neighbours, the node itself included
    int64_t n = 0;
    std::vector<int64_t> ptr;
    std::vector<int32_t> nb;
};

HostGraph graph_of(const std::vector<int64_t>& row_ptr, const std::vector<int32_t>& col, int64_t n_nodes, int bs) {
    HostGraph g;
    g.n = n_nodes;
    g.ptr.assign((size_t)n_nodes + 1, 0);
    for (int64_t i = 0; i < n_nodes; ++i) g.ptr[(size_t)i + 1] = g.ptr[(size_t)i] + (row_ptr[(size_t)(i * bs) + 1] - row_ptr[(size_t)(i * bs)]) / bs;
    g.nb.resize((size_t)g.ptr.back());
    for (int64_t i = 0; i < n_nodes; ++i) {
        const int64_t r0 = row_ptr[(size_t)(i * bs)];
        const int64_t nnb = g.ptr[(size_t)i + 1] - g.ptr[(size_t)i];
        for (int64_t k = 0; k < nnb; ++k) g.nb[(size_t)(g.ptr[(size_t)i] + k)] = col[(size_t)(r0 + k * bs)] / bs;
    }
    return g;
}

// three passes in ascending node order; inactive nodes keep -1. Returns the number of aggregates
int64_t aggregate(const HostGraph& g, const std::vector<uint8_t>& active, std::vector<int32_t>& agg) {
    const int64_t n = g.n;
    agg.assign((size_t)n, -1);
    int32_t na = 0;
    for (int64_t i = 0; i < n; ++i) {                    // 1: a free neighbourhood founds an aggregate
        if (!active[(size_t)i]) continue;
        bool free_nb = true;
        for (int64_t e = g.ptr[(size_t)i]; e < g.ptr[(size_t)i + 1] && free_nb; ++e) {
            const int32_t j = g.nb[(size_t)e];
            if (active[(size_t)j] && agg[(size_t)j] >= 0) free_nb = false;
        }
        if (!free_nb) continue;
        for (int64_t e = g.ptr[(size_t)i]; e < g.ptr[(size_t)i + 1]; ++e) {
            const int32_t j = g.nb[(size_t)e];
            if (active[(size_t)j]) agg[(size_t)j] = na;
        }
        agg[(size_t)i] = na++;
    }
    const std::vector<int32_t> first(agg);
    for (int64_t i = 0; i < n; ++i) {                    // 2: join the lowest pass-1 aggregate of a neighbour
        if (!active[(size_t)i] || first[(size_t)i] >= 0) continue;
        int32_t best = -1;
        for (int64_t e = g.ptr[(size_t)i]; e < g.ptr[(size_t)i + 1]; ++e) {
            const int32_t a = first[(size_t)g.nb[(size_t)e]];
            if (a >= 0 && (best < 0 || a < best)) best = a;
        }
        agg[(size_t)i] = best;
    }
    for (int64_t i = 0; i < n; ++i) {                    // 3: the rest found aggregates with their free neighbours
        if (!active[(size_t)i] || agg[(size_t)i] >= 0) continue;
        for (int64_t e = g.ptr[(size_t)i]; e < g.ptr[(size_t)i + 1]; ++e) {
            const int32_t j = g.nb[(size_t)e];
            if (active[(size_t)j] && agg[(size_t)j] < 0) agg[(size_t)j] = na;
        }
        agg[(size_t)i] = na++;
    }
    return na;
}

struct HostTransfer {
    std::vector<int64_t> p_ptr, pt_ptr, pt_blk, ap_ptr, c_bptr;
    std::vector<int32_t> p_col, p_row, ap_col, ap_row, c_row;
    HostGraph coarse;
};

void sort_unique(std::vector<int32_t>& v) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
}

// the tables that follow from the rows of P (p_ptr, p_col, p_row of t, na columns) and the graph g of the matrix
void transfer_tables(HostTransfer& t, const HostGraph& g, int64_t na) {
    const int64_t n = g.n;
    std::vector<int32_t> tmp;
    t.pt_ptr.assign((size_t)na + 1, 0);                  // its transposed incidence, ascending block = ascending fine node
    for (int32_t a : t.p_col) ++t.pt_ptr[(size_t)a + 1];
    for (int64_t a = 0; a < na; ++a) t.pt_ptr[(size_t)a + 1] += t.pt_ptr[(size_t)a];
    t.pt_blk.resize(t.p_col.size());
    {
        std::vector<int64_t> fill(t.pt_ptr.begin(), t.pt_ptr.end() - 1);
        for (size_t e = 0; e < t.p_col.size(); ++e) t.pt_blk[(size_t)fill[(size_t)t.p_col[e]]++] = (int64_t)e;
    }
    t.ap_ptr.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {                    // A P: the union of the rows of P of the neighbours
        tmp.clear();
        for (int64_t e = g.ptr[(size_t)i]; e < g.ptr[(size_t)i + 1]; ++e) {
            const int64_t j = g.nb[(size_t)e];
            tmp.insert(tmp.end(), t.p_col.begin() + t.p_ptr[(size_t)j], t.p_col.begin() + t.p_ptr[(size_t)j + 1]);
        }
        sort_unique(tmp);
        t.ap_col.insert(t.ap_col.end(), tmp.begin(), tmp.end());
        t.ap_row.insert(t.ap_row.end(), tmp.size(), (int32_t)i);
        t.ap_ptr[(size_t)i + 1] = (int64_t)t.ap_col.size();
    }
    t.coarse.n = na;                                     // P^T (A P): the union of the rows of A P over a column of P, and the diagonal
    t.coarse.ptr.assign((size_t)na + 1, 0);
    for (int64_t a = 0; a < na; ++a) {
        tmp.clear();
        tmp.push_back((int32_t)a);
        for (int64_t e = t.pt_ptr[(size_t)a]; e < t.pt_ptr[(size_t)a + 1]; ++e) {
            const int64_t i = t.p_row[(size_t)t.pt_blk[(size_t)e]];
            tmp.insert(tmp.end(), t.ap_col.begin() + t.ap_ptr[(size_t)i], t.ap_col.begin() + t.ap_ptr[(size_t)i + 1]);
        }
        sort_unique(tmp);
        t.coarse.nb.insert(t.coarse.nb.end(), tmp.begin(), tmp.end());
        t.c_row.insert(t.c_row.end(), tmp.size(), (int32_t)a);
        t.coarse.ptr[(size_t)a + 1] = (int64_t)t.coarse.nb.size();
    }
    t.c_bptr = t.coarse.ptr;
}

// gp: the graph P is smoothed with (the strong graph; g itself without strength of connection)
HostTransfer transfer_of(const HostGraph& gp, const HostGraph& g, const std::vector<int32_t>& agg, int64_t na) {
    HostTransfer t;
    const int64_t n = g.n;
    std::vector<int32_t> tmp;
    t.p_ptr.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {                    // P: the aggregates of the neighbours
        tmp.clear();
        for (int64_t e = gp.ptr[(size_t)i]; e < gp.ptr[(size_t)i + 1]; ++e)
            if (agg[(size_t)gp.nb[(size_t)e]] >= 0) tmp.push_back(agg[(size_t)gp.nb[(size_t)e]]);
        sort_unique(tmp);
        t.p_col.insert(t.p_col.end(), tmp.begin(), tmp.end());
        t.p_row.insert(t.p_row.end(), tmp.size(), (int32_t)i);
        t.p_ptr[(size_t)i + 1] = (int64_t)t.p_col.size();
    }
    transfer_tables(t, g, na);
    return t;
}

// the rows of P as the caller gave them (dxo_amg_create_transfer; validated there)
HostTransfer transfer_given(const HostGraph& g, const dxo_amg_transfer& w) {
    HostTransfer t;
    t.p_ptr.assign(w.ptr, w.ptr + g.n + 1);
    t.p_col.assign(w.col, w.col + w.ptr[g.n]);
    t.p_row.resize(t.p_col.size());
    for (int64_t i = 0; i < g.n; ++i)
        for (int64_t e = w.ptr[i]; e < w.ptr[i + 1]; ++e) t.p_row[(size_t)e] = (int32_t)i;
    transfer_tables(t, g, w.n_coarse);
    return t;
}

// the csr.h layout of a node graph
void rows_of(const HostGraph& g, int bs, std::vector<int64_t>& row_ptr, std::vector<int32_t>& col) {
    row_ptr.assign((size_t)(g.n * bs) + 1, 0);
    for (int64_t i = 0; i < g.n; ++i)
        for (int r = 0; r < bs; ++r) row_ptr[(size_t)(i * bs + r) + 1] = row_ptr[(size_t)(i * bs + r)] + bs * (g.ptr[(size_t)i + 1] - g.ptr[(size_t)i]);
    col.resize((size_t)row_ptr.back());
    for (int64_t i = 0; i < g.n; ++i)
        for (int r = 0; r < bs; ++r) {
            int64_t w = row_ptr[(size_t)(i * bs + r)];
            for (int64_t e = g.ptr[(size_t)i]; e < g.ptr[(size_t)i + 1]; ++e)
                for (int c = 0; c < bs; ++c) col[(size_t)w++] = g.nb[(size_t)e] * bs + c;
        }
}

struct Uploader {
    dxo_ctx* ctx;
    dxo_amg* amg;
    const char* who;                   // the entry point, for the error text
    int rc = DXO_OK;
    template <class T>
    T* alloc(size_t n) {
        if (rc != DXO_OK) return nullptr;
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T) + 16);
        if (e != hipSuccess) {
            rc = dxo_hip_fail(ctx, e, (std::string(who) + ": hipMalloc").c_str());
            return nullptr;
        }
        amg->allocs.push_back(p);
        return (T*)p;
    }
    template <class T>
    T* up(const std::vector<T>& v) {
        T* p = alloc<T>(v.size());
        if (p && !v.empty()) {
            const hipError_t e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
            if (e != hipSuccess) rc = dxo_hip_fail(ctx, e, (std::string(who) + ": hipMemcpy").c_str());
        }
        return p;
    }
};

void amg_free(dxo_amg* a) {
    for (void* p : a->allocs) (void)hipFree(p);
    for (amg_level& v : a->L) delete v.own;
    delete a;
}

int lanes_for(int64_t nnzb, int64_t n_nodes) { return n_nodes > 0 && (double)nnzb / (double)n_nodes > 16.0 ? 32 : 8; }

// lanes per aggregate of amg_tentative from the mean number of rows of an aggregate
int tentative_lanes(int64_t rows, int64_t n_agg) {
    const double mean = n_agg > 0 ? (double)rows / (double)n_agg : 0.0;
    return mean > 32.0 ? 64 : mean > 16.0 ? 32 : mean > 8.0 ? 16 : 8;
}

// the nodes of every aggregate, ascending
void nodes_of_aggregates(const std::vector<int32_t>& agg, int64_t na, std::vector<int64_t>& ptr, std::vector<int32_t>& node) {
    ptr.assign((size_t)na + 1, 0);
    for (int32_t a : agg)
        if (a >= 0) ++ptr[(size_t)a + 1];
    for (int64_t a = 0; a < na; ++a) ptr[(size_t)a + 1] += ptr[(size_t)a];
    node.resize((size_t)ptr.back());
    std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1);
    for (size_t i = 0; i < agg.size(); ++i)
        if (agg[i] >= 0) node[(size_t)fill[(size_t)agg[i]]++] = (int32_t)i;
}

bool amg_misaligned(const void* p) { return ((uintptr_t)p & 7u) != 0; }

// the near-null space at creation: B_0 = the caller's B with the rows of constrained dofs zero, ...
int amg_nns_first(dxo_ctx* ctx, dxo_amg* amg, const amg_level& f, const double* B, hipStream_t s) {
    if (f.n_rows > 0) {
        DXO_HIP(ctx, hipMemcpyAsync(f.b_val, B, (size_t)(f.n_rows * amg->k) * sizeof(double), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(amg_zero_rows, amg_grid(f.n_rows), dim3(DXO_AMG_BLOCK), 0, s, f.n_rows, amg->k, f.mask, f.b_val);
    }
    return DXO_OK;
}

// ... then level by level T_l and B_{l+1}, as soon as the aggregates of level l are known ...
int amg_nns_level(dxo_ctx* ctx, dxo_amg* amg, const amg_level& v, double* b_next, hipStream_t s) {
    const double tol = std::pow(10.0, -(double)ctx->amg_rank_tol);
    DXO_HIP(ctx, hipMemsetAsync(v.t_val, 0, (size_t)(v.n_nodes * v.bs * amg->k) * sizeof(double), s));      // nodes without an aggregate
    if (v.n_agg > 0)
        with_nns_pair(v.bs, v.bsc, [&](auto BSR, auto K) {
            with_int<8, 16, 32, 64>(v.tl, [&](auto LG) {
                amg_launch(amg_tentative<BSR, K, LG>, v.n_agg, DXO_AMG_BLOCK / LG, s, v.n_agg, v.agg_ptr, v.agg_node, v.b_val, tol, v.t_val, b_next, v.dead_a);
            }, amg_miss);
        });
    return DXO_OK;
}

// ... and the dead columns of every level, after a wait
int amg_nns_dead(dxo_ctx* ctx, dxo_amg* amg, hipStream_t s) {
    const int nl = (int)amg->L.size();
    DXO_HIP(ctx, hipGetLastError());
    DXO_HIP(ctx, hipStreamSynchronize(s));
    for (int l = 0; l + 1 < nl; ++l) {
        amg_level& v = amg->L[(size_t)l];
        std::vector<uint8_t> d((size_t)v.n_agg);
        if (v.n_agg > 0 && v.dead_a) DXO_HIP(ctx, hipMemcpy(d.data(), v.dead_a, d.size(), hipMemcpyDeviceToHost));      // none: a given transfer
        v.dead = 0;
        for (uint8_t x : d) v.dead += x;
    }
    return DXO_OK;
}

// rho, omega = (4/3) / rho and (unfiltered only) the Chebyshev pairs of a level from the estimate chosen by dxo_amg_set_smoother;
// filtered: of Dinv_F A^F, for the prolongator smoothing alone
void amg_estimate_rho(dxo_amg* amg, const amg_level& v, bool filtered, double* rho, double* omega, double* cheb, hipStream_t s) {
    const dim3 B(DXO_AMG_BLOCK);
    const double* dinv = filtered ? v.dinv_f : v.dinv;
    const uint8_t* strong = filtered ? v.strong : nullptr;
    if (amg->rho_kind == DXO_AMG_RHO_POWER) {
        // v_0 in xa, then w = Dinv A (v / |v|) back and forth between xa and xb: the cycle's vectors are free during a setup
        double *from = v.xa, *to = v.xb;
        hipLaunchKernelGGL(amg_power_init, amg_grid(v.n_rows), B, 0, s, v.n_rows, from, amg->part);
        hipLaunchKernelGGL(amg_power_norm, dim3(1), B, 0, s, amg->part, init_parts(v), 0, amg->safety, amg->lower, amg->degree, amg->scal, rho, omega,
                           cheb);
        for (int it = 0; it < amg->rho_iters; ++it) {
            with_level(v, [&](auto BS, auto LW) {
                amg_launch(amg_power_step<BS, LW>, v.n_nodes, DXO_AMG_BLOCK / LW, s, v.n_nodes, v.A->d_row_ptr, v.A->d_col, v.values, dinv, strong, v.diag_f,
                           amg->scal, from, to, amg->part);
            });
            hipLaunchKernelGGL(amg_power_norm, dim3(1), B, 0, s, amg->part, rho_parts(v), it + 1 == amg->rho_iters ? 1 : 0, amg->safety, amg->lower,
                               amg->degree, amg->scal, rho, omega, cheb);
            std::swap(from, to);
        }
    } else {
        with_level(v, [&](auto BS, auto LW) {
            amg_launch(amg_rho<BS, LW>, v.n_nodes, DXO_AMG_BLOCK / LW, s, v.n_nodes, v.A->d_row_ptr, v.A->d_col, v.values, dinv, strong, v.diag_f, amg->part);
        });
        hipLaunchKernelGGL(amg_omega, dim3(1), B, 0, s, amg->part, rho_parts(v), omega, rho);
        if (!filtered && amg->smooth_kind == DXO_AMG_SMOOTH_CHEBYSHEV)
            hipLaunchKernelGGL(amg_cheby_coeffs, dim3(1), dim3(64), 0, s, rho, amg->lower, amg->degree, cheb);
    }
}

// the numeric phase of level l: from the values of v to those of the next level c
void amg_setup_level(dxo_amg* amg, int l, const amg_level& v, const amg_level& c, hipStream_t s) {
    const bool nns = amg->k > 0;
    (void)dxo_kr_bj_setup_launch(v.A, v.values, v.dinv, amg->flag, s);      // a level has block size 1, 2, 3 or 6 (with_bs)
    if (v.p_diag) {      // a given transfer: P is frozen, and the mask of the next level with it; the level keeps what it smooths with
        amg_estimate_rho(amg, v, false, amg->rho + l, amg->omega + l, amg->cheb + (size_t)l * AMG_CHEB_STRIDE, s);
        with_square(v.bs, v.bsc, [&](auto BS, auto) {
            amg_launch(amg_build_ap_w<BS>, v.ap_blocks, DXO_AMG_BLOCK, s, v.ap_blocks, v.ap_row, v.ap_col, v.A->d_row_ptr, v.A->d_col, v.values, v.p_ptr,
                       v.p_col, v.p_diag, v.ap_val);
            amg_launch(amg_build_c_w<BS>, v.c_blocks, DXO_AMG_BLOCK, s, v.c_blocks, v.c_row, v.c_bptr, c.A->d_row_ptr, c.A->d_col, v.pt_ptr, v.pt_blk,
                       v.p_row, v.p_diag, v.ap_ptr, v.ap_col, v.ap_val, const_cast<double*>(c.values));
        });
        return;
    }
    const double* omega_p = amg->omega + l;
    if (v.strong) {
        with_bs(v.bs, [&](auto BS) {
            amg_launch(amg_lump<BS>, v.n_nodes, DXO_AMG_BLOCK, s, v.n_nodes, v.A->d_row_ptr, v.A->d_col, v.values, v.strong, v.dinv, v.diag_f, v.dinv_f,
                       v.unlumped);
        }, amg_miss);
        amg_estimate_rho(amg, v, true, amg->rho_f + l, amg->omega_f + l, amg->cheb_f, s);
        omega_p = amg->omega_f + l;      // P is smoothed with the filtered matrix: dinv_f and omega_F
    }
    amg_estimate_rho(amg, v, false, amg->rho + l, amg->omega + l, amg->cheb + (size_t)l * AMG_CHEB_STRIDE, s);
    auto build_p = [&](auto BSR, auto BSC, auto NNS) {
        amg_launch(amg_build_p<BSR, BSC, NNS>, v.p_blocks, DXO_AMG_BLOCK, s, v.p_blocks, v.p_row, v.p_col, v.A->d_row_ptr, v.A->d_col, v.values,
                   v.strong ? v.dinv_f : v.dinv, v.agg, v.mask, v.t_val, omega_p, v.strong, v.diag_f, v.p_val);
    };
    if (nns) with_nns_pair(v.bs, v.bsc, [&](auto BSR, auto BSC) { build_p(BSR, BSC, std::true_type{}); });
    else with_square(v.bs, v.bsc, [&](auto BSR, auto BSC) { build_p(BSR, BSC, std::false_type{}); });
    with_pair(v.bs, v.bsc, [&](auto BSR, auto BSC) {
        amg_launch(amg_build_ap<BSR, BSC>, v.ap_blocks, DXO_AMG_BLOCK, s, v.ap_blocks, v.ap_row, v.ap_col, v.A->d_row_ptr, v.A->d_col, v.values, v.p_ptr,
                   v.p_col, v.p_val, v.ap_val);
        amg_launch(amg_build_c<BSR, BSC>, v.c_blocks, DXO_AMG_BLOCK, s, v.c_blocks, v.c_row, v.c_bptr, c.A->d_row_ptr, c.A->d_col, v.pt_ptr, v.pt_blk,
                   v.p_row, v.p_val, v.ap_ptr, v.ap_col, v.ap_val, const_cast<double*>(c.values));
    });
    // the values-dependent mask belongs to the identity form of T; with a near-null space T is fixed at creation
    if (!nns) hipLaunchKernelGGL(amg_row_mask, amg_grid(c.n_rows), dim3(DXO_AMG_BLOCK), 0, s, c.n_rows, c.A->d_row_ptr, c.A->d_col, c.values, c.mask);
}

// the strong part of a node graph: mask[e] per entry of g
HostGraph strong_graph(const HostGraph& g, const std::vector<uint8_t>& mask) {
    HostGraph gs;
    gs.n = g.n;
    gs.ptr.assign((size_t)g.n + 1, 0);
    for (int64_t i = 0; i < g.n; ++i) {
        for (int64_t e = g.ptr[(size_t)i]; e < g.ptr[(size_t)i + 1]; ++e)
            if (mask[(size_t)e]) gs.nb.push_back(g.nb[(size_t)e]);
        gs.ptr[(size_t)i + 1] = (int64_t)gs.nb.size();
    }
    return gs;
}

// what the three creators ask for
struct amg_options {
    int max_levels = 0, coarse_rows = 0, sweeps = 1;
    int k = 0;                         // columns of the near-null space (every coarse level then has block size k); 0: none (every level
    const double* B = nullptr;         // keeps the block size). B: the near-null space [n_rows][k] on the device
    double theta = 0.0;                // strength of connection: > 0 with `values`, the matrix; every level is then followed by its numeric
    const double* values = nullptr;    // phase, whose coarse matrix gives the mask of the next level
    const dxo_amg_transfer* first = nullptr;      // the given transfer of level 0 (host arrays, validated); strength then starts on level 1
};

// the pattern and the constraints on the host: the node graph, the constrained dofs, the nodes with a free dof
int amg_read_pattern(dxo_ctx* ctx, const dxo_csr* csr, const int32_t* constrained, int64_t n_constrained, HostGraph& g, std::vector<uint8_t>& mask,
                     std::vector<uint8_t>& active) {
    std::vector<int64_t> row_ptr((size_t)csr->n_rows + 1);
    std::vector<int32_t> col((size_t)csr->nnz);
    DXO_HIP(ctx, hipMemcpy(row_ptr.data(), csr->d_row_ptr, row_ptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (csr->nnz > 0) DXO_HIP(ctx, hipMemcpy(col.data(), csr->d_col, col.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    mask.assign((size_t)csr->n_rows, 0);
    if (n_constrained > 0) {
        std::vector<int32_t> dofs((size_t)n_constrained);
        DXO_HIP(ctx, hipMemcpy(dofs.data(), constrained, dofs.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int32_t d : dofs)
            if (d >= 0 && d < csr->n_rows) mask[(size_t)d] = 1;
    }
    g = graph_of(row_ptr, col, csr->n_nodes, csr->bs);
    active.assign((size_t)g.n, 1);
    for (int64_t i = 0; i < g.n; ++i) {
        bool all = true;
        for (int r = 0; r < csr->bs; ++r) all = all && mask[(size_t)(i * csr->bs + r)];
        active[(size_t)i] = all ? 0 : 1;
    }
    return DXO_OK;
}

// the strength mask of a level from its values: |A_ii|_F in xa (free until the first cycle), the mask on the device and, after the
// one wait of this level, on the host as the strong graph
int amg_strength_mask(dxo_ctx* ctx, Uploader& U, const amg_level& v, const HostGraph& g, double theta, hipStream_t s, uint8_t*& d_strong,
                      int64_t& n_strong, HostGraph& gs) {
    d_strong = U.alloc<uint8_t>((size_t)v.nnzb);
    if (U.rc != DXO_OK) return U.rc;
    std::vector<uint8_t> hmask((size_t)v.nnzb);
    with_level(v, [&](auto BS, auto LW) {
        amg_launch(amg_diag_norm<BS>, v.n_nodes, DXO_AMG_BLOCK, s, v.n_nodes, v.A->d_row_ptr, v.A->d_col, v.values, v.xa);
        amg_launch(amg_strength<BS, LW>, v.n_nodes, DXO_AMG_BLOCK / LW, s, v.n_nodes, v.A->d_row_ptr, v.A->d_col, v.values, v.xa, theta * theta, d_strong);
    });
    DXO_HIP(ctx, hipGetLastError());
    if (v.nnzb > 0) DXO_HIP(ctx, hipMemcpyAsync(hmask.data(), d_strong, hmask.size(), hipMemcpyDeviceToHost, s));
    DXO_HIP(ctx, hipStreamSynchronize(s));
    n_strong = 0;
    for (uint8_t m : hmask) n_strong += m;
    gs = strong_graph(g, hmask);
    return DXO_OK;
}

// the tables and the value arrays of the transfer from a level to the next, on the device
void amg_upload_transfer(Uploader& U, amg_level& v, const HostTransfer& t, const std::vector<int32_t>& agg, int64_t na, bool given) {
    v.n_agg = na;
    v.p_blocks = (int64_t)t.p_col.size();
    v.ap_blocks = (int64_t)t.ap_col.size();
    v.c_blocks = (int64_t)t.c_row.size();
    if (!given) v.agg = U.up(agg);
    v.p_ptr = U.up(t.p_ptr);
    v.p_col = U.up(t.p_col);
    v.p_row = U.up(t.p_row);
    v.pt_ptr = U.up(t.pt_ptr);
    v.pt_blk = U.up(t.pt_blk);
    v.ap_ptr = U.up(t.ap_ptr);
    v.ap_col = U.up(t.ap_col);
    v.ap_row = U.up(t.ap_row);
    v.c_bptr = U.up(t.c_bptr);
    v.c_row = U.up(t.c_row);
    if (!given) v.p_val = U.alloc<double>((size_t)(v.p_blocks * v.bs * v.bsc));      // given: p_diag, filled by the caller
    v.ap_val = U.alloc<double>((size_t)(v.ap_blocks * v.bs * v.bsc));
}

// the coarse level of a node graph: a dxo_csr without a mesh, its values and its B (k > 0) or mask. `fixed`: the level below a given
// transfer, whose mask is the constraints of its nodes, known now (kept beside B too: it is a finest level in all but its matrix)
amg_level amg_coarse_level(Uploader& U, const HostGraph& coarse, int bsc, int k, const std::vector<uint8_t>* fixed = nullptr) {
    std::vector<int64_t> crp;
    std::vector<int32_t> ccol;
    rows_of(coarse, bsc, crp, ccol);
    amg_level c;
    c.own = new dxo_csr;
    c.own->bs = bsc;
    c.own->n_nodes = coarse.n;
    c.own->n_rows = coarse.n * bsc;
    c.own->nnz = crp.back();
    c.own->d_row_ptr = U.up(crp);
    c.own->d_col = U.up(ccol);
    c.A = c.own;
    c.n_nodes = coarse.n;
    c.n_rows = coarse.n * bsc;
    c.nnzb = (int64_t)coarse.nb.size();
    c.bs = c.bsc = bsc;
    c.values = U.alloc<double>((size_t)c.own->nnz);
    if (k > 0) c.b_val = U.alloc<double>((size_t)(c.n_rows * k));      // T is fixed at creation: no values-dependent mask
    if (fixed) c.mask = U.up(*fixed);
    else if (k == 0) c.mask = U.alloc<uint8_t>((size_t)c.n_rows);
    return c;
}

// the symbolic phase, level by level; with a near-null space T_l and B_{l+1} follow the aggregates of level l at once, and a level
// with a strength mask is followed by its numeric phase, which gives the matrix the next mask is made from
int amg_build(dxo_ctx* ctx, const char* who, dxo_amg* amg, const dxo_csr* csr, const int32_t* constrained, int64_t n_constrained,
              const amg_options& opt, hipStream_t s) {
    const bool soc = opt.theta > 0.0;
    const int k = opt.k, bsc = k > 0 ? k : csr->bs;
    Uploader U{ctx, amg, who};
    HostGraph g;
    std::vector<uint8_t> mask, active;
    int rc = amg_read_pattern(ctx, csr, constrained, n_constrained, g, mask, active);
    if (rc != DXO_OK) return rc;
    amg_level lev;
    lev.A = csr;
    lev.n_nodes = csr->n_nodes;
    lev.n_rows = csr->n_rows;
    lev.nnzb = (int64_t)g.nb.size();
    lev.mask = U.up(mask);
    lev.bs = csr->bs;
    lev.bsc = bsc;
    lev.values = opt.values;
    if (k > 0) lev.b_val = U.alloc<double>((size_t)(lev.n_rows * k));
    const int64_t nnzb0 = std::max<int64_t>(1, lev.nnzb * lev.bs * lev.bs);
    int64_t total = 0;
    // what the numeric phase needs, before the number of levels is known: every level keeps at most 0.8 of its parent's rows
    const int max_levels = std::min(opt.max_levels, 128);
    amg->part_cap = (lev.n_nodes + 7) / 8 + 1;     // no level has more nodes than the first, and at least 8 nodes go to a workgroup
    amg->omega = U.alloc<double>((size_t)max_levels);
    amg->rho = U.alloc<double>((size_t)max_levels);
    amg->cheb = U.alloc<double>((size_t)max_levels * AMG_CHEB_STRIDE);
    amg->omega_f = U.alloc<double>((size_t)max_levels);
    amg->rho_f = U.alloc<double>((size_t)max_levels);
    amg->cheb_f = U.alloc<double>(AMG_CHEB_STRIDE);
    amg->scal = U.alloc<double>(2);
    amg->part = U.alloc<double>((size_t)amg->part_cap);
    amg->flag = U.alloc<int>(4);
    if (U.rc != DXO_OK) return U.rc;
    DXO_HIP(ctx, hipMemsetAsync(amg->flag, 0, 4 * sizeof(int), s));
    if (k > 0 && (rc = amg_nns_first(ctx, amg, lev, opt.B, s)) != DXO_OK) return rc;
    for (;;) {
        lev.lw = lanes_for(lev.nnzb, lev.n_nodes);
        total += lev.nnzb * lev.bs * lev.bs;
        bool last = lev.n_rows <= opt.coarse_rows || (int)amg->L.size() + 1 >= max_levels;
        std::vector<int32_t> agg;
        int64_t na = 0;
        lev.r = U.alloc<double>((size_t)lev.n_rows);
        lev.xa = U.alloc<double>((size_t)lev.n_rows);
        HostGraph gs;
        uint8_t* d_strong = nullptr;
        int64_t n_strong = 0;
        const bool given = opt.first && amg->L.empty();      // level 0 of dxo_amg_create_transfer: no mask, no aggregates
        if (!last && !given && soc && (rc = amg_strength_mask(ctx, U, lev, g, opt.theta, s, d_strong, n_strong, gs)) != DXO_OK) return rc;
        const HostGraph& gp = d_strong ? gs : g;      // the graph of the aggregates and of the pattern of P
        if (!last && given) {
            na = opt.first->n_coarse;                  // below the 0.8 of the stagnation rule: checked with the arrays
            lev.bsc = lev.bs;
        } else if (!last) {
            na = aggregate(gp, active, agg);
            last = na == 0 || (double)(na * bsc) > 0.8 * (double)lev.n_rows;
        }
        if (last) {
            amg->L.push_back(lev);
            break;
        }
        lev.xb = U.alloc<double>((size_t)lev.n_rows);
        lev.t = U.alloc<double>((size_t)lev.n_rows);
        lev.d = U.alloc<double>((size_t)lev.n_rows);
        lev.dinv = U.alloc<double>((size_t)(lev.n_nodes * lev.bs * lev.bs));
        HostTransfer t = given ? transfer_given(g, *opt.first) : transfer_of(gp, g, agg, na);
        if (d_strong) {
            lev.strong = d_strong;
            lev.n_strong = n_strong;
            lev.diag_f = U.alloc<double>((size_t)(lev.n_nodes * lev.bs * lev.bs));
            lev.dinv_f = U.alloc<double>((size_t)(lev.n_nodes * lev.bs * lev.bs));
            lev.unlumped = U.alloc<uint8_t>((size_t)lev.n_nodes);
        }
        amg_upload_transfer(U, lev, t, agg, na, given);
        std::vector<uint8_t> mask_c;                   // given: the constraints of the coarse nodes, those of the nodes they are
        if (given) {
            const dxo_amg_transfer& w = *opt.first;
            const int bs = lev.bs;
            mask_c.resize((size_t)(na * bs));
            for (int64_t v = 0; v < na; ++v)
                for (int c = 0; c < bs; ++c) mask_c[(size_t)(v * bs + c)] = mask[(size_t)((int64_t)w.coarse_to_fine[v] * bs + c)];
            std::vector<double> pd((size_t)(lev.p_blocks * bs));
            for (int64_t i = 0; i < lev.n_nodes; ++i)
                for (int64_t e = w.ptr[i]; e < w.ptr[i + 1]; ++e)
                    for (int c = 0; c < bs; ++c)
                        pd[(size_t)(e * bs + c)] = w.w[e] * (mask[(size_t)(i * bs + c)] ? 0.0 : 1.0) * (mask_c[(size_t)((int64_t)w.col[e] * bs + c)] ? 0.0 : 1.0);
            lev.p_diag = U.up(pd);
            lev.ctf = U.up(std::vector<int32_t>(w.coarse_to_fine, w.coarse_to_fine + na));
        }
        if (k > 0 && !given) {
            std::vector<int64_t> aptr;
            std::vector<int32_t> anode;
            nodes_of_aggregates(agg, na, aptr, anode);
            lev.tl = tentative_lanes((int64_t)anode.size() * lev.bs, na);
            lev.agg_ptr = U.up(aptr);
            lev.agg_node = U.up(anode);
            lev.t_val = U.alloc<double>((size_t)(lev.n_nodes * lev.bs * k));
            lev.dead_a = U.alloc<uint8_t>((size_t)na);
        }
        amg->L.push_back(lev);
        amg_level c = given ? amg_coarse_level(U, t.coarse, lev.bs, k, &mask_c) : amg_coarse_level(U, t.coarse, bsc, k);
        if (given) c.bsc = bsc;        // the first level of the aggregation
        rc = U.rc;
        if (rc == DXO_OK && k > 0 && !given) rc = amg_nns_level(ctx, amg, lev, c.b_val, s);
        if (rc == DXO_OK && k > 0 && given && c.n_rows > 0)      // degree-1 functions reproduce the rigid-body modes: B_1 is B_0 at the coarse nodes
            hipLaunchKernelGGL(amg_gather_b, amg_grid(c.n_rows), dim3(DXO_AMG_BLOCK), 0, s, c.n_rows, lev.bs, k, lev.ctf, lev.b_val, c.b_val);
        if (rc != DXO_OK) {
            amg->L.push_back(c);       // owned: freed with the object
            return rc;
        }
        if ((lev.strong || (given && soc)) && lev.n_nodes > 0) amg_setup_level(amg, (int)amg->L.size() - 1, lev, c, s);
        lev = c;
        g = std::move(t.coarse);
        active.assign((size_t)g.n, 1);
        if (given)                     // as on a finest level: a node all of whose dofs are constrained joins no aggregate
            for (int64_t v = 0; v < g.n; ++v) {
                bool all = true;
                for (int r = 0; r < lev.bs; ++r) all = all && mask_c[(size_t)(v * lev.bs + r)];
                active[(size_t)v] = all ? 0 : 1;
            }
    }
    if (U.rc != DXO_OK) return U.rc;
    amg->complexity = (double)total / (double)nnzb0;
    amg->nc = amg->L.back().n_rows;
    if (amg->nc > AMG_MAX_DENSE) {
        char msg[200];
        snprintf(msg, sizeof msg, "%s: the coarsest level keeps %lld rows, the dense solve takes at most %lld (raise max_levels)", who,
                 (long long)amg->nc, (long long)AMG_MAX_DENSE);
        return dxo_fail(ctx, DXO_E_SIZE, msg);
    }
    for (const amg_level& v : amg->L)      // a defect of the sizing rule above, not of the caller
        if (std::max(rho_parts(v), init_parts(v)) > amg->part_cap) return dxo_fail(ctx, DXO_E_SIZE, "amg.hip: a level outgrew the partials of the first");
    if (soc) {                             // the numeric phases that ran: their one flag word
        int h = 0;
        DXO_HIP(ctx, hipGetLastError());
        DXO_HIP(ctx, hipMemcpyAsync(&h, amg->flag, sizeof h, hipMemcpyDeviceToHost, s));
        DXO_HIP(ctx, hipStreamSynchronize(s));
        if (h) return dxo_fail(ctx, DXO_E_SINGULAR, (std::string(who) + ": a diagonal block of a level is singular").c_str());
    }
    amg->dense[0] = U.alloc<double>((size_t)(2 * amg->nc * amg->nc));
    amg->dense[1] = U.alloc<double>((size_t)(2 * amg->nc * amg->nc));
    return U.rc;
}

}  // namespace

// ---- shared with krylov.hip
int dxo_amg_pc_check(dxo_ctx* ctx, const char* who, const dxo_amg* amg, const dxo_csr* op_csr, int bs, int64_t n) {
    char msg[256];
    if (!amg) return dxo_fail(ctx, DXO_E_NULL, (std::string(who) + ": the preconditioner carries no dxo_amg").c_str());
    if (bs != amg->bs || (op_csr && op_csr->bs != amg->bs)) {
        snprintf(msg, sizeof msg, "%s: multigrid of bs %d on a pattern of bs %d", who, amg->bs, op_csr ? op_csr->bs : bs);
        return dxo_fail(ctx, DXO_E_DIM, msg);
    }
    if (n != amg->L[0].n_rows) {
        snprintf(msg, sizeof msg, "%s: the multigrid covers %lld rows, the operator has %lld", who, (long long)amg->L[0].n_rows, (long long)n);
        return dxo_fail(ctx, DXO_E_SIZE, msg);
    }
    if (!amg->ready) return dxo_fail(ctx, DXO_E_OPTION, (std::string(who) + ": dxo_amg_setup has not run (or failed)").c_str());
    return DXO_OK;
}

namespace {

struct CycleRun {
    dxo_ctx* ctx;
    dxo_amg* amg;
    hipStream_t s;
    bool cheby;
    int nl, nu;                        // levels; sweeps or the Chebyshev degree
};

template <class T>
const T* amg_solve_level(const CycleRun& C, int l, const T* rin);

// the cycle body of level l in the scalar T: B_l(rin). The result lies in `out` (always double: the caller's z, or a K vector) if one
// is given, and nothing is returned then: the last sweep of the post-smoothing writes it there. Otherwise it lies in xa or xb of the
// level; the coarsest level is the dense product into xa
template <class T>
const T* amg_body(const CycleRun& C, int l, const T* rin, double* out) {
    dxo_amg* amg = C.amg;
    const hipStream_t s = C.s;
    amg_level& v = amg->L[(size_t)l];
    const level_view<T> w(v);
    if (l == C.nl - 1) {
        const double* W = amg->dense[amg->nc % 2];
        hipLaunchKernelGGL(amg_dense_apply<T>, amg_grid(amg->nc, DXO_AMG_BLOCK / 64), dim3(DXO_AMG_BLOCK), 0, s, amg->nc, W, rin, w.xa);
        return w.xa;
    }
    const double* om = amg->omega + l;
    const double* ch = amg->cheb + (size_t)l * AMG_CHEB_STRIDE;
    T *cur = w.xa, *other = w.xb;
    with_bs(v.bs, [&](auto BS) {      // from x = 0: omega Dinv r, or c2 Dinv r into the direction as well
        amg_launch(amg_first_step<BS, T>, v.n_nodes, DXO_AMG_BLOCK, s, v.n_nodes, w.dinv, C.cheby ? ch + 1 : om, rin, C.cheby ? w.d : (T*)nullptr, cur);
    }, amg_miss);
    for (int k = 1; k < C.nu; ++k) {
        if (C.cheby) cheby_step(v, ch + 2 * k, rin, (const T*)cur, other, s);
        else sweep<false>(v, om, rin, (const T*)cur, other, s);
        std::swap(cur, other);
    }
    sweep<true>(v, om, rin, (const T*)cur, w.t, s);
    const level_view<T> wc(amg->L[(size_t)l + 1]);
    const int64_t nrc = v.n_agg * v.bsc;
    if (v.p_diag)
        with_square(v.bs, v.bsc, [&](auto BS, auto) {
            amg_launch(amg_restrict_w<BS, T>, nrc, DXO_AMG_BLOCK, s, nrc, v.pt_ptr, v.pt_blk, v.p_row, w.p_diag, (const T*)w.t, wc.r);
        });
    else
        with_pair(v.bs, v.bsc, [&](auto BSR, auto BSC) {
            amg_launch(amg_restrict<BSR, BSC, T>, v.n_agg, DXO_AMG_BLOCK, s, v.n_agg, v.pt_ptr, v.pt_blk, v.p_row, w.p_val, (const T*)w.t, wc.r);
        });
    const T* xc = amg_solve_level<T>(C, l + 1, wc.r);
    if (v.p_diag)
        with_square(v.bs, v.bsc, [&](auto BS, auto) {
            amg_launch(amg_prolong_w<BS, T>, v.n_rows, DXO_AMG_BLOCK, s, v.n_rows, v.p_ptr, v.p_col, w.p_diag, xc, cur);
        });
    else
        with_pair(v.bs, v.bsc, [&](auto BSR, auto BSC) {
            amg_launch(amg_prolong<BSR, BSC, T>, v.n_nodes, DXO_AMG_BLOCK, s, v.n_nodes, v.p_ptr, v.p_col, w.p_val, xc, cur);
        });
    for (int k = 0; k < C.nu; ++k) {
        if (out && k == C.nu - 1) {      // the last sweep writes the result where the caller wants it
            if (C.cheby) cheby_step(v, ch + 2 * k, rin, (const T*)cur, out, s);
            else sweep<false>(v, om, rin, (const T*)cur, out, s);
            return nullptr;
        }
        if (C.cheby) cheby_step(v, ch + 2 * k, rin, (const T*)cur, other, s);
        else sweep<false>(v, om, rin, (const T*)cur, other, s);
        std::swap(cur, other);
    }
    return cur;
}

// the solution of A_l x = rin the level above prolongs. V-cycle, and the coarsest level of either cycle: the body, once. K-cycle on
// an intermediate level (double only: dxo_amg_set_cycle and dxo_amg_set_precision exclude each other): two GCR steps preconditioned
// by the body
template <class T>
const T* amg_solve_level(const CycleRun& C, int l, const T* rin) {
    dxo_amg* amg = C.amg;
    if (amg->cycle != DXO_AMG_CYCLE_K || l == C.nl - 1) return amg_body<T>(C, l, rin, nullptr);
    if constexpr (std::is_same_v<T, double>) {
        const hipStream_t s = C.s;
        amg_level& v = amg->L[(size_t)l];
        const dim3 G((unsigned)v.knb), B(DXO_AMG_BLOCK), One(1);
        amg_body<double>(C, l, rin, v.kc1);
        (void)dxo_kr_spmv_launch(C.ctx, v.A, v.values, v.kc1, v.kv1, s);      // a level has block size 1, 2, 3 or 6
        hipLaunchKernelGGL(amg_k_dots, G, B, 0, s, v.n_rows, v.kv1, rin, (const double*)nullptr, v.kpart);
        hipLaunchKernelGGL(amg_k_scalar, One, B, 0, s, v.kpart, v.knb, 1, v.kco);
        hipLaunchKernelGGL(amg_k_residual, G, B, 0, s, v.n_rows, v.kco, rin, v.kv1, v.kr1);
        amg_body<double>(C, l, v.kr1, v.kc2);      // reuses xa, xb, t, d of this level and everything below: c1 and v1 are safe in the K vectors
        (void)dxo_kr_spmv_launch(C.ctx, v.A, v.values, v.kc2, v.kv2, s);
        hipLaunchKernelGGL(amg_k_dots, G, B, 0, s, v.n_rows, v.kv2, v.kv1, v.kr1, v.kpart);
        hipLaunchKernelGGL(amg_k_scalar, One, B, 0, s, v.kpart, v.knb, 2, v.kco);
        hipLaunchKernelGGL(amg_k_combine, G, B, 0, s, v.n_rows, v.kco, v.kc1, v.kc2);
        return v.kc1;
    } else {
        amg_no_shape(-1, -1);      // unreachable: a float cycle is a V-cycle
    }
}

// the grid of amg_narrow: one thread per entry up to a cap, the stride of the loop beyond it
dim3 narrow_grid(int64_t n) { return dim3((unsigned)std::min<int64_t>(1 << 16, std::max<int64_t>(1, (n + DXO_AMG_BLOCK - 1) / DXO_AMG_BLOCK))); }

}  // namespace

bool dxo_amg_cycle_is_k(const dxo_amg* amg) { return amg->cycle == DXO_AMG_CYCLE_K; }

void dxo_amg_cycle(dxo_ctx* ctx, dxo_amg* amg, const double* r, double* z, hipStream_t s) {
    const bool cheby = amg->smooth_kind == DXO_AMG_SMOOTH_CHEBYSHEV;
    const CycleRun C{ctx, amg, s, cheby, (int)amg->L.size(), cheby ? amg->degree : amg->sweeps};
    if (amg->L[0].n_rows == 0) return;
    if (C.nl == 1) {                 // one dense product, in double under either precision
        const double* x = amg_body<double>(C, 0, r, nullptr);
        (void)hipMemcpyAsync(z, x, (size_t)amg->L[0].n_rows * sizeof(double), hipMemcpyDeviceToDevice, s);
        return;
    }
    if (amg->precision == DXO_AMG_PRECISION_FP32) {      // the V-cycle in float: r is narrowed once (so r may be z), the last sweep writes z
        const amg_level& v = amg->L[0];
        hipLaunchKernelGGL(amg_narrow, narrow_grid(v.n_rows), dim3(DXO_AMG_BLOCK), 0, s, v.n_rows, r, v.r32, (int*)nullptr, 0);
        amg_body<float>(C, 0, v.r32, z);
        return;
    }
    amg_body<double>(C, 0, r, z);      // level 0 is one body in either cycle: the Krylov method outside is its acceleration
}

// ---- C ABI
namespace {

// the hierarchy and, with a near-null space, the dead columns of T of every level
int amg_create(dxo_ctx* ctx, const char* who, const dxo_csr* csr, const int32_t* constrained, int64_t n_constrained, const amg_options& opt,
               dxo_amg** out) {
    if (n_constrained < 0 || opt.max_levels < 1 || opt.coarse_rows < 1 || opt.sweeps < 1)
        return dxo_fail(ctx, DXO_E_SIZE, (std::string(who) + ": n_constrained < 0, or max_levels, coarse_rows or sweeps < 1").c_str());
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipStreamSynchronize(s));      // the list may have been written on the stream
    const auto t0 = std::chrono::steady_clock::now();
    dxo_amg* a = new dxo_amg;
    a->device = ctx->device;
    a->bs = csr->bs;
    a->sweeps = opt.sweeps;
    a->k = opt.k;
    a->theta = opt.theta;
    int rc = amg_build(ctx, who, a, csr, constrained, n_constrained, opt, s);
    if (rc == DXO_OK && opt.k > 0) rc = amg_nns_dead(ctx, a, s);
    if (rc != DXO_OK) {
        amg_free(a);
        return rc;
    }
    a->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = a;
    return DXO_OK;
}

}  // namespace

extern "C" int dxo_amg_create(dxo_ctx* ctx, const dxo_csr* csr, const int32_t* constrained, int64_t n_constrained, int max_levels, int coarse_rows,
                              int sweeps, dxo_amg** out) {
    if (!ctx || !out) return DXO_E_NULL;
    DXO_LOCK(ctx);
    *out = nullptr;
    if (!csr || (n_constrained > 0 && !constrained)) return dxo_fail(ctx, DXO_E_NULL, "dxo_amg_create: NULL argument");
    if (csr->bs < 1 || csr->bs > 3) return dxo_fail(ctx, DXO_E_DIM, "dxo_amg_create: bs must be 1, 2 or 3");
    amg_options opt;
    opt.max_levels = max_levels, opt.coarse_rows = coarse_rows, opt.sweeps = sweeps;
    return amg_create(ctx, "dxo_amg_create", csr, constrained, n_constrained, opt, out);
}

extern "C" int dxo_amg_create_nns(dxo_ctx* ctx, const dxo_csr* csr, const int32_t* constrained, int64_t n_constrained, const double* B, int n_modes,
                                  int max_levels, int coarse_rows, int sweeps, dxo_amg** out) {
    if (!ctx || !out) return DXO_E_NULL;
    DXO_LOCK(ctx);
    *out = nullptr;
    if (!csr || !B || (n_constrained > 0 && !constrained)) return dxo_fail(ctx, DXO_E_NULL, "dxo_amg_create_nns: NULL argument");
    if (!((csr->bs == 2 && n_modes == 3) || (csr->bs == 3 && n_modes == 6)))
        return dxo_fail(ctx, DXO_E_DIM, "dxo_amg_create_nns: (bs, n_modes) must be (2, 3) or (3, 6)");
    if (amg_misaligned(B)) return dxo_fail(ctx, DXO_E_ALIGN, "dxo_amg_create_nns: B must be 8-byte aligned");
    amg_options opt;
    opt.max_levels = max_levels, opt.coarse_rows = coarse_rows, opt.sweeps = sweeps;
    opt.k = n_modes, opt.B = B;
    return amg_create(ctx, "dxo_amg_create_nns", csr, constrained, n_constrained, opt, out);
}

extern "C" int dxo_amg_create_soc(dxo_ctx* ctx, const dxo_csr* csr, const double* values, const int32_t* constrained, int64_t n_constrained,
                                  const double* B, int n_modes, double theta, int max_levels, int coarse_rows, int sweeps, dxo_amg** out) {
    if (!ctx || !out) return DXO_E_NULL;
    DXO_LOCK(ctx);
    *out = nullptr;
    if (!csr || !values || (n_constrained > 0 && !constrained) || (n_modes != 0 && !B))
        return dxo_fail(ctx, DXO_E_NULL, "dxo_amg_create_soc: NULL argument");
    if (!(theta >= 0.0 && theta < 1.0)) return dxo_fail(ctx, DXO_E_OPTION, "dxo_amg_create_soc: theta must lie in [0, 1)");
    if (csr->bs < 1 || csr->bs > 3) return dxo_fail(ctx, DXO_E_DIM, "dxo_amg_create_soc: bs must be 1, 2 or 3");
    if (n_modes != 0 && !((csr->bs == 2 && n_modes == 3) || (csr->bs == 3 && n_modes == 6)))
        return dxo_fail(ctx, DXO_E_DIM, "dxo_amg_create_soc: (bs, n_modes) must be (2, 3) or (3, 6), or n_modes 0");
    if (amg_misaligned(values) || (n_modes != 0 && amg_misaligned(B)))
        return dxo_fail(ctx, DXO_E_ALIGN, "dxo_amg_create_soc: values and B must be 8-byte aligned");
    amg_options opt;
    opt.max_levels = max_levels, opt.coarse_rows = coarse_rows, opt.sweeps = sweeps;
    opt.k = n_modes, opt.B = n_modes ? B : nullptr;
    if (theta > 0.0) opt.theta = theta, opt.values = values;      // theta == 0: dxo_amg_create_nns / dxo_amg_create
    return amg_create(ctx, "dxo_amg_create_soc", csr, constrained, n_constrained, opt, out);
}

extern "C" int dxo_amg_create_transfer(dxo_ctx* ctx, const dxo_csr* csr, const double* values, const int32_t* constrained, int64_t n_constrained,
                                       const double* B, int n_modes, double theta, const dxo_amg_transfer* first, int max_levels, int coarse_rows,
                                       int sweeps, dxo_amg** out) {
    if (!first) return dxo_amg_create_soc(ctx, csr, values, constrained, n_constrained, B, n_modes, theta, max_levels, coarse_rows, sweeps, out);
    if (!ctx || !out) return DXO_E_NULL;
    DXO_LOCK(ctx);
    *out = nullptr;
    const char* who = "dxo_amg_create_transfer";
    auto fail = [&](int code, const char* what) { return dxo_fail(ctx, code, (std::string(who) + ": " + what).c_str()); };
    if (!csr || !values || (n_constrained > 0 && !constrained) || (n_modes != 0 && !B) || !first->ptr || !first->col || !first->w || !first->coarse_to_fine)
        return fail(DXO_E_NULL, "NULL argument");
    if (!(theta >= 0.0 && theta < 1.0)) return fail(DXO_E_OPTION, "theta must lie in [0, 1)");
    if (csr->bs < 1 || csr->bs > 3) return fail(DXO_E_DIM, "bs must be 1, 2 or 3");
    if (n_modes != 0 && !((csr->bs == 2 && n_modes == 3) || (csr->bs == 3 && n_modes == 6)))
        return fail(DXO_E_DIM, "(bs, n_modes) must be (2, 3) or (3, 6), or n_modes 0");
    if (amg_misaligned(values) || (n_modes != 0 && amg_misaligned(B))) return fail(DXO_E_ALIGN, "values and B must be 8-byte aligned");
    // the given transfer, host arrays
    const int64_t n = csr->n_nodes, nc = first->n_coarse;
    if (nc < 1 || (double)(nc * csr->bs) > 0.8 * (double)csr->n_rows)
        return fail(DXO_E_SIZE, "n_coarse must be at least 1 and at most 0.8 of the nodes (the stagnation rule)");
    if (first->ptr[0] != 0) return fail(DXO_E_SIZE, "ptr[0] must be 0");
    for (int64_t i = 0; i < n; ++i) {
        if (first->ptr[i + 1] <= first->ptr[i]) return fail(DXO_E_SIZE, "every node needs at least one entry (ptr must increase)");
        for (int64_t e = first->ptr[i]; e < first->ptr[i + 1]; ++e) {
            if (first->col[e] < 0 || first->col[e] >= nc) return fail(DXO_E_SIZE, "a column lies outside [0, n_coarse)");
            if (e > first->ptr[i] && first->col[e] <= first->col[e - 1]) return fail(DXO_E_OPTION, "the columns of a row must ascend");
            if (!std::isfinite(first->w[e])) return fail(DXO_E_OPTION, "a weight is not finite");
        }
    }
    {
        std::vector<uint8_t> seen((size_t)n, 0);
        for (int64_t v = 0; v < nc; ++v) {
            const int64_t i = first->coarse_to_fine[v];
            if (i < 0 || i >= n) return fail(DXO_E_SIZE, "coarse_to_fine lies outside [0, n_nodes)");
            if (seen[(size_t)i]) return fail(DXO_E_OPTION, "coarse_to_fine names a node twice");
            seen[(size_t)i] = 1;
            const int64_t e = first->ptr[i];
            if (first->ptr[i + 1] != e + 1 || first->col[e] != v || first->w[e] != 1.0)
                return fail(DXO_E_OPTION, "the row of coarse_to_fine[v] must be the single entry (v, 1)");
        }
    }
    amg_options opt;
    opt.max_levels = max_levels, opt.coarse_rows = coarse_rows, opt.sweeps = sweeps;
    opt.k = n_modes, opt.B = n_modes ? B : nullptr;
    opt.first = first;
    if (theta > 0.0) opt.theta = theta, opt.values = values;
    return amg_create(ctx, who, csr, constrained, n_constrained, opt, out);
}

extern "C" int dxo_amg_transfer_info(dxo_ctx* ctx, const dxo_amg* amg, int* present, int64_t* n_coarse, int64_t* p_blocks, const double** p_diag,
                                     const int32_t** coarse_to_fine) {
    if (!amg) return DXO_E_NULL;
    DXO_LOCK(ctx);
    const amg_level& v = amg->L[0];
    const bool on = v.p_diag != nullptr;
    if (present) *present = on ? 1 : 0;
    if (n_coarse) *n_coarse = on ? v.n_agg : 0;
    if (p_blocks) *p_blocks = on ? v.p_blocks : 0;
    if (p_diag) *p_diag = v.p_diag;
    if (coarse_to_fine) *coarse_to_fine = v.ctf;
    return DXO_OK;
}

extern "C" int dxo_amg_soc_info(dxo_ctx* ctx, const dxo_amg* amg, int level, double* theta, const uint8_t** strong, int64_t* n_strong_blocks,
                                int64_t* n_unlumped_nodes, const double** dinv_f, const double** omega_f) {
    if (!ctx || !amg) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (level < 0 || level >= (int)amg->L.size()) return dxo_fail(ctx, DXO_E_SIZE, "dxo_amg_soc_info: no such level");
    const amg_level& v = amg->L[(size_t)level];
    if (theta) *theta = amg->theta;
    if (strong) *strong = v.strong;
    if (n_strong_blocks) *n_strong_blocks = v.strong ? v.n_strong : v.nnzb;
    if (dinv_f) *dinv_f = v.dinv_f;
    if (omega_f) *omega_f = v.strong ? amg->omega_f + level : nullptr;
    if (n_unlumped_nodes) {
        *n_unlumped_nodes = 0;
        if (v.strong && v.n_nodes > 0) {      // the marks of the last setup: a wait and a copy
            std::vector<uint8_t> h((size_t)v.n_nodes);
            DXO_HIP(ctx, hipSetDevice(amg->device));
            DXO_HIP(ctx, hipStreamSynchronize(dxo_launch_stream(ctx)));
            DXO_HIP(ctx, hipMemcpy(h.data(), v.unlumped, h.size(), hipMemcpyDeviceToHost));
            for (uint8_t m : h) *n_unlumped_nodes += m;
        }
    }
    return DXO_OK;
}

extern "C" int dxo_rigid_body_modes(dxo_ctx* ctx, const double* x, int64_t n_nodes, int gdim, double* B) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!x || !B) return dxo_fail(ctx, DXO_E_NULL, "dxo_rigid_body_modes: NULL argument");
    if (gdim != 2 && gdim != 3) return dxo_fail(ctx, DXO_E_DIM, "dxo_rigid_body_modes: gdim must be 2 or 3");
    if (n_nodes < 0) return dxo_fail(ctx, DXO_E_SIZE, "dxo_rigid_body_modes: n_nodes < 0");
    if (amg_misaligned(x) || amg_misaligned(B)) return dxo_fail(ctx, DXO_E_ALIGN, "dxo_rigid_body_modes: arrays must be 8-byte aligned");
    if (n_nodes == 0) return DXO_OK;
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    int rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    if (gdim == 2) hipLaunchKernelGGL(amg_rigid_body_modes<2>, amg_grid(n_nodes), dim3(DXO_AMG_BLOCK), 0, s, n_nodes, x, B);
    else hipLaunchKernelGGL(amg_rigid_body_modes<3>, amg_grid(n_nodes), dim3(DXO_AMG_BLOCK), 0, s, n_nodes, x, B);
    return dxo_device_end(ctx, s);
}

extern "C" int dxo_amg_nns_info(dxo_ctx* ctx, const dxo_amg* amg, int level, int* bs, int* bs_coarse, int64_t* dead_columns, const double** t_val,
                                const double** b_val) {
    if (!amg) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (level < 0 || level >= (int)amg->L.size()) return dxo_fail(ctx, DXO_E_SIZE, "dxo_amg_nns_info: no such level");
    const amg_level& v = amg->L[(size_t)level];
    if (bs) *bs = v.bs;
    if (bs_coarse) *bs_coarse = v.bsc;
    if (dead_columns) *dead_columns = v.dead;
    if (t_val) *t_val = v.t_val;
    if (b_val) *b_val = v.b_val;
    return DXO_OK;
}

extern "C" int dxo_amg_set_smoother(dxo_ctx* ctx, dxo_amg* amg, int kind, int degree, int rho_kind, int rho_iters, double lower, double safety) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!amg) return dxo_fail(ctx, DXO_E_NULL, "dxo_amg_set_smoother: NULL argument");
    const bool cheby = kind == DXO_AMG_SMOOTH_CHEBYSHEV;
    if ((!cheby && kind != DXO_AMG_SMOOTH_JACOBI) || (rho_kind != DXO_AMG_RHO_INF_NORM && rho_kind != DXO_AMG_RHO_POWER))
        return dxo_fail(ctx, DXO_E_OPTION, "dxo_amg_set_smoother: unknown smoother or rho kind");
    if ((cheby && (degree < 1 || degree > AMG_MAX_DEGREE)) || rho_iters < 1 || !(lower > 0.0 && lower < 1.0) || !(safety >= 1.0))
        return dxo_fail(ctx, DXO_E_OPTION, "dxo_amg_set_smoother: degree outside 1..8, rho_iters < 1, lower outside (0, 1) or safety < 1");
    amg->ready = false;      // omega, P, the coarse matrices and the Chebyshev pairs are those of the last setup
    amg->smooth_kind = kind;
    if (cheby) amg->degree = degree;
    amg->rho_kind = rho_kind;
    amg->rho_iters = rho_iters;
    amg->lower = lower;
    amg->safety = safety;
    return DXO_OK;
}

extern "C" int dxo_amg_smoother_info(dxo_ctx* ctx, const dxo_amg* amg, int level, int* kind, int* degree, int* rho_kind, int* rho_iters,
                                     const double** rho) {
    if (!amg) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (level < 0 || level >= (int)amg->L.size()) return dxo_fail(ctx, DXO_E_SIZE, "dxo_amg_smoother_info: no such level");
    if (kind) *kind = amg->smooth_kind;
    if (degree) *degree = amg->smooth_kind == DXO_AMG_SMOOTH_CHEBYSHEV ? amg->degree : amg->sweeps;
    if (rho_kind) *rho_kind = amg->rho_kind;
    if (rho_iters) *rho_iters = amg->rho_iters;
    if (rho) *rho = level + 1 < (int)amg->L.size() ? amg->rho + level : nullptr;
    return DXO_OK;
}

extern "C" int dxo_amg_set_cycle(dxo_ctx* ctx, dxo_amg* amg, int kind) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!amg) return dxo_fail(ctx, DXO_E_NULL, "dxo_amg_set_cycle: NULL argument");
    if (kind != DXO_AMG_CYCLE_V && kind != DXO_AMG_CYCLE_K) return dxo_fail(ctx, DXO_E_OPTION, "dxo_amg_set_cycle: unknown cycle");
    if (kind == DXO_AMG_CYCLE_K && amg->precision == DXO_AMG_PRECISION_FP32)
        return dxo_fail(ctx, DXO_E_OPTION, "dxo_amg_set_cycle: the K-cycle runs in double only (dxo_amg_set_precision selected DXO_AMG_PRECISION_FP32)");
    if (kind == DXO_AMG_CYCLE_K) {      // the K vectors of the intermediate levels, once; dxo_amg_apply stays allocation-free
        DXO_HIP(ctx, hipSetDevice(amg->device));
        Uploader U{ctx, amg, "dxo_amg_set_cycle"};
        for (size_t l = 1; l + 1 < amg->L.size(); ++l) {
            amg_level& v = amg->L[l];
            if (v.kco) continue;
            const int knb = (int)std::min<int64_t>(AMG_K_MAX_PARTS, std::max<int64_t>(1, (v.n_rows + DXO_AMG_BLOCK - 1) / DXO_AMG_BLOCK));
            double* vec = U.alloc<double>((size_t)(5 * v.n_rows));
            double* part = U.alloc<double>((size_t)(3 * knb));
            double* co = U.alloc<double>(KCO_COUNT);
            if (U.rc != DXO_OK) return U.rc;      // what was allocated goes with the object; the cycle is unchanged
            DXO_HIP(ctx, hipMemset(co, 0, KCO_COUNT * sizeof(double)));
            v.kc1 = vec, v.kv1 = vec + v.n_rows, v.kc2 = vec + 2 * v.n_rows, v.kv2 = vec + 3 * v.n_rows, v.kr1 = vec + 4 * v.n_rows;
            v.kpart = part;
            v.knb = knb;
            v.kco = co;
        }
    }
    amg->cycle = kind;
    return DXO_OK;
}

extern "C" int dxo_amg_cycle_info(dxo_ctx* ctx, const dxo_amg* amg, int* kind, int64_t* visits) {
    if (!amg) return DXO_E_NULL;
    DXO_LOCK(ctx);
    const int nl = (int)amg->L.size();
    if (kind) *kind = amg->cycle;
    if (visits) {
        *visits = nl;      // V: every level once
        if (amg->cycle == DXO_AMG_CYCLE_K && nl >= 2) {      // K: level l 2^l times, the coarsest as often as the level above it
            *visits = 0;
            for (int l = 0; l + 1 < nl; ++l) *visits += (int64_t)1 << l;
            *visits += (int64_t)1 << (nl - 2);
        }
    }
    return DXO_OK;
}

extern "C" int dxo_amg_set_precision(dxo_ctx* ctx, dxo_amg* amg, int kind) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!amg) return dxo_fail(ctx, DXO_E_NULL, "dxo_amg_set_precision: NULL argument");
    if (kind != DXO_AMG_PRECISION_FP64 && kind != DXO_AMG_PRECISION_FP32) return dxo_fail(ctx, DXO_E_OPTION, "dxo_amg_set_precision: unknown precision");
    if (kind == amg->precision) return DXO_OK;
    if (kind == DXO_AMG_PRECISION_FP32 && amg->cycle == DXO_AMG_CYCLE_K)
        return dxo_fail(ctx, DXO_E_OPTION, "dxo_amg_set_precision: single precision runs the V-cycle only (dxo_amg_set_cycle selected DXO_AMG_CYCLE_K)");
    const size_t nl = amg->L.size();
    if (kind == DXO_AMG_PRECISION_FP32 && amg->fp32_bytes == 0 && nl > 1) {      // the copies and the vectors, once; one level: a dense product
        DXO_HIP(ctx, hipSetDevice(amg->device));
        Uploader U{ctx, amg, "dxo_amg_set_precision"};
        int64_t entries = 0;
        for (size_t l = 0; l < nl; ++l) {
            amg_level& v = amg->L[l];
            const bool last = l + 1 == nl;
            const int64_t nv = last ? 0 : v.A->nnz, nd = last ? 0 : v.n_nodes * v.bs * v.bs;
            const int64_t np = last ? 0 : v.p_blocks * v.bs * (v.p_diag ? 1 : v.bsc);      // a given transfer: the diagonals of its blocks
            v.r32 = U.alloc<float>((size_t)v.n_rows);
            v.xa32 = U.alloc<float>((size_t)v.n_rows);
            entries += 2 * v.n_rows;
            if (last) break;
            v.xb32 = U.alloc<float>((size_t)v.n_rows);
            v.t32 = U.alloc<float>((size_t)v.n_rows);
            v.d32 = U.alloc<float>((size_t)v.n_rows);
            v.values32 = U.alloc<float>((size_t)nv);
            v.dinv32 = U.alloc<float>((size_t)nd);
            (v.p_diag ? v.p_diag32 : v.p_val32) = U.alloc<float>((size_t)np);
            entries += 3 * v.n_rows + nv + nd + np;
        }
        if (U.rc != DXO_OK) return U.rc;      // what was allocated goes with the object; the precision is unchanged
        amg->fp32_bytes = entries * (int64_t)sizeof(float);
    }
    amg->ready = false;      // the copies are those of the last single-precision setup, if any
    amg->precision = kind;
    return DXO_OK;
}

extern "C" int dxo_amg_precision_info(dxo_ctx* ctx, const dxo_amg* amg, int* kind, int64_t* fp32_bytes) {
    if (!amg) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (kind) *kind = amg->precision;
    if (fp32_bytes) *fp32_bytes = amg->fp32_bytes;
    return DXO_OK;
}

extern "C" int dxo_amg_destroy(dxo_ctx* ctx, dxo_amg* amg) {
    if (!amg) return DXO_E_NULL;
    DXO_LOCK(ctx);
    (void)hipSetDevice(amg->device);
    (void)hipDeviceSynchronize();
    amg_free(amg);
    return DXO_OK;
}

extern "C" int dxo_amg_setup(dxo_ctx* ctx, dxo_amg* amg, const double* values) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!amg || !values) return dxo_fail(ctx, DXO_E_NULL, "dxo_amg_setup: NULL argument");
    if (amg_misaligned(values)) return dxo_fail(ctx, DXO_E_ALIGN, "dxo_amg_setup: values must be 8-byte aligned");
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    amg->ready = false;
    const int nl = (int)amg->L.size();
    const dim3 B(DXO_AMG_BLOCK);
    amg->L[0].values = values;
    int rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    DXO_HIP(ctx, hipMemsetAsync(amg->flag, 0, 4 * sizeof(int), s));
    for (int l = 0; l + 1 < nl; ++l) {
        amg_level& v = amg->L[(size_t)l];
        amg_level& c = amg->L[(size_t)l + 1];
        if (v.n_nodes == 0) continue;
        amg_setup_level(amg, l, v, c, s);
    }
    const amg_level& c = amg->L.back();
    const int64_t n = amg->nc;
    if (n > 0) {
        hipLaunchKernelGGL(amg_dense_fill, dim3((unsigned)n), B, 0, s, n, c.A->d_row_ptr, c.A->d_col, c.values, amg->dense[0]);
        for (int64_t k = 0; k < n; ++k)
            hipLaunchKernelGGL(amg_dense_step, dim3((unsigned)n), B, 0, s, n, k, amg->dense[k % 2], amg->dense[(k + 1) % 2], amg->flag);
    }
    if (amg->precision == DXO_AMG_PRECISION_FP32)      // all of the above is double; the cycle's copies, before the one wait
        for (int l = 0; l + 1 < nl; ++l) {
            const amg_level& v = amg->L[(size_t)l];
            const int64_t len[3] = {v.A->nnz, v.n_nodes * v.bs * v.bs, v.p_blocks * v.bs * (v.p_diag ? 1 : v.bsc)};
            const double* from[3] = {v.values, v.dinv, v.p_diag ? v.p_diag : v.p_val};
            float* to[3] = {v.values32, v.dinv32, v.p_diag ? v.p_diag32 : v.p_val32};
            for (int q = 0; q < 3; ++q)
                if (len[q] > 0) hipLaunchKernelGGL(amg_narrow, narrow_grid(len[q]), B, 0, s, len[q], from[q], to[q], amg->flag, l + 1);
        }
    int h[3] = {0, 0, 0};
    DXO_HIP(ctx, hipMemcpyAsync(h, amg->flag, sizeof h, hipMemcpyDeviceToHost, s));
    DXO_HIP(ctx, hipStreamSynchronize(s));
    rc = dxo_device_end(ctx, s);
    if (h[0]) return dxo_fail(ctx, DXO_E_SINGULAR, "dxo_amg_setup: a diagonal block of a level is singular");
    if (h[1]) return dxo_fail(ctx, DXO_E_SINGULAR, "dxo_amg_setup: zero pivot in the coarsest matrix");
    if (h[2]) {
        char msg[200];
        snprintf(msg, sizeof msg, "dxo_amg_setup: a finite entry of level %d leaves the range of float (DXO_AMG_PRECISION_FP32)", h[2] - 1);
        return dxo_fail(ctx, DXO_E_OPTION, msg);
    }
    if (rc != DXO_OK) return rc;
    amg->ready = true;
    return DXO_OK;
}

extern "C" int dxo_amg_apply(dxo_ctx* ctx, dxo_amg* amg, const double* r, double* z) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!amg || !r || !z) return dxo_fail(ctx, DXO_E_NULL, "dxo_amg_apply: NULL argument");
    if (amg_misaligned(r) || amg_misaligned(z)) return dxo_fail(ctx, DXO_E_ALIGN, "dxo_amg_apply: arrays must be 8-byte aligned");
    if (!amg->ready) return dxo_fail(ctx, DXO_E_OPTION, "dxo_amg_apply: dxo_amg_setup has not run (or failed)");
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    int rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    dxo_amg_cycle(ctx, amg, r, z, s);
    return dxo_device_end(ctx, s);
}

extern "C" int dxo_amg_info(dxo_ctx* ctx, const dxo_amg* amg, int* n_levels, double* build_ms, double* operator_complexity, int level,
                            dxo_amg_level_info* out) {
    if (!amg) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (n_levels) *n_levels = (int)amg->L.size();
    if (build_ms) *build_ms = amg->build_ms;
    if (operator_complexity) *operator_complexity = amg->complexity;
    if (!out) return DXO_OK;
    if (level < 0 || level >= (int)amg->L.size()) return dxo_fail(ctx, DXO_E_SIZE, "dxo_amg_info: no such level");
    const amg_level& v = amg->L[(size_t)level];
    const bool last = level + 1 == (int)amg->L.size();
    *out = dxo_amg_level_info{};
    out->n_rows = v.n_rows;
    out->n_nodes = v.n_nodes;
    out->nnz_blocks = v.nnzb;
    out->csr = v.A;
    out->values = v.values;
    if (!last) {
        out->dinv = v.dinv;
        out->omega = amg->omega + level;
        out->n_aggregates = v.n_agg;
        out->aggregate = v.agg;
        out->p_blocks = v.p_blocks;
        out->p_ptr = v.p_ptr;
        out->p_col = v.p_col;
        out->p_values = v.p_val;
        out->ap_blocks = v.ap_blocks;
        out->ap_ptr = v.ap_ptr;
        out->ap_col = v.ap_col;
    }
    return DXO_OK;
}
