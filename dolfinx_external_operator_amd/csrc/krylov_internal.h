// krylov_internal.h — what krylov.hip and amg.hip share. Device code: the row of a node in the csr.h layout (NodeRow), the search for
// a block in it (block_pos), the lane-group row product behind every SpMV-shaped kernel of the two files (row_product) and the
// inverse of a diagonal block with its singularity test (invert_block: closed form up to bs 3, Gauss-Jordan in registers for bs 6).
// Host code: the block-size list of the dispatcher from run-time shapes to template arguments (with_bs over with_int of form_host.h) and the launchers one file calls in the
// other (device pointers, explicit stream, no locking, no event bracket).
#pragma once

#include "csr.h"
#include "form_host.h"      // int_c, with_int

// the block sizes with an SpMV and a block inverse: 1, 2, 3 of the patterns of dxo_csr_create, 6 of a multigrid level
template <class F, class Miss>
void with_bs(int bs, F&& f, Miss&& miss) { with_int<1, 2, 3, 6>(bs, f, miss); }

// the run of a node's rows in the csr.h layout: the bs rows of a node share their columns, row i of block k starts at
// r0 + i * len + k * BS
template <int BS>
struct NodeRow {
    int64_t r0, len;      // first entry of the node's first row; entries per row = BS * neighbours
    int nnb;              // neighbour blocks
    __device__ __forceinline__ NodeRow(const int64_t* __restrict__ row_ptr, int64_t node) {
        r0 = row_ptr[node * BS];
        len = row_ptr[node * BS + 1] - r0;
        nnb = (int)(len / BS);
    }
};

// position of the block of column `node` among the blocks of a node's row (its own: the diagonal block), or -1 (an empty row has
// no block to read)
template <int BS>
__device__ __forceinline__ int block_pos(const NodeRow<BS>& R, const int32_t* __restrict__ col, int64_t node) {
    int lo = 0, hi = R.nnb - 1;
    const int64_t self = node * BS;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[R.r0 + (int64_t)mid * BS] < self) lo = mid + 1;
        else hi = mid;
    }
    return hi >= 0 && col[R.r0 + (int64_t)lo * BS] == self ? lo : -1;
}

// acc = (A x)_node over a group of LW lanes: lane l takes the blocks k = l, l + LW, ... in ascending order (one column index per
// block, the BS entries of x at it, fma(v[j], xb[j], acc[i]) with j innermost), then the xor-butterfly from LW / 2 down leaves the
// sums on every lane. All lanes of a group call it; those of a node >= n_nodes add nothing. pick(R, k, c, ab, ld), c the first column
// of block k, may skip the block (false) or replace its pointer and leading dimension; SCALED: x is taken as sx x. T is the scalar of
// the values, of x and of the sums: double everywhere but in the single-precision multigrid cycle (float: the fma is v_fma_f32).
template <int BS, int LW, bool SCALED = false, class T, class Pick>
__device__ __forceinline__ void row_product(int64_t n_nodes, int64_t node, int lane, const int64_t* __restrict__ row_ptr,
                                            const int32_t* __restrict__ col, const T* __restrict__ values, const T* __restrict__ x,
                                            T sx, T (&acc)[BS], Pick pick) {
#pragma unroll
    for (int i = 0; i < BS; ++i) acc[i] = 0.0;
    if (node < n_nodes) {
        const NodeRow<BS> R(row_ptr, node);
        for (int k = lane; k < R.nnb; k += LW) {
            const int64_t c = col[R.r0 + (int64_t)k * BS];
            const T* ab = values + R.r0 + (int64_t)k * BS;
            int64_t ld = R.len;
            if (!pick(R, k, c, ab, ld)) continue;
            T xb[BS];
#pragma unroll
            for (int j = 0; j < BS; ++j) xb[j] = SCALED ? sx * x[c + j] : x[c + j];
#pragma unroll
            for (int i = 0; i < BS; ++i) {
                const T* v = ab + i * ld;
#pragma unroll
                for (int j = 0; j < BS; ++j) acc[i] = fma(v[j], xb[j], acc[i]);
            }
        }
    }
#pragma unroll
    for (int off = LW / 2; off > 0; off >>= 1)
#pragma unroll
        for (int i = 0; i < BS; ++i) acc[i] += __shfl_xor(acc[i], off, LW);
}

// the matrix as it is stored: every block, x unscaled
template <int BS, int LW, class T>
__device__ __forceinline__ void row_product(int64_t n_nodes, int64_t node, int lane, const int64_t* __restrict__ row_ptr,
                                            const int32_t* __restrict__ col, const T* __restrict__ values, const T* __restrict__ x,
                                            T (&acc)[BS]) {
    row_product<BS, LW>(n_nodes, node, lane, row_ptr, col, values, x, T(1), acc, [](const NodeRow<BS>&, int, int64_t, const T*&, int64_t&) { return true; });
}

// Gauss-Jordan on [A | I] with partial pivoting (the lowest row among equals). Rows are exchanged by compare-and-select over static
// indices, so the 72 doubles stay in registers. M = [A | I] on entry, [. | A^-1] on return; false for a zero, NaN or nearly singular
// block (the rule of invert_block)
__device__ __forceinline__ bool gj6(double (&M)[6][12]) {
    constexpr int BS = 6;
    double had = 1.0, det = 1.0;
#pragma unroll
    for (int i = 0; i < BS; ++i) {
        double n2 = 0.0;
#pragma unroll
        for (int j = 0; j < BS; ++j) n2 = fma(M[i][j], M[i][j], n2);
        had *= sqrt(n2);
    }
#pragma unroll
    for (int k = 0; k < BS; ++k) {
        int p = k;
        double best = fabs(M[k][k]);
#pragma unroll
        for (int i = k + 1; i < BS; ++i) {
            const double v = fabs(M[i][k]);
            if (v > best) {
                best = v;
                p = i;
            }
        }
#pragma unroll
        for (int i = k + 1; i < BS; ++i) {
            const bool sw = p == i;
#pragma unroll
            for (int c = k; c < 2 * BS; ++c) {
                const double x = M[k][c], y = M[i][c];
                M[k][c] = sw ? y : x;
                M[i][c] = sw ? x : y;
            }
        }
        if (p != k) det = -det;
        const double piv = M[k][k];
        det *= piv;
#pragma unroll
        for (int c = k; c < 2 * BS; ++c) M[k][c] = M[k][c] / piv;
#pragma unroll
        for (int i = 0; i < BS; ++i) {
            if (i == k) continue;
            const double fct = M[i][k];
#pragma unroll
            for (int c = k; c < 2 * BS; ++c) M[i][c] = fma(-fct, M[k][c], M[i][c]);
        }
    }
    return fabs(det) > 1e-14 * had;
}

// the inverse of a diagonal block and its singularity test (|det| at most 1e-14 of the product of the row norms: false), for
// dxo_csr_block_jacobi, the block-Jacobi inverses of the multigrid levels and the lumped diagonal blocks of the filtered prolongator
// smoothing: in closed form for bs <= 3, by gj6 for the coarse levels of block size 6. The test and the inverse do not depend on the
// scale of the block: it is inverted as 2^-e a, e the exponent of its largest entry, and the result multiplied by 2^-e. Both
// scalings are exact, so wherever the determinant and the squared row norms of `a` itself neither overflow nor underflow the
// result is the one of the unscaled arithmetic bit for bit; entries of 1e300 or 1e-300 no longer count as singular.
template <int BS>
__device__ __forceinline__ bool invert_block_scaled(const double (&a0)[BS][BS], double s, double (&b)[BS][BS]);

template <int BS>
__device__ __forceinline__ bool invert_block(const double (&a0)[BS][BS], double (&b)[BS][BS]) {
    double m = 0.0;
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
        for (int j = 0; j < BS; ++j) m = fmax(m, fabs(a0[i][j]));
    int e = 0;
    if (m > 0.0 && m <= 1.7976931348623157e308) (void)frexp(m, &e);      // a zero, NaN or infinite block: as it is
    e = e > 1000 ? 1000 : (e < -1000 ? -1000 : e);                        // 2^-e stays a normal number
    const double s = ldexp(1.0, -e);
    const bool ok = invert_block_scaled<BS>(a0, s, b);
#pragma unroll
    for (int i = 0; i < BS; ++i)
#pragma unroll
        for (int j = 0; j < BS; ++j) b[i][j] *= s;
    return ok;
}

// the inverse of s a0 and its singularity test
template <int BS>
__device__ __forceinline__ bool invert_block_scaled(const double (&a0)[BS][BS], double s, double (&b)[BS][BS]) {
    static_assert(BS <= 3 || BS == 6, "no inverse for this block size");
    if constexpr (BS == 6) {
        double M[BS][2 * BS];
#pragma unroll
        for (int i = 0; i < BS; ++i)
#pragma unroll
            for (int j = 0; j < BS; ++j) {
                M[i][j] = a0[i][j] * s;
                M[i][BS + j] = i == j ? 1.0 : 0.0;
            }
        const bool ok = gj6(M);
#pragma unroll
        for (int i = 0; i < BS; ++i)
#pragma unroll
            for (int j = 0; j < BS; ++j) b[i][j] = M[i][BS + j];
        return ok;
    } else {
        double a[BS][BS];
#pragma unroll
        for (int i = 0; i < BS; ++i)
#pragma unroll
            for (int j = 0; j < BS; ++j) a[i][j] = a0[i][j] * s;
        double had = 1.0;
#pragma unroll
        for (int i = 0; i < BS; ++i) {
            double n2 = 0.0;
#pragma unroll
            for (int j = 0; j < BS; ++j) n2 += a[i][j] * a[i][j];
            had *= sqrt(n2);
        }
        double det;
        if constexpr (BS == 1) {
            det = a[0][0];
            b[0][0] = 1.0 / det;
        } else if constexpr (BS == 2) {
            det = a[0][0] * a[1][1] - a[0][1] * a[1][0];
            const double id = 1.0 / det;
            b[0][0] = a[1][1] * id;
            b[0][1] = -a[0][1] * id;
            b[1][0] = -a[1][0] * id;
            b[1][1] = a[0][0] * id;
        } else {
            const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1];
            const double c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2];
            const double c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
            det = a[0][0] * c00 + a[0][1] * c01 + a[0][2] * c02;
            const double id = 1.0 / det;
            b[0][0] = c00 * id;
            b[1][0] = c01 * id;
            b[2][0] = c02 * id;
            b[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) * id;
            b[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) * id;
            b[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) * id;
            b[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) * id;
            b[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) * id;
            b[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) * id;
        }
        return fabs(det) > 1e-14 * had;     // false for a zero, NaN or nearly singular block
    }
}

// krylov.hip: the block-inverse kernel of dxo_csr_block_jacobi without its wait, for bs 1, 2, 3 and 6 (DXO_E_DIM and no launch for any
// other); a singular block raises flag[0]
int dxo_kr_bj_setup_launch(const dxo_csr* csr, const double* values, double* inv, int* flag, hipStream_t s);

// krylov.hip: y = A x by the kernel of dxo_csr_spmv (bs 1, 2, 3, 6), for the coarse operators of the K-cycle
int dxo_kr_spmv_launch(dxo_ctx* ctx, const dxo_csr* csr, const double* values, const double* x, double* y, hipStream_t s);

// krylov.hip: the lanes per node dxo_csr_spmv takes on this pattern (option "spmv_lanes", or from the mean neighbour count), for the
// transposed product of transpose.hip
int dxo_kr_spmv_lanes(const dxo_ctx* ctx, const dxo_csr* csr);

// krylov.hip: z = inv r per block by the kernel of dxo_block_jacobi_apply (bs 1, 2, 3; DXO_E_DIM and no launch for any other), for the
// coarse step of the p-multigrid
int dxo_kr_bj_apply_launch(dxo_ctx* ctx, const char* who, int bs, int64_t n, const double* inv, const double* r, double* z, hipStream_t s);

// amg.hip: the checks of a DXO_PC_AMG preconditioner against the operator, one cycle z = M(r) on the stream (V or K, as set by
// dxo_amg_set_cycle), and whether that cycle is the K-cycle (not a fixed linear operator: flexible GMRES only)
int dxo_amg_pc_check(dxo_ctx* ctx, const char* who, const dxo_amg* amg, const dxo_csr* op_csr, int bs, int64_t n);
void dxo_amg_cycle(dxo_ctx* ctx, dxo_amg* amg, const double* r, double* z, hipStream_t s);
bool dxo_amg_cycle_is_k(const dxo_amg* amg);

// pmg.hip: the checks of a DXO_PC_PMG preconditioner against the operator, and one cycle z = M(r) on the stream (nonzero: a callback of
// the object failed)
struct dxo_pmg;
int dxo_pmg_pc_check(dxo_ctx* ctx, const char* who, const dxo_pmg* pmg, const dxo_csr* op_csr, int64_t n);
int dxo_pmg_cycle(dxo_ctx* ctx, dxo_pmg* pmg, const double* r, double* z, hipStream_t s);
