// transpose.hip — the transposed matrix on a dxo_csr pattern, for adjoint solves (dxo_csr_transpose / dxo_csr_spmv_t).
//
// The pattern of dxo_csr_create is structurally symmetric (rows and columns are "nodes that share a cell"), so A^T lives on the same
// row pointers and columns: only the values are permuted. The MIRROR MAP holds, for block k of node n (column node m), the position
// p of node n among the blocks of node m's row: block (n, k) of A^T is the transposed block (m, p) of A. It is one uint16_t per block
// (2 bytes per bs^2 values, as d_pos), built on the device by block_pos at the first call on a pattern and kept in the dxo_csr. That
// first call allocates and synchronises once (it reads back whether some block had no mirror: a pattern that is not structurally
// symmetric); later calls allocate and synchronise nothing.
//
// Block k of node n has the index row_ptr[n * bs] / bs^2 + k: the rows of the nodes before n hold bs * bs entries per block.
//
// dxo_csr_transpose: a group of TR_LW lanes owns a node, lane l its blocks k = l, l + TR_LW, ... Out of place every block of A^T is
// written by the lane that owns it. In place each off-diagonal pair (n, k) <-> (m, p) is exchanged through registers by the one lane
// that owns the block of the smaller node, and a diagonal block is transposed by its own lane: no entry is touched by two lanes.
//
// dxo_csr_spmv_t: y = alpha A^T x + beta y without forming A^T, in the lane-group shape of csr_spmv (krylov.hip). Lane l of node n
// takes the blocks k = l, l + LW, ..., reads the mirrored block in the rows of m, and adds fma(At[i][j], x[m * bs + j], acc[i]) with j
// innermost; the xor-butterfly of row_product follows. These are the operations of row_product on the transposed values in the same
// order, so the result equals dxo_csr_spmv of dxo_csr_transpose's output bit for bit. No atomics.
#include "csr.h"
#include "dxo_common.h"
#include "krylov_internal.h"

#ifndef DXO_TR_BLOCK
#define DXO_TR_BLOCK 256
#endif

namespace {

constexpr int TR_LW = 8;      // lanes per node of the map build and the transposition

template <int BS>
__device__ __forceinline__ int64_t first_block(const NodeRow<BS>& R) { return R.r0 / (BS * BS); }

// mirror[block (n, k)] = position of n in the rows of the block's column node; flag[0] = 1 where there is none
template <int BS>
__global__ __launch_bounds__(DXO_TR_BLOCK) void mirror_build(int64_t n_nodes, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                             uint16_t* __restrict__ mirror, int* __restrict__ flag) {
    const int lane = threadIdx.x % TR_LW;
    const int64_t stride = (int64_t)gridDim.x * (DXO_TR_BLOCK / TR_LW);
    for (int64_t node = (int64_t)blockIdx.x * (DXO_TR_BLOCK / TR_LW) + threadIdx.x / TR_LW; node < n_nodes; node += stride) {
        const NodeRow<BS> R(row_ptr, node);
        const int64_t b0 = first_block(R);
        for (int k = lane; k < R.nnb; k += TR_LW) {
            const int64_t m = col[R.r0 + (int64_t)k * BS] / BS;
            const NodeRow<BS> Rm(row_ptr, m);
            const int p = block_pos(Rm, col, node);
            if (p < 0) flag[0] = 1;
            mirror[b0 + k] = (uint16_t)(p < 0 ? 0 : p);
        }
    }
}

// vt = v^T on the pattern. INPLACE: vt == v
template <int BS, bool INPLACE>
__global__ __launch_bounds__(DXO_TR_BLOCK) void csr_transpose(int64_t n_nodes, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                              const uint16_t* __restrict__ mirror, const double* v, double* vt) {
    const int lane = threadIdx.x % TR_LW;
    const int64_t stride = (int64_t)gridDim.x * (DXO_TR_BLOCK / TR_LW);
    for (int64_t node = (int64_t)blockIdx.x * (DXO_TR_BLOCK / TR_LW) + threadIdx.x / TR_LW; node < n_nodes; node += stride) {
        const NodeRow<BS> R(row_ptr, node);
        const int64_t b0 = first_block(R);
        for (int k = lane; k < R.nnb; k += TR_LW) {
            const int64_t m = col[R.r0 + (int64_t)k * BS] / BS;
            if (INPLACE && m < node) continue;      // the pair belongs to the lane of the smaller node
            const NodeRow<BS> Rm(row_ptr, m);
            const int64_t own = R.r0 + (int64_t)k * BS, mir = Rm.r0 + (int64_t)mirror[b0 + k] * BS;
            double a[BS][BS];
#pragma unroll
            for (int i = 0; i < BS; ++i)
#pragma unroll
                for (int j = 0; j < BS; ++j) a[i][j] = v[mir + i * Rm.len + j];
            if constexpr (INPLACE) {
                if (m != node) {
                    double b[BS][BS];
#pragma unroll
                    for (int i = 0; i < BS; ++i)
#pragma unroll
                        for (int j = 0; j < BS; ++j) b[i][j] = v[own + i * R.len + j];
#pragma unroll
                    for (int i = 0; i < BS; ++i)
#pragma unroll
                        for (int j = 0; j < BS; ++j) vt[mir + i * Rm.len + j] = b[j][i];
                }
            }
#pragma unroll
            for (int i = 0; i < BS; ++i)
#pragma unroll
                for (int j = 0; j < BS; ++j) vt[own + i * R.len + j] = a[j][i];
        }
    }
}

// y = alpha A^T x + beta y: csr_spmv (krylov.hip) with the blocks of row_product read through the mirror map
template <int BS, int LW>
__global__ __launch_bounds__(DXO_TR_BLOCK) void csr_spmv_t(int64_t n_nodes, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                           const uint16_t* __restrict__ mirror, const double* __restrict__ values, double alpha,
                                                           const double* __restrict__ x, double beta, double* __restrict__ y) {
    constexpr int NPB = DXO_TR_BLOCK / LW;
    const int64_t node = (int64_t)blockIdx.x * NPB + threadIdx.x / LW;
    const int lane = threadIdx.x % LW;
    double acc[BS];
#pragma unroll
    for (int i = 0; i < BS; ++i) acc[i] = 0.0;
    if (node < n_nodes) {
        const NodeRow<BS> R(row_ptr, node);
        const int64_t b0 = first_block(R);
        for (int k = lane; k < R.nnb; k += LW) {
            const int64_t c = col[R.r0 + (int64_t)k * BS];
            const NodeRow<BS> Rm(row_ptr, c / BS);
            const double* ab = values + Rm.r0 + (int64_t)mirror[b0 + k] * BS;
            double xb[BS], at[BS][BS];
#pragma unroll
            for (int j = 0; j < BS; ++j) xb[j] = x[c + j];
#pragma unroll
            for (int j = 0; j < BS; ++j)
#pragma unroll
                for (int i = 0; i < BS; ++i) at[i][j] = ab[j * Rm.len + i];
#pragma unroll
            for (int i = 0; i < BS; ++i)
#pragma unroll
                for (int j = 0; j < BS; ++j) acc[i] = fma(at[i][j], xb[j], acc[i]);
        }
    }
#pragma unroll
    for (int off = LW / 2; off > 0; off >>= 1)
#pragma unroll
        for (int i = 0; i < BS; ++i) acc[i] += __shfl_xor(acc[i], off, LW);
    if (node < n_nodes && lane == 0) {
#pragma unroll
        for (int i = 0; i < BS; ++i) {
            const int64_t r = node * BS + i;
            y[r] = beta == 0.0 ? alpha * acc[i] : alpha * acc[i] + beta * y[r];
        }
    }
}

// ---- host side
const auto tr_no_shape = [](int v) {
    fprintf(stderr, "transpose.hip: no kernel instantiation for %d\n", v);
    std::abort();
};

bool misaligned8(const void* p) { return ((uintptr_t)p & 7u) != 0; }

int node_grid(const dxo_ctx* ctx, int64_t n_nodes) { return capped_grid(ctx, n_nodes, DXO_TR_BLOCK / TR_LW, 16); }

// the checks both entry points share, and the mirror map of the pattern (built at the first call)
int mirror_of(dxo_ctx* ctx, const char* who, dxo_csr* A, hipStream_t s) {
    if (!A->mesh) return fail_who(ctx, DXO_E_DIM, who, "a pattern without a mesh (a multigrid level) has no transpose here");
    if (A->bs < 1 || A->bs > 3) return fail_who(ctx, DXO_E_DIM, who, "the block size must be 1, 2 or 3");
    if (A->mirror_state > 0 || A->n_nodes == 0) return DXO_OK;
    if (A->mirror_state == 0) {
        const size_t nb = (size_t)(A->nnz / ((int64_t)A->bs * A->bs));
        const size_t map_bytes = (nb * sizeof(uint16_t) + 15) & ~(size_t)15;
        DXO_HIP(ctx, hipMalloc((void**)&A->d_mirror, map_bytes + 16));      // the flag word behind the map
        int* flag = reinterpret_cast<int*>(reinterpret_cast<char*>(A->d_mirror) + map_bytes);
        DXO_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(int), s));
        with_int<1, 2, 3>(A->bs, [&](auto BS) {
            hipLaunchKernelGGL(mirror_build<BS>, dim3(node_grid(ctx, A->n_nodes)), dim3(DXO_TR_BLOCK), 0, s, A->n_nodes, A->d_row_ptr, A->d_col,
                               A->d_mirror, flag);
        }, tr_no_shape);
        int h = 0;
        DXO_HIP(ctx, hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, s));
        DXO_HIP(ctx, hipStreamSynchronize(s));
        A->mirror_state = h ? -1 : 1;
    }
    if (A->mirror_state < 0) return fail_who(ctx, DXO_E_OPTION, who, "the pattern is not structurally symmetric: a block has no mirrored block");
    return DXO_OK;
}

}  // namespace

extern "C" int dxo_csr_transpose(dxo_ctx* ctx, dxo_csr* csr, const double* values, double* values_t) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    const char* who = "dxo_csr_transpose";
    if (!csr || !values || !values_t) return fail_who(ctx, DXO_E_NULL, who, "NULL argument");
    if (misaligned8(values) || misaligned8(values_t)) return fail_who(ctx, DXO_E_ALIGN, who, "arrays must be 8-byte aligned");
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    int rc = mirror_of(ctx, who, csr, s);
    if (rc != DXO_OK || csr->n_nodes == 0) return rc;
    rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    with_int<1, 2, 3>(csr->bs, [&](auto BS) {
        const dim3 grid(node_grid(ctx, csr->n_nodes)), block(DXO_TR_BLOCK);
        if (values_t == values)
            hipLaunchKernelGGL((csr_transpose<BS, true>), grid, block, 0, s, csr->n_nodes, csr->d_row_ptr, csr->d_col, csr->d_mirror, values, values_t);
        else
            hipLaunchKernelGGL((csr_transpose<BS, false>), grid, block, 0, s, csr->n_nodes, csr->d_row_ptr, csr->d_col, csr->d_mirror, values, values_t);
    }, tr_no_shape);
    return dxo_device_end(ctx, s);
}

extern "C" int dxo_csr_spmv_t(dxo_ctx* ctx, dxo_csr* csr, const double* values, double alpha, const double* x, double beta, double* y) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    const char* who = "dxo_csr_spmv_t";
    if (!csr || !values || !x || !y) return fail_who(ctx, DXO_E_NULL, who, "NULL argument");
    if (misaligned8(values) || misaligned8(x) || misaligned8(y)) return fail_who(ctx, DXO_E_ALIGN, who, "arrays must be 8-byte aligned");
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    int rc = mirror_of(ctx, who, csr, s);
    if (rc != DXO_OK || csr->n_nodes == 0) return rc;
    rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    with_int<1, 2, 3>(csr->bs, [&](auto BS) {
        with_int<8, 16, 32, 64>(dxo_kr_spmv_lanes(ctx, csr), [&](auto LW) {
            constexpr int NPB = DXO_TR_BLOCK / LW;
            hipLaunchKernelGGL((csr_spmv_t<BS, LW>), dim3((unsigned)((csr->n_nodes + NPB - 1) / NPB)), dim3(DXO_TR_BLOCK), 0, s, csr->n_nodes,
                               csr->d_row_ptr, csr->d_col, csr->d_mirror, values, alpha, x, beta, y);
        }, tr_no_shape);
    }, tr_no_shape);
    return dxo_device_end(ctx, s);
}
