// krylov.hip — linear solves on the device for the matrices of dxo_bilinear_assemble and for matrix-free operators
// (dxo_csr_spmv / dxo_csr_block_jacobi / dxo_block_jacobi_apply / dxo_krylov_*).
//
// SpMV on a dxo_csr pattern, y = alpha A x + beta y. The rows node*bs + i, i < bs, of one node share their columns, and the columns
// come in runs m*bs + j. A group of LW lanes (LW from the mean neighbour count of the pattern, option "spmv_lanes") owns one node:
// lane l takes the neighbour blocks k = l, l + LW, ... in ascending order, reads ONE column index per block (col[r0 + k*bs]), the bs
// entries of x at it and the bs contiguous values of each of the node's bs rows, and keeps bs sums. A fixed xor-butterfly over the
// LW lanes then adds them. Index traffic is 4 B per bs^2 nonzeros; no atomics: the result is bit-reproducible.
//
// Block Jacobi: one thread per node finds the diagonal block (binary search for the node's own column run), inverts it (invert_block:
// in closed form for bs <= 3; bs 6 is reached by the multigrid levels alone) and writes inv[node][bs][bs]. A block whose |det| is at most 1e-14 of the product of its row norms (Hadamard's bound)
// is singular: its inverse is written as zero, a flag is raised and the call returns DXO_E_SINGULAR after its one synchronisation.
//
// Restarted GMRES(m), right preconditioning, classical Gram-Schmidt with one reorthogonalisation pass (option "krylov_reorth",
// default 1). One Arnoldi step is a fixed sequence of launches on the context's stream: z = M v_j, v_{j+1} = A z, h = V^T v_{j+1}
// (multi-dot: every workgroup reads its rows of w once for all j + 1 products and writes per-block partials, a one-workgroup-per-
// product pass adds them in a fixed order), v_{j+1} -= V h (also the partials of |w|^2), the same again for the second pass, the
// norm, the scaling and a one-wave kernel that applies the previous Givens rotations to the new column, forms the next one, updates
// g and records the first step whose estimate |g_{j+1}| fell below the tolerance. The host reads that record every check_every
// steps only; the solution update uses the recorded step, so steps run past it change nothing. Every reduction has a fixed shape
// (fixed grid for a workspace, fixed butterflies, fixed order across waves): a solve is bit-reproducible.
// CG runs on the same kernels; once its residual test passes on the device, alpha is 0 for the steps that follow.
//
// Flexible GMRES (dxo_krylov_fgmres) is the same sequence with z_j = M v_j kept in a second basis Z [m][ld]: w = A z_j, and the update
// at the end of a cycle is x += sum_j y_j z_j (kr_combine<double, 1> on Z), with no further preconditioner call. M may therefore change from
// step to step (a callback that iterates, the K-cycle of amg.hip). Z is allocated at the first flexible solve on a workspace.
//
// Compressed basis (dxo_krylov_create_basis, DXO_KRYLOV_BASIS_FP32): the rows of V are stored as float [m + 1][ldf], everything else
// (dot products, updates, H, the rotations, x, the second basis of the flexible solver) stays double. A new basis vector is rounded
// once, t = (float)(w[i] hinv), written to V[j + 1] and widened back into w, which the next step hands to M and A: the vector the
// solver works with is exactly the one it stored, so the Arnoldi relation holds for the stored basis and no row is ever widened in a
// pass of its own. w alternates between two double vectors W0 / W1.
//
// The row kernels of the Gram-Schmidt step (kr_multidot, kr_update, kr_combine, kr_scale_store) are one family over the type T of the
// stored rows and the rows FW a thread owns per trip of the grid, instantiated for (double, 1) and (float, 1 | 2 | 4): the same grid,
// per-thread order and reductions for both bases. FW of a float basis is the option "krylov_basis_width"; a double basis, the second
// basis of the flexible solver and the single products of CG run (double, 1) whatever the option says. KrBasis::rows is the one
// place that turns a workspace into (typed row pointer, stride, FW).
//
// Host side. Run-time shapes (block size, lanes per node, KMAX, FW) reach the templates through with_int / with_bs of
// krylov_internal.h, so a kernel's argument list is written once and a value without an instantiation is refused, never served by
// another kernel.
#include "csr.h"
#include "dxo_common.h"
#include "krylov_internal.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>

#ifndef DXO_KR_BLOCK
#define DXO_KR_BLOCK 256
#endif

struct dxo_krylov {
    int64_t n = 0, ld = 0;     // vector length and its padded stride (a multiple of 32 doubles)
    int m = 0;                 // restart length
    int nb = 0;                // workgroups of the row kernels = partials per product (fixed for the workspace)
    int basis = DXO_KRYLOV_BASIS_FP64;
    int64_t ldf = 0;           // FP32 basis: the stride of a float row (n padded to a multiple of 64 floats: rows are 256-byte aligned)
    float* vf = nullptr;       // FP32 basis: [m + 1][ldf]
    double* vec = nullptr;     // FP64 basis: [m + 1 + 4][ld]: the basis V, then Z, R, T, Q; FP32 basis: [6][ld]: Z, R, T, Q, W0, W1
    double* zb = nullptr;      // [m][ld]: the preconditioned basis of dxo_krylov_fgmres, absent until its first solve here
    double* part = nullptr;    // [m + 2][nb] per-block partials (the last row: |w|^2)
    double* sc = nullptr;      // small state (offsets below)
    int* st = nullptr;         // status words
    double* V() const { return vec; }
    double* Z() const { return vec + (int64_t)(basis == DXO_KRYLOV_BASIS_FP32 ? 0 : m + 1) * ld; }
    double* R() const { return Z() + ld; }
    double* T() const { return Z() + 2 * ld; }
    double* Q() const { return Z() + 3 * ld; }
    double* W(int k) const { return Z() + (int64_t)(4 + (k & 1)) * ld; }      // FP32 basis only
    int64_t work_rows() const { return basis == DXO_KRYLOV_BASIS_FP32 ? 6 : m + 5; }
    // state layout: H [m][m + 1] (column j at j*(m+1)), g [m + 1], cs [m], sn [m], y [m], c [m + 1], scalars [16]
    int64_t o_g() const { return (int64_t)m * (m + 1); }
    int64_t o_cs() const { return o_g() + m + 1; }
    int64_t o_sn() const { return o_cs() + m; }
    int64_t o_y() const { return o_sn() + m; }
    int64_t o_c() const { return o_y() + m; }
    int64_t o_s() const { return o_c() + m + 1; }
    int64_t sc_doubles() const { return o_s() + 16; }
};

namespace {

constexpr int KR_MAX_RESTART = 64;
// scalar slots (sc + o_s())
enum { S_NORM = 0, S_INV = 1, S_ONE = 2, S_HNORM = 3, S_HINV = 4, S_RZ = 5, S_PQ = 6, S_ALPHA = 7, S_BETA = 8, S_RR = 9, S_EST = 10 };
// status words
enum { W_CONV = 0, W_BREAK = 1, W_SING = 2 };

// ---- reductions with a fixed shape
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// sum over the workgroup; the result is valid in thread 0. lds: DXO_KR_BLOCK / 64 doubles
__device__ __forceinline__ double block_sum(double v, double* lds) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[w] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < DXO_KR_BLOCK / 64; ++k) s += lds[k];
    __syncthreads();
    return s;
}

// ---- SpMV
template <int BS, int LW>
__global__ __launch_bounds__(DXO_KR_BLOCK) void csr_spmv(int64_t n_nodes, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                         const double* __restrict__ values, double alpha, const double* __restrict__ x,
                                                         double beta, double* __restrict__ y) {
    constexpr int NPB = DXO_KR_BLOCK / LW;
    const int64_t node = (int64_t)blockIdx.x * NPB + threadIdx.x / LW;
    const int lane = threadIdx.x % LW;
    double acc[BS];
    row_product<BS, LW>(n_nodes, node, lane, row_ptr, col, values, x, acc);
    if (node < n_nodes && lane == 0) {
#pragma unroll
        for (int i = 0; i < BS; ++i) {
            const int64_t r = node * BS + i;
            y[r] = beta == 0.0 ? alpha * acc[i] : alpha * acc[i] + beta * y[r];
        }
    }
}

// ---- block Jacobi
template <int BS>
__global__ __launch_bounds__(DXO_KR_BLOCK) void bj_setup(int64_t n_nodes, const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                         const double* __restrict__ values, double* __restrict__ inv, int* __restrict__ singular) {
    const int64_t node = (int64_t)blockIdx.x * DXO_KR_BLOCK + threadIdx.x;
    if (node >= n_nodes) return;
    const NodeRow<BS> R(row_ptr, node);
    const int lo = block_pos<BS>(R, col, node);
    double* out = inv + node * BS * BS;
    bool ok = false;
    if (lo >= 0) {
        double a[BS][BS], b[BS][BS];
#pragma unroll
        for (int i = 0; i < BS; ++i)
#pragma unroll
            for (int j = 0; j < BS; ++j) a[i][j] = values[R.r0 + i * R.len + (int64_t)lo * BS + j];
        ok = invert_block<BS>(a, b);
#pragma unroll
        for (int i = 0; i < BS; ++i)
#pragma unroll
            for (int j = 0; j < BS; ++j) out[i * BS + j] = ok ? b[i][j] : 0.0;
    } else {      // an absent block is not read: a zero inverse and the flag, which is also what inverting a block of zeros ends with
#pragma unroll
        for (int i = 0; i < BS * BS; ++i) out[i] = 0.0;
    }
    if (!ok) singular[0] = 1;     // every writer stores the same word
}

template <int BS>
__global__ __launch_bounds__(DXO_KR_BLOCK) void bj_apply(int64_t n_nodes, const double* __restrict__ inv, const double* __restrict__ r,
                                                         double* __restrict__ z) {
    const int64_t stride = (int64_t)gridDim.x * DXO_KR_BLOCK;
    for (int64_t node = (int64_t)blockIdx.x * DXO_KR_BLOCK + threadIdx.x; node < n_nodes; node += stride) {
        const double* B = inv + node * BS * BS;
        double rb[BS];
#pragma unroll
        for (int j = 0; j < BS; ++j) rb[j] = r[node * BS + j];
#pragma unroll
        for (int i = 0; i < BS; ++i) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < BS; ++j) s = fma(B[i * BS + j], rb[j], s);
            z[node * BS + i] = s;
        }
    }
}

// ---- Krylov building blocks. Row kernels run on exactly nb workgroups (grid stride): the rows a thread adds are fixed. They read the
// rows of a basis stored as T [.][ld], T double (the vectors themselves) or float (the compressed basis); everything else is double.
// A thread owns FW consecutive rows i0 .. i0 + FW - 1 of every trip of the grid: one sizeof(T) FW-byte load per basis row and as
// many doubles of w. With FW = 1 (the only width of a double basis: its vectors are the caller's in dot_partials, aligned to 8
// bytes and no more) a group is one entry and all of this folds to the plain loop. Row starts of wider groups are aligned (ld and
// i0 are multiples of FW, the buffers of hipMalloc); n is not, so the last group of a vector is ragged: it is loaded entry by entry
// and the absent entries take no part. Sums run over a thread's entries in ascending order, then over the wave and across waves.
template <int FW>
struct KrRows {
    int64_t i0;
    int cnt;      // entries of this group that exist: FW, or fewer at the tail
    __device__ __forceinline__ KrRows(int64_t i, int64_t n) : i0(i), cnt(n - i >= FW ? FW : (int)(n - i)) {}
    __device__ __forceinline__ bool full() const { return cnt == FW; }
    template <class T>
    __device__ __forceinline__ void load(const T* __restrict__ p, T (&v)[FW]) const {
        if (full()) {
            struct alignas(sizeof(T) * FW) Pack { T e[FW]; };
            const Pack q = *reinterpret_cast<const Pack*>(p + i0);
#pragma unroll
            for (int c = 0; c < FW; ++c) v[c] = q.e[c];
        } else {
#pragma unroll
            for (int c = 0; c < FW; ++c) v[c] = c < cnt ? p[i0 + c] : T(0);
        }
    }
    template <class T>
    __device__ __forceinline__ void store(T* __restrict__ p, const T (&v)[FW]) const {
        if (full()) {
            struct alignas(sizeof(T) * FW) Pack { T e[FW]; };
            Pack q;
#pragma unroll
            for (int c = 0; c < FW; ++c) q.e[c] = v[c];
            *reinterpret_cast<Pack*>(p + i0) = q;
        } else {
#pragma unroll
            for (int c = 0; c < FW; ++c)
                if (c < cnt) p[i0 + c] = v[c];
        }
    }
};

// part[k * nb + block] = sum over the block's rows of V_k[i] w[i], k < nk; w is read once for all nk products
template <int KMAX, class T, int FW>
__global__ __launch_bounds__(DXO_KR_BLOCK) void kr_multidot(int64_t n, const T* __restrict__ V, int64_t ld, int nk,
                                                            const double* __restrict__ w, double* __restrict__ part) {
    __shared__ double lds[DXO_KR_BLOCK / 64][KMAX];
    double acc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * DXO_KR_BLOCK * FW;
    for (int64_t i = ((int64_t)blockIdx.x * DXO_KR_BLOCK + threadIdx.x) * FW; i < n; i += stride) {
        const KrRows<FW> g(i, n);
        double wi[FW];
        g.load(w, wi);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k < nk) {
                T v[FW];
                g.load(V + k * ld, v);
#pragma unroll
                for (int c = 0; c < FW; ++c) acc[k] = fma((double)v[c], wi[c], acc[k]);      // an absent entry adds 0 * 0
            }
        }
    }
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < nk) {
            const double s = wave_sum(acc[k]);
            if ((threadIdx.x & 63) == 0) lds[wv][k] = s;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nk; k += DXO_KR_BLOCK) {
        double s = 0.0;
        for (int q = 0; q < DXO_KR_BLOCK / 64; ++q) s += lds[q][k];
        part[(int64_t)k * gridDim.x + blockIdx.x] = s;
    }
}

// one workgroup per product k: out[k] = sum_b part[k * nb + b]; acc (optional) += out; norm mode (nk = 1): out[0] = sqrt(sum),
// inv_out[0] = 1 / out[0] (0 for a zero sum)
__global__ __launch_bounds__(DXO_KR_BLOCK) void kr_reduce(const double* __restrict__ part, int nb, double* __restrict__ out,
                                                          double* __restrict__ acc, int norm, double* __restrict__ inv_out) {
    __shared__ double lds[DXO_KR_BLOCK / 64];
    const int k = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += DXO_KR_BLOCK) s += part[(int64_t)k * nb + b];
    s = block_sum(s, lds);
    if (threadIdx.x == 0) {
        if (norm) {
            const double r = sqrt(s);
            out[k] = r;
            inv_out[k] = r > 0.0 ? 1.0 / r : 0.0;
        } else {
            out[k] = s;
            if (acc) acc[k] += s;
        }
    }
}
// w -= sum_k V_k h_k (k ascending), and npart[block] = the block's share of |w|^2
template <class T, int FW>
__global__ __launch_bounds__(DXO_KR_BLOCK) void kr_update(int64_t n, const T* __restrict__ V, int64_t ld, int nk, const double* __restrict__ h,
                                                          double* __restrict__ w, double* __restrict__ npart) {
    __shared__ double lds[DXO_KR_BLOCK / 64];
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * DXO_KR_BLOCK * FW;
    for (int64_t i = ((int64_t)blockIdx.x * DXO_KR_BLOCK + threadIdx.x) * FW; i < n; i += stride) {
        const KrRows<FW> g(i, n);
        double s[FW];
        g.load(w, s);
        for (int k = 0; k < nk; ++k) {
            T v[FW];
            g.load(V + k * ld, v);
            const double hk = h[k];
#pragma unroll
            for (int c = 0; c < FW; ++c) s[c] = fma(-(double)v[c], hk, s[c]);
        }
        g.store(w, s);
#pragma unroll
        for (int c = 0; c < FW; ++c) acc = fma(s[c], s[c], acc);      // absent entries are 0
    }
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) npart[blockIdx.x] = acc;
}

// out = sum_k V_k y_k (k ascending)
template <class T, int FW>
__global__ __launch_bounds__(DXO_KR_BLOCK) void kr_combine(int64_t n, const T* __restrict__ V, int64_t ld, int nk, const double* __restrict__ y,
                                                           double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * DXO_KR_BLOCK * FW;
    for (int64_t i = ((int64_t)blockIdx.x * DXO_KR_BLOCK + threadIdx.x) * FW; i < n; i += stride) {
        const KrRows<FW> g(i, n);
        double s[FW];
#pragma unroll
        for (int c = 0; c < FW; ++c) s[c] = 0.0;
        for (int k = 0; k < nk; ++k) {
            T v[FW];
            g.load(V + k * ld, v);
            const double yk = y[k];
#pragma unroll
            for (int c = 0; c < FW; ++c) s[c] = fma((double)v[c], yk, s[c]);
        }
        g.store(out, s);
    }
}

// the new basis vector: t = (T)(x[i] s[0]) (float: round to nearest even), row[i] = t, and for a float basis y[i] = (double)t as
// well (y may be x). A double row is the vector itself: one store, y is not touched, and row may be x, so it is not __restrict__
template <class T>
using KrRowOut = std::conditional_t<std::is_same_v<T, double>, double*, T* __restrict__>;

template <class T, int FW>
__global__ __launch_bounds__(DXO_KR_BLOCK) void kr_scale_store(int64_t n, const double* x, const double* __restrict__ s, KrRowOut<T> row, double* y) {
    const double a = s[0];
    const int64_t stride = (int64_t)gridDim.x * DXO_KR_BLOCK * FW;
    for (int64_t i = ((int64_t)blockIdx.x * DXO_KR_BLOCK + threadIdx.x) * FW; i < n; i += stride) {
        const KrRows<FW> g(i, n);
        double xi[FW];
        T t[FW];
        g.load(x, xi);
#pragma unroll
        for (int c = 0; c < FW; ++c) {
            t[c] = (T)(xi[c] * a);
            xi[c] = (double)t[c];
        }
        g.store(row, t);
        if constexpr (!std::is_same_v<T, double>) g.store(y, xi);
    }
}

// y += sign * a[0] * x
__global__ __launch_bounds__(DXO_KR_BLOCK) void kr_axpy(int64_t n, const double* __restrict__ a, double sign, const double* __restrict__ x,
                                                        double* __restrict__ y) {
    const double s = sign * a[0];
    const int64_t stride = (int64_t)gridDim.x * DXO_KR_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * DXO_KR_BLOCK + threadIdx.x; i < n; i += stride) y[i] = fma(s, x[i], y[i]);
}

// y = x + b[0] * y
__global__ __launch_bounds__(DXO_KR_BLOCK) void kr_xpay(int64_t n, const double* __restrict__ x, const double* __restrict__ b, double* __restrict__ y) {
    const double s = b[0];
    const int64_t stride = (int64_t)gridDim.x * DXO_KR_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * DXO_KR_BLOCK + threadIdx.x; i < n; i += stride) y[i] = fma(s, y[i], x[i]);
}

// y = b - y
__global__ __launch_bounds__(DXO_KR_BLOCK) void kr_bminus(int64_t n, const double* __restrict__ b, double* __restrict__ y) {
    const int64_t stride = (int64_t)gridDim.x * DXO_KR_BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * DXO_KR_BLOCK + threadIdx.x; i < n; i += stride) y[i] = b[i] - y[i];
}

// start of a GMRES cycle: g = (beta, 0, ...), no converged step, no breakdown
__global__ void kr_cycle_init(double* __restrict__ sc, int* __restrict__ st, int m, int64_t o_g, int64_t o_s) {
    for (int i = threadIdx.x; i <= m; i += blockDim.x) sc[o_g + i] = i == 0 ? sc[o_s + S_NORM] : 0.0;
    if (threadIdx.x == 0) {
        st[W_CONV] = -1;
        st[W_BREAK] = 0;
    }
}

// one thread: the Givens step of column j. H[j+1][j] is in S_HNORM
__global__ void kr_givens(double* __restrict__ sc, int* __restrict__ st, int j, int m, int64_t o_g, int64_t o_cs, int64_t o_sn, int64_t o_s,
                          double tol) {
    if (threadIdx.x != 0) return;
    double* h = sc + (int64_t)j * (m + 1);
    double* g = sc + o_g;
    double* cs = sc + o_cs;
    double* sn = sc + o_sn;
    const double hn = sc[o_s + S_HNORM];
    h[j + 1] = hn;
    for (int i = 0; i < j; ++i) {
        const double t = cs[i] * h[i] + sn[i] * h[i + 1];
        h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1];
        h[i] = t;
    }
    const double r = hypot(h[j], hn);
    double c = 1.0, s = 0.0;
    if (r > 0.0) {
        c = h[j] / r;
        s = hn / r;
    }
    cs[j] = c;
    sn[j] = s;
    h[j] = r;
    h[j + 1] = 0.0;
    g[j + 1] = -s * g[j];
    g[j] = c * g[j];
    const double est = fabs(g[j + 1]);
    sc[o_s + S_EST] = est;
    // steps run past the recorded one (check_every > 1) are not part of the solve: a zero vector there is no breakdown
    if (st[W_CONV] < 0 && (est <= tol || !(hn > 0.0))) {
        st[W_CONV] = j + 1;
        if (!(hn > 0.0)) st[W_BREAK] = 1;
    }
}

// one thread: R y = g on the first k columns (back substitution); a zero pivot gives y_i = 0
__global__ void kr_trisolve(double* __restrict__ sc, int k, int m, int64_t o_g, int64_t o_y) {
    if (threadIdx.x != 0) return;
    const double* g = sc + o_g;
    double* y = sc + o_y;
    for (int i = k - 1; i >= 0; --i) {
        double s = g[i];
        for (int c = i + 1; c < k; ++c) s -= sc[(int64_t)c * (m + 1) + i] * y[c];
        const double d = sc[(int64_t)i * (m + 1) + i];
        y[i] = d != 0.0 ? s / d : 0.0;
    }
}

// CG scalars, one workgroup: reduce the partials of one dot product, then
//   phase 0: S_RZ = (r, z);  phase 1: S_ALPHA = rz / (p, q) (0 once converged or at (p, q) = 0);
//   phase 2: (r, r) -> records the first step `it` with |r| <= tol;  phase 3: S_BETA = (r, z)_new / S_RZ, S_RZ = (r, z)_new
__global__ __launch_bounds__(DXO_KR_BLOCK) void kr_cg_scalar(const double* __restrict__ part, int nb, double* __restrict__ s, int* __restrict__ st,
                                                             int phase, int it, double tol) {
    __shared__ double lds[DXO_KR_BLOCK / 64];
    double v = 0.0;
    for (int b = threadIdx.x; b < nb; b += DXO_KR_BLOCK) v += part[b];
    v = block_sum(v, lds);
    if (threadIdx.x != 0) return;
    const bool done = st[W_CONV] >= 0;
    if (phase == 0) {
        s[S_RZ] = v;
    } else if (phase == 1) {
        s[S_PQ] = v;
        if (!done && !(v != 0.0 && std::isfinite(v))) {
            st[W_BREAK] = 1;
            st[W_CONV] = it - 1;
        }
        s[S_ALPHA] = (st[W_CONV] >= 0) ? 0.0 : s[S_RZ] / v;
    } else if (phase == 2) {
        s[S_RR] = v;
        s[S_EST] = sqrt(v);
        if (!done && sqrt(v) <= tol) st[W_CONV] = it;
    } else {
        s[S_BETA] = s[S_RZ] != 0.0 ? v / s[S_RZ] : 0.0;
        s[S_RZ] = v;
    }
}

// ---- host side
int kr_grid(const dxo_ctx* ctx, int64_t n, int per_cu) {
    int64_t blocks = (n + DXO_KR_BLOCK - 1) / DXO_KR_BLOCK;
    const int64_t cap = (int64_t)ctx->compute_units * per_cu;
    if (blocks > cap) blocks = cap;
    return blocks < 1 ? 1 : (int)blocks;
}

// a value that the checks of this file let through and no list below holds: a defect here, not of the caller
const auto kr_no_shape = [](int v) {
    fprintf(stderr, "krylov.hip: no kernel instantiation for %d\n", v);
    std::abort();
};

// lanes per node: the option, or the smallest of 8 / 16 / 32 / 64 that covers the mean neighbour count
int spmv_lanes(const dxo_ctx* ctx, const dxo_csr* A) {
    if (ctx->spmv_lanes == 8 || ctx->spmv_lanes == 16 || ctx->spmv_lanes == 32 || ctx->spmv_lanes == 64) return (int)ctx->spmv_lanes;
    const double mean = A->n_nodes > 0 ? (double)A->nnz / ((double)A->bs * A->bs * (double)A->n_nodes) : 1.0;
    int lw = 8;
    while (lw < 64 && lw < mean) lw *= 2;
    return lw;
}

// a block size without a kernel is refused, never served by the kernel of another one
int bs_refused(dxo_ctx* ctx, const char* who, const char* takes, int bs) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: no kernel for block size %d (%s)", who, bs, takes);
    return dxo_fail(ctx, DXO_E_DIM, msg);
}

// the block sizes of the product and of the block inverse are those of with_bs: 1, 2, 3 the patterns of dxo_csr_create, 6 the pattern
// of a multigrid level (dxo_amg_info hands its dxo_csr out)
#define KR_BS_LIST "1, 2, 3 or 6"
constexpr char SPMV_TAKES[] = "the product takes " KR_BS_LIST;

bool has_bs(int bs) {
    bool found = true;
    with_bs(bs, [](auto) {}, [&](int) { found = false; });
    return found;
}

int spmv_launch(dxo_ctx* ctx, const char* who, const dxo_csr* A, const double* values, double alpha, const double* x, double beta, double* y,
                hipStream_t s) {
    if (!has_bs(A->bs)) return bs_refused(ctx, who, SPMV_TAKES, A->bs);
    if (A->n_nodes == 0) return DXO_OK;
    with_bs(A->bs, [&](auto BS) {
        with_int<8, 16, 32, 64>(spmv_lanes(ctx, A), [&](auto LW) {
            constexpr int NPB = DXO_KR_BLOCK / LW;      // nodes per workgroup
            hipLaunchKernelGGL((csr_spmv<BS, LW>), dim3((unsigned)((A->n_nodes + NPB - 1) / NPB)), dim3(DXO_KR_BLOCK), 0, s, A->n_nodes, A->d_row_ptr,
                               A->d_col, values, alpha, x, beta, y);
        }, kr_no_shape);
    }, kr_no_shape);
    return DXO_OK;
}

// bs 1, 2, 3 (kr_validate and dxo_block_jacobi_apply let nothing else through: the levels of block size 6 apply their inverses
// inside the sweeps of amg.hip)
int bj_apply_launch(dxo_ctx* ctx, const char* who, int bs, int64_t n, const double* inv, const double* r, double* z, hipStream_t s) {
    int rc = DXO_OK;
    with_int<1, 2, 3>(bs, [&](auto BS) {
        const int64_t nn = n / BS;
        if (nn > 0) hipLaunchKernelGGL(bj_apply<BS>, dim3(kr_grid(ctx, nn, 8)), dim3(DXO_KR_BLOCK), 0, s, nn, inv, r, z);
    }, [&](int) { rc = bs_refused(ctx, who, "block Jacobi takes 1, 2 or 3", bs); });
    return rc;
}

bool misaligned(const void* p) { return ((uintptr_t)p & 7u) != 0; }

// the operator and preconditioner of one solve, validated
struct KrCall {
    dxo_ctx* ctx;
    dxo_krylov* ws;
    const dxo_krylov_op* op;
    const dxo_krylov_pc* pc;
    hipStream_t s;
    int apply(const double* v, double* out) {
        if (op->csr) return spmv_launch(ctx, "dxo_krylov", op->csr, op->values, 1.0, v, 0.0, out, s);
        const int rc = op->apply(op->user, v, out);
        if (rc != DXO_OK) {
            char msg[128];
            snprintf(msg, sizeof msg, "dxo_krylov: the operator callback returned %d", rc);
            return dxo_fail(ctx, rc < 0 ? rc : DXO_E_OPTION, msg);
        }
        return DXO_OK;
    }
    int precond(const double* r, double* z) {
        if (!pc || pc->kind == DXO_PC_NONE) {
            DXO_HIP(ctx, hipMemcpyAsync(z, r, (size_t)ws->n * sizeof(double), hipMemcpyDeviceToDevice, s));
            return DXO_OK;
        }
        if (pc->kind == DXO_PC_AMG) {
            dxo_amg_cycle(ctx, (dxo_amg*)pc->inv, r, z, s);
            return DXO_OK;
        }
        if (pc->kind == DXO_PC_PMG) return dxo_pmg_cycle(ctx, (dxo_pmg*)pc->inv, r, z, s);
        if (pc->kind == DXO_PC_CALLBACK) {
            const dxo_krylov_callback* cb = (const dxo_krylov_callback*)pc->inv;
            const int rc = cb->apply(cb->user, r, z);
            if (rc != DXO_OK) {
                char msg[128];
                snprintf(msg, sizeof msg, "dxo_krylov: the preconditioner callback returned %d", rc);
                return dxo_fail(ctx, rc < 0 ? rc : DXO_E_OPTION, msg);
            }
            return DXO_OK;
        }
        return bj_apply_launch(ctx, "dxo_krylov", pc->kind == DXO_PC_JACOBI ? 1 : pc->bs, ws->n, pc->inv, r, z, s);
    }
    // part[0..nb) = partials of (a, b); reduce into out (norm: sqrt and inverse into out[0], out[1])
    void dot_partials(const double* a, const double* b, double* part) {
        hipLaunchKernelGGL((kr_multidot<1, double, 1>), dim3(ws->nb), dim3(DXO_KR_BLOCK), 0, s, ws->n, a, ws->ld, 1, b, part);
    }
    void norm(const double* a, double* out) {
        dot_partials(a, a, ws->part);
        hipLaunchKernelGGL(kr_reduce, dim3(1), dim3(DXO_KR_BLOCK), 0, s, ws->part, ws->nb, out, (double*)nullptr, 1, out + 1);
    }
    int read(void* host, const void* dev, size_t bytes) {
        DXO_HIP(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s));
        DXO_HIP(ctx, hipStreamSynchronize(s));
        return DXO_OK;
    }
    // R = b - A x, its norm into S_NORM / S_INV; host copy in *beta
    int residual(const double* b, const double* x, double* beta) {
        int rc = apply(x, ws->R());
        if (rc != DXO_OK) return rc;
        hipLaunchKernelGGL(kr_bminus, dim3(ws->nb), dim3(DXO_KR_BLOCK), 0, s, ws->n, b, ws->R());
        norm(ws->R(), ws->sc + ws->o_s() + S_NORM);
        return read(beta, ws->sc + ws->o_s() + S_NORM, sizeof(double));
    }
    // the opening of every solver: *bnorm = |b| and *tol = max(rtol |b|, atol). b = 0 is solved here: x = 0, converged, *bnorm = 0
    int begin(const double* b, double* x, double rtol, double atol, dxo_krylov_info* info, double* bnorm, double* tol) {
        double* S = ws->sc + ws->o_s();
        norm(b, S + S_NORM);
        const int rc = read(bnorm, S + S_NORM, sizeof(double));
        if (rc != DXO_OK) return rc;
        if (*bnorm == 0.0) {
            DXO_HIP(ctx, hipMemsetAsync(x, 0, (size_t)ws->n * sizeof(double), s));
            DXO_HIP(ctx, hipStreamSynchronize(s));
            info->converged = 1;
        }
        *tol = std::max(rtol * *bnorm, atol);
        return DXO_OK;
    }
};

int kr_validate(dxo_ctx* ctx, const char* who, bool flexible, dxo_krylov* ws, const dxo_krylov_op* op, const dxo_krylov_pc* pc, const double* b,
                double* x, double rtol, double atol, int max_it, int check_every) {
    char msg[256];
    auto fail = [&](int code, const char* what) { return dxo_fail(ctx, code, (std::string(who) + ": " + what).c_str()); };
    if (!ws || !op || !b || !x) return fail(DXO_E_NULL, "NULL argument");
    if (!op->csr && !op->apply) return fail(DXO_E_NULL, "the operator has neither a matrix nor a callback");
    if (op->csr && !op->values) return fail(DXO_E_NULL, "the operator's matrix has no values");
    if (op->n != ws->n || (op->csr && op->csr->n_rows != ws->n)) {
        snprintf(msg, sizeof msg, "operator size %lld (matrix rows %lld) differs from the workspace's %lld", (long long)op->n,
                 (long long)(op->csr ? op->csr->n_rows : op->n), (long long)ws->n);
        return fail(DXO_E_SIZE, msg);
    }
    if (op->csr && !has_bs(op->csr->bs)) return bs_refused(ctx, who, SPMV_TAKES, op->csr->bs);
    if (pc && pc->kind != DXO_PC_NONE) {
        // pc->inv carries the dxo_amg*, the dxo_pmg*, a dxo_krylov_callback* or the inverses
        const dxo_krylov_callback* cb = (const dxo_krylov_callback*)pc->inv;
        if (pc->kind == DXO_PC_CALLBACK) {
            if (!cb || !cb->apply) return fail(DXO_E_NULL, "the preconditioner has no callback");
        } else if (pc->kind != DXO_PC_AMG && pc->kind != DXO_PC_PMG) {
            if (pc->kind != DXO_PC_JACOBI && pc->kind != DXO_PC_BLOCK_JACOBI) return fail(DXO_E_OPTION, "unknown preconditioner kind");
            if (!pc->inv) return fail(DXO_E_NULL, "the preconditioner has no inverse");
            if (misaligned(pc->inv)) return fail(DXO_E_ALIGN, "the preconditioner's inverse is not 8-byte aligned");
        }
        if (pc->n != ws->n) {
            snprintf(msg, sizeof msg, "the preconditioner covers %lld rows, the operator has %lld", (long long)pc->n, (long long)ws->n);
            return fail(DXO_E_SIZE, msg);
        }
        if (pc->kind == DXO_PC_PMG) {
            const int rc = dxo_pmg_pc_check(ctx, who, (const dxo_pmg*)pc->inv, op->csr, pc->n);
            if (rc != DXO_OK) return rc;
        } else if (pc->kind == DXO_PC_AMG) {
            const int rc = dxo_amg_pc_check(ctx, who, (const dxo_amg*)pc->inv, op->csr, pc->bs, pc->n);
            if (rc != DXO_OK) return rc;
            if (!flexible && dxo_amg_cycle_is_k((const dxo_amg*)pc->inv))
                return fail(DXO_E_OPTION, "a K-cycle is not a fixed linear operator: use dxo_krylov_fgmres");
        } else if (pc->kind == DXO_PC_BLOCK_JACOBI) {
            if (pc->bs < 1 || pc->bs > 3) return fail(DXO_E_DIM, "block Jacobi takes bs 1, 2 or 3");
            if (op->csr && op->csr->bs != pc->bs) {
                snprintf(msg, sizeof msg, "block Jacobi of bs %d on a pattern of bs %d", pc->bs, op->csr->bs);
                return fail(DXO_E_DIM, msg);
            }
            if (ws->n % pc->bs != 0) return fail(DXO_E_SIZE, "n is not a multiple of the preconditioner's bs");
        }
    }
    if ((op->values && misaligned(op->values)) || misaligned(b) || misaligned(x)) return fail(DXO_E_ALIGN, "arrays must be 8-byte aligned");
    if (max_it < 0 || check_every < 1) return fail(DXO_E_SIZE, "max_it < 0 or check_every < 1");
    if (!(rtol >= 0.0) || !(atol >= 0.0)) return fail(DXO_E_OPTION, "negative or NaN tolerance");
    return DXO_OK;
}

// the smallest KMAX of kr_multidot that holds nk products
int kr_kmax(int nk) {
    int kmax = 4;
    while (kmax < nk) kmax *= 2;
    return kmax;
}

// the steps of a cycle that touch the basis, on either kind of workspace. FP64: the rows of V are the vectors themselves.
// FP32: the vector of step j is W(j), its rounded copy row j of vf
struct KrBasis {
    const KrCall& K;
    dxo_krylov* ws;
    const dim3 G, B;
    const bool f32;
    explicit KrBasis(const KrCall& k) : K(k), ws(k.ws), G(k.ws->nb), B(DXO_KR_BLOCK), f32(k.ws->basis == DXO_KRYLOV_BASIS_FP32) {}
    double* vector(int j) const { return f32 ? ws->W(j) : ws->V() + (int64_t)j * ws->ld; }
    // f(rows, ld, FW): the stored rows with their type and stride, and the rows per thread of their kernels: a float basis takes FW
    // from the option "krylov_basis_width", a double one has FW = 1 alone
    template <class F>
    void rows(F f) const {
        if (f32) with_int<1, 2, 4>((int)K.ctx->krylov_basis_width, [&](auto FW) { f(ws->vf, ws->ldf, FW); }, kr_no_shape);
        else f(ws->V(), ws->ld, int_c<1>{});
    }
    // vector(j) = x * s[0], stored as row j (x may be vector(j))
    void scale_store(int j, const double* x, const double* s) const {
        rows([&](auto* V, int64_t ld, auto FW) {
            using T = std::remove_pointer_t<decltype(V)>;
            hipLaunchKernelGGL((kr_scale_store<T, FW>), G, B, 0, K.s, ws->n, x, s, V + (int64_t)j * ld, vector(j));
        });
    }
    // part = partials of the products of w with rows 0 .. nk - 1
    void multidot(int nk, const double* w) const {
        rows([&](auto* V, int64_t ld, auto FW) {
            using T = std::remove_pointer_t<decltype(V)>;
            with_int<4, 8, 16, 32, 64>(kr_kmax(nk), [&](auto KMAX) {
                hipLaunchKernelGGL((kr_multidot<KMAX, T, FW>), G, B, 0, K.s, ws->n, V, ld, nk, w, ws->part);
            }, kr_no_shape);
        });
    }
    // w -= sum_k row_k h_k, npart = partials of |w|^2
    void update(int nk, const double* h, double* w, double* npart) const {
        rows([&](auto* V, int64_t ld, auto FW) {
            using T = std::remove_pointer_t<decltype(V)>;
            hipLaunchKernelGGL((kr_update<T, FW>), G, B, 0, K.s, ws->n, V, ld, nk, h, w, npart);
        });
    }
    // out = sum_k row_k y_k
    void combine(int nk, const double* y, double* out) const {
        rows([&](auto* V, int64_t ld, auto FW) {
            using T = std::remove_pointer_t<decltype(V)>;
            hipLaunchKernelGGL((kr_combine<T, FW>), G, B, 0, K.s, ws->n, V, ld, nk, y, out);
        });
    }
};

// FLEX: z_j = M v_j goes to row j of the second basis and the update combines those rows; otherwise one Z and M once more at the update
template <bool FLEX>
int gmres_impl(KrCall& K, const double* b, double* x, double rtol, double atol, int max_it, int check_every, dxo_krylov_info* info) {
    dxo_ctx* ctx = K.ctx;
    dxo_krylov* ws = K.ws;
    const hipStream_t s = K.s;
    const int m = ws->m;
    const int64_t n = ws->n;
    double* sc = ws->sc;
    double* S = sc + ws->o_s();
    double* npart = ws->part + (int64_t)(m + 1) * ws->nb;
    const dim3 G(ws->nb), B(DXO_KR_BLOCK);
    const bool reorth = ctx->krylov_reorth != 0;
    const KrBasis V(K);
    double bnorm = 0.0, tol = 0.0;
    int rc = K.begin(b, x, rtol, atol, info, &bnorm, &tol);
    if (rc != DXO_OK || bnorm == 0.0) return rc;
    int total = 0;
    double beta = 0.0;
    for (;;) {
        if ((rc = K.residual(b, x, &beta)) != DXO_OK) return rc;
        info->residual = beta / bnorm;
        if (beta <= tol) {
            info->converged = 1;
            break;
        }
        if (total >= max_it || info->breakdown) break;
        ++info->restarts;
        V.scale_store(0, ws->R(), S + S_INV);
        hipLaunchKernelGGL(kr_cycle_init, dim3(1), dim3(64), 0, s, sc, ws->st, m, ws->o_g(), ws->o_s());
        int done = 0, status[2] = {-1, 0};
        for (int j = 0; j < m && total + j < max_it; ++j) {
            double* w = V.vector(j + 1);
            double* h = sc + (int64_t)j * (m + 1);
            double* zj = FLEX ? ws->zb + (int64_t)j * ws->ld : ws->Z();
            if ((rc = K.precond(V.vector(j), zj)) != DXO_OK) return rc;
            if ((rc = K.apply(zj, w)) != DXO_OK) return rc;
            V.multidot(j + 1, w);
            hipLaunchKernelGGL(kr_reduce, dim3(j + 1), B, 0, s, ws->part, ws->nb, h, (double*)nullptr, 0, (double*)nullptr);
            V.update(j + 1, h, w, npart);
            if (reorth) {
                double* c = sc + ws->o_c();
                V.multidot(j + 1, w);
                hipLaunchKernelGGL(kr_reduce, dim3(j + 1), B, 0, s, ws->part, ws->nb, c, h, 0, (double*)nullptr);
                V.update(j + 1, c, w, npart);
            }
            hipLaunchKernelGGL(kr_reduce, dim3(1), B, 0, s, npart, ws->nb, S + S_HNORM, (double*)nullptr, 1, S + S_HINV);
            V.scale_store(j + 1, w, S + S_HINV);
            hipLaunchKernelGGL(kr_givens, dim3(1), dim3(64), 0, s, sc, ws->st, j, m, ws->o_g(), ws->o_cs(), ws->o_sn(), ws->o_s(), tol);
            done = j + 1;
            if ((total + done) % check_every == 0 || done == m || total + done == max_it) {
                if ((rc = K.read(status, ws->st, sizeof status)) != DXO_OK) return rc;
                if (status[W_CONV] >= 0) break;
            }
        }
        if (status[W_CONV] < 0 && (rc = K.read(status, ws->st, sizeof status)) != DXO_OK) return rc;
        const int k = status[W_CONV] >= 0 ? status[W_CONV] : done;
        if (status[W_BREAK]) info->breakdown = 1;
        total += k;
        if (k > 0) {
            hipLaunchKernelGGL(kr_trisolve, dim3(1), dim3(64), 0, s, sc, k, m, ws->o_g(), ws->o_y());
            if constexpr (FLEX) {
                hipLaunchKernelGGL((kr_combine<double, 1>), G, B, 0, s, n, ws->zb, ws->ld, k, sc + ws->o_y(), ws->T());
                hipLaunchKernelGGL(kr_axpy, G, B, 0, s, n, S + S_ONE, 1.0, ws->T(), x);
            } else {
                V.combine(k, sc + ws->o_y(), ws->T());
                if ((rc = K.precond(ws->T(), ws->Z())) != DXO_OK) return rc;
                hipLaunchKernelGGL(kr_axpy, G, B, 0, s, n, S + S_ONE, 1.0, ws->Z(), x);
            }
        }
        if (k == 0) break;
    }
    info->iterations = total;
    return DXO_OK;
}

int cg_impl(KrCall& K, const double* b, double* x, double rtol, double atol, int max_it, int check_every, dxo_krylov_info* info) {
    dxo_ctx* ctx = K.ctx;
    dxo_krylov* ws = K.ws;
    const hipStream_t s = K.s;
    const int64_t n = ws->n;
    double* S = ws->sc + ws->o_s();
    int* st = ws->st;
    const dim3 G(ws->nb), B(DXO_KR_BLOCK), One(1);
    double bnorm = 0.0, tol = 0.0;
    int rc = K.begin(b, x, rtol, atol, info, &bnorm, &tol);
    if (rc != DXO_OK || bnorm == 0.0) return rc;
    double* r = ws->R();
    double* z = ws->Z();
    double* p = ws->T();
    double* q = ws->Q();
    double beta = 0.0;
    if ((rc = K.residual(b, x, &beta)) != DXO_OK) return rc;
    int it = 0;
    if (beta > tol && max_it > 0) {
        info->restarts = 1;
        hipLaunchKernelGGL(kr_cycle_init, One, dim3(64), 0, s, ws->sc, st, 0, ws->o_g(), ws->o_s());
        if ((rc = K.precond(r, z)) != DXO_OK) return rc;
        DXO_HIP(ctx, hipMemcpyAsync(p, z, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
        K.dot_partials(r, z, ws->part);
        hipLaunchKernelGGL(kr_cg_scalar, One, B, 0, s, ws->part, ws->nb, S, st, 0, 0, tol);
        int status[2] = {-1, 0};
        for (it = 1; it <= max_it; ++it) {
            if ((rc = K.apply(p, q)) != DXO_OK) return rc;
            K.dot_partials(p, q, ws->part);
            hipLaunchKernelGGL(kr_cg_scalar, One, B, 0, s, ws->part, ws->nb, S, st, 1, it, tol);
            hipLaunchKernelGGL(kr_axpy, G, B, 0, s, n, S + S_ALPHA, 1.0, p, x);
            hipLaunchKernelGGL(kr_axpy, G, B, 0, s, n, S + S_ALPHA, -1.0, q, r);
            K.dot_partials(r, r, ws->part);
            hipLaunchKernelGGL(kr_cg_scalar, One, B, 0, s, ws->part, ws->nb, S, st, 2, it, tol);
            if ((rc = K.precond(r, z)) != DXO_OK) return rc;
            K.dot_partials(r, z, ws->part);
            hipLaunchKernelGGL(kr_cg_scalar, One, B, 0, s, ws->part, ws->nb, S, st, 3, it, tol);
            hipLaunchKernelGGL(kr_xpay, G, B, 0, s, n, z, S + S_BETA, p);
            if (it % check_every == 0 || it == max_it) {
                if ((rc = K.read(status, st, sizeof status)) != DXO_OK) return rc;
                if (status[W_CONV] >= 0) break;
            }
        }
        it = status[W_CONV] >= 0 ? status[W_CONV] : max_it;
        if (status[W_BREAK]) info->breakdown = 1;
        if ((rc = K.residual(b, x, &beta)) != DXO_OK) return rc;
    }
    info->iterations = it;
    info->residual = beta / bnorm;
    info->converged = beta <= tol;
    return DXO_OK;
}

typedef int (*kr_solver)(KrCall&, const double*, double*, double, double, int, int, dxo_krylov_info*);

int kr_solve(dxo_ctx* ctx, const char* who, kr_solver solver, bool flexible, dxo_krylov* ws, const dxo_krylov_op* op, const dxo_krylov_pc* pc, const double* b,
             double* x, double rtol, double atol, int max_it, int check_every, dxo_krylov_info* info) {
    const auto t0 = std::chrono::steady_clock::now();
    int rc = kr_validate(ctx, who, flexible, ws, op, pc, b, x, rtol, atol, max_it, check_every);
    if (rc != DXO_OK) return rc;
    dxo_krylov_info local;
    dxo_krylov_info* inf = info ? info : &local;
    *inf = dxo_krylov_info{};
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    if (flexible && !ws->zb) {      // the second basis: at the first flexible solve, kept with the workspace
        const size_t bytes = (size_t)ws->m * ws->ld * sizeof(double);
        hipError_t e = hipMalloc((void**)&ws->zb, bytes);
        if (e == hipSuccess && (e = hipMemset(ws->zb, 0, bytes)) != hipSuccess) {
            (void)hipFree(ws->zb);
            ws->zb = nullptr;
        }
        if (e != hipSuccess) {
            ws->zb = nullptr;
            return dxo_hip_fail(ctx, e, "dxo_krylov_fgmres: second basis");
        }
    }
    KrCall K{ctx, ws, op, pc, dxo_launch_stream(ctx)};
    rc = solver(K, b, x, rtol, atol, max_it, check_every, inf);
    inf->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

}  // namespace

int dxo_kr_bj_setup_launch(const dxo_csr* csr, const double* values, double* inv, int* flag, hipStream_t s) {
    int rc = DXO_OK;
    with_bs(csr->bs, [&](auto BS) {
        if (csr->n_nodes == 0) return;
        hipLaunchKernelGGL(bj_setup<BS>, dim3((unsigned)((csr->n_nodes + DXO_KR_BLOCK - 1) / DXO_KR_BLOCK)), dim3(DXO_KR_BLOCK), 0, s, csr->n_nodes,
                           csr->d_row_ptr, csr->d_col, values, inv, flag);
    }, [&](int) { rc = DXO_E_DIM; });
    return rc;
}

int dxo_kr_spmv_launch(dxo_ctx* ctx, const dxo_csr* csr, const double* values, const double* x, double* y, hipStream_t s) {
    return spmv_launch(ctx, "dxo_amg_apply", csr, values, 1.0, x, 0.0, y, s);
}

int dxo_kr_spmv_lanes(const dxo_ctx* ctx, const dxo_csr* csr) { return spmv_lanes(ctx, csr); }

int dxo_kr_bj_apply_launch(dxo_ctx* ctx, const char* who, int bs, int64_t n, const double* inv, const double* r, double* z, hipStream_t s) {
    return bj_apply_launch(ctx, who, bs, n, inv, r, z, s);
}

extern "C" int dxo_csr_spmv(dxo_ctx* ctx, const dxo_csr* csr, const double* values, double alpha, const double* x, double beta, double* y) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!csr || !values || !x || !y) return dxo_fail(ctx, DXO_E_NULL, "dxo_csr_spmv: NULL argument");
    if (misaligned(values) || misaligned(x) || misaligned(y)) return dxo_fail(ctx, DXO_E_ALIGN, "dxo_csr_spmv: arrays must be 8-byte aligned");
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    int rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    rc = spmv_launch(ctx, "dxo_csr_spmv", csr, values, alpha, x, beta, y, s);
    const int end = dxo_device_end(ctx, s);
    return rc != DXO_OK ? rc : end;
}

extern "C" int dxo_csr_block_jacobi(dxo_ctx* ctx, const dxo_csr* csr, const double* values, double* inv) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!csr || !values || !inv) return dxo_fail(ctx, DXO_E_NULL, "dxo_csr_block_jacobi: NULL argument");
    if (misaligned(values) || misaligned(inv)) return dxo_fail(ctx, DXO_E_ALIGN, "dxo_csr_block_jacobi: arrays must be 8-byte aligned");
    if (!has_bs(csr->bs)) return bs_refused(ctx, "dxo_csr_block_jacobi", "the block inverse takes " KR_BS_LIST, csr->bs);
    if (csr->n_nodes == 0) return DXO_OK;
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    int* flag = (int*)dxo_scratch(ctx, s, 16);
    if (!flag) return dxo_fail(ctx, DXO_E_SIZE, "dxo_csr_block_jacobi: scratch allocation failed");
    DXO_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(int), s));
    (void)dxo_kr_bj_setup_launch(csr, values, inv, flag, s);      // the block size was checked above
    int h = 0;
    DXO_HIP(ctx, hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, s));
    DXO_HIP(ctx, hipStreamSynchronize(s));
    if (h) return dxo_fail(ctx, DXO_E_SINGULAR, "dxo_csr_block_jacobi: a diagonal block is singular (its inverse was set to zero)");
    return DXO_OK;
}

extern "C" int dxo_block_jacobi_apply(dxo_ctx* ctx, int bs, int64_t n, const double* inv, const double* r, double* z) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!inv || !r || !z) return dxo_fail(ctx, DXO_E_NULL, "dxo_block_jacobi_apply: NULL argument");
    if (bs < 1 || bs > 3) return dxo_fail(ctx, DXO_E_DIM, "dxo_block_jacobi_apply: bs must be 1, 2 or 3");
    if (n < 0 || n % bs != 0) return dxo_fail(ctx, DXO_E_SIZE, "dxo_block_jacobi_apply: n < 0 or not a multiple of bs");
    if (misaligned(inv) || misaligned(r) || misaligned(z)) return dxo_fail(ctx, DXO_E_ALIGN, "dxo_block_jacobi_apply: arrays must be 8-byte aligned");
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    int rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    rc = bj_apply_launch(ctx, "dxo_block_jacobi_apply", bs, n, inv, r, z, s);
    const int end = dxo_device_end(ctx, s);
    return rc != DXO_OK ? rc : end;
}

extern "C" int dxo_krylov_create_basis(dxo_ctx* ctx, int64_t n, int restart, int basis, dxo_krylov** out) {
    if (!ctx || !out) return DXO_E_NULL;
    DXO_LOCK(ctx);
    *out = nullptr;
    if (n < 0) return dxo_fail(ctx, DXO_E_SIZE, "dxo_krylov_create: n < 0");
    if (restart < 1 || restart > KR_MAX_RESTART) return dxo_fail(ctx, DXO_E_SIZE, "dxo_krylov_create: restart must lie in [1, 64]");
    if (basis != DXO_KRYLOV_BASIS_FP64 && basis != DXO_KRYLOV_BASIS_FP32)
        return dxo_fail(ctx, DXO_E_OPTION, "dxo_krylov_create_basis: basis must be DXO_KRYLOV_BASIS_FP64 (0) or DXO_KRYLOV_BASIS_FP32 (1)");
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    dxo_krylov* w = new dxo_krylov;
    w->n = n;
    w->m = restart;
    w->basis = basis;
    w->ld = std::max<int64_t>(32, (n + 31) / 32 * 32);
    w->nb = kr_grid(ctx, n, 4);
    const bool f32 = basis == DXO_KRYLOV_BASIS_FP32;
    if (f32) w->ldf = std::max<int64_t>(64, (n + 63) / 64 * 64);
    auto fail = [&](hipError_t e, const char* what) {
        for (void* p : {(void*)w->vec, (void*)w->vf, (void*)w->part, (void*)w->sc, (void*)w->st})
            if (p) (void)hipFree(p);
        delete w;
        return dxo_hip_fail(ctx, e, what);
    };
    hipError_t e;
    const size_t vec_bytes = (size_t)w->work_rows() * w->ld * sizeof(double), vf_bytes = (size_t)(w->m + 1) * w->ldf * sizeof(float);
    if ((e = hipMalloc((void**)&w->vec, vec_bytes)) != hipSuccess) return fail(e, "dxo_krylov_create: basis");
    if (f32 && (e = hipMalloc((void**)&w->vf, vf_bytes)) != hipSuccess) return fail(e, "dxo_krylov_create: float basis");
    if ((e = hipMalloc((void**)&w->part, (size_t)(w->m + 2) * w->nb * sizeof(double))) != hipSuccess) return fail(e, "dxo_krylov_create: partials");
    if ((e = hipMalloc((void**)&w->sc, (size_t)w->sc_doubles() * sizeof(double))) != hipSuccess) return fail(e, "dxo_krylov_create: state");
    if ((e = hipMalloc((void**)&w->st, 16 * sizeof(int))) != hipSuccess) return fail(e, "dxo_krylov_create: status");
    std::vector<double> init((size_t)w->sc_doubles(), 0.0);
    init[(size_t)(w->o_s() + S_ONE)] = 1.0;
    if ((e = hipMemcpy(w->sc, init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return fail(e, "dxo_krylov_create: state");
    if ((e = hipMemset(w->vec, 0, vec_bytes)) != hipSuccess) return fail(e, "dxo_krylov_create: basis");
    if (f32 && (e = hipMemset(w->vf, 0, vf_bytes)) != hipSuccess) return fail(e, "dxo_krylov_create: float basis");
    if ((e = hipMemset(w->st, 0, 16 * sizeof(int))) != hipSuccess) return fail(e, "dxo_krylov_create: status");
    *out = w;
    return DXO_OK;
}

extern "C" int dxo_krylov_create(dxo_ctx* ctx, int64_t n, int restart, dxo_krylov** out) {
    return dxo_krylov_create_basis(ctx, n, restart, DXO_KRYLOV_BASIS_FP64, out);
}

extern "C" int dxo_krylov_basis_info(dxo_ctx* ctx, const dxo_krylov* ws, int* basis, int64_t* basis_bytes, const void** rows, int64_t* ld) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!ws) return dxo_fail(ctx, DXO_E_NULL, "dxo_krylov_basis_info: NULL workspace");
    const bool f32 = ws->basis == DXO_KRYLOV_BASIS_FP32;
    if (basis) *basis = ws->basis;
    if (basis_bytes) *basis_bytes = f32 ? (int64_t)(ws->m + 1) * ws->ldf * (int64_t)sizeof(float) : (int64_t)(ws->m + 1) * ws->ld * (int64_t)sizeof(double);
    if (rows) *rows = f32 ? (const void*)ws->vf : (const void*)ws->vec;
    if (ld) *ld = f32 ? ws->ldf : ws->ld;
    return DXO_OK;
}

extern "C" int dxo_krylov_destroy(dxo_ctx* ctx, dxo_krylov* ws) {
    if (!ws) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (ctx) (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (void* p : {(void*)ws->vec, (void*)ws->vf, (void*)ws->zb, (void*)ws->part, (void*)ws->sc, (void*)ws->st})
        if (p) (void)hipFree(p);
    delete ws;
    return DXO_OK;
}

extern "C" int dxo_krylov_gmres(dxo_ctx* ctx, dxo_krylov* ws, const dxo_krylov_op* op, const dxo_krylov_pc* pc, const double* b, double* x,
                                double rtol, double atol, int max_it, int check_every, dxo_krylov_info* info) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    return kr_solve(ctx, "dxo_krylov_gmres", gmres_impl<false>, false, ws, op, pc, b, x, rtol, atol, max_it, check_every, info);
}

extern "C" int dxo_krylov_cg(dxo_ctx* ctx, dxo_krylov* ws, const dxo_krylov_op* op, const dxo_krylov_pc* pc, const double* b, double* x,
                             double rtol, double atol, int max_it, int check_every, dxo_krylov_info* info) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (ws && ws->basis != DXO_KRYLOV_BASIS_FP64)
        return dxo_fail(ctx, DXO_E_OPTION, "dxo_krylov_cg: CG keeps no basis: the workspace must be of kind DXO_KRYLOV_BASIS_FP64");
    return kr_solve(ctx, "dxo_krylov_cg", cg_impl, false, ws, op, pc, b, x, rtol, atol, max_it, check_every, info);
}

extern "C" int dxo_krylov_fgmres(dxo_ctx* ctx, dxo_krylov* ws, const dxo_krylov_op* op, const dxo_krylov_pc* pc, const double* b, double* x,
                                 double rtol, double atol, int max_it, int check_every, dxo_krylov_info* info) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    return kr_solve(ctx, "dxo_krylov_fgmres", gmres_impl<true>, true, ws, op, pc, b, x, rtol, atol, max_it, check_every, info);
}
