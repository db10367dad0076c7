// functional.hip — scalar functionals (rank-0 forms): quadrature data reduced to a few numbers on the device.
//
// Reference: `fem.assemble_scalar(fem.form(J))` as the package's tests and demos use it — J = g(u) * ds and f(u * u) * dx over a cell
// subset with their Gateaux derivatives (test/test_codim_external_operator.py), and the error norm
// sqrt(assemble_scalar((u - u_UFL)**2 * dx)) that ends demo_hyperelasticity.py (:817).
//
//   dxo_eval_cell_measure   dx[c][q] = w_q |det J|, the cell counterpart of dS (dxo_eval_facet_geometry)
//   dxo_integrate           out[k] = sum_c sum_q dx f[c][q][k]  (g == NULL)   or   out[0] = sum dx sum_k f_k g_k  (the pairing f : g)
//   dxo_facet_integrate     the same two forms over a facet set with dS
//   dxo_operand_moments     out[k] = int operand_k(u) dx, out[D] = int |operand(u)|^2 dx, the operand formed in registers, never written
//
// Geometry comes from the helpers the other kernels use: gather_vertices / point_jacobian and operand_compute_geo (operand_core.h) for
// the cells, facet_point_geometry (facet_tabs.h) for the facets.
//
// Reduction order. A GROUP is what one wave takes in one trip: the cells_per_wave = floor(64 / nq) consecutive cells of the list that a
// wave of operand_eval owns, or floor(64 / nq_facet) consecutive entities of the set (one entity for a rule of more than 64 points).
// The group's points are summed in a fixed lane order (wave_sum: a butterfly over the 64 lanes, idle lanes carry +0.0) and ONE partial per
// output goes to the scratch part[k][group]. What a group holds depends on the list and on nq alone, so which wave of which workgroup
// forms a partial — the grid, the compute-unit count, the walk over the XCDs — never reaches the bits. fn_final, one workgroup per
// output, adds that output's partials: lane t of FN_FINAL takes groups t, t + FN_FINAL, ... in ascending order, then a fixed LDS tree
// joins the lanes. No atomics; `out` is SET; no groups (an empty list) leaves +0.0.
// The scratch is grow-only, owned by the mesh (cell calls) or by the facet set: the first call of a size allocates, later ones neither
// allocate nor synchronise (capture-safe).
#include "dxo_common.h"
#include "facet_tabs.h"
#include "form_host.h"

namespace {

constexpr int FN_FINAL = 256;      // lanes of the final pass (W in the tests)
constexpr int FN_AHEAD = 32;       // partials a lane of the final pass has in flight
constexpr int FN_WAVES = DXO_BLOCK / DXO_WAVE;
constexpr int FN_BLOCKS_PER_CU = 8;
constexpr int FN_MAX_D = 1 << 24;  // the pairing's D: a group's 64 * D values are indexed with an int

// the sum over the wave's 64 lanes, the same bits in every lane: lane i adds its partner i ^ off at every level, and the partner adds the
// same two numbers the other way round
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 1; off < DXO_WAVE; off <<= 1) v += __shfl_xor(v, off, DXO_WAVE);
    return v;
}

// t[0 .. N) of every lane -> part[k][grp], written by lane k
template <int N>
__device__ __forceinline__ void group_partials(double (&t)[N], int lane, int64_t n_groups, int64_t grp, double* __restrict__ part) {
#pragma unroll
    for (int k = 0; k < N; ++k) t[k] = wave_sum(t[k]);
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (lane == k) part[(int64_t)k * n_groups + grp] = t[k];
}

// out[b] = the sum of part[b][0 .. n_groups), one workgroup per output
__global__ __launch_bounds__(FN_FINAL) void fn_final(const double* __restrict__ part, int64_t n_groups, double* __restrict__ out) {
    __shared__ double s[FN_FINAL];
    const double* col = part + (int64_t)blockIdx.x * n_groups;
    double acc = 0.0;
    int64_t g = threadIdx.x;
    // FN_AHEAD loads in flight, then added in the order of the plain loop below: the same chain of additions without its latency (one
    // workgroup reads all partials of its output; a load per addition, waited for, took 0.2 ms at 1.6e5 groups)
    for (; g + (int64_t)(FN_AHEAD - 1) * FN_FINAL < n_groups; g += (int64_t)FN_AHEAD * FN_FINAL) {
        double v[FN_AHEAD];
#pragma unroll
        for (int i = 0; i < FN_AHEAD; ++i) v[i] = col[g + (int64_t)i * FN_FINAL];
#pragma unroll
        for (int i = 0; i < FN_AHEAD; ++i) acc += v[i];
    }
    for (; g < n_groups; g += FN_FINAL) acc += col[g];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int h = FN_FINAL / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}

// LDS of a wave of the geometry-only cell kernels: the group's vertices, then `extra` doubles
__host__ __device__ __forceinline__ int fn_vertex_doubles(const OperandDev& m, int G) { return op_even(m.cells_per_wave * op_odd(m.ngeom * G)); }

// w |det J| of this lane's point from the vertices gathered in X; 0 for a lane without a point
template <int G>
__device__ __forceinline__ double lane_measure(const OperandDev& m, const double* tab, const double* X, double w_l, int c, int q, int ncell) {
    if (c >= ncell) return 0.0;
    const OperandLayout<G> L(m);
    double K[G][G];
    return w_l * fabs(point_jacobian<G>(tab + L.o_dpsi + q * L.sdpsi, X + c * L.sx, m.ngeom, K));
}

// dx[c][q] = w_q |det J|: lane = (cell, point) is the order of the output
template <int G>
__global__ __launch_bounds__(DXO_BLOCK) void fn_cell_measure(OperandDev m, const double* __restrict__ wq, int lds_wave,
                                                             const int32_t* __restrict__ cells, int64_t n_cells, double* __restrict__ dx) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* tab = lds;
    operand_load_tables<G>(m, tab);
    __syncthreads();
    const int lane = threadIdx.x & (DXO_WAVE - 1), wave = threadIdx.x >> 6;
    double* X = lds + m.table_doubles + wave * lds_wave;
    const int cpw = m.cells_per_wave;
    const int c = lane / m.nq, q = lane - c * m.nq;
    const double w_l = c < cpw ? wq[q] : 0.0;
    const int64_t n_groups = (n_cells + cpw - 1) / cpw;
    const GroupWalk walk = xcd_group_walk(n_groups, FN_WAVES, wave);
    for (int64_t grp = walk.first; grp < walk.end; grp += walk.stride) {
        const int64_t c0 = grp * cpw;
        const int ncell = group_cells(walk, n_cells, cpw, grp);
        gather_vertices<G>(m, X, cells, c0, ncell, lane);
        op_fence();
        const double v = lane_measure<G>(m, tab, X, w_l, c, q, ncell);
        if (c < ncell) dx[c0 * m.nq + lane] = v;
        op_fence();      // X is gathered again
    }
}

// part[k][grp] = sum over the group's points of dx f_k. The group's ncell * nq * D values are consecutive in f: they are read
// lane-linearly into the wave's LDS slice F and every lane takes its point's D values from there (store_points of operand_eval, reversed)
template <int G, int D>
__global__ __launch_bounds__(DXO_BLOCK) void fn_integrate(OperandDev m, const double* __restrict__ wq, int lds_wave, const double* __restrict__ f,
                                                          const int32_t* __restrict__ cells, int64_t n_cells, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* tab = lds;
    operand_load_tables<G>(m, tab);
    __syncthreads();
    const int lane = threadIdx.x & (DXO_WAVE - 1), wave = threadIdx.x >> 6;
    double* X = lds + m.table_doubles + wave * lds_wave;
    double* F = X + fn_vertex_doubles(m, G);
    const int cpw = m.cells_per_wave;
    const int c = lane / m.nq, q = lane - c * m.nq;
    const double w_l = c < cpw ? wq[q] : 0.0;
    const int64_t n_groups = (n_cells + cpw - 1) / cpw;
    const GroupWalk walk = xcd_group_walk(n_groups, FN_WAVES, wave);
    for (int64_t grp = walk.first; grp < walk.end; grp += walk.stride) {
        const int64_t c0 = grp * cpw;
        const int ncell = group_cells(walk, n_cells, cpw, grp);
        const int nval = ncell * m.nq * D;
        const double* f_g = f + c0 * m.nq * D;
        for (int idx = lane; idx < nval; idx += DXO_WAVE) F[idx] = __builtin_nontemporal_load(f_g + idx);
        gather_vertices<G>(m, X, cells, c0, ncell, lane);
        op_fence();
        const double dx = lane_measure<G>(m, tab, X, w_l, c, q, ncell);
        double t[D];
#pragma unroll
        for (int k = 0; k < D; ++k) t[k] = c < ncell ? dx * F[lane * D + k] : 0.0;
        group_partials<D>(t, lane, n_groups, grp, part);
        op_fence();      // X and F are filled again
    }
}

// part[0][grp] = sum over the group's points of dx sum_k f_k g_k, any D (DT = 0: D at run time). The measures of the group's points
// are parked in LDS and the values are read lane-linearly straight from f and g: value idx belongs to point idx / D
template <int G, int DT>
__global__ __launch_bounds__(DXO_BLOCK) void fn_pair(OperandDev m, const double* __restrict__ wq, int lds_wave, int d_rt, const double* f,
                                                     const double* g, const int32_t* __restrict__ cells, int64_t n_cells,
                                                     double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* tab = lds;
    operand_load_tables<G>(m, tab);
    __syncthreads();
    const int D = DT ? DT : d_rt;
    const int lane = threadIdx.x & (DXO_WAVE - 1), wave = threadIdx.x >> 6;
    double* X = lds + m.table_doubles + wave * lds_wave;
    double* DX = X + fn_vertex_doubles(m, G);
    const int cpw = m.cells_per_wave;
    const int c = lane / m.nq, q = lane - c * m.nq;
    const double w_l = c < cpw ? wq[q] : 0.0;
    const int64_t n_groups = (n_cells + cpw - 1) / cpw;
    const GroupWalk walk = xcd_group_walk(n_groups, FN_WAVES, wave);
    for (int64_t grp = walk.first; grp < walk.end; grp += walk.stride) {
        const int64_t c0 = grp * cpw;
        const int ncell = group_cells(walk, n_cells, cpw, grp);
        gather_vertices<G>(m, X, cells, c0, ncell, lane);
        op_fence();
        DX[lane] = lane_measure<G>(m, tab, X, w_l, c, q, ncell);
        op_fence();
        const int64_t base = c0 * m.nq * D;
        const int nval = ncell * m.nq * D;      // D <= FN_MAX_D: below 2^31
        const double* f_g = f + base;
        const double* g_g = g + base;
        double t[1] = {0.0};
        for (int idx = lane; idx < nval; idx += DXO_WAVE)
            t[0] += __builtin_nontemporal_load(f_g + idx) * __builtin_nontemporal_load(g_g + idx) * DX[idx / D];
        group_partials<1>(t, lane, n_groups, grp, part);
        op_fence();      // X and DX are filled again
    }
}

// part[k][grp] = sum dx operand_k(u) for k < D, part[D][grp] = sum dx |operand(u)|^2: the group loop of operand_eval (operand.hip) with
// the output store replaced by the group's partial sums
template <int G, int BS, int KIND>
__global__ __launch_bounds__(DXO_BLOCK) void fn_moments(OperandDev m, const double* __restrict__ wq, const double* __restrict__ u,
                                                        const int32_t* __restrict__ cells, int64_t n_cells, double* __restrict__ part) {
    constexpr int D = OperandShape<G, BS, KIND>::D;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* tab = lds;
    operand_load_tables<G>(m, tab);
    __syncthreads();
    const int lane = threadIdx.x & (DXO_WAVE - 1), wave = threadIdx.x >> 6;
    double* W = lds + m.table_doubles + wave * m.wave_doubles;
    const int cpw = m.cells_per_wave;
    const int q = lane % m.nq;
    const double w_l = lane / m.nq < cpw ? wq[q] : 0.0;
    const int64_t n_groups = (n_cells + cpw - 1) / cpw;
    const GroupWalk walk = xcd_group_walk(n_groups, FN_WAVES, wave);
    const int64_t stride = walk.stride;
    auto reduce_points = [&](int64_t grp, bool active, const double (&o)[D], double detJ) {
        double t[D + 1];
#pragma unroll
        for (int k = 0; k <= D; ++k) t[k] = 0.0;
        if (active) {
            const double dx = w_l * fabs(detJ);
            double sq = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                t[k] = dx * o[k];
                sq += o[k] * o[k];
            }
            t[D] = dx * sq;
        }
        group_partials<D + 1>(t, lane, n_groups, grp, part);
    };
    int64_t grp = walk.first;
    if (cells == nullptr && operand_can_pipe(m)) {
        OperandPipe<G, BS> pf;
        pipe_load_indices<G, BS>(m, pf, grp * cpw, group_cells(walk, n_cells, cpw, grp), lane);
        pipe_load_values<G, BS>(m, pf, u);
        pipe_load_indices<G, BS>(m, pf, (grp + stride) * cpw, group_cells(walk, n_cells, cpw, grp + stride), lane);
        for (; grp < walk.end; grp += stride) {
            const int ncell = group_cells(walk, n_cells, cpw, grp);
            pipe_commit<G, BS>(m, pf, W, ncell, lane);
            pipe_load_values<G, BS>(m, pf, u);
            pipe_load_indices<G, BS>(m, pf, (grp + 2 * stride) * cpw, group_cells(walk, n_cells, cpw, grp + 2 * stride), lane);
            double o[D], K[G][G], detJ = 0.0;
            const bool active = operand_compute_geo<G, BS, KIND>(m, tab, W, ncell, lane, o, K, detJ);
            reduce_points(grp, active, o, detJ);
        }
        return;
    }
    for (; grp < walk.end; grp += stride) {
        const int ncell = group_cells(walk, n_cells, cpw, grp);
        operand_gather<G, BS>(m, W, u, cells, grp * cpw, ncell, lane);
        double o[D], K[G][G], detJ = 0.0;
        const bool active = operand_compute_geo<G, BS, KIND>(m, tab, W, ncell, lane, o, K, detJ);
        reduce_points(grp, active, o, detJ);
    }
}

// entities of a facet group: floor(64 / nq_facet), one for a rule of 64 points or more
__host__ __device__ __forceinline__ int fn_facet_epw(int nqf) { return nqf >= DXO_WAVE ? 1 : DXO_WAVE / nqf; }

// the facet forms: part[k][grp] = sum dS f_k (PAIR false, N = DT outputs) or part[0][grp] = sum dS sum_k f_k g_k (PAIR, DT = 0: D at
// run time). Lane = (entity, point) of the group; a rule of more than 64 points takes several trips per lane. Boundary work: the values
// are read per point
template <int G, int DT, bool PAIR>
__global__ __launch_bounds__(DXO_BLOCK) void fn_facet(OperandDev m, FacetTabs<G> t, const int32_t* __restrict__ ents, int64_t n, int d_rt,
                                                      const double* f, const double* g, double* __restrict__ part) {
    constexpr int N = PAIR ? 1 : DT;
    const int D = DT ? DT : d_rt;
    const int lane = threadIdx.x & (DXO_WAVE - 1), wave = threadIdx.x >> 6;
    const int nqf = t.nqf, epw = fn_facet_epw(nqf);
    const int64_t n_groups = (n + epw - 1) / epw;
    for (int64_t grp = (int64_t)blockIdx.x * FN_WAVES + wave; grp < n_groups; grp += (int64_t)gridDim.x * FN_WAVES) {
        const int64_t e0 = grp * epw;
        const int np = (int)(n - e0 < epw ? n - e0 : epw) * nqf;
        double acc[N];
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] = 0.0;
        for (int p = lane; p < np; p += DXO_WAVE) {
            const int le = p / nqf, q = p - le * nqf;
            const int64_t e = e0 + le;
            double K[G][G], nrm[G], ds;
            facet_point_geometry<G>(m, t, ents[2 * e], ents[2 * e + 1], q, K, nrm, ds);
            const double* fp = f + (e * nqf + q) * (int64_t)D;
            if constexpr (PAIR) {
                const double* gp = g + (e * nqf + q) * (int64_t)D;
                double s = 0.0;
                for (int k = 0; k < D; ++k) s += fp[k] * gp[k];
                acc[0] += ds * s;
            } else {
#pragma unroll
                for (int k = 0; k < DT; ++k) acc[k] += ds * fp[k];
            }
        }
        group_partials<N>(acc, lane, n_groups, grp, part);
    }
}

// ---- host side
// the value sizes of the per-component form (the operators of this library): f(int_c<D>) and true, or false
template <class F>
bool with_value_size(int D, F&& f) {
    bool found = true;
    with_int<1, 2, 3, 4, 6, 9>(D, f, [&](int) { found = false; });
    return found;
}

// the pairing's D: a compile-time divisor for the served value sizes, 0 (run time) for any other
template <class F>
void with_pair_size(int D, F&& f) {
    with_int<1, 2, 3, 4, 6, 9>(D, f, [&](int) { f(int_c<0>{}); });
}

void launch_final(int n_out, const double* part, int64_t n_groups, double* out, hipStream_t s) {
    hipLaunchKernelGGL(fn_final, dim3(n_out), dim3(FN_FINAL), 0, s, part, n_groups, out);
}

// the opening of the cell calls: mesh, weights, the list's length
int cells_ready(dxo_ctx* ctx, const dxo_mesh* m, const int32_t* cells, int64_t* n_cells, const char* who) {
    if (!m) return fail_who(ctx, DXO_E_NULL, who, "mesh is NULL");
    if (!m->d_wq) return fail_who(ctx, DXO_E_OPTION, who, "quadrature weights not set (dxo_mesh_set_weights)");
    if (!cells) *n_cells = *n_cells < 0 ? m->num_cells : *n_cells;
    if (*n_cells < 0 || (!cells && *n_cells > m->num_cells)) return fail_who(ctx, DXO_E_SIZE, who, "bad n_cells");
    if ((uintptr_t)cells & 3u) return fail_who(ctx, DXO_E_ALIGN, who, "cells must be 4-byte aligned");
    return DXO_OK;
}

// dynamic LDS of the geometry-only cell kernels with `extra` doubles per wave behind the vertices; 0 if it exceeds 64 KiB
size_t geometry_lds(const dxo_mesh* m, int extra, int* lds_wave) {
    *lds_wave = fn_vertex_doubles(m->dev, m->gdim) + op_even(extra);
    const size_t shm = (size_t)(m->dev.table_doubles + FN_WAVES * *lds_wave) * sizeof(double);
    return shm > 64 * 1024 ? 0 : shm;
}

}  // namespace

extern "C" int dxo_eval_cell_measure(dxo_ctx* ctx, dxo_mesh* m, const int32_t* cells, int64_t n_cells, double* dx) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    const char* who = "dxo_eval_cell_measure";
    int rc = cells_ready(ctx, m, cells, &n_cells, who);
    if (rc != DXO_OK) return rc;
    if (n_cells == 0) return DXO_OK;
    if (!dx) return fail_who(ctx, DXO_E_NULL, who, "dx is NULL");
    if ((uintptr_t)dx & 7u) return fail_who(ctx, DXO_E_ALIGN, who, "dx must be 8-byte aligned");
    int lds_wave = 0;
    const size_t shm = geometry_lds(m, 0, &lds_wave);
    if (!shm) return fail_who(ctx, DXO_E_SIZE, who, "element too large for the 64 KiB LDS budget");
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    const int blocks = wave_group_grid(ctx, wave_groups(m->dev, n_cells), FN_BLOCKS_PER_CU);
    with_gdim(m->gdim, [&](auto G) {
        hipLaunchKernelGGL(fn_cell_measure<G>, dim3(blocks), dim3(DXO_BLOCK), shm, s, m->dev, m->d_wq, lds_wave, cells, n_cells, dx);
    });
    return dxo_device_end(ctx, s);
}

extern "C" int dxo_integrate(dxo_ctx* ctx, dxo_mesh* m, const int32_t* cells, int64_t n_cells, int D, const double* f, const double* g,
                             double* out) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    const char* who = "dxo_integrate";
    int rc = cells_ready(ctx, m, cells, &n_cells, who);
    if (rc != DXO_OK) return rc;
    if (D < 1 || D > FN_MAX_D) return fail_who(ctx, DXO_E_DIM, who, "D must be in 1 .. 2^24");
    if (!g && !with_value_size(D, [](auto) {}))
        return fail_who(ctx, DXO_E_DIM, who, "the per-component form serves D = 1, 2, 3, 4, 6, 9 (the pairing, g != NULL, any D)");
    if (!out || (n_cells > 0 && !f)) return fail_who(ctx, DXO_E_NULL, who, "NULL array");
    if (((uintptr_t)f | (uintptr_t)g | (uintptr_t)out) & 7u) return fail_who(ctx, DXO_E_ALIGN, who, "arrays must be 8-byte aligned");
    const int n_out = g ? 1 : D;
    int lds_wave = 0;
    const size_t shm = geometry_lds(m, g ? DXO_WAVE : DXO_WAVE * D, &lds_wave);
    if (!shm) return fail_who(ctx, DXO_E_SIZE, who, "element too large for the 64 KiB LDS budget");
    const int64_t n_groups = wave_groups(m->dev, n_cells);
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    rc = device_buf(ctx, (void**)&m->d_fn_part, &m->fn_cap, (size_t)n_groups * n_out * sizeof(double));
    if (rc == DXO_OK) rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    if (n_groups > 0) {
        const int blocks = wave_group_grid(ctx, n_groups, FN_BLOCKS_PER_CU);
        with_gdim(m->gdim, [&](auto G) {
            if (g)
                with_pair_size(D, [&](auto DT) {
                    hipLaunchKernelGGL((fn_pair<G, DT>), dim3(blocks), dim3(DXO_BLOCK), shm, s, m->dev, m->d_wq, lds_wave, D, f, g, cells, n_cells,
                                       m->d_fn_part);
                });
            else
                with_value_size(D, [&](auto DT) {
                    hipLaunchKernelGGL((fn_integrate<G, DT>), dim3(blocks), dim3(DXO_BLOCK), shm, s, m->dev, m->d_wq, lds_wave, f, cells, n_cells,
                                       m->d_fn_part);
                });
        });
    }
    launch_final(n_out, m->d_fn_part, n_groups, out, s);
    return dxo_device_end(ctx, s);
}

extern "C" int dxo_facet_integrate(dxo_ctx* ctx, dxo_mesh* m, dxo_facet_set* set, int D, const double* f, const double* g, double* out) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    const char* who = "dxo_facet_integrate";
    int rc = facet_ready(ctx, m, set, who);
    if (rc != DXO_OK) return rc;
    if (D < 1 || D > FN_MAX_D) return fail_who(ctx, DXO_E_DIM, who, "D must be in 1 .. 2^24");
    if (!g && !with_value_size(D, [](auto) {}))
        return fail_who(ctx, DXO_E_DIM, who, "the per-component form serves D = 1, 2, 3, 4, 6, 9 (the pairing, g != NULL, any D)");
    if (!out || (set->n > 0 && !f)) return fail_who(ctx, DXO_E_NULL, who, "NULL array");
    if (((uintptr_t)f | (uintptr_t)g | (uintptr_t)out) & 7u) return fail_who(ctx, DXO_E_ALIGN, who, "arrays must be 8-byte aligned");
    const int n_out = g ? 1 : D, epw = fn_facet_epw(m->nq_facet);
    const int64_t n_groups = (set->n + epw - 1) / epw;
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    rc = device_buf(ctx, (void**)&set->d_fn_part, &set->fn_cap, (size_t)n_groups * n_out * sizeof(double));
    if (rc == DXO_OK) rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    if (n_groups > 0) {
        const int blocks = capped_grid(ctx, n_groups, FN_WAVES, FN_BLOCKS_PER_CU);
        with_gdim(m->gdim, [&](auto G) {
            const FacetTabs<G> t = facet_tabs<G>(m);
            if (g)
                hipLaunchKernelGGL((fn_facet<G, 0, true>), dim3(blocks), dim3(DXO_BLOCK), 0, s, m->dev, t, set->d_ents, set->n, D, f, g, set->d_fn_part);
            else
                with_value_size(D, [&](auto DT) {
                    hipLaunchKernelGGL((fn_facet<G, DT, false>), dim3(blocks), dim3(DXO_BLOCK), 0, s, m->dev, t, set->d_ents, set->n, D, f, g,
                                       set->d_fn_part);
                });
        });
    }
    launch_final(n_out, set->d_fn_part, n_groups, out, s);
    return dxo_device_end(ctx, s);
}

extern "C" int dxo_operand_moments(dxo_ctx* ctx, dxo_mesh* m, int kind, int bs, const double* u, const int32_t* cells, int64_t n_cells,
                                   double* out) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    const char* who = "dxo_operand_moments";
    int rc = cells_ready(ctx, m, cells, &n_cells, who);
    if (rc != DXO_OK) return rc;
    const int D = dxo_operand_value_size(m->gdim, bs, kind);
    if (D == DXO_E_OPTION) return fail_who(ctx, DXO_E_OPTION, who, "unknown operand kind");
    if (D < 0 || (bs != 1 && bs != m->gdim))
        return fail_who(ctx, DXO_E_DIM, who, "block size does not fit the operand kind / gdim (the fused form takes bs = 1 or gdim)");
    if (!out || (n_cells > 0 && !u)) return fail_who(ctx, DXO_E_NULL, who, "NULL array");
    if (((uintptr_t)u | (uintptr_t)out) & 7u) return fail_who(ctx, DXO_E_ALIGN, who, "arrays must be 8-byte aligned");
    const int64_t n_groups = wave_groups(m->dev, n_cells);
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    rc = device_buf(ctx, (void**)&m->d_fn_part, &m->fn_cap, (size_t)n_groups * (D + 1) * sizeof(double));
    if (rc == DXO_OK) rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    if (n_groups > 0) {
        const int blocks = wave_group_grid(ctx, n_groups, FN_BLOCKS_PER_CU);
        const size_t shm = (size_t)(m->dev.table_doubles + FN_WAVES * m->dev.wave_doubles) * sizeof(double);      // operand_eval's
        rc = with_form_shape(m->gdim, bs, [&](auto G, auto BS) {
            return with_operand_kind<G, BS, false>(kind, [&](auto KIND) {
                hipLaunchKernelGGL((fn_moments<G, BS, KIND>), dim3(blocks), dim3(DXO_BLOCK), shm, s, m->dev, m->d_wq, u, cells, n_cells,
                                   m->d_fn_part);
            });
        });
        if (rc != DXO_OK) return fail_who(ctx, rc, who, "unsupported (gdim, bs, kind)");
    }
    launch_final(D + 1, m->d_fn_part, n_groups, out, s);
    return dxo_device_end(ctx, s);
}
