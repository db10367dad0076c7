// bilinear.h — the action and the diagonal of a bilinear form between two linear operand kinds of one field, with a per-point
// block C_q (dxo_bilinear_apply / dxo_bilinear_diagonal). Included at the end of adjoint.hip: it reuses that file's gather,
// geometry, dual_tensor, adjoint_scatter and the two-pass scatter (element vectors fe + node_sum).
//   out[dof]  += sum_q w_q |det J_q| B_test,q^T C_q B_trial,q v           C_q: [D_test][D_trial] row-major fp64 per point
//   diag[dof] += sum_q w_q |det J_q| (B_test,q^T C_q B_trial,q)_(dof,dof)
//   out[dof]  += sum_q w_q |det J_q| B_trial,q^T C_q^T B_test,q v         the transposed action (dxo_bilinear_apply_t), same C
// dxo_tangent_apply is the pair (eps, eps) with bs = gdim; the finite-strain Jacobian of the hyperelasticity demo is (grad, grad) with
// C = dP/dF, the heat demo's Jacobian (grad, value_grad) with bs = 1 and C = [dq/dT | dq/dsigma].
#pragma once

#include <cstdio>
#include <type_traits>

#include "operand_coef.h"

#ifndef DXO_BL_WAVES
#define DXO_BL_WAVES 2       // waves per SIMD the kernels are compiled for (as tangent_apply)
#endif
#ifndef DXO_BL_BLOCKS_PER_CU
#define DXO_BL_BLOCKS_PER_CU 8
#endif

namespace {

// ---- the C blocks of a wave group. The group's points are consecutive, so its blocks are one contiguous run of npts * DT * DR doubles:
// it is requested LANE-LINEAR (consecutive lanes, consecutive 16-byte pieces: every cache line is fetched once, as TangentRows does for
// dxo_tangent_apply) and passes through the wave's LDS region in chunks of PC points, where every lane of the chunk picks up its own
// block. Small blocks (at most 40 doubles per lane for the whole group) are requested at the top of the iteration and sit in registers
// until the region is free; large ones (3-D grad / grad with bs = 3: 81 doubles per point) are STREAMED, one chunk of 8 points in
// registers at a time, the next chunk requested as soon as the current one is in LDS. Blocks of an odd number of doubles (1, 9, 81)
// cannot all start on a 16-byte boundary and are read 8 bytes at a time.
template <int DT, int DR>
struct BlockRows {
    static constexpr int DD = DT * DR;
    static constexpr int U = DD % 2 == 0 ? 2 : 1;                 // doubles per load
    using unit = typename std::conditional<U == 2, dxo_f64x2, double>::type;
    static constexpr int PC = DD <= 36 ? 32 : 8;                  // points per chunk
    static constexpr int NCH = DXO_WAVE / PC;
    static constexpr int UPP = DD / U;                            // units per point
    static constexpr int UPC = PC * UPP;                          // units per chunk
    static constexpr int LPC = (UPC + DXO_WAVE - 1) / DXO_WAVE;   // loads per lane and chunk
    static constexpr bool HOLD = NCH * LPC * U <= 40;
    static constexpr int NB = HOLD ? NCH : 1;
    static constexpr int RSU = U == 2 ? (UPP | 1) : UPP;          // staged stride of a point in units: odd (bank spread of the lanes' reads)
    static constexpr int LDS_DOUBLES = PC * RSU * U;
    unit r[NB][LPC];
    const unit* base;
    int nunits;

    static __device__ __forceinline__ unit zero() {
        if constexpr (U == 2) return dxo_f64x2{0.0, 0.0};
        else return 0.0;
    }
    __device__ __forceinline__ void request(int k, int b, int lane) {
#pragma unroll
        for (int j = 0; j < LPC; ++j) {
            const int w = j * DXO_WAVE + lane, u = k * UPC + w;
            r[b][j] = (w < UPC && u < nunits) ? base[u] : zero();
        }
    }
    // p0: first point of the group, npts: its points. C is 16-byte aligned and DD even when U = 2, so every piece is.
    __device__ __forceinline__ void begin(const double* __restrict__ C, int64_t p0, int npts, int lane) {
        base = reinterpret_cast<const unit*>(C + p0 * DD);
        nunits = npts * UPP;
        if constexpr (HOLD) {
#pragma unroll
            for (int k = 0; k < NCH; ++k) request(k, k, lane);
        } else {
            request(0, 0, lane);
        }
    }
    // f(R) on the lane's own block R[DD] (row-major, in LDS), chunk by chunk; S = the wave's region (16-byte aligned). Ends fenced.
    template <class Fn>
    __device__ __forceinline__ void chunk(double* S, int lane, int k, int b, Fn& f) {
        unit* Su = reinterpret_cast<unit*>(S);
#pragma unroll
        for (int j = 0; j < LPC; ++j) {
            const int w = j * DXO_WAVE + lane;
            if (w < UPC) {
                const int p = w / UPP;
                Su[p * RSU + (w - p * UPP)] = r[b][j];
            }
        }
        if constexpr (!HOLD) {
            if (k + 1 < NCH) request(k + 1, 0, lane);
        }
        op_fence();
        if (lane / PC == k) f(static_cast<const double*>(S) + (lane - k * PC) * RSU * U);
        op_fence();
    }
    template <class Fn>
    __device__ __forceinline__ void for_each(double* S, int lane, Fn&& f) {
        if constexpr (HOLD) {
#pragma unroll
            for (int k = 0; k < NCH; ++k) chunk(S, lane, k, k, f);
        } else {
            // a rolled loop: unrolled, the compiler hoists every chunk's loads to the top and runs out of registers
#pragma unroll 1
            for (int k = 0; k < NCH; ++k) chunk(S, lane, k, 0, f);
        }
    }
    // t = C e for the lane's point
    __device__ __forceinline__ void times(double* S, int lane, const double (&e)[DR], double (&t)[DT]) {
#pragma unroll
        for (int i = 0; i < DT; ++i) t[i] = 0.0;
        for_each(S, lane, [&](const double* R) {
            const unit* Ru = reinterpret_cast<const unit*>(R);
#pragma unroll
            for (int u = 0; u < UPP; ++u) {
                const unit c = Ru[u];
                if constexpr (U == 2) {
                    t[(2 * u) / DR] += c.x * e[(2 * u) % DR];
                    t[(2 * u + 1) / DR] += c.y * e[(2 * u + 1) % DR];
                } else {
                    t[u / DR] += c * e[u % DR];
                }
            }
        });
    }
    // t = C^T e for the lane's point: the same staged block, read once in the same order, t[c] += R[r * DR + c] e[r]
    __device__ __forceinline__ void times_t(double* S, int lane, const double (&e)[DT], double (&t)[DR]) {
#pragma unroll
        for (int i = 0; i < DR; ++i) t[i] = 0.0;
        for_each(S, lane, [&](const double* R) {
            const unit* Ru = reinterpret_cast<const unit*>(R);
#pragma unroll
            for (int u = 0; u < UPP; ++u) {
                const unit c = Ru[u];
                if constexpr (U == 2) {
                    t[(2 * u) % DR] += c.x * e[(2 * u) / DR];
                    t[(2 * u + 1) % DR] += c.y * e[(2 * u + 1) / DR];
                } else {
                    t[u % DR] += c * e[u / DR];
                }
            }
        });
    }
};

// K v: gather v, the trial operand e = B_trial v per point, t = C e through the staged blocks, scatter B_test^T t (adjoint_scatter).
// The shape of tangent_apply's general form (register-pipelined gather, C requested before the contraction).
// TRANS: K^T v with the roles of the kinds swapped on the same blocks: e = B_test v, t = C^T e, scatter B_trial^T t.
template <int G, int BS, int TEST, int TRIAL, bool TRANS = false>
__global__ __launch_bounds__(DXO_BLOCK, DXO_BL_WAVES) void bilinear_apply(OperandDev m, const double* __restrict__ wq, int lds_wave,
                                                                         const double* __restrict__ C, const double* __restrict__ v,
                                                                         int64_t n_cells, double* __restrict__ out, double* __restrict__ fe) {
    constexpr int DT = OperandShape<G, BS, TEST>::D, DR = OperandShape<G, BS, TRIAL>::D;
    constexpr int KIN = TRANS ? TEST : TRIAL, KOUT = TRANS ? TRIAL : TEST;      // the kind of the operand of v, the kind scattered
    constexpr int DIN = TRANS ? DT : DR, DOUT = TRANS ? DR : DT;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* tab = lds;
    operand_load_tables<G>(m, tab);
    __syncthreads();
    const int lane = threadIdx.x & (DXO_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    double* W = lds + m.table_doubles + wave * lds_wave;
    const int cpw = m.cells_per_wave;
    double* Tm = W + cpw * (op_odd(m.ndofs * BS) + op_odd(m.ngeom * G));
    const int64_t n_groups = (n_cells + cpw - 1) / cpw;
    const GroupWalk walk = xcd_group_walk(n_groups, DXO_BLOCK / DXO_WAVE, wave);
    const int64_t stride = walk.stride;
    const bool piped = operand_can_pipe(m);
    OperandPipe<G, BS> pf;
    int64_t grp = walk.first;
    if (piped) {
        pipe_load_indices<G, BS>(m, pf, grp * cpw, group_cells(walk, n_cells, cpw, grp), lane);
        pipe_load_values<G, BS>(m, pf, v);
        pipe_load_indices<G, BS>(m, pf, (grp + stride) * cpw, group_cells(walk, n_cells, cpw, grp + stride), lane);
    }
    const int q_l = lane - (lane / m.nq) * m.nq;
    const double w_l = lane < cpw * m.nq ? wq[q_l] : 0.0;
    for (; grp < walk.end; grp += stride) {
        const int64_t c0 = grp * cpw;
        const int ncell = group_cells(walk, n_cells, cpw, grp);
        BlockRows<DT, DR> rows;
        rows.begin(C, c0 * m.nq, ncell * m.nq, lane);
        if (piped) {
            pipe_commit<G, BS>(m, pf, W, ncell, lane);
            pipe_load_values<G, BS>(m, pf, v);
            pipe_load_indices<G, BS>(m, pf, (grp + 2 * stride) * cpw, group_cells(walk, n_cells, cpw, grp + 2 * stride), lane);
        } else {
            operand_gather<G, BS>(m, W, v, nullptr, c0, ncell, lane);
        }
        double e[DIN], K[G][G], det = 0.0;
#pragma unroll
        for (int i = 0; i < G; ++i)
#pragma unroll
            for (int j = 0; j < G; ++j) K[i][j] = 0.0;
        const bool active = operand_compute_geo<G, BS, KIN>(m, tab, W, ncell, lane, e, K, det);
        if (!active) {
#pragma unroll
            for (int k = 0; k < DIN; ++k) e[k] = 0.0;
        }
        double t[DOUT];
        if constexpr (TRANS) rows.times_t(W, lane, e, t);
        else rows.times(W, lane, e, t);      // compute_geo has fenced: the gather buffer is free, the parked tensors are not written yet
        double vh[BS], gh[BS][G], scale = 0.0;
#pragma unroll
        for (int i = 0; i < BS; ++i) {
            vh[i] = 0.0;
#pragma unroll
            for (int j = 0; j < G; ++j) gh[i][j] = 0.0;
        }
        if (active) {
            scale = w_l * fabs(det);
            dual_tensor<G, BS, KOUT>(t, vh, gh);
        }
        adjoint_scatter<G, BS>(m, tab, Tm, active, lane, vh, gh, K, scale, c0, ncell, nullptr, out, fe);
    }
}

// diag(K): the unit dof (node a, component i) has the operand slots sum_z coef(r, i, z) z_phys with z_phys = (phi_a, grad phi_a), so its
// entry is z_phys^T M_i z_phys, M_i[z1][z2] = sum_rc coef_test(r, i, z1) C[r][c] coef_trial(c, i, z2). Phase 1, lane = (cell, point):
// M_i pulled back to reference derivatives (z_phys = P z_ref, P = diag(1, K^T)) and symmetrised, NZ (NZ + 1) / 2 numbers per component,
// parked in LDS; phase 2, lane = (cell, node): sum over the cell's points of z_ref^T NS_i z_ref. tangent_diag's scheme for any pair.
template <int G, int BS, int TEST, int TRIAL>
__global__ __launch_bounds__(DXO_BLOCK, DXO_BL_WAVES) void bilinear_diag(OperandDev m, const double* __restrict__ wq, int lds_wave,
                                                                        const double* __restrict__ C, int64_t n_cells,
                                                                        double* __restrict__ out, double* __restrict__ fe) {
    constexpr int DT = OperandShape<G, BS, TEST>::D, DR = OperandShape<G, BS, TRIAL>::D;
    constexpr int Z0 = (op_has_value<TEST>() || op_has_value<TRIAL>()) ? 0 : 1;    // z = 0 (the value) only where a kind has it
    constexpr int NZ = G + 1 - Z0;
    constexpr int NS1 = NZ * (NZ + 1) / 2;
    constexpr int PT = (BS * NS1) | 1;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* tab = lds;
    operand_load_tables<G>(m, tab);
    __syncthreads();
    const OperandLayout<G> L(m);
    const int lane = threadIdx.x & (DXO_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    double* W = lds + m.table_doubles + wave * lds_wave;
    const int cpw = m.cells_per_wave, nd = m.ndofs, nq = m.nq, ng = m.ngeom;
    const int sx = op_odd(ng * G);
    double* X = W;
    double* Pm = X + op_even(cpw * sx);             // staging of the C blocks, then the parked matrices [point][PT]
    const int64_t n_groups = (n_cells + cpw - 1) / cpw;
    const GroupWalk walk = xcd_group_walk(n_groups, DXO_BLOCK / DXO_WAVE, wave);
    const int c_l = lane / nq, q_l = lane - c_l * nq;
    const double w_l = lane < cpw * nq ? wq[q_l] : 0.0;
    for (int64_t grp = walk.first; grp < walk.end; grp += walk.stride) {
        const int64_t c0 = grp * cpw;
        const int ncell = (n_cells - c0 < cpw) ? (int)(n_cells - c0) : cpw;
        const bool has_point = c_l < ncell;
        BlockRows<DT, DR> rows;
        rows.begin(C, c0 * nq, ncell * nq, lane);
        gather_vertices<G>(m, X, nullptr, c0, ncell, lane);
        op_fence();
        double K[G][G], scale = 0.0;
#pragma unroll
        for (int j = 0; j < G; ++j)
#pragma unroll
            for (int k = 0; k < G; ++k) K[j][k] = 0.0;
        if (has_point) scale = w_l * fabs(point_jacobian<G>(tab + L.o_dpsi + q_l * L.sdpsi, X + c_l * sx, ng, K));
        double NSr[BS * NS1];
#pragma unroll
        for (int k = 0; k < BS * NS1; ++k) NSr[k] = 0.0;
        rows.for_each(Pm, lane, [&](const double* R) {      // the vertex buffer X lies before Pm: untouched by the staging
            if (!has_point) return;
#pragma unroll
            for (int i = 0; i < BS; ++i) {
                double M[NZ][NZ];
#pragma unroll
                for (int z1 = 0; z1 < NZ; ++z1)
#pragma unroll
                    for (int z2 = 0; z2 < NZ; ++z2) {
                        double acc = 0.0;
#pragma unroll
                        for (int r = 0; r < DT; ++r) {
                            const double a = op_coef<G, BS, TEST>(r, i, z1 + Z0);
                            if (a == 0.0) continue;
#pragma unroll
                            for (int c = 0; c < DR; ++c) {
                                const double b = op_coef<G, BS, TRIAL>(c, i, z2 + Z0);
                                if (b == 0.0) continue;
                                acc += (a * b) * R[r * DR + c];
                            }
                        }
                        M[z1][z2] = acc;
                    }
                // P^T M P: rows / columns 1 + j of the physical derivatives become sum_j K[k][j] (.)_(1+j)
                double KM[NZ][NZ], Mr[NZ][NZ];
#pragma unroll
                for (int a = 0; a < NZ; ++a)
#pragma unroll
                    for (int z2 = 0; z2 < NZ; ++z2) {
                        if (a + Z0 == 0) { KM[a][z2] = M[a][z2]; continue; }
                        const int k = a + Z0 - 1;
                        double s = 0.0;
#pragma unroll
                        for (int j = 0; j < G; ++j) s += K[k][j] * M[1 + j - Z0][z2];
                        KM[a][z2] = s;
                    }
#pragma unroll
                for (int a = 0; a < NZ; ++a)
#pragma unroll
                    for (int b = 0; b < NZ; ++b) {
                        if (b + Z0 == 0) { Mr[a][b] = KM[a][b]; continue; }
                        const int k = b + Z0 - 1;
                        double s = 0.0;
#pragma unroll
                        for (int j = 0; j < G; ++j) s += KM[a][1 + j - Z0] * K[k][j];
                        Mr[a][b] = s;
                    }
                int slot = 0;
#pragma unroll
                for (int a = 0; a < NZ; ++a)
#pragma unroll
                    for (int b = a; b < NZ; ++b) {
                        NSr[i * NS1 + slot] = scale * (a == b ? Mr[a][a] : Mr[a][b] + Mr[b][a]);
                        ++slot;
                    }
            }
        });
        if (has_point) {
#pragma unroll
            for (int k = 0; k < BS * NS1; ++k) Pm[lane * PT + k] = NSr[k];
        }
        op_fence();
        for (int idx = lane; idx < ncell * nd; idx += DXO_WAVE) {
            const int c = idx / nd, a = idx - c * nd;
            double acc[BS];
#pragma unroll
            for (int i = 0; i < BS; ++i) acc[i] = 0.0;
            for (int q = 0; q < nq; ++q) {
                const double* P = Pm + (c * nq + q) * PT;
                const double* dp = tab + L.o_dphi + q * L.sdphi + a * G;
                double z[NZ], pp[NS1];
                if constexpr (Z0 == 0) z[0] = tab[q * L.sphi + a];
#pragma unroll
                for (int k = 0; k < G; ++k) z[1 + k - Z0] = dp[k];
                sym_products<NZ>(z, pp);
#pragma unroll
                for (int i = 0; i < BS; ++i) acc[i] += sym_dot<NS1>(pp, P + i * NS1);
            }
            store_entry<BS>(m, fe, out, c0 + c, a, nd, acc);
        }
        op_fence();      // the parked matrices are overwritten by the next group's staged blocks
    }
}

// host side: LDS per wave and launch of one (G, BS, TEST, TRIAL), for the action, the diagonal or the transposed action
enum { BL_APPLY = 0, BL_DIAG = 1, BL_APPLY_T = 2 };
template <int G, int BS, int TEST, int TRIAL>
struct Bilinear {
    using Rows = BlockRows<OperandShape<G, BS, TEST>::D, OperandShape<G, BS, TRIAL>::D>;
    static int lds_wave(const dxo_mesh* mesh, int mode) {
        if (mode == BL_DIAG) {
            constexpr int NZ = G + 1 - ((op_has_value<TEST>() || op_has_value<TRIAL>()) ? 0 : 1);
            const int park = DXO_WAVE * ((BS * NZ * (NZ + 1) / 2) | 1);
            return op_even(vertex_doubles(mesh->dev, G) + (park > Rows::LDS_DOUBLES ? park : Rows::LDS_DOUBLES));
        }
        return wave_region(gather_doubles(mesh->dev, G, BS) + parked_doubles(G, BS), Rows::LDS_DOUBLES);
    }
    static void launch(const dxo_mesh* mesh, int mode, int wd, int blocks, size_t shm, const double* C, const double* v, double* out,
                       double* fe, hipStream_t s) {
        if (mode == BL_APPLY_T) hipLaunchKernelGGL((bilinear_apply<G, BS, TEST, TRIAL, true>), dim3(blocks), dim3(DXO_BLOCK), shm, s, mesh->dev, mesh->d_wq,
                                                   wd, C, v, mesh->num_cells, out, fe);
        else if (mode == BL_DIAG) hipLaunchKernelGGL((bilinear_diag<G, BS, TEST, TRIAL>), dim3(blocks), dim3(DXO_BLOCK), shm, s, mesh->dev, mesh->d_wq, wd, C,
                                     mesh->num_cells, out, fe);
        else hipLaunchKernelGGL((bilinear_apply<G, BS, TEST, TRIAL>), dim3(blocks), dim3(DXO_BLOCK), shm, s, mesh->dev, mesh->d_wq, wd, C, v,
                                mesh->num_cells, out, fe);
    }
};

struct BilinearOps {
    int (*lds_wave)(const dxo_mesh*, int) = nullptr;
    void (*launch)(const dxo_mesh*, int, int, int, size_t, const double*, const double*, double*, double*, hipStream_t) = nullptr;
};

int bilinear_impl(dxo_ctx* ctx, dxo_mesh* mesh, int test, int trial, int bs, const double* C, const double* v, double* out, int mode) {
    const bool diag = mode == BL_DIAG;
    const char* who = diag ? "dxo_bilinear_diagonal" : mode == BL_APPLY_T ? "dxo_bilinear_apply_t" : "dxo_bilinear_apply";
    if (!mesh) return fail_who(ctx, DXO_E_NULL, who, "mesh is NULL");
    BilinearOps ops;
    int rc = bilinear_pair_check(ctx, who, mesh, test, trial, bs, ops, [](auto G, auto BS, auto T, auto R) {
        return BilinearOps{&Bilinear<G, BS, T, R>::lds_wave, &Bilinear<G, BS, T, R>::launch};
    });
    if (rc != DXO_OK) return rc;
    if (mesh->num_cells == 0) return DXO_OK;
    if (!C || !out || (!diag && !v)) return fail_who(ctx, DXO_E_NULL, who, "NULL array");
    if (((uintptr_t)C & 15u) != 0) return fail_who(ctx, DXO_E_ALIGN, who, "C must be 16-byte aligned");
    const int wd = ops.lds_wave(mesh, mode);
    const size_t shm = (size_t)(mesh->dev.table_doubles + (DXO_BLOCK / DXO_WAVE) * wd) * sizeof(double);
    if (shm > 64 * 1024) return fail_who(ctx, DXO_E_SIZE, who, "element too large for the LDS budget");
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    double* fe = two_pass_buffer(ctx, mesh, bs, nullptr, mesh->num_cells);
    rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    rc = clear_for_atomics(ctx, mesh, bs, out, fe, s);
    if (rc != DXO_OK) return rc;
    ops.launch(mesh, mode, wd, wave_group_grid(ctx, wave_groups(mesh->dev, mesh->num_cells), DXO_BL_BLOCKS_PER_CU), shm, C, v, out, fe, s);
    if (fe) launch_node_sum(ctx, mesh, bs, out, s);
    return dxo_device_end(ctx, s);
}

}  // namespace

extern "C" int dxo_bilinear_apply(dxo_ctx* ctx, dxo_mesh* mesh, int test_kind, int trial_kind, int bs, const double* C, const double* v,
                                  double* out) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    return bilinear_impl(ctx, mesh, test_kind, trial_kind, bs, C, v, out, BL_APPLY);
}

extern "C" int dxo_bilinear_apply_t(dxo_ctx* ctx, dxo_mesh* mesh, int test_kind, int trial_kind, int bs, const double* C, const double* v,
                                    double* out) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    return bilinear_impl(ctx, mesh, test_kind, trial_kind, bs, C, v, out, BL_APPLY_T);
}

extern "C" int dxo_bilinear_diagonal(dxo_ctx* ctx, dxo_mesh* mesh, int test_kind, int trial_kind, int bs, const double* C, double* out) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    return bilinear_impl(ctx, mesh, test_kind, trial_kind, bs, C, nullptr, out, BL_DIAG);
}
