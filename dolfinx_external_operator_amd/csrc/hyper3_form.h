// hyper3_form.h — the 3-D hyperelastic residual, tangent action and tangent diagonal of the analytic Isihara model as functions of the
// dof vector u alone (dxo_isihara3_residual / _tangent_apply / _tangent_diagonal): what dxo_isihara3_field followed by
// dxo_operand_adjoint("F") / dxo_bilinear_apply / dxo_bilinear_diagonal ("grad", "grad", 3) compute, WITHOUT the quadrature arrays
// dP[n][9][9] and P[n][9] (720 B per point written per Newton iteration, 648 of them read again by every Krylov matvec). The model has
// no history, so F = I + grad u is formed again in registers by every call (operand_compute_geo), the stress is isihara3_stress, and the
// tangent's action on grad v is isihara3_tangent_times (hyper3_core.h): about 150 flops from the point's 27 doubles and 7 coefficients,
// the 45-entry Hessian never formed. Included at the end of adjoint.hip beside bilinear.h: the gather pipeline, adjoint_scatter,
// store_entry and the two-pass scatter (fe + node_sum) are that file's, and the calls have its consumer semantics (out +=, SET with
// option consumer_overwrite, no atomics, bit-reproducible, capture-safe).
//   residual   gather u -> F, K, det -> P -> scatter B^T P
//   action     gather u -> F, K, det;  gather v INTO THE SAME BUFFER -> grad v with the K already there;  q(F) -> t = H : grad v -> scatter
//              (a 6-component gather of (u, v) does not fit beside the tables of Q2 hexahedra: 4 waves x 8 cells x 27 nodes x 6 doubles)
//   diagonal   gather u into the slice that later parks the matrices -> F -> the three 3x3 diagonal blocks H_(i.)(i.) of the Hessian,
//              pulled back and symmetrised in registers (bilinear_diag's NS_i) -> bilinear_diag's phase 2
// LDS per wave: residual and action take the gather buffer and the parked tensors, what bilinear_apply takes without its staging
// region (dxo_operand_adjoint's request includes the staging region of the tangent rows: Q2 hexahedra under the 27-point rule are
// served here and not there); the diagonal takes the vertex buffer and max(parked matrices of the group's cells_per_wave * nq points,
// gathered u): at most bilinear_diag's request wherever the gathered u of a wave group is at most 64 x 19 doubles (every element
// with ndofs <= 6 nq), and never more than the action's.
#pragma once

#include "hyper3_core.h"

#ifndef DXO_H3F_WAVES
#define DXO_H3F_WAVES 2      // waves per SIMD the three kernels are compiled for (no scratch: profiles/hyper3_mf_resources.txt)
#endif
#ifndef DXO_H3F_BLOCKS_PER_CU
#define DXO_H3F_BLOCKS_PER_CU 8
#endif

namespace {

// the dof values of the NEXT wave group in flight beside OperandPipe's: the second field of the action shares the pipe's node indices
struct H3fValues {
    double d[OP_GI][3];
};

__device__ __forceinline__ void h3f_load_values(const OperandPipe<3, 3>& pf, H3fValues& pv, const double* __restrict__ v) {
#pragma unroll
    for (int it = 0; it < OP_GI; ++it)
        if (pf.un[it] >= 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) pv.d[it][i] = v[(int64_t)pf.un[it] * 3 + i];
        }
}

// -> U[ncell] x op_odd(nd * 3), the dof part of the gather buffer (the vertices behind it stay)
__device__ __forceinline__ void h3f_commit_values(const OperandDev& m, const H3fValues& pv, double* U, int ncell, int lane) {
    const int nd = m.ndofs, su = op_odd(nd * 3);
#pragma unroll
    for (int it = 0; it < OP_GI; ++it) {
        const int idx = it * DXO_WAVE + lane;
        if (idx < ncell * nd) {
            const int c = idx / nd, a = idx - c * nd;
#pragma unroll
            for (int i = 0; i < 3; ++i) U[c * su + a * 3 + i] = pv.d[it][i];
        }
    }
}

// the same without the pipeline
__device__ __forceinline__ void h3f_gather_values(const OperandDev& m, double* U, const double* __restrict__ v, int64_t c0, int ncell, int lane) {
    const int nd = m.ndofs, su = op_odd(nd * 3);
    for (int idx = lane; idx < ncell * nd; idx += DXO_WAVE) {
        const int c = idx / nd, a = idx - c * nd;
        const int64_t node = m.dofmap[(c0 + c) * nd + a];
#pragma unroll
        for (int i = 0; i < 3; ++i) U[c * su + a * 3 + i] = v[node * 3 + i];
    }
}

// g = grad of the field gathered in U at the lane's point, with the K = J^-1 the lane already holds: g[3 i + j] = d field_i / d x_j.
// The caller fences before (U written) and after (U reused).
__device__ __forceinline__ void h3f_grad(const OperandDev& m, const double* tab, const double* U, int lane, const double (&K)[3][3],
                                         double (&g)[9]) {
    const OperandLayout<3> L(m);
    const int nd = m.ndofs, su = op_odd(nd * 3);
    const int c = lane / m.nq, q = lane - c * m.nq;
    const double* dphi = tab + L.o_dphi + q * L.sdphi;
    const double* Uc = U + c * su;
    double gref[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) gref[i][k] = 0.0;
#pragma unroll DXO_OP_UNROLL
    for (int a = 0; a < nd; ++a) {
        double ua[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) ua[i] = Uc[a * 3 + i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double dk = dphi[a * 3 + k];
#pragma unroll
            for (int i = 0; i < 3; ++i) gref[i][k] += ua[i] * dk;
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) g[3 * i + j] = gref[i][0] * K[0][j] + gref[i][1] * K[1][j] + gref[i][2] * K[2][j];
}

// R (+)= sum_q w |det J| B^T P(I + grad u), and with ACTION out (+)= sum_q w |det J| B^T (dP/dF(I + grad u) : grad v).
// bilinear_apply's shape: lane = (cell, point), a wave owns cells_per_wave cells, the gather of u register-pipelined two groups deep
// where the element allows it, the values of v one group deep on the same node indices.
template <bool ACTION>
__global__ __launch_bounds__(DXO_BLOCK, DXO_H3F_WAVES) void isihara3_form(IsiPrm prm, OperandDev m, const double* __restrict__ wq, int lds_wave,
                                                                         const double* __restrict__ u, const double* __restrict__ v,
                                                                         int64_t n_cells, double* __restrict__ out, double* __restrict__ fe) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* tab = lds;
    operand_load_tables<3>(m, tab);
    __syncthreads();
    const int lane = threadIdx.x & (DXO_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    double* W = lds + m.table_doubles + wave * lds_wave;
    const int cpw = m.cells_per_wave;
    double* Tm = W + cpw * (op_odd(m.ndofs * 3) + op_odd(m.ngeom * 3));
    const int64_t n_groups = (n_cells + cpw - 1) / cpw;
    const GroupWalk walk = xcd_group_walk(n_groups, DXO_BLOCK / DXO_WAVE, wave);
    const int64_t stride = walk.stride;
    const bool piped = operand_can_pipe(m);
    OperandPipe<3, 3> pf;
    [[maybe_unused]] OperandPipe<3, 3> nx;      // ACTION: the node indices of the group after next wait here (its value slots are unused)
    [[maybe_unused]] H3fValues pv;
    int64_t grp = walk.first;
    if (piped) {
        pipe_load_indices<3, 3>(m, pf, grp * cpw, group_cells(walk, n_cells, cpw, grp), lane);
        pipe_load_values<3, 3>(m, pf, u);
        if constexpr (ACTION) {
            h3f_load_values(pf, pv, v);
            pipe_load_indices<3, 3>(m, nx, (grp + stride) * cpw, group_cells(walk, n_cells, cpw, grp + stride), lane);
        } else {
            pipe_load_indices<3, 3>(m, pf, (grp + stride) * cpw, group_cells(walk, n_cells, cpw, grp + stride), lane);
        }
    }
    const int q_l = lane - (lane / m.nq) * m.nq;
    const double w_l = lane < cpw * m.nq ? wq[q_l] : 0.0;
    for (; grp < walk.end; grp += stride) {
        const int64_t c0 = grp * cpw;
        const int ncell = group_cells(walk, n_cells, cpw, grp);
        if (piped) {
            pipe_commit<3, 3>(m, pf, W, ncell, lane);
            if constexpr (!ACTION) {
                pipe_load_values<3, 3>(m, pf, u);
                pipe_load_indices<3, 3>(m, pf, (grp + 2 * stride) * cpw, group_cells(walk, n_cells, cpw, grp + 2 * stride), lane);
            }
        } else {
            operand_gather<3, 3>(m, W, u, nullptr, c0, ncell, lane);
        }
        double F[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, K[3][3], det = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) K[i][j] = 0.0;
        const bool active = operand_compute_geo<3, 3, DXO_OPERAND_DEFGRAD>(m, tab, W, ncell, lane, F, K, det);   // ends fenced: W is free
        double t[9];
        Isi3Point q;
        isihara3_stress(prm, F, q, t);      // lanes without a point evaluate the identity
        if constexpr (ACTION) {
            // the second field into the dof part of the same buffer; then both fields of the next group are requested on its node
            // indices, and the indices of the group after that
            if (piped) {
                h3f_commit_values(m, pv, W, ncell, lane);
#pragma unroll
                for (int it = 0; it < OP_GI; ++it) pf.un[it] = nx.un[it];
#pragma unroll
                for (int it = 0; it < OP_XI; ++it) pf.xn[it] = nx.xn[it];
                pipe_load_values<3, 3>(m, pf, u);
                h3f_load_values(pf, pv, v);
                pipe_load_indices<3, 3>(m, nx, (grp + 2 * stride) * cpw, group_cells(walk, n_cells, cpw, grp + 2 * stride), lane);
            } else {
                h3f_gather_values(m, W, v, c0, ncell, lane);
            }
            op_fence();
            double dF[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) dF[k] = 0.0;
            if (active) h3f_grad(m, tab, W, lane, K, dF);
            op_fence();
            isihara3_tangent_times(q, dF, t);
        }
        double vh[3], gh[3][3], scale = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            vh[i] = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) gh[i][j] = 0.0;
        }
        if (active) {
            scale = w_l * fabs(det);
            dual_tensor<3, 3, DXO_OPERAND_DEFGRAD>(t, vh, gh);
        }
        adjoint_scatter<3, 3>(m, tab, Tm, active, lane, vh, gh, K, scale, c0, ncell, nullptr, out, fe);
    }
}

// diag(K(u)): the unit dof (node a, component i) has grad = e_i (x) grad phi_a, so its entry is grad phi_a^T M_i grad phi_a with
// M_i = H_(i.)(i.), the i-th 3x3 diagonal block of the Hessian: 18 of its 45 entries. Phase 1, lane = (cell, point): K M_i K^T,
// symmetrised, six numbers per component, parked in LDS; phase 2, lane = (cell, node): bilinear_diag's sum over the cell's points.
__global__ __launch_bounds__(DXO_BLOCK, DXO_H3F_WAVES) void isihara3_form_diag(IsiPrm prm, OperandDev m, const double* __restrict__ wq, int lds_wave,
                                                                              const double* __restrict__ u, int64_t n_cells,
                                                                              double* __restrict__ out, double* __restrict__ fe) {
    constexpr int NS1 = 6, PT = (3 * NS1) | 1;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* tab = lds;
    operand_load_tables<3>(m, tab);
    __syncthreads();
    const OperandLayout<3> L(m);
    const int lane = threadIdx.x & (DXO_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    double* W = lds + m.table_doubles + wave * lds_wave;
    const int cpw = m.cells_per_wave, nd = m.ndofs, nq = m.nq, ng = m.ngeom;
    const int sx = op_odd(ng * 3);
    double* X = W;
    double* Pm = X + op_even(cpw * sx);             // the gathered u, then the parked matrices [point][PT]
    const int64_t n_groups = (n_cells + cpw - 1) / cpw;
    const GroupWalk walk = xcd_group_walk(n_groups, DXO_BLOCK / DXO_WAVE, wave);
    const int c_l = lane / nq, q_l = lane - c_l * nq;
    const double w_l = lane < cpw * nq ? wq[q_l] : 0.0;
    for (int64_t grp = walk.first; grp < walk.end; grp += walk.stride) {
        const int64_t c0 = grp * cpw;
        const int ncell = (n_cells - c0 < cpw) ? (int)(n_cells - c0) : cpw;
        const bool has_point = c_l < ncell;
        gather_vertices<3>(m, X, nullptr, c0, ncell, lane);
        h3f_gather_values(m, Pm, u, c0, ncell, lane);
        op_fence();
        double K[3][3], scale = 0.0, F[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) K[j][k] = 0.0;
        if (has_point) {
            scale = w_l * fabs(point_jacobian<3>(tab + L.o_dpsi + q_l * L.sdpsi, X + c_l * sx, ng, K));
            double g[9];
            h3f_grad(m, tab, Pm, lane, K, g);
#pragma unroll
            for (int k = 0; k < 9; ++k) F[k] += g[k];
        }
        op_fence();      // every lane has read the gathered u: the slice takes the matrices
        Isi3Point q;
        double H[HYPER3_SYM];
        {
            double P[9];
            isihara3_stress(prm, F, q, P);
        }
        isihara3_tangent(q, H);
        if (has_point) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                double KM[3][3];      // K M_i, M_i[j][l] = H[(3 i + j, 3 i + l)]
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int l = 0; l < 3; ++l) {
                        double s = 0.0;
#pragma unroll
                        for (int j = 0; j < 3; ++j) s += K[a][j] * H[j <= l ? hyper3_tri(3 * i + j, 3 * i + l) : hyper3_tri(3 * i + l, 3 * i + j)];
                        KM[a][l] = s;
                    }
                int slot = 0;
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = a; b < 3; ++b) {
                        const double mr = KM[a][0] * K[b][0] + KM[a][1] * K[b][1] + KM[a][2] * K[b][2];
                        Pm[lane * PT + i * NS1 + slot] = scale * (a == b ? mr : 2.0 * mr);      // M_i is symmetric: (K M K^T)_ab = (K M K^T)_ba
                        ++slot;
                    }
            }
        }
        op_fence();
        for (int idx = lane; idx < ncell * nd; idx += DXO_WAVE) {
            const int c = idx / nd, a = idx - c * nd;
            double acc[3] = {0.0, 0.0, 0.0};
            for (int q2 = 0; q2 < nq; ++q2) {
                const double* P = Pm + (c * nq + q2) * PT;
                const double* dp = tab + L.o_dphi + q2 * L.sdphi + a * 3;
                double z[3], pp[NS1];
#pragma unroll
                for (int k = 0; k < 3; ++k) z[k] = dp[k];
                sym_products<3>(z, pp);
#pragma unroll
                for (int i = 0; i < 3; ++i) acc[i] += sym_dot<NS1>(pp, P + i * NS1);
            }
            store_entry<3>(m, fe, out, c0 + c, a, nd, acc);
        }
        op_fence();      // the parked matrices are overwritten by the next group's gather
    }
}

enum { H3F_RESIDUAL = 0, H3F_APPLY = 1, H3F_DIAG = 2 };

// doubles of a wave's LDS region
int h3f_lds_wave(const dxo_mesh* mesh, int mode) {
    const OperandDev& d = mesh->dev;
    if (mode == H3F_DIAG) {
        // the matrices of the group's own points: cells_per_wave * nq <= 64 of them (54 under the 27-point rule, whose tables leave no more)
        const int park = d.cells_per_wave * d.nq * ((3 * 6) | 1), gath = d.cells_per_wave * op_odd(d.ndofs * 3);
        return op_even(vertex_doubles(d, 3) + (park > gath ? park : gath));
    }
    return wave_region(gather_doubles(d, 3, 3) + parked_doubles(3, 3), 0);
}

// shared body of the three entry points: the argument checks, stream, lock and begin / end protocol of bilinear_impl
int isihara3_form_impl(dxo_ctx* ctx, const dxo_isihara_params* prm, dxo_mesh* mesh, const double* u, const double* v, double* out, int mode) {
    const char* who = mode == H3F_DIAG ? "dxo_isihara3_tangent_diagonal" : mode == H3F_APPLY ? "dxo_isihara3_tangent_apply" : "dxo_isihara3_residual";
    if (!prm) return fail_who(ctx, DXO_E_NULL, who, "params is NULL");
    if (!mesh) return fail_who(ctx, DXO_E_NULL, who, "mesh is NULL");
    if (mesh->gdim != 3) return fail_who(ctx, DXO_E_DIM, who, "F is 3x3, the mesh must have gdim = 3");
    if (!mesh->d_wq) return fail_who(ctx, DXO_E_OPTION, who, "quadrature weights not set (dxo_mesh_set_weights)");
    if (mesh->num_cells == 0) return DXO_OK;
    if (!u || !out || (mode == H3F_APPLY && !v)) return fail_who(ctx, DXO_E_NULL, who, "NULL array");
    if (((uintptr_t)u | (uintptr_t)v | (uintptr_t)out) & 7u) return fail_who(ctx, DXO_E_ALIGN, who, "arrays must be 8-byte aligned");
    const int wd = h3f_lds_wave(mesh, mode);
    const size_t shm = (size_t)(mesh->dev.table_doubles + (DXO_BLOCK / DXO_WAVE) * wd) * sizeof(double);
    if (shm > 64 * 1024) return fail_who(ctx, DXO_E_SIZE, who, "element too large for the LDS budget");
    const IsiPrm k{prm->c1, prm->c2, prm->c3, prm->c4};
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    double* fe = two_pass_buffer(ctx, mesh, 3, nullptr, mesh->num_cells);
    int rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    rc = clear_for_atomics(ctx, mesh, 3, out, fe, s);
    if (rc != DXO_OK) return rc;
    const int blocks = wave_group_grid(ctx, wave_groups(mesh->dev, mesh->num_cells), DXO_H3F_BLOCKS_PER_CU);
    if (mode == H3F_DIAG)
        hipLaunchKernelGGL(isihara3_form_diag, dim3(blocks), dim3(DXO_BLOCK), shm, s, k, mesh->dev, mesh->d_wq, wd, u, mesh->num_cells, out, fe);
    else if (mode == H3F_APPLY)
        hipLaunchKernelGGL(isihara3_form<true>, dim3(blocks), dim3(DXO_BLOCK), shm, s, k, mesh->dev, mesh->d_wq, wd, u, v, mesh->num_cells, out, fe);
    else
        hipLaunchKernelGGL(isihara3_form<false>, dim3(blocks), dim3(DXO_BLOCK), shm, s, k, mesh->dev, mesh->d_wq, wd, u, v, mesh->num_cells, out, fe);
    if (fe) launch_node_sum(ctx, mesh, 3, out, s);
    return dxo_device_end(ctx, s);
}

}  // namespace

extern "C" int dxo_isihara3_residual(dxo_ctx* ctx, const dxo_isihara_params* prm, dxo_mesh* mesh, const double* u, double* R) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    return isihara3_form_impl(ctx, prm, mesh, u, nullptr, R, H3F_RESIDUAL);
}

extern "C" int dxo_isihara3_tangent_apply(dxo_ctx* ctx, const dxo_isihara_params* prm, dxo_mesh* mesh, const double* u, const double* v,
                                          double* out) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    return isihara3_form_impl(ctx, prm, mesh, u, v, out, H3F_APPLY);
}

extern "C" int dxo_isihara3_tangent_diagonal(dxo_ctx* ctx, const dxo_isihara_params* prm, dxo_mesh* mesh, const double* u, double* out) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    return isihara3_form_impl(ctx, prm, mesh, u, nullptr, out, H3F_DIAG);
}
