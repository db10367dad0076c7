// facet_form.hip — boundary-facet integrals (ds): facet normals, the facet measure, and the load vectors of a residual's
// boundary term. The demo's residual inner(sigma, eps(v)) dx - inner(loading * -n, v) ds(inner) (demo_plasticity_von_mises.py:249-253)
// is dxo_operand_adjoint(EPS_MANDEL) + dxo_facet_pressure(scale = loading).
//
// Geometry at a facet point of the entity (cell, f): J = sum_v X_v dpsi_f,v (the facet dpsi table, exactly as operand_facet.hip
// rebuilds it), J_f = J J_ref_f, dS = w_q sqrt(det(J_f^T J_f)), n = J^-T n_ref / |J^-T n_ref|. J^-T maps a covector, so n is outward
// for either sign of det J (J v points out of the cell when v points out of the reference cell, and n . J v = n_ref . v / |.|).
//
// Boundary work is O(N^((d-1)/d)): this is not a bandwidth kernel. Every call that ends in a dof vector is two launches:
//   facet_element<.., MODE>: a workgroup takes floor(256 / nq) entities. Phase 1, lane = (entity, point): geometry and what the mode parks
//                   in LDS (FE_LOAD: vh[BS], T[BS][G] = dS * the dual tensor pulled back to reference gradients; FE_PRESSURE: dS p n;
//                   FE_APPLY and FE_DIAG: see the bilinear forms below).
//                   Phase 2, lane = (entity, local dof): the fixed-order sum over the entity's points into fe[entity][a][i].
//   facet_node_sum: lane = touched node, adds the node's entries of fe in ascending entity order (the set's transposed incidence).
// No atomics: the result is bit-reproducible. The calls always accumulate into out.
// The Jacobian of a state-dependent boundary term (dxo_facet_bilinear_apply / _diagonal / _assemble) is at the end of the file.
#include "csr.h"
#include "dxo_common.h"
#include "facet_tabs.h"
#include "operand_coef.h"

#include <algorithm>

namespace {

template <int G>
__global__ __launch_bounds__(DXO_BLOCK) void facet_geometry(OperandDev m, FacetTabs<G> t, const int32_t* __restrict__ ents, int64_t n,
                                                            double* __restrict__ normals, double* __restrict__ dS) {
    const int64_t total = n * t.nqf, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t e = i / t.nqf;
        const int q = (int)(i - e * t.nqf);
        double K[G][G], nrm[G], ds;
        facet_point_geometry<G>(m, t, ents[2 * e], ents[2 * e + 1], q, K, nrm, ds);
        if (normals) {
#pragma unroll
            for (int j = 0; j < G; ++j) normals[i * G + j] = nrm[j];
        }
        if (dS) dS[i] = ds;
    }
}

// what facet_element forms: the load of a linear operand kind (A = S [n][nq][D]), the pressure load (A = p [n][nq] or NULL), K v or diag K
// of a bilinear form (A = C [n][nq][BS][D])
enum FacetMode { FE_LOAD, FE_PRESSURE, FE_APPLY, FE_DIAG };

// slots per (i, j) of a bilinear form's dual data: the value slot where the kind has one, G reference-gradient slots where it has a gradient
template <int G, int KIND>
constexpr int facet_nz() { return (op_has_value<KIND>() ? 1 : 0) + (op_has_grad<KIND>() ? G : 0); }

// doubles a point parks: a load (vh[BS], T[BS][G]) or vh alone, the diagonal its BS slot groups, the pressure and apply BS values
template <int G, int BS, int KIND, FacetMode MODE>
constexpr int facet_parked() { return MODE == FE_DIAG ? BS * facet_nz<G, KIND>() : (MODE == FE_LOAD && op_has_grad<KIND>()) ? BS * (1 + G) : BS; }

// the dual data of an operand value s[D] at a point: vh = dS * value part, T = dS * gradient part pulled back to reference gradients
template <int G, int BS, int KIND>
__device__ __forceinline__ void facet_dual(const double* __restrict__ sp, const double (&K)[G][G], double ds, double (&vh)[BS],
                                           double (&T)[BS][G]) {
    constexpr int D = OperandShape<G, BS, KIND>::D;
    double s[D], gh[BS][G];
#pragma unroll
    for (int k = 0; k < D; ++k) s[k] = sp[k];
    dual_tensor<G, BS, KIND>(s, vh, gh);
#pragma unroll
    for (int i = 0; i < BS; ++i) vh[i] *= ds;
    pull_back<G, BS>(gh, K, ds, T);
}

// the slot vector (phi, dphi[:]) of a dof, row = (f * nqf + q) * nd + dof of the facet tables
template <int G, int KIND>
__device__ __forceinline__ void facet_dof_slots(const FacetTabs<G>& t, size_t row, double (&z)[facet_nz<G, KIND>()]) {
    int n = 0;
    if constexpr (op_has_value<KIND>()) z[n++] = t.phi[row];
    if constexpr (op_has_grad<KIND>()) {
#pragma unroll
        for (int k = 0; k < G; ++k) z[n + k] = t.dphi[row * G + k];
    }
}

// element vectors of the entities into fe[e][a][i], summed over the entity's facet points in a fixed order:
//   FE_LOAD      sum_q (vh_q[i] phi_a + sum_k T_q[i][k] dphi_a,k), (vh, T) the dual data of S_q
//   FE_PRESSURE  sum_q scale dS p_q n_i phi_a
//   FE_APPLY     sum_q dS (C_q w_q)[i] phi_a, w_q the trial operand of v at the point
//   FE_DIAG      sum_q phi_a (vh_i[i] phi_a + sum_k T_i[i][k] dphi_a,k), (vh_i, T_i) the dual data of row i of C_q
template <int G, int BS, int KIND, FacetMode MODE>
__global__ __launch_bounds__(DXO_BLOCK) void facet_element(OperandDev m, FacetTabs<G> t, const int32_t* __restrict__ ents, int64_t n,
                                                           const double* __restrict__ A, const double* __restrict__ v, double scale,
                                                           double* __restrict__ fe) {
    constexpr int NZ = facet_nz<G, KIND>(), PW = facet_parked<G, BS, KIND, MODE>();
    constexpr bool GRAD_SUM = PW == BS * (1 + G);        // a load with a gradient part
    extern __shared__ double lds[];
    const int nqf = t.nqf, nd = t.nd;
    const int epb = DXO_BLOCK / nqf;                      // entities per workgroup and round
    for (int64_t e0 = (int64_t)blockIdx.x * epb; e0 < n; e0 += (int64_t)gridDim.x * epb) {
        const int ne = (int)(n - e0 < epb ? n - e0 : epb);
        if ((int)threadIdx.x < ne * nqf) {
            const int le = threadIdx.x / nqf, q = threadIdx.x - le * nqf;
            const int64_t e = e0 + le;
            const int64_t cell = ents[2 * e];
            const int f = ents[2 * e + 1];
            double K[G][G], nrm[G], ds;
            facet_point_geometry<G>(m, t, cell, f, q, K, nrm, ds);
            double* P = lds + threadIdx.x * PW;
            if constexpr (MODE == FE_PRESSURE) {
                const double pv = scale * ds * (A ? A[e * nqf + q] : 1.0);
#pragma unroll
                for (int i = 0; i < G; ++i) P[i] = pv * nrm[i];
            } else {
                constexpr int D = OperandShape<G, BS, KIND>::D;
                const double* Ap = A + (e * nqf + q) * (int64_t)((MODE == FE_LOAD ? 1 : BS) * D);
                if constexpr (MODE == FE_LOAD) {
                    double s[D], vh[BS], gh[BS][G];
#pragma unroll
                    for (int k = 0; k < D; ++k) s[k] = Ap[k];
                    dual_tensor<G, BS, KIND>(s, vh, gh);
#pragma unroll
                    for (int i = 0; i < BS; ++i) P[i] = ds * vh[i];
                    if constexpr (GRAD_SUM) {
                        double T[BS][G];
                        pull_back<G, BS>(gh, K, ds, T);
#pragma unroll
                        for (int i = 0; i < BS; ++i)
#pragma unroll
                            for (int k = 0; k < G; ++k) P[BS + i * G + k] = T[i][k];
                    }
                } else if constexpr (MODE == FE_DIAG) {
#pragma unroll
                    for (int i = 0; i < BS; ++i) {
                        double vh[BS], T[BS][G];
                        facet_dual<G, BS, KIND>(Ap + i * D, K, ds, vh, T);
                        int z = 0;
                        if constexpr (op_has_value<KIND>()) P[i * NZ + z++] = vh[i];
                        if constexpr (op_has_grad<KIND>()) {
#pragma unroll
                            for (int k = 0; k < G; ++k) P[i * NZ + z + k] = T[i][k];
                        }
                    }
                } else {
                    // the trial operand of v at the point, as operand_eval_facets forms it
                    const size_t row = ((size_t)f * nqf + q) * nd;
                    double val[BS], gref[BS][G];
#pragma unroll
                    for (int i = 0; i < BS; ++i) {
                        val[i] = 0.0;
#pragma unroll
                        for (int k = 0; k < G; ++k) gref[i][k] = 0.0;
                    }
                    for (int a = 0; a < nd; ++a) {
                        const int64_t node = m.dofmap[cell * nd + a];
                        double va[BS];
#pragma unroll
                        for (int i = 0; i < BS; ++i) va[i] = v[node * BS + i];
                        if constexpr (op_has_value<KIND>()) {
                            const double ph = t.phi[row + a];
#pragma unroll
                            for (int i = 0; i < BS; ++i) val[i] += va[i] * ph;
                        }
                        if constexpr (op_has_grad<KIND>()) {
#pragma unroll
                            for (int k = 0; k < G; ++k) {
                                const double dk = t.dphi[(row + a) * G + k];
#pragma unroll
                                for (int i = 0; i < BS; ++i) gref[i][k] += va[i] * dk;
                            }
                        }
                    }
                    double g[BS][G];
#pragma unroll
                    for (int i = 0; i < BS; ++i)
#pragma unroll
                        for (int j = 0; j < G; ++j) {
                            double s = 0.0;
#pragma unroll
                            for (int k = 0; k < G; ++k) s += gref[i][k] * K[k][j];
                            g[i][j] = s;
                        }
                    double o[D];
                    shape_operand<G, BS, KIND>(val, g, o);
#pragma unroll
                    for (int i = 0; i < BS; ++i) {
                        double w = 0.0;
#pragma unroll
                        for (int r = 0; r < D; ++r) w += Ap[i * D + r] * o[r];
                        P[i] = ds * w;
                    }
                }
            }
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < ne * nd; idx += blockDim.x) {
            const int le = idx / nd, a = idx - le * nd;
            const int64_t e = e0 + le;
            const int f = ents[2 * e + 1];
            double acc[BS];
#pragma unroll
            for (int i = 0; i < BS; ++i) acc[i] = 0.0;
            for (int q = 0; q < nqf; ++q) {
                const double* P = lds + (le * nqf + q) * PW;
                const size_t row = ((size_t)f * nqf + q) * nd + a;
                const double ph = t.phi[row];
                if constexpr (MODE == FE_DIAG) {
                    double za[NZ];
                    facet_dof_slots<G, KIND>(t, row, za);
#pragma unroll
                    for (int i = 0; i < BS; ++i) {
                        double s = 0.0;
#pragma unroll
                        for (int z = 0; z < NZ; ++z) s += P[i * NZ + z] * za[z];
                        acc[i] += ph * s;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < BS; ++i) acc[i] += P[i] * ph;
                    if constexpr (GRAD_SUM) {
#pragma unroll
                        for (int k = 0; k < G; ++k) {
                            const double dk = t.dphi[row * G + k];
#pragma unroll
                            for (int i = 0; i < BS; ++i) acc[i] += P[BS + i * G + k] * dk;
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < BS; ++i) fe[(e * nd + a) * BS + i] = acc[i];
        }
        __syncthreads();     // the next round overwrites the parked points
    }
}

// out[node] += the node's element-vector entries, added in ascending entity order
template <int BS>
__global__ __launch_bounds__(DXO_BLOCK) void facet_node_sum(int64_t n_touched, const int32_t* __restrict__ tnode,
                                                            const int64_t* __restrict__ tptr, const uint32_t* __restrict__ tent,
                                                            const double* __restrict__ fe, double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_touched; t += stride) {
        double acc[BS];
#pragma unroll
        for (int i = 0; i < BS; ++i) acc[i] = 0.0;
        for (int64_t j = tptr[t]; j < tptr[t + 1]; ++j) {
            const double* src = fe + (int64_t)tent[j] * BS;
#pragma unroll
            for (int i = 0; i < BS; ++i) acc[i] += src[i];
        }
        const int64_t node = tnode[t];
#pragma unroll
        for (int i = 0; i < BS; ++i) out[node * BS + i] += acc[i];
    }
}

// the launch of facet_element into the set's fe: epb entities per workgroup and round, their parked points in dynamic LDS
template <int G, int BS, int KIND, FacetMode MODE>
void launch_element(const dxo_ctx* ctx, const dxo_mesh* m, const dxo_facet_set* set, const double* A, const double* v, double scale, hipStream_t s) {
    const FacetTabs<G> t = facet_tabs<G>(m);
    const int epb = DXO_BLOCK / t.nqf;
    const size_t shm = (size_t)epb * t.nqf * facet_parked<G, BS, KIND, MODE>() * sizeof(double);
    hipLaunchKernelGGL((facet_element<G, BS, KIND, MODE>), dim3(capped_grid(ctx, set->n, epb, 8)), dim3(DXO_BLOCK), shm, s, m->dev, t, set->d_ents,
                       set->n, A, v, scale, set->d_fe);
}

void launch_node_sum(const dxo_ctx* ctx, const dxo_facet_set* set, int bs, double* out, hipStream_t s) {
    with_node_bs(bs, [&](auto BS) {
        hipLaunchKernelGGL(facet_node_sum<BS>, dim3(capped_grid(ctx, set->n_touched, DXO_BLOCK, 8)), dim3(DXO_BLOCK), 0, s, set->n_touched,
                           set->d_tnode, set->d_tptr, set->d_tent, set->d_fe, out);
    });
}

void set_free(dxo_facet_set* set) {
    free_all({set->d_ents, set->d_fe, set->d_tnode, set->d_tptr, set->d_tent, set->d_ae, set->d_fn_part});
    delete set;
}

int set_build(dxo_ctx* ctx, dxo_facet_set* set, const dxo_mesh* m, const int32_t* ents) {
    const int64_t n = set->n, nd = set->nd;
    // transposed incidence, entries visited in ascending (entity, a), kept for the touched nodes alone
    std::vector<int64_t> ptr, tptr(1, 0);
    std::vector<uint32_t> tent;
    if (!transpose_incidence(n * nd, m->num_field_nodes, [&](int64_t i) { return m->h_dofmap[(size_t)(ents[2 * (i / nd)] * nd + i % nd)]; },
                             [](int64_t i) { return i; }, ptr, tent))
        return dxo_fail(ctx, DXO_E_SIZE, "dxo_facet_set_create: dofmap entry out of range");      // not reached: dxo_mesh_create refuses it
    std::vector<int32_t> tnode;
    for (int64_t v = 0; v < m->num_field_nodes; ++v)
        if (ptr[(size_t)v + 1] > ptr[(size_t)v]) {
            tnode.push_back((int32_t)v);
            tptr.push_back(ptr[(size_t)v + 1]);
        }
    set->n_touched = (int64_t)tnode.size();
    DXO_HIP(ctx, hipMalloc((void**)&set->d_fe, (size_t)(n * nd) * m->gdim * sizeof(double)));
    int rc = to_device(ctx, &set->d_ents, ents, (size_t)n * 2);
    if (rc == DXO_OK) rc = to_device(ctx, &set->d_tnode, tnode);
    if (rc == DXO_OK) rc = to_device(ctx, &set->d_tptr, tptr);
    if (rc == DXO_OK) rc = to_device(ctx, &set->d_tent, tent);
    return rc;
}

}  // namespace

extern "C" int dxo_mesh_set_facet_geometry(dxo_ctx* ctx, dxo_mesh* m, int n_local_facets, int nq, const double* weights,
                                           const double* ref_normals, const double* ref_jacobians) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!m || !weights || !ref_normals || !ref_jacobians) return dxo_fail(ctx, DXO_E_NULL, "dxo_mesh_set_facet_geometry: NULL argument");
    if (!m->d_facet_tab) return dxo_fail(ctx, DXO_E_OPTION, "dxo_mesh_set_facet_geometry: call dxo_mesh_set_facet_tables first");
    if (n_local_facets != m->n_local_facets || nq != m->nq_facet)
        return dxo_fail(ctx, DXO_E_DIM, "dxo_mesh_set_facet_geometry: n_local_facets / nq differ from the facet tables'");
    const size_t G = (size_t)m->gdim, nf = (size_t)n_local_facets, n_w = (size_t)nq, n_n = nf * G, n_j = nf * G * (G - 1);
    m->nf_geom = m->nq_geom = 0;
    const int rc = upload_slab(ctx, &m->d_facet_geom, {{weights, n_w}, {ref_normals, n_n}, {ref_jacobians, n_j}});
    if (rc != DXO_OK) return rc;
    m->nf_geom = n_local_facets;
    m->nq_geom = nq;
    return DXO_OK;
}

extern "C" int dxo_facet_set_create(dxo_ctx* ctx, dxo_mesh* m, const int32_t* entities, int64_t n, dxo_facet_set** out) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!m || !out || (n > 0 && !entities)) return dxo_fail(ctx, DXO_E_NULL, "dxo_facet_set_create: NULL argument");
    *out = nullptr;
    if (!m->d_facet_tab) return dxo_fail(ctx, DXO_E_OPTION, "dxo_facet_set_create: call dxo_mesh_set_facet_tables first");
    if (n < 0) return dxo_fail(ctx, DXO_E_SIZE, "dxo_facet_set_create: n < 0");
    if (n * m->dev.ndofs >= ((int64_t)1 << 32)) return dxo_fail(ctx, DXO_E_SIZE, "dxo_facet_set_create: 2^32 or more (entity, dof) entries");
    if (!facet_entities_ok(m, entities, n)) return dxo_fail(ctx, DXO_E_SIZE, "dxo_facet_set_create: entity outside [0, num_cells) x [0, n_local_facets)");
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    dxo_facet_set* set = new dxo_facet_set;
    set->mesh = m;
    set->n = n;
    set->nd = m->dev.ndofs;
    set->nf = m->n_local_facets;
    if (n > 0) {
        const int rc = set_build(ctx, set, m, entities);
        if (rc != DXO_OK) {
            set_free(set);
            return rc;
        }
    }
    *out = set;
    return DXO_OK;
}

extern "C" int dxo_facet_set_destroy(dxo_ctx* ctx, dxo_facet_set* set) {
    if (!set) return DXO_OK;
    DXO_LOCK(ctx);
    if (ctx) (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();       // the scratch may still be read by a queued launch
    set_free(set);
    return DXO_OK;
}

extern "C" int dxo_eval_facet_geometry(dxo_ctx* ctx, dxo_mesh* m, const dxo_facet_set* set, double* normals, double* dS) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    int rc = facet_ready(ctx, m, set, "dxo_eval_facet_geometry");
    if (rc != DXO_OK) return rc;
    if (((uintptr_t)normals | (uintptr_t)dS) & 7u) return dxo_fail(ctx, DXO_E_ALIGN, "dxo_eval_facet_geometry: arrays must be 8-byte aligned");
    if (set->n == 0 || (!normals && !dS)) return DXO_OK;
    hipStream_t s = dxo_launch_stream(ctx);
    rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    with_gdim(m->gdim, [&](auto G) {
        hipLaunchKernelGGL(facet_geometry<G>, dim3(capped_grid(ctx, set->n * m->nq_facet, DXO_BLOCK, 8)), dim3(DXO_BLOCK), 0, s, m->dev,
                           facet_tabs<G>(m), set->d_ents, set->n, normals, dS);
    });
    return dxo_device_end(ctx, s);
}

extern "C" int dxo_facet_adjoint(dxo_ctx* ctx, dxo_mesh* m, const dxo_facet_set* set, int kind, int bs, const double* S, double* out) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    int rc = facet_ready(ctx, m, set, "dxo_facet_adjoint");
    if (rc != DXO_OK) return rc;
    if (op_is_nonlinear(kind)) return dxo_fail(ctx, DXO_E_OPTION, "dxo_facet_adjoint: a nonlinear operand (C, I1, det F) has no adjoint");
    const int D = dxo_operand_value_size(m->gdim, bs, kind);
    if (D == DXO_E_OPTION) return dxo_fail(ctx, DXO_E_OPTION, "dxo_facet_adjoint: unknown operand kind");
    if (D < 0 || (bs != 1 && bs != m->gdim)) return dxo_fail(ctx, DXO_E_DIM, "dxo_facet_adjoint: block size does not fit the operand kind / gdim (bs = 1 or gdim)");
    if (set->n == 0) return DXO_OK;
    if (!S || !out) return dxo_fail(ctx, DXO_E_NULL, "dxo_facet_adjoint: NULL array");
    if (((uintptr_t)S | (uintptr_t)out) & 7u) return dxo_fail(ctx, DXO_E_ALIGN, "dxo_facet_adjoint: arrays must be 8-byte aligned");
    hipStream_t s = dxo_launch_stream(ctx);
    rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    rc = with_form_shape(m->gdim, bs, [&](auto G, auto BS) {
        return with_operand_kind<G, BS, true>(kind, [&](auto KIND) { launch_element<G, BS, KIND, FE_LOAD>(ctx, m, set, S, nullptr, 1.0, s); });
    });
    if (rc != DXO_OK) return dxo_fail(ctx, rc, "dxo_facet_adjoint: unsupported (gdim, bs, kind)");
    launch_node_sum(ctx, set, bs, out, s);
    return dxo_device_end(ctx, s);
}

extern "C" int dxo_facet_pressure(dxo_ctx* ctx, dxo_mesh* m, const dxo_facet_set* set, const double* p, double scale, double* out) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    int rc = facet_ready(ctx, m, set, "dxo_facet_pressure");
    if (rc != DXO_OK) return rc;
    if (set->n == 0) return DXO_OK;
    if (!out) return dxo_fail(ctx, DXO_E_NULL, "dxo_facet_pressure: out is NULL");
    if (((uintptr_t)p | (uintptr_t)out) & 7u) return dxo_fail(ctx, DXO_E_ALIGN, "dxo_facet_pressure: arrays must be 8-byte aligned");
    hipStream_t s = dxo_launch_stream(ctx);
    rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    with_gdim(m->gdim, [&](auto G) { launch_element<G, G, DXO_OPERAND_VALUE, FE_PRESSURE>(ctx, m, set, p, nullptr, scale, s); });
    launch_node_sum(ctx, set, m->gdim, out, s);
    return dxo_device_end(ctx, s);
}

// ---- bilinear forms on the set's facets: the Jacobian of a boundary term g(operand(u)) . v ds,
//   K[(a,i),(b,j)] = sum_e sum_q dS_eq phi_a(x_eq) sum_r C_eq[i][r] (B_trial,eq)_r,(b,j),   C [n][nq][BS][D_trial]
// with dS and the tables those of dxo_facet_adjoint. The test side is the value; row i of the point's block is an operand value of the
// trial kind, so its dual data (vh[BS], T[BS][G] = dS * dual_tensor of C[i][:] pulled back to reference gradients) is the row of K:
//   K[(a,i),(b,j)] = sum_q phi_a (vh_i[j] phi_b + sum_k T_i[j][k] dphi_b,k).
//   apply    facet_element<.., FE_APPLY>: lane = (entity, point) forms the trial operand of v and parks dS C w; lane = (entity,
//            local dof) sums over the points into the set's fe; facet_node_sum finishes (two launches, as the loads).
//   diagonal facet_element<.., FE_DIAG>: parks (vh_i[i], T_i[i][:]), then phi_a (vh_i[i] phi_a + sum_k T_i[i][k] dphi_a,k).
//   assemble two passes per chunk of entities, as assemble.hip: facet_assemble_elem parks the point's BS x BS x NZ block and lane =
//            (entity, a, b) writes ae[e][a*BS+i][b*BS+j]; assemble_rows<.., FacetRows> (csr.h), lane = (touched node, component), walks the node's
//            incidences in ascending entity order and adds into values through row_ptr / pos. Every value is the same chain of
//            additions whatever the chunk size.
// No atomics; the calls always accumulate.
namespace {

constexpr int FB_LDS_DOUBLES = 64 * 1024 / 8;

// parked doubles per point of the assembly: the BS x BS x NZ block, odd stride (bank spread across points)
template <int G, int BS, int KIND>
constexpr int fb_block_stride() { return (BS * BS * facet_nz<G, KIND>()) | 1; }

// pass 1: the element matrices of the entities [e_begin, e_end) into ae[e - e_begin][a*BS + i][b*BS + j]; epb entities per round
template <int G, int BS, int KIND>
__global__ __launch_bounds__(DXO_BLOCK) void facet_assemble_elem(OperandDev m, FacetTabs<G> t, const int32_t* __restrict__ ents,
                                                                 int64_t e_begin, int64_t e_end, int epb, const double* __restrict__ C,
                                                                 double* __restrict__ ae) {
    constexpr int D = OperandShape<G, BS, KIND>::D, NZ = facet_nz<G, KIND>(), PS = fb_block_stride<G, BS, KIND>();
    extern __shared__ double lds[];
    const int nqf = t.nqf, nd = t.nd, ndb = nd * BS;
    for (int64_t e0 = e_begin + (int64_t)blockIdx.x * epb; e0 < e_end; e0 += (int64_t)gridDim.x * epb) {
        const int ne = (int)(e_end - e0 < epb ? e_end - e0 : epb);
        if ((int)threadIdx.x < ne * nqf) {               // epb * nqf <= DXO_BLOCK
            const int le = threadIdx.x / nqf, q = threadIdx.x - le * nqf;
            const int64_t e = e0 + le;
            double K[G][G], nrm[G], ds;
            facet_point_geometry<G>(m, t, ents[2 * e], ents[2 * e + 1], q, K, nrm, ds);
            const double* Cp = C + (e * nqf + q) * (int64_t)(BS * D);
            double* P = lds + threadIdx.x * PS;
#pragma unroll
            for (int i = 0; i < BS; ++i) {
                double vh[BS], T[BS][G];
                facet_dual<G, BS, KIND>(Cp + i * D, K, ds, vh, T);
#pragma unroll
                for (int j = 0; j < BS; ++j) {
                    double* Pij = P + (i * BS + j) * NZ;
                    int z = 0;
                    if constexpr (op_has_value<KIND>()) Pij[z++] = vh[j];
                    if constexpr (op_has_grad<KIND>()) {
#pragma unroll
                        for (int k = 0; k < G; ++k) Pij[z + k] = T[j][k];
                    }
                }
            }
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < ne * nd * nd; idx += blockDim.x) {
            const int le = idx / (nd * nd), ab = idx - le * nd * nd, a = ab / nd, b = ab - a * nd;
            const int64_t e = e0 + le;
            const int f = ents[2 * e + 1];
            double acc[BS][BS];
#pragma unroll
            for (int i = 0; i < BS; ++i)
#pragma unroll
                for (int j = 0; j < BS; ++j) acc[i][j] = 0.0;
            for (int q = 0; q < nqf; ++q) {
                const double* P = lds + (le * nqf + q) * PS;
                const size_t row = ((size_t)f * nqf + q) * nd;
                const double pa = t.phi[row + a];
                double zb[NZ];
                facet_dof_slots<G, KIND>(t, row + b, zb);
#pragma unroll
                for (int i = 0; i < BS; ++i)
#pragma unroll
                    for (int j = 0; j < BS; ++j) {
                        double s = 0.0;
#pragma unroll
                        for (int zz = 0; zz < NZ; ++zz) s += P[(i * BS + j) * NZ + zz] * zb[zz];
                        acc[i][j] += pa * s;
                    }
            }
            double* dst = ae + ((e - e_begin) * ndb + (int64_t)a * BS) * ndb + b * BS;
#pragma unroll
            for (int i = 0; i < BS; ++i)
#pragma unroll
                for (int j = 0; j < BS; ++j) dst[(int64_t)i * ndb + j] = acc[i][j];
        }
        __syncthreads();     // the next round overwrites the parked blocks
    }
}

// f(int_c<G>, int_c<BS>, int_c<KIND>) for the trial kinds and shapes of the facet forms (DEFGRAD has been replaced by GRAD)
template <class F>
int with_facet_trial(int gdim, int bs, int kind, F&& f) {
    return with_form_shape(gdim, bs, [&](auto G, auto BS) {
        int rc = DXO_E_OPTION;
        auto any = [&](auto K) { f(G, BS, K); rc = DXO_OK; };
        auto vec = [&](auto K) {
            if constexpr (decltype(BS)::value == decltype(G)::value) any(K);
            else rc = DXO_E_DIM;
        };
        with_int<DXO_OPERAND_VALUE, DXO_OPERAND_GRAD, DXO_OPERAND_VALUE_GRAD>(
            kind, any, [&](int) { with_int<DXO_OPERAND_EPS_MANDEL, DXO_OPERAND_DIV>(kind, vec, [](int) {}); });
        return rc;
    });
}

// the opening of the three calls: facet_ready, the test kind, the trial kind (*kind = the kind the kernels take) and the block size
int facet_bilinear_ready(dxo_ctx* ctx, const dxo_mesh* m, const dxo_facet_set* set, int test, int trial, int bs, const char* who, int* kind) {
    const int rc = facet_ready(ctx, m, set, who);
    if (rc != DXO_OK) return rc;
    if (test != DXO_OPERAND_VALUE) return fail_who(ctx, DXO_E_OPTION, who, "the test kind must be DXO_OPERAND_VALUE (a boundary residual g . v ds)");
    if (op_is_nonlinear(trial)) return fail_who(ctx, DXO_E_OPTION, who, "a nonlinear trial operand (C, I1, det F) has no bilinear form — pass its linearisation's block");
    const int D = dxo_operand_value_size(m->gdim, bs, trial);
    if (D == DXO_E_OPTION) return fail_who(ctx, DXO_E_OPTION, who, "unknown trial operand kind");
    if (D < 0 || (bs != 1 && bs != m->gdim)) return fail_who(ctx, DXO_E_DIM, who, "block size does not fit the trial kind / gdim (bs = 1 or gdim)");
    *kind = trial == DXO_OPERAND_DEFGRAD ? DXO_OPERAND_GRAD : trial;
    // the shape lookup the launches repeat: a miss is reported here, before dxo_device_begin
    const int shape = with_facet_trial(m->gdim, bs, *kind, [](auto, auto, auto) {});
    if (shape != DXO_OK) return fail_who(ctx, shape, who, "unsupported (gdim, bs, trial kind)");
    return DXO_OK;
}

// dxo_facet_bilinear_apply (v != NULL) and dxo_facet_bilinear_diagonal (v == NULL, diag)
int facet_bilinear_vector(dxo_ctx* ctx, dxo_mesh* m, const dxo_facet_set* set, int test, int trial, int bs, const double* C, const double* v,
                          bool diag, double* out, const char* who) {
    int kind = 0;
    int rc = facet_bilinear_ready(ctx, m, set, test, trial, bs, who, &kind);
    if (rc != DXO_OK) return rc;
    if (set->n == 0) return DXO_OK;
    if (!C || !out || (!diag && !v)) return fail_who(ctx, DXO_E_NULL, who, "NULL array");
    if (((uintptr_t)C | (uintptr_t)v | (uintptr_t)out) & 7u) return fail_who(ctx, DXO_E_ALIGN, who, "arrays must be 8-byte aligned");
    hipStream_t s = dxo_launch_stream(ctx);
    rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    with_facet_trial(m->gdim, bs, kind, [&](auto G, auto BS, auto KIND) {
        if (diag) launch_element<G, BS, KIND, FE_DIAG>(ctx, m, set, C, v, 0.0, s);
        else launch_element<G, BS, KIND, FE_APPLY>(ctx, m, set, C, v, 0.0, s);
    });
    launch_node_sum(ctx, set, bs, out, s);
    return dxo_device_end(ctx, s);
}

}  // namespace

extern "C" int dxo_facet_bilinear_apply(dxo_ctx* ctx, dxo_mesh* m, const dxo_facet_set* set, int test_kind, int trial_kind, int bs,
                                        const double* C, const double* v, double* out) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    return facet_bilinear_vector(ctx, m, set, test_kind, trial_kind, bs, C, v, false, out, "dxo_facet_bilinear_apply");
}

extern "C" int dxo_facet_bilinear_diagonal(dxo_ctx* ctx, dxo_mesh* m, const dxo_facet_set* set, int test_kind, int trial_kind, int bs,
                                           const double* C, double* out) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    return facet_bilinear_vector(ctx, m, set, test_kind, trial_kind, bs, C, nullptr, true, out, "dxo_facet_bilinear_diagonal");
}

extern "C" int dxo_facet_bilinear_assemble(dxo_ctx* ctx, dxo_mesh* m, dxo_facet_set* set, dxo_csr* csr, int test_kind, int trial_kind, int bs,
                                           const double* C, double* values) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    const char* who = "dxo_facet_bilinear_assemble";
    if (!csr) return fail_who(ctx, DXO_E_NULL, who, "pattern is NULL");
    int kind = 0;
    int rc = facet_bilinear_ready(ctx, m, set, test_kind, trial_kind, bs, who, &kind);
    if (rc != DXO_OK) return rc;
    if (csr->mesh != m || csr->bs != bs) return fail_who(ctx, DXO_E_DIM, who, "the pattern was made for another mesh or block size");
    if (set->n == 0) return DXO_OK;
    if (!C || !values) return fail_who(ctx, DXO_E_NULL, who, "NULL array");
    if (((uintptr_t)C | (uintptr_t)values) & 7u) return fail_who(ctx, DXO_E_ALIGN, who, "arrays must be 8-byte aligned");
    const int nd = set->nd, nqf = m->nq_facet;
    int ps = 0;
    with_facet_trial(m->gdim, bs, kind, [&](auto G, auto BS, auto KIND) { ps = fb_block_stride<G, BS, KIND>(); });
    if (nqf * ps > FB_LDS_DOUBLES) return fail_who(ctx, DXO_E_SIZE, who, "facet rule too large for the LDS budget");
    const int epb = std::min(DXO_BLOCK / nqf, FB_LDS_DOUBLES / (nqf * ps));      // the parked blocks of a round stay within 64 KiB
    const size_t ent_bytes = (size_t)nd * bs * nd * bs * sizeof(double);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = dxo_launch_stream(ctx);
    const int rblocks = capped_grid(ctx, set->n_touched * bs, DXO_BLOCK, 8);
    const FacetRows rows{set->n_touched, set->d_tptr, set->d_tent, set->d_tnode, set->d_ents};
    rc = assemble_two_pass(
        ctx, set->n, ent_bytes, &set->d_ae, &set->ae_cap, [&] { return dxo_device_begin(ctx, s); },
        [&](int64_t e0, int64_t e1) {
            with_facet_trial(m->gdim, bs, kind, [&](auto G, auto BS, auto KIND) {
                hipLaunchKernelGGL((facet_assemble_elem<G, BS, KIND>), dim3(capped_grid(ctx, e1 - e0, epb, 8)), dim3(DXO_BLOCK),
                                   (size_t)epb * nqf * ps * sizeof(double), s, m->dev, facet_tabs<G>(m), set->d_ents, e0, e1, epb, C, set->d_ae);
            });
        },
        [&](int64_t e0, int64_t e1) {
            with_node_bs(bs, [&](auto BS) {
                hipLaunchKernelGGL((assemble_rows<BS, DXO_BLOCK, FacetRows>), dim3(rblocks), dim3(DXO_BLOCK), 0, s, rows, nd, csr->d_row_ptr,
                                   csr->d_pos, set->d_ae, e0, e1, values);
            });
        });
    return rc != DXO_OK ? rc : dxo_device_end(ctx, s);
}
