// facet_tabs.h — what operand_facet.hip, facet_form.hip and functional.hip share: the facet tables and facet geometry of a mesh as device
// pointers, the facet set, the geometry of a facet point (facet_point_geometry) and the checks of a facet call (facet_ready).
// The gather of the cell's Jacobian at a facet point stays written out in operand_eval_facets and in facet_point_geometry: behind
// a shared function, in each of seven formulations tried, facet_element<3, *, VALUE_GRAD, FE_LOAD> changed its registers, and in six its occupancy
// (profiles/form_fold_resources.txt).
#pragma once

#include "form_host.h"

struct dxo_facet_set {
    const dxo_mesh* mesh = nullptr;
    int64_t n = 0;
    int nd = 0, nf = 0;
    int32_t* d_ents = nullptr;       // [n][2] (cell, local facet)
    double* d_fe = nullptr;          // [n][nd][gdim] element vectors of the last call
    int64_t n_touched = 0;           // nodes with at least one incidence
    int32_t* d_tnode = nullptr;      // [n_touched] the nodes, ascending
    int64_t* d_tptr = nullptr;       // [n_touched + 1]
    uint32_t* d_tent = nullptr;      // [n * nd] entries e * nd + a of each node, ascending entity order
    double* d_ae = nullptr;          // element-matrix scratch of one chunk of entities (dxo_facet_bilinear_assemble), grow-only
    size_t ae_cap = 0;
    double* d_fn_part = nullptr;     // functional.hip: partial sums [n_out][n_groups] of the last dxo_facet_integrate, grow-only
    size_t fn_cap = 0;
};

namespace {

template <int G>
struct FacetTabs {
    int nqf, nd, ng;
    const double* phi;      // [nf][nqf][nd]
    const double* dphi;     // [nf][nqf][nd][G]
    const double* dpsi;     // [nf][nqf][ng][G]
    const double* w;        // [nqf]            these three: null until dxo_mesh_set_facet_geometry
    const double* nref;     // [nf][G]
    const double* jref;     // [nf][G][G-1]
};

template <int G>
FacetTabs<G> facet_tabs(const dxo_mesh* m) {
    const size_t nd = (size_t)m->dev.ndofs, nf = (size_t)m->n_local_facets, nqf = (size_t)m->nq_facet;
    FacetTabs<G> t;
    t.nqf = (int)nqf;
    t.nd = (int)nd;
    t.ng = m->dev.ngeom;
    t.phi = m->d_facet_tab;
    t.dphi = t.phi + nf * nqf * nd;
    t.dpsi = t.dphi + nf * nqf * nd * G;
    t.w = m->d_facet_geom;
    t.nref = t.w ? t.w + nqf : nullptr;
    t.jref = t.w ? t.nref + nf * G : nullptr;
    return t;
}

// J^-1 (K), the outward unit normal and the point measure at point q of facet f of `cell`
template <int G>
__device__ __forceinline__ void facet_point_geometry(const OperandDev& m, const FacetTabs<G>& t, int64_t cell, int f, int q,
                                                     double (&K)[G][G], double (&nrm)[G], double& dS) {
    const double* dpsi = t.dpsi + ((size_t)f * t.nqf + q) * t.ng * G;
    double J[G][G];
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
        for (int k = 0; k < G; ++k) J[j][k] = 0.0;
    for (int v = 0; v < t.ng; ++v) {
        const int64_t node = m.geom_dofmap[cell * t.ng + v];
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const double xj = m.x[node * G + j];
#pragma unroll
            for (int k = 0; k < G; ++k) J[j][k] += xj * dpsi[v * G + k];
        }
    }
    (void)invert<G>(J, K);
    // n ~ J^-T n_ref: n_j = sum_k K[k][j] n_ref_k
    const double* nr = t.nref + (size_t)f * G;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < G; ++j) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < G; ++k) v += K[k][j] * nr[k];
        nrm[j] = v;
        s += v * v;
    }
    const double inv = 1.0 / sqrt(s);
#pragma unroll
    for (int j = 0; j < G; ++j) nrm[j] *= inv;
    // J_f = J J_ref_f (G x (G-1)); sqrt(det(J_f^T J_f)) = |column| in 2-D, |a x b| in 3-D
    const double* jr = t.jref + (size_t)f * G * (G - 1);
    double Jf[G][G - 1];
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
        for (int l = 0; l < G - 1; ++l) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < G; ++k) v += J[j][k] * jr[k * (G - 1) + l];
            Jf[j][l] = v;
        }
    double meas;
    if constexpr (G == 2) {
        meas = sqrt(Jf[0][0] * Jf[0][0] + Jf[1][0] * Jf[1][0]);
    } else {
        const double c0 = Jf[1][0] * Jf[2][1] - Jf[2][0] * Jf[1][1];
        const double c1 = Jf[2][0] * Jf[0][1] - Jf[0][0] * Jf[2][1];
        const double c2 = Jf[0][0] * Jf[1][1] - Jf[1][0] * Jf[0][1];
        meas = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
    }
    dS = t.w[q] * meas;
}

// checks shared by the facet calls (facet_form.hip, functional.hip); DXO_OK when the set may be used on the mesh
inline int facet_ready(dxo_ctx* ctx, const dxo_mesh* m, const dxo_facet_set* set, const char* who) {
    if (!m || !set) return fail_who(ctx, DXO_E_NULL, who, "mesh or facet set is NULL");
    if (!m->d_facet_tab || !m->d_facet_geom)
        return fail_who(ctx, DXO_E_OPTION, who, "facet tables or facet geometry not set (dxo_mesh_set_facet_tables, dxo_mesh_set_facet_geometry)");
    if (set->mesh != m) return fail_who(ctx, DXO_E_DIM, who, "the facet set was created on another mesh");
    if (m->nf_geom != m->n_local_facets || m->nq_geom != m->nq_facet || set->nf > m->n_local_facets || m->nq_facet > DXO_BLOCK)
        return fail_who(ctx, DXO_E_DIM, who, "facet tables, facet geometry and facet set disagree on (n_local_facets, nq)");
    return DXO_OK;
}

}  // namespace
