// facet_tabs.h — what operand_facet.hip and facet_form.hip share: the facet tables and facet geometry of a mesh as device pointers.
// The gather of the cell's Jacobian at a facet point stays written out in operand_eval_facets and in facet_point_geometry: behind
// a shared function, in each of seven formulations tried, facet_element<3, *, VALUE_GRAD, FE_LOAD> changed its registers, and in six its occupancy
// (profiles/form_fold_resources.txt).
#pragma once

#include "form_host.h"

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

}  // namespace
