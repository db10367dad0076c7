"""The NumPy yardstick of the boundary-facet integrals (dxo_eval_facet_geometry, dxo_facet_adjoint, dxo_facet_pressure), pinned on
the CPU.

The oracle restates the geometry the header defines: J from the facet dpsi table, J_f = J J_ref_f, dS = w sqrt(det(J_f^T J_f)),
n = J^-T n_ref / |J^-T n_ref|. It is pinned by known answers: the reference data of tools.synthetic.facet_geometry maps the reference
facet onto the cell's facet, physical normals point out of their cell (also where det J < 0), the measures add up to the boundary
length / area, and the pressure vector with p = 1 over the whole boundary is the divergence vector int div v dx (divergence theorem).
"""
import numpy as np
import pytest

from oracle.operand_oracle import DEFGRAD, DIV, EPS_MANDEL, GRAD, VALUE, VALUE_GRAD, operand_adjoint
from tools.synthetic import (FACETS, LagrangeElement, exterior_facets, facet_geometry, facet_quadrature_degree2, facet_tables,
                             quarter_annulus, structured_mesh)

CELLS = {"triangle": (4, 3), "quadrilateral": (3, 4), "tetrahedron": (2, 3, 2), "hexahedron": (2, 3, 2)}
REF_FACET_MEASURE = {"triangle": 1.0, "quadrilateral": 1.0, "tetrahedron": 0.5, "hexahedron": 1.0}


def mirrored(m):
    """The mesh reflected in x = 0: every cell's det J changes sign (quadrilaterals and hexahedra then have det J < 0 too)."""
    import dataclasses

    x, node_x = m.x.copy(), m.node_x.copy()
    x[:, 0] *= -1.0
    node_x[:, 0] *= -1.0
    return dataclasses.replace(m, x=x, node_x=node_x)


def cell_jacobians(m, ents):
    """(n, nq, G, G) J at the facet points of the entities."""
    _, _, dpsi_f, _ = facet_tables(m)
    ents = np.asarray(ents, dtype=np.int64)
    X = m.x[m.geom_dofmap[ents[:, 0]]]
    return np.einsum("evj,eqvk->eqjk", X, dpsi_f[ents[:, 1]])


def facet_geometry_ref(m, ents):
    """normals (n, nq, G), dS (n, nq) of the (cell, local facet) entities."""
    w, nref, jref = facet_geometry(m.cell)
    ents = np.asarray(ents, dtype=np.int64)
    J = cell_jacobians(m, ents)
    nv = np.einsum("eqkj,ek->eqj", np.linalg.inv(J), nref[ents[:, 1]])
    n = nv / np.linalg.norm(nv, axis=2, keepdims=True)
    Jf = np.einsum("eqjk,ekl->eqjl", J, jref[ents[:, 1]])
    dS = w[None, :] * np.sqrt(np.linalg.det(np.einsum("eqjl,eqjm->eqlm", Jf, Jf)))
    return n, dS


def facet_pressure_ref(m, ents, p=None, scale=1.0):
    """(num_nodes * G,): scale * sum_e sum_q dS p phi_a n_i."""
    phi_f = facet_tables(m)[0]
    ents = np.asarray(ents, dtype=np.int64)
    n, dS = facet_geometry_ref(m, ents)
    pv = dS * (1.0 if p is None else np.asarray(p).reshape(dS.shape)) * scale
    contrib = np.einsum("eq,eqi,eqa->eai", pv, n, phi_f[ents[:, 1]])
    out = np.zeros((m.node_x.shape[0], m.gdim))
    np.add.at(out, m.dofmap[ents[:, 0]], contrib)
    return out.reshape(-1)


def facet_adjoint_ref(m, ents, kind, bs, S):
    """(num_nodes * bs,): sum_e sum_q dS B^T S, the facet adjoint of eval_operand_facets."""
    phi_f, dphi_f, _, _ = facet_tables(m)
    ents = np.asarray(ents, dtype=np.int64)
    G = m.gdim
    J = cell_jacobians(m, ents)
    K = np.linalg.inv(J)
    _, dS = facet_geometry_ref(m, ents)
    ne, nq = dS.shape
    S = np.asarray(S, dtype=np.float64).reshape(ne, nq, -1)
    vh, gh = np.zeros((ne, nq, bs)), np.zeros((ne, nq, bs, G))
    r = np.sqrt(2.0) * 0.5
    if kind == VALUE:
        vh = S
    elif kind in (GRAD, DEFGRAD):
        gh = S.reshape(ne, nq, bs, G)
    elif kind == VALUE_GRAD:
        vh, gh = S[..., :bs], S[..., bs:].reshape(ne, nq, bs, G)
    elif kind == EPS_MANDEL:
        pairs = [(0, 1, 3)] if G == 2 else [(0, 1, 3), (0, 2, 4), (1, 2, 5)]
        for i in range(G):
            gh[..., i, i] = S[..., i]
        for i, j, k in pairs:
            gh[..., i, j] = gh[..., j, i] = r * S[..., k]
    elif kind == DIV:
        for i in range(G):
            gh[..., i, i] = S[..., 0]
    gphys = np.einsum("eqak,eqkj->eqaj", dphi_f[ents[:, 1]], K)
    contrib = np.einsum("eq,eqi,eqa->eai", dS, vh, phi_f[ents[:, 1]]) + np.einsum("eq,eqij,eqaj->eai", dS, gh, gphys)
    out = np.zeros((m.node_x.shape[0], bs))
    np.add.at(out, m.dofmap[ents[:, 0]], contrib)
    return out.reshape(-1)


def divergence_ref(m):
    """(num_nodes * G,): int div v dx over all cells (the oracle's adjoint of DIV with S = 1)."""
    S = np.ones((m.num_cells, m.nq, 1))
    return operand_adjoint(DIV, m.gdim, S, m.weights, m.dofmap, m.geom_dofmap, m.x, m.phi, m.dphi, m.dpsi, m.node_x.shape[0])


def cell_centroids(m, cells):
    return m.x[m.geom_dofmap[np.asarray(cells)]].mean(axis=1)


def annulus_perimeter(n_r, n_theta, R_i, R_e):
    chord = 2.0 * np.sin(np.pi / (4 * n_theta))
    return n_theta * chord * (R_i + R_e) + 2.0 * (R_e - R_i)


@pytest.mark.parametrize("cell", list(CELLS))
def test_reference_facet_data(cell):
    w, nref, jref = facet_geometry(cell)
    fpts, _ = facet_quadrature_degree2(cell)
    tdim = nref.shape[1]
    assert w.shape == (fpts.shape[0],) and nref.shape == (len(FACETS[cell]), tdim) and jref.shape == (len(FACETS[cell]), tdim, tdim - 1)
    assert w.sum() == pytest.approx(REF_FACET_MEASURE[cell], rel=1e-15)
    verts = LagrangeElement(cell, 1).nodes
    fcell = {"tetrahedron": "triangle", "hexahedron": "quadrilateral"}.get(cell)
    fverts = LagrangeElement(fcell, 1).nodes if fcell else np.array([[0.0], [1.0]])   # reference facet vertices, lattice order
    centre = verts.mean(axis=0)
    for f, fv in enumerate(FACETS[cell]):
        v = verts[list(fv)]
        assert np.allclose(v[0] + fverts @ jref[f].T, v, atol=1e-15)                  # J_ref_f maps the facet's vertices onto the cell's
        assert np.linalg.norm(nref[f]) == pytest.approx(1.0, rel=1e-15)
        assert np.abs(nref[f] @ jref[f]).max() < 1e-15                                # normal to the facet
        assert nref[f] @ (v.mean(axis=0) - centre) > 0                                # and outward


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("mirror", [False, True])
def test_physical_normals_point_out_of_their_cell(cell, mirror):
    m = structured_mesh(cell, CELLS[cell], 2, distort=0.2, seed=3)
    if mirror:
        m = mirrored(m)
    nf = len(FACETS[cell])
    ents = np.array([(c, f) for c in range(m.num_cells) for f in range(nf)], dtype=np.int32)   # every facet, interior ones too
    det = np.linalg.det(cell_jacobians(m, ents))
    if cell in ("triangle", "tetrahedron") or mirror:
        assert (det < 0).any()                                                        # Kuhn simplices: half of them; mirrored: all
    n, dS = facet_geometry_ref(m, ents)
    _, _, _, ref_pts = facet_tables(m)
    psi = np.array([LagrangeElement(cell, 1).tabulate(ref_pts[f])[0] for f in range(nf)])
    xq = np.einsum("eqv,evj->eqj", psi[ents[:, 1]], m.x[m.geom_dofmap[ents[:, 0]]])
    away = np.einsum("eqj,eqj->eq", n, xq - cell_centroids(m, ents[:, 0])[:, None, :])
    assert (away > 0).all()
    assert np.allclose(np.linalg.norm(n, axis=2), 1.0, atol=1e-14) and (dS > 0).all()


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("distort", [0.0, 0.2])
def test_measure_of_the_boundary(cell, distort):
    m = structured_mesh(cell, CELLS[cell], 1, distort=distort, seed=4)
    ents = exterior_facets(m)
    _, dS = facet_geometry_ref(m, ents)
    assert dS.sum() == pytest.approx(4.0 if m.gdim == 2 else 6.0, rel=1e-13)
    on_x0 = exterior_facets(m, where=lambda X: np.all(X[..., 0] == 0.0, axis=1))
    assert facet_geometry_ref(m, on_x0)[1].sum() == pytest.approx(1.0, rel=1e-13)
    assert len(on_x0) == {"triangle": 3, "quadrilateral": 4, "tetrahedron": 2 * 3 * 2, "hexahedron": 6}[cell]


def test_quarter_annulus_tags_and_perimeter():
    n_r, n_theta, R_i, R_e = 3, 10, 1.0, 1.3
    m, tags = quarter_annulus(n_r, n_theta, R_i, R_e)
    ents = exterior_facets(m)
    assert sorted(map(tuple, np.concatenate(list(tags.values())))) == sorted(map(tuple, ents))      # the tags cover the boundary once
    assert {k: len(v) for k, v in tags.items()} == {"Lx": n_r, "Ly": n_r, "inner": n_theta, "outer": n_theta}
    _, dS = facet_geometry_ref(m, ents)
    assert dS.sum() == pytest.approx(annulus_perimeter(n_r, n_theta, R_i, R_e), rel=1e-14)
    r = np.linalg.norm(m.node_x, axis=1)
    assert r.min() >= R_i * np.cos(np.pi / (4 * n_theta)) - 1e-14 and r.max() <= R_e + 1e-14
    verts = m.x[m.geom_dofmap[tags["inner"][:, 0][:, None], np.array(FACETS["triangle"])[tags["inner"][:, 1]]]]
    assert np.allclose(np.linalg.norm(verts, axis=2), R_i, rtol=1e-15)
    assert (m.x[m.geom_dofmap[tags["Ly"][:, 0]]][..., 0] >= 0).all()
    # int n ds over the inner arc: the chord (0, R_i) - (R_i, 0) turned outward of the solid (towards the axis)
    n, dS = facet_geometry_ref(m, tags["inner"])
    assert np.allclose(np.einsum("eqi,eq->i", n, dS), [-R_i, -R_i], rtol=1e-14)


@pytest.mark.parametrize("cell,distort", [("triangle", 0.2), ("tetrahedron", 0.2), ("quadrilateral", 0.0), ("hexahedron", 0.0)])
@pytest.mark.parametrize("degree", [1, 2])
def test_pressure_over_the_boundary_is_the_divergence_vector(cell, distort, degree):
    m = structured_mesh(cell, CELLS[cell], degree, distort=distort, seed=5)
    got = facet_pressure_ref(m, exterior_facets(m))
    ref = divergence_ref(m)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize("cell", list(CELLS))
def test_adjoint_oracle_value_is_pressure_and_div_is_traced(cell):
    """facet_adjoint_ref(VALUE, gdim, S = p n) is the pressure vector; DIV with S = s equals GRAD with S = s I."""
    m = structured_mesh(cell, CELLS[cell], 2, distort=0.15, seed=6)
    ents = exterior_facets(m)
    rng = np.random.Generator(np.random.PCG64(1))
    n, dS = facet_geometry_ref(m, ents)
    p = rng.normal(size=dS.shape)
    assert np.allclose(facet_adjoint_ref(m, ents, VALUE, m.gdim, p[..., None] * n), facet_pressure_ref(m, ents, p), atol=1e-14)
    s = rng.normal(size=dS.shape)
    eye = np.eye(m.gdim).reshape(-1)
    assert np.allclose(facet_adjoint_ref(m, ents, DIV, m.gdim, s[..., None]),
                       facet_adjoint_ref(m, ents, GRAD, m.gdim, s[..., None] * eye), atol=1e-14)


def test_library_exports_the_facet_entry_points(hip_library):
    from dolfinx_external_operator_amd import DeviceMesh, FacetSet
    from dolfinx_external_operator_amd._lib import declared_symbols

    names = ("dxo_mesh_set_facet_geometry", "dxo_facet_set_create", "dxo_facet_set_destroy", "dxo_eval_facet_geometry",
             "dxo_facet_adjoint", "dxo_facet_pressure")
    for name in names:
        assert name in declared_symbols() and hasattr(hip_library, name)
    for meth in ("set_facet_geometry", "facet_set", "facet_geometry", "facet_adjoint", "facet_pressure"):
        assert callable(getattr(DeviceMesh, meth))
    assert callable(FacetSet.close)
