"""The NumPy yardstick of the boundary-facet bilinear forms (tests/facet_bilinear_cases.py), pinned on the CPU by known answers on the
CELLS meshes of test_facet_oracle_cpu.py, degrees 1 and 2, whole exterior:

  ("value", 1), C = 1  is the boundary mass matrix: 1^T K 1 = the boundary measure (4 in 2-D, 6 in 3-D), K = K^T, and every nonzero
                       lies inside the pattern of dxo_csr_create (oracle.form_oracle.pattern_ref);
  ("div", gdim), C[i][0] = n_i  gives K u = the pressure vector of p = div u at the facet points (facet_pressure_ref);
  ("grad", 1), C = n^T  gives 1^T K u = int n . grad u ds = int laplace u dx = 0 for a linear u (undistorted meshes).

Bounds: every entry of K is a sum of at most (entities of a node) x (facet points) <= 100 products of O(1) factors, each formed with a
few roundings of 1.1e-16; 1e-13 relative to the scale of the terms leaves a factor of ten. Symmetry compares two sums of the same
products taken in the same order, so it holds to a few units of the last place: 1e-15 of the largest entry.
"""
import numpy as np
import pytest

from facet_bilinear_cases import (CELLS, DEGREES, facet_bilinear_apply_ref, facet_bilinear_dense_ref, facet_operand_ref, mesh_case,
                                  trial_cases)
from oracle.form_oracle import pattern_ref
from test_facet_oracle_cpu import facet_geometry_ref, facet_pressure_ref
from tools.synthetic import exterior_facets, facet_tables


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("degree", DEGREES)
def test_boundary_mass_matrix(cell, degree):
    m = mesh_case(cell, degree)
    ents = exterior_facets(m)
    nq = facet_tables(m)[0].shape[1]
    K = facet_bilinear_dense_ref(m, ents, "value", 1, np.ones((len(ents), nq, 1, 1)))
    measure = 4.0 if m.gdim == 2 else 6.0
    print(f"{cell} P{degree}: |1^T K 1 - measure| = {abs(K.sum() - measure):.2e}, |K - K^T| = {np.abs(K - K.T).max():.2e}")
    assert abs(K.sum() - measure) <= 1e-13 * measure
    assert np.abs(K - K.T).max() <= 1e-15 * np.abs(K).max()
    indptr, indices = pattern_ref(m, 1)
    inside = np.zeros_like(K, dtype=bool)
    inside[np.repeat(np.arange(K.shape[0]), np.diff(indptr)), indices] = True
    assert np.abs(K[~inside]).max(initial=0.0) == 0.0
    assert (np.abs(K[inside]) > 0).any()
    # the matrix-free oracle is the same operator
    v = np.random.Generator(np.random.PCG64(1)).normal(size=K.shape[0])
    Kv = facet_bilinear_apply_ref(m, ents, "value", 1, np.ones((len(ents), nq, 1, 1)), v)
    assert np.abs(K @ v - Kv).max() <= 1e-13 * np.abs(Kv).max()


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("degree", DEGREES)
def test_div_trial_with_the_normal_is_the_pressure_of_div_u(cell, degree):
    m = mesh_case(cell, degree)
    G = m.gdim
    ents = exterior_facets(m)
    n, _ = facet_geometry_ref(m, ents)
    u = np.random.Generator(np.random.PCG64(2)).normal(size=m.node_x.shape[0] * G)
    got = facet_bilinear_apply_ref(m, ents, "div", G, n[..., None], u)
    ref = facet_pressure_ref(m, ents, p=facet_operand_ref(m, ents, "div", G, u)[..., 0])
    print(f"{cell} P{degree}: |K u - pressure| = {np.abs(got - ref).max():.2e} of {np.abs(ref).max():.2e}")
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("degree", DEGREES)
def test_normal_flux_of_a_linear_field_sums_to_zero(cell, degree):
    m = mesh_case(cell, degree, distort=0.0)
    G = m.gdim
    ents = exterior_facets(m)
    n, dS = facet_geometry_ref(m, ents)
    a = np.array([0.7, -1.3, 0.4])[:G]
    u = 0.25 + m.node_x @ a
    Ku = facet_bilinear_apply_ref(m, ents, "grad", 1, n[:, :, None, :], u)
    scale = np.abs(a).sum() * dS.sum()                     # sum of |n . grad u| dS is at most this
    print(f"{cell} P{degree}: 1^T K u = {Ku.sum():.2e} of {scale:.2e}")
    assert abs(Ku.sum()) <= 1e-13 * scale
    assert np.abs(Ku).max() > 0.1                          # the entries themselves are not small: they cancel


@pytest.mark.parametrize("cell", ["triangle", "hexahedron"])
def test_dense_oracle_is_the_matrix_free_oracle(cell):
    """Every (trial, bs): the dense matrix applied to a vector is the composed action, "F" equals "grad"."""
    from facet_bilinear_cases import entity_list, random_block

    m = mesh_case(cell, 2)
    ents = entity_list(m, "subset")
    rng = np.random.Generator(np.random.PCG64(3))
    for trial, bs in trial_cases(m.gdim):
        Cb = random_block(m, ents, trial, bs)
        K = facet_bilinear_dense_ref(m, ents, trial, bs, Cb)
        v = rng.normal(size=K.shape[0])
        Kv = facet_bilinear_apply_ref(m, ents, trial, bs, Cb, v)
        assert np.abs(K @ v - Kv).max() <= 1e-13 * np.abs(Kv).max(), (trial, bs)
        if trial == "F":        # (I + grad u) - I keeps grad u to an absolute 1.1e-16
            assert np.abs(K - facet_bilinear_dense_ref(m, ents, "grad", bs, Cb)).max() <= 1e-13 * np.abs(K).max()


def test_library_exports_the_facet_bilinear_entry_points(hip_library):
    from dolfinx_external_operator_amd import DeviceMesh
    from dolfinx_external_operator_amd._lib import declared_symbols

    for name in ("dxo_facet_bilinear_apply", "dxo_facet_bilinear_diagonal", "dxo_facet_bilinear_assemble"):
        assert name in declared_symbols() and hasattr(hip_library, name)
    for meth in ("facet_bilinear_apply", "facet_bilinear_diagonal", "facet_bilinear_assemble"):
        assert callable(getattr(DeviceMesh, meth))
    assert set(DeviceMesh.FACET_BILINEAR_TRIALS) == {"value", "grad", "value_grad", "eps", "div", "F"}
