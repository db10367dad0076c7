"""oracle/facet_reference.py (long double) tied to what the suite already trusts, on the CPU: the float64 facet oracles, and known
answers that do not pass through them. The figures measured here are the constants the componentwise bound of
tests/test_facet_reference_gpu.py is built from (facet_reference_cases.C_REF, facet_reference_cases.RESOLVES)."""
import functools

import numpy as np
import pytest

from facet_reference_cases import (ALL_CASES, C_REF, MARGIN, RESOLVES, case_id, check_rounds, entity_lists, float64_side, item_id, mesh_of,
                                   old_criterion, on_pattern, reference, rule_tables, strang_fix_6, work_items)
from oracle import facet_reference as R
from oracle.consumer_reference import ref_adjoint_eps
from oracle.facet_reference import LD, worst_ratio
from test_facet_oracle_cpu import CELLS, REF_FACET_MEASURE
from tools.synthetic import exterior_facets, facet_geometry, facet_tables, structured_mesh

EPS64, EPS53 = LD(2.0) ** -64, LD(2.0) ** -53
SIZE_B = [c for c in ALL_CASES if c[1] == 2 and c[2] == "b" and not c[3] and c[4] == "deg2"]
# Known answers that pass through the element tables hold to the tables' own rounding: tools.synthetic tabulates by inverting a
# Vandermonde matrix in float64, so that sum_a phi_a = 1, sum_a dphi_a = 0 and the reproduction of linear fields hold to a few 2^-53 of
# the sum of magnitudes times the condition of that matrix, not to long-double accuracy. TABLES = 256 of those units (measured: 34 on
# Q2 hexahedra, whose 27 x 27 matrix is the worst conditioned, below 7 elsewhere). A wrong slot, sign or transposition is an error of
# order 1 in these identities.
TABLES = 256 * EPS53


# ------------------------------------------------------------------------------------------------ C_REF
@functools.lru_cache(maxsize=None)
def float64_ratios(case):
    """-> {entry: (worst ratio, list, work item)} over every entity list and work item of the case: the float64 oracle (or, where
    facet_reference_cases.float64_side says so, the twin) and ALWAYS the float64 twin of the reference, against the long-double reference."""
    m = mesh_of(case)
    out = {}
    for name, ents in entity_lists(case).items():
        for item in work_items(case, name):
            refs = reference(case, ents, item)
            if len(ents) == 0:
                assert all(not np.any(r) and not np.any(mag) and r.dtype == LD for r, mag in refs.values())
                continue
            got, twin = float64_side(case, ents, item), reference(case, ents, item, dtype=np.float64)
            for k, (r, mag) in refs.items():
                tw = twin[k][0]
                assert tw.dtype == np.float64 and r.dtype == LD
                if item.what == "matrix":
                    r, mag, tw = (on_pattern(case, ents, item.bs, x) for x in (r, mag, tw))
                ratio = max(worst_ratio(got[k], r, mag), worst_ratio(tw, r, mag))
                if ratio >= out.get(k, (-1.0,))[0]:
                    out[k] = (ratio, name, item_id(item))
    return out


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_float64_oracles_stay_within_c_ref_of_the_long_double_reference(case):
    """|f64[k] - ref[k]| <= C_REF[entry] * 2^-53 * mag[k] in every entry of every result, on every mesh, rule, entity list and input
    variant of the GPU file, for the float64 oracles and for the reference's own float64 twin."""
    got = float64_ratios(case)
    print(case_id(case), " ".join(f"{k}={v[0]:.2f}" for k, v in got.items()))
    for k, v in got.items():
        assert v[0] <= C_REF[k], (k, v)


def test_c_ref_is_within_a_factor_two_of_what_is_measured():
    """A stale or generous constant fails: every C_REF figure is at least the worst ratio over ALL_CASES and at most twice it."""
    worst = {}
    for case in ALL_CASES:
        for k, v in float64_ratios(case).items():
            if v[0] > worst.get(k, (0.0,))[0]:
                worst[k] = v + (case_id(case),)
    assert set(worst) == set(C_REF)
    for k, v in worst.items():
        print(f"{k:20s} measured {v[0]:6.2f}   C_REF {C_REF[k]:5.1f}   {v[3]}, list {v[1]}, {v[2]}")
        assert v[0] <= C_REF[k] <= 2.0 * v[0], (k, v, C_REF[k])


def test_the_case_list_covers_the_workgroup_rounds():
    """Every (rule, trial, bs) meets a list shorter than a workgroup round, one with a ragged last round and one of whole rounds, in the
    vector kernels and in facet_assemble_elem (facet_reference_cases.check_rounds asserts it; the lines say with which lengths)."""
    lines = check_rounds()
    print("\n".join(lines))
    assert any(" epb  28" in line for line in lines) and any(" epb  24" in line for line in lines)      # the hexahedra's 9-point rule
    assert any(" epb  85" in line for line in lines) and any(" epb  42" in line for line in lines)


def test_the_six_point_triangle_rule_is_exact_to_degree_four():
    """int_T x^i y^j = i! j! / (i + j + 2)! on the reference triangle, every i + j <= 4, to float64 rounding."""
    from math import factorial

    pts, w = strang_fix_6()
    assert pts.shape == (6, 2) and (w > 0).all() and (pts > 0).all() and (pts.sum(axis=1) < 1).all()
    for i in range(5):
        for j in range(5 - i):
            exact = factorial(i) * factorial(j) / factorial(i + j + 2)
            assert abs(np.sum(w * pts[:, 0] ** i * pts[:, 1] ** j) - exact) <= 4 * np.finfo(float).eps * exact, (i, j)


# ------------------------------------------------------------------------------------------------ known answers
def _tabs(m):
    return facet_tables(m)[:3], facet_geometry(m.cell)


@pytest.mark.parametrize("cell", list(CELLS))
def test_measure_of_the_boundary_in_long_double(cell):
    """Undistorted mesh of the unit square / cube: the point measures add up to 4 / 6, and to 1 on the face x = 0, times the sum of the
    rule's float64 weights over the reference facet's measure (1/6 is not a float64). Simplices, whose dpsi table holds the integers
    0 and +-1, reach long-double accuracy (a few 2^-64); quadrilaterals and hexahedra are held to the rounding of their table."""
    m = structured_mesh(cell, CELLS[cell], 1, distort=0.0, seed=4)
    tabs, geom = _tabs(m)
    unit = np.sum(np.asarray(geom[0], dtype=LD)) / LD(REF_FACET_MEASURE[cell])
    tol = 16 * EPS64 if cell in ("triangle", "tetrahedron") else TABLES
    for ents, measure in ((exterior_facets(m), 4 if m.gdim == 2 else 6), (exterior_facets(m, where=lambda X: np.all(X[..., 0] == 0.0, axis=1)), 1)):
        _, _, dS, dS_mag = R.ref_facet_geometry(m, tabs, geom, ents)
        err = abs(dS.sum() - measure * unit)
        print(f"{cell}: measure {measure}: error {float(err):.2e}")
        assert dS.dtype == LD and err <= tol * measure and np.all(dS_mag >= dS) and np.all(dS > 0)


@pytest.mark.parametrize("case", SIZE_B + [c for c in ALL_CASES if c[3] and c[1] == 2], ids=case_id)
def test_normals_have_unit_length_and_point_out_of_their_cell(case):
    """On every local facet of every cell of the distorted size-b meshes and their mirrored twins (det J < 0 in every cell)."""
    m = mesh_of(case)
    tabs, geom, pts = rule_tables(case)
    ents = entity_lists(case)["all"]
    n, n_mag, _, _ = R.ref_facet_geometry(m, tabs, geom, ents)
    assert np.abs(np.sum(n * n, axis=2) - 1).max() <= 8 * EPS64 and np.all(n_mag >= np.abs(n))
    from tools.synthetic import LagrangeElement

    psi = np.array([LagrangeElement(m.cell, 1).tabulate(p)[0] for p in pts])
    X = m.x[m.geom_dofmap[ents[:, 0]]]
    xq = np.einsum("eqv,evj->eqj", psi[ents[:, 1]], X)
    assert (np.einsum("eqj,eqj->eq", n.astype(np.float64), xq - X.mean(axis=1)[:, None, :]) > 0).all()
    if case[3]:
        J = np.einsum("evj,eqvk->eqjk", X, tabs[2][ents[:, 1]])
        assert (np.linalg.det(J) < 0).all() or m.cell in ("triangle", "tetrahedron")


@pytest.mark.parametrize("cell,distort", [("triangle", 0.2), ("tetrahedron", 0.2), ("quadrilateral", 0.0), ("hexahedron", 0.0)])
@pytest.mark.parametrize("degree", [1, 2])
def test_unit_pressure_over_the_boundary_is_the_internal_force_of_a_unit_divergence_load(cell, distort, degree):
    """Divergence theorem, both sides in long double: ref_facet_pressure(p = 1) over the whole boundary equals
    oracle.consumer_reference.ref_adjoint_eps with the Mandel vector of the identity (int div v dx), where both rules integrate exactly
    (affine simplices, undistorted quadrilaterals and hexahedra). Held to the rounding of the tables."""
    m = structured_mesh(cell, CELLS[cell], degree, distort=distort, seed=5)
    tabs, geom = _tabs(m)
    got, mag = R.ref_facet_pressure(m, tabs, geom, exterior_facets(m))
    D = 4 if m.gdim == 2 else 6
    S = np.zeros((m.num_cells, m.nq, D))
    S[..., :m.gdim] = 1.0
    ref, ref_mag = ref_adjoint_eps(m, S)
    ratio = worst_ratio(got, ref, mag + ref_mag)
    print(f"{cell} degree {degree}: {ratio:.2f} * 2^-53 * (mag + mag)")
    assert np.max(np.abs(got - ref) - TABLES * (mag + ref_mag)) <= 0 and np.abs(ref).max() > 0.01


def _affine(m, bs, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    A, b = rng.normal(size=(bs, m.gdim)), rng.normal(size=bs)
    return A, (m.node_x @ A.T + b).reshape(-1)


def _operand_of_gradient(trial, A):
    """The trial operand of v = A x + b in closed form (value kinds excluded): grad and F's linear part A row-major, eps the Mandel
    vector of sym A, div the trace."""
    G = A.shape[1]
    if trial in ("grad", "F"):
        return A.reshape(-1)
    if trial == "div":
        return np.array([np.trace(A)])
    sym, r = 0.5 * (A + A.T), np.sqrt(2.0)
    shear = [(0, 1)] if G == 2 else [(0, 1), (0, 2), (1, 2)]
    return np.array([sym[i, i] for i in range(G)] + ([0.0] if G == 2 else []) + [r * sym[i, j] for i, j in shear])


@pytest.mark.parametrize("case", SIZE_B + [c for c in ALL_CASES if c[1] == 1 and c[2] == "b" and c[4] != "deg2"], ids=case_id)
def test_bilinear_reference_known_answers(case):
    """Trial `value`, C = I: the entries of the matrix sum to bs times the boundary measure, and K 1 is the adjoint of S = 1.
    Trial grad / eps / div / F with v = A x + b, which the space holds on every mesh: K v = ref_facet_adjoint("value", C . operand(A))
    with the operand in closed form. All to the rounding of the tables and of the node coordinates."""
    m = mesh_of(case)
    G, nn = m.gdim, m.node_x.shape[0]
    tabs, geom, _ = rule_tables(case)
    ents = entity_lists(case)["exterior"]
    nq = geom[0].size
    _, _, dS, _ = R.ref_facet_geometry(m, tabs, geom, ents)
    for bs in (1, G):
        eye = np.broadcast_to(np.eye(bs), (len(ents), nq, bs, bs))
        Ke, Ka = R.ref_facet_bilinear_elements(m, tabs, geom, ents, "value", bs, eye)
        assert abs(Ke.sum() - bs * dS.sum()) <= TABLES * Ka.sum()
        Kv, mag = R.ref_facet_bilinear_apply(m, tabs, geom, ents, "value", bs, eye, np.ones(nn * bs))
        f, f_mag = R.ref_facet_adjoint(m, tabs, geom, ents, "value", bs, np.ones((len(ents), nq, bs)))
        assert np.max(np.abs(Kv - f) - TABLES * (mag + f_mag)) <= 0 and np.abs(f).max() > 0
    rng = np.random.Generator(np.random.PCG64(3))
    for trial in ("grad", "eps", "div", "F"):
        for bs in ((1, G) if trial == "grad" else (G,)):
            A, v = _affine(m, bs, 7)
            o = _operand_of_gradient(trial, A)
            C = rng.normal(size=(len(ents), nq, bs, o.size))
            Kv, mag = R.ref_facet_bilinear_apply(m, tabs, geom, ents, trial, bs, C, v)
            f, f_mag = R.ref_facet_adjoint(m, tabs, geom, ents, "value", bs, C @ o)
            worst = worst_ratio(Kv, f, mag + f_mag)
            print(f"{case_id(case)} {trial} bs {bs}: {worst:.2f} * 2^-53 * (mag + mag)")
            assert np.max(np.abs(Kv - f) - TABLES * (mag + f_mag)) <= 0 and np.abs(f).max() > 0.01


@pytest.mark.parametrize("case", SIZE_B + [c for c in ALL_CASES if c[4] != "deg2" and c[1] == 2], ids=case_id)
def test_diagonal_apply_and_element_matrices_are_one_form(case):
    """In long double: the diagonal is the diagonal of the scattered element matrices, the action the scattered matrix times v, the CSR
    scatter the dense one entry by entry — to 64 * 2^-64 * mag, the depth of the longest of these sums being nq * D * nd * bs terms per
    entity (a rounding each, in two different orders) — and nothing lies outside the pattern."""
    from oracle.form_oracle import pattern_ref

    m = mesh_of(case)
    tabs, geom, _ = rule_tables(case)
    ents = entity_lists(case)["all"]
    for item in work_items(case, "all"):
        if item.what != "apply" or item.variant == "offset":
            continue
        Ke, Ka = R.ref_facet_bilinear_elements(m, tabs, geom, ents, item.kind, item.bs, item.C)
        K, Kmag = R.scatter_dense(m, ents, item.bs, Ke), R.scatter_dense(m, ents, item.bs, Ka)
        d, d_mag = R.ref_facet_bilinear_diagonal(m, tabs, geom, ents, item.kind, item.bs, item.C)
        Kv, mag = R.ref_facet_bilinear_apply(m, tabs, geom, ents, item.kind, item.bs, item.C, item.v)
        assert np.max(np.abs(np.diag(K) - d) - 64 * EPS64 * d_mag) <= 0 and np.max(np.abs(np.diag(Kmag) - d_mag) - 64 * EPS64 * d_mag) <= 0
        assert np.max(np.abs(K @ item.v.astype(LD) - Kv) - 64 * EPS64 * mag) <= 0
        assert np.max(np.abs(Kmag @ np.abs(item.v).astype(LD) - mag) - 64 * EPS64 * mag) <= 0
        indptr, indices = pattern_ref(m, item.bs)
        values = R.scatter_csr(m, ents, item.bs, Ke, indptr, indices)
        rows = np.repeat(np.arange(K.shape[0]), np.diff(indptr))
        inside = np.zeros(K.shape, dtype=bool)
        inside[rows, indices] = True
        assert np.array_equal(values, K[rows, indices]) and not np.any(K[~inside]) and values.dtype == LD


# ------------------------------------------------------------------------------------------------ what the bound resolves
@functools.lru_cache(maxsize=None)
def scaled_entity_miss(case, p):
    """-> {entry: (miss, old_ok)}: the float64 oracle fed S / C / p with entity 0 scaled by 1 + 10^-p against the reference of the
    unscaled input (the whole boundary, block size gdim, the plain input variant): its worst ratio as a multiple of
    MARGIN * C_REF[entry], and whether it still meets max|got - ref| <= 1e-12 max|ref|, the criterion of the older facet tests."""
    m = mesh_of(case)
    ents = entity_lists(case)["exterior"]
    out = {}
    for item in work_items(case, "exterior"):
        if item.what == "geometry" or item.variant not in ("", "p") or item.bs != m.gdim:
            continue
        key = {"pressure": "p", "adjoint": "S"}.get(item.what, "C")
        scaled = np.array(getattr(item, key))
        scaled[0] *= 1.0 + 10.0 ** -p
        got = float64_side(case, ents, type(item)(**{**vars(item), key: scaled}))[item.entry]
        (ref, mag), = reference(case, ents, item).values()
        if item.what == "matrix":
            ref, mag = (on_pattern(case, ents, item.bs, x) for x in (ref, mag))
        out[item.entry] = (worst_ratio(got, ref, mag) / (MARGIN * C_REF[item.entry]), old_criterion(got, ref))
    return out


def test_resolves_is_the_finest_relative_error_in_one_entity_that_misses_the_bound():
    """facet_reference_cases.RESOLVES[entry] = p: with entity 0 scaled by 1 + 10^-p the float64 oracle misses MARGIN * C_REF[entry] on
    each of the four quadratic size-b meshes, and with 1 + 10^-(p + 1) it is back inside on at least one of them. At p the same result
    still passes the max-norm criterion of the older facet tests: the gap the componentwise bound closes."""
    ps = sorted(set(RESOLVES.values()))
    at = {p: [scaled_entity_miss(c, p) for c in SIZE_B] for p in sorted(set(ps) | {p + 1 for p in ps})}
    assert set(RESOLVES) == set(at[ps[0]][0]) == {k for k in C_REF if k not in ("normal", "dS")}
    for entry, p in RESOLVES.items():
        here, finer = [r[entry] for r in at[p]], [r[entry] for r in at[p + 1]]
        print(f"{entry:20s} p = {p}: miss {[round(x[0], 2) for x in here]}   p + 1: {[round(x[0], 2) for x in finer]}")
        assert all(miss > 1.0 for miss, _ in here), entry
        assert any(miss <= 1.0 for miss, _ in finer), entry
        assert all(ok for _, ok in here), entry
