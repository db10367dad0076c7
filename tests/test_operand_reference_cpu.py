"""oracle/operand_reference.py (long double) tied to what the suite already trusts, on the CPU: the float64 NumPy oracle and the
polynomial known answers of tests/test_operand_eval.py. The figures measured here are the constants the componentwise bound of
tests/test_operand_reference_gpu.py is built from (operand_cases.C_REF, operand_cases.RESOLVES)."""
import dataclasses
import functools
import itertools
import types
from fractions import Fraction

import numpy as np
import pytest

from operand_cases import (ALL_CASES, C_REF, CELL_KINDS, MARGIN, RESOLVES, SIZES, block_sizes, build_mesh, case_id, element_name,
                           entity_lists, facet_lists, facet_tabs, fields, kinds_of, resolution_case, scale_one_cell)
from oracle.operand_oracle import eval_operand, eval_operand_facets
from oracle.operand_reference import KIND_ID, LD, ref_coordinate, ref_operand, ref_operand_facets, value_size, worst_ratio
from test_operand_eval import expected, poly_field


@functools.lru_cache(maxsize=None)
def float64_ratios(case):
    """Worst componentwise distance of float64 NumPy from the long-double reference on one mesh, in units of 2^-53 * mag[k], over
    every block size, field, entity list and facet list of operand_cases: {kind, kind@facet, x: ratio}, and under "twin:kind" the
    distance of the reference's own float64 twin from eval_operand over all cells."""
    m = build_mesh(case)
    tabs = facet_tabs(m)
    lists, flists = entity_lists(m), facet_lists(m)
    tables = (m.dofmap, m.geom_dofmap, m.x, m.phi, m.dphi, m.dpsi)
    out = {}

    def update(key, ratio):
        out[key] = max(out.get(key, 0.0), ratio)

    ref, mag = ref_coordinate(m)
    update("x", worst_ratio(ref_coordinate(m, dtype=np.float64)[0], ref, mag))
    for bs in block_sizes(m.gdim):
        for u in fields(case, m, bs).values():
            for kind in kinds_of(m.gdim, bs):
                ref, mag = ref_operand(m, kind, bs, u)
                got = eval_operand(KIND_ID[kind], bs, u, *tables)
                update(kind, worst_ratio(got, ref, mag))
                update("twin:" + kind, worst_ratio(ref_operand(m, kind, bs, u, dtype=np.float64)[0], got, mag))
                for cells in lists.values():
                    if len(cells):
                        update(kind, worst_ratio(eval_operand(KIND_ID[kind], bs, u, *tables, cells), ref[cells], mag[cells]))
                for ents in flists.values():
                    ref_f, mag_f = ref_operand_facets(m, kind, bs, u, *tabs, ents)
                    got = eval_operand_facets(KIND_ID[kind], bs, u, m.dofmap, m.geom_dofmap, m.x, *tabs, ents)
                    update(kind + "@facet", worst_ratio(got, ref_f, mag_f))
    return out


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_float64_oracle_stays_within_c_ref_of_the_long_double_reference(case):
    """oracle.operand_oracle.eval_operand / eval_operand_facets and the float64 twin of ref_coordinate against the long-double
    reference on every mesh, block size, field, entity list and facet list of the GPU file: |f64[k] - ref[k]| <= C_REF * 2^-53 * mag[k]
    in every entry; and the reference's own float64 twin equals eval_operand to within the same C_REF.

    Measured worst ratio per element over its meshes (sizes a-e; `gauss3`: the 3-point-per-direction rule), x86-64 long double, cells
    (the gradient kinds value_grad = grad; facets in operand_cases.py):

        element                  value    grad     eps       F       C      I1    detF     div       x
        triangle P1               2.24    2.98    2.88    2.53    3.12    2.19    2.30    2.16    2.01
        triangle P2               2.61    3.96    3.04    2.80    2.91    1.80    1.42    2.03    2.01
        quadrilateral Q1          3.20   31.06   26.44   25.24   14.78    8.26    5.48   12.07    2.38
        quadrilateral Q2          3.77   25.25   20.41   25.25   12.19    7.56    9.39   20.39    2.38
        tetrahedron P1            2.70    4.54    3.74    3.23    2.76    1.25    2.48    1.44    2.07
        tetrahedron P2            2.88    3.94    2.73    3.35    2.94    1.14    0.78    1.52    2.07
        hexahedron Q1             3.18   11.47    8.66   11.47    3.54    2.45    2.26    3.90    3.10
        hexahedron Q2             4.06    7.42    6.40    6.46    3.32    1.40    1.41    3.52    3.10
        quadrilateral Q1 gauss3   2.33   14.68   14.68    6.59    4.56    1.97    1.75    3.20    2.07
        quadrilateral Q2 gauss3   2.63   19.66   14.29   16.82    8.01    2.17    1.96    5.96    2.07
        hexahedron Q1 gauss3      3.08    8.64    5.18    8.64    2.93    1.79    2.21    4.12    2.54
        hexahedron Q2 gauss3      4.31   44.59   44.59   36.71   10.85    1.96    2.11    4.92    2.54

    The large figures are the non-affine cells, where J is a difference of coordinates that mag does not contain."""
    got = float64_ratios(case)
    print(case_id(case), element_name(case), " ".join(f"{k}={v:.2f}" for k, v in got.items()))
    for k, v in got.items():
        assert v <= C_REF[k.replace("twin:", "")], (k, v)


def test_c_ref_is_within_a_factor_two_of_what_is_measured():
    """A stale or generous constant fails: every C_REF figure is at least the worst ratio over ALL_CASES and at most twice it."""
    worst = {}
    for case in ALL_CASES:
        for k, v in float64_ratios(case).items():
            if not k.startswith("twin:"):
                worst[k] = max(worst.get(k, 0.0), v)
    assert set(worst) == set(C_REF)
    for k, v in worst.items():
        print(f"{k:18s} measured {v:6.2f}   C_REF {C_REF[k]:5.1f}")
        assert v <= C_REF[k] <= 2.0 * v, (k, v, C_REF[k])


def test_the_det_field_puts_det_f_through_zero():
    """The field "det" of size b does what operand_cases.fields says: det F is negative at points of some cells (measured: 23 of 24
    triangles, all 18 quadrilaterals, 63 of 72 tetrahedra, all 12 hexahedra) and positive at others, of size 1 either way, and at its
    smallest less than 1e-3 of its mag (measured 2e-4 to 2e-5): the cofactor expansion cancels."""
    for cell in SIZES:
        case = resolution_case(cell)
        m = build_mesh(case)
        det, mag = ref_operand(m, "detF", m.gdim, fields(case, m, m.gdim)["det"])
        neg = (det < 0).any(axis=(1, 2)).sum()
        print(cell, f"{neg} of {m.num_cells} cells with det F < 0 at a point, det F in [{float(det.min()):.2f}, {float(det.max()):.2f}], "
                    f"least |det F| / mag {float(np.min(np.abs(det) / mag)):.2e}")
        assert neg >= m.num_cells // 2 and det.min() < -0.5 and det.max() > 0.5
        assert float(np.min(np.abs(det) / mag)) < 1e-3


# ------------------------------------------------------------------------------------------------ polynomial known answers
def _exact_coefficients(cell, degree):
    """Monomial coefficients of the Lagrange basis on the lattice nodes of tools.synthetic, by Gauss-Jordan in rational arithmetic:
    (exponents, coeff) with phi_a = sum_m coeff[m, a] x^e_m. For degrees 1 and 2 the entries are dyadic, so exact in long double."""
    from tools.synthetic import _exponents, _lattice_nodes

    ex = _exponents(cell, degree)
    nodes = [[Fraction(int(round(v * degree)), degree) for v in p] for p in _lattice_nodes(cell, degree)]
    n = len(nodes)
    A = [[functools.reduce(lambda a, b: a * b, (x ** int(e) for x, e in zip(p, em)), Fraction(1)) for em in ex] +
         [Fraction(int(i == r)) for i in range(n)] for r, p in enumerate(nodes)]
    for col in range(n):
        piv = next(r for r in range(col, n) if A[r][col] != 0)
        A[col], A[piv] = A[piv], A[col]
        A[col] = [v / A[col][col] for v in A[col]]
        for r in range(n):
            if r != col and A[r][col] != 0:
                A[r] = [v - A[r][col] * w for v, w in zip(A[r], A[col])]
    return ex, [row[n:] for row in A]


def _to_ld(v):
    """A Fraction as a long double, within 0.52 ulp: the quotient truncated to 70 bits, handed over in two halves that a double holds."""
    if v == 0:
        return LD(0)
    n, d = abs(v.numerator), v.denominator
    shift = 70 - (n.bit_length() - d.bit_length())
    q = (n << shift) // d if shift >= 0 else n // (d << -shift)
    out = np.ldexp(np.ldexp(LD(q >> 32), 32) + LD(q & 0xFFFFFFFF), -shift)
    return -out if v < 0 else out


def _tabulate_ld(cell, degree, points):
    """phi (npts, nd), dphi (npts, nd, tdim): the basis at the float64 points in exact rational arithmetic (the monomial form
    cancels, so long double alone would lose a few bits here), each entry then rounded to long double."""
    ex, coeff = _exact_coefficients(cell, degree)
    pts = [[Fraction(float(v)) for v in p] for p in np.asarray(points, dtype=np.float64)]
    nd, tdim = len(coeff[0]), ex.shape[1]

    def monomial(p, em, deriv):
        out = Fraction(1)
        for k in range(tdim):
            e = int(em[k])
            out *= (e * p[k] ** max(e - 1, 0) if e else Fraction(0)) if deriv == k else p[k] ** e
        return out

    def table(deriv):
        return np.array([[_to_ld(sum(monomial(p, em, deriv) * coeff[mi][a] for mi, em in enumerate(ex))) for a in range(nd)] for p in pts])

    return table(None), np.stack([table(k) for k in range(tdim)], axis=2)


def long_double_mesh(m):
    """The mesh with its tables and field-node positions restated in long double (the float64 tables of tools.synthetic carry their
    own rounding of about 2^-53, which a known-answer test at 2^-58 would see)."""
    from tools.synthetic import LagrangeElement

    phi, dphi = _tabulate_ld(m.cell, m.degree, m.points)
    psi, dpsi = _tabulate_ld(m.cell, 1, m.points)
    psi_nodes, _ = _tabulate_ld(m.cell, 1, LagrangeElement(m.cell, m.degree).nodes)
    node_x = np.zeros(m.node_x.shape, dtype=LD)
    node_x[m.dofmap.reshape(-1)] = np.einsum("av,cvj->caj", psi_nodes, np.asarray(m.x, dtype=LD)[m.geom_dofmap]).reshape(-1, m.gdim)
    assert float(np.abs(phi - m.phi).max()) < 1e-14 and float(np.abs(dphi - m.dphi).max()) < 1e-13 and float(np.abs(node_x - m.node_x).max()) < 1e-15
    return types.SimpleNamespace(gdim=m.gdim, num_cells=m.num_cells, nq=m.nq, x=m.x, geom_dofmap=m.geom_dofmap, dofmap=m.dofmap,
                                 phi=phi, dphi=dphi, dpsi=dpsi, psi=psi, node_x=node_x)


@pytest.mark.parametrize("cell", list(SIZES))
@pytest.mark.parametrize("degree", [1, 2])
def test_reference_reproduces_polynomial_known_answers(cell, degree):
    """Polynomial fields of the element's degree (test_operand_eval.py: poly_field, expected, evaluated here in long double) are
    represented exactly, also on the non-affine cells of size b, so their analytic operands at the physical quadrature points are
    the expected output: |ref[k] - exact[k]| <= 64 * 2^-64 * mag[k] in every entry, all nine kinds."""
    m = long_double_mesh(build_mesh(next(c for c in ALL_CASES if c[0] == cell and c[1] == degree and c[4] == "b")))
    xq, _ = ref_coordinate(m)
    for bs in (1, m.gdim):
        u, grad = poly_field(m.gdim, bs, degree, seed=50 + bs)
        uvec = u(m.node_x).reshape(-1)
        assert uvec.dtype == LD and xq.dtype == LD
        for kind in kinds_of(m.gdim, bs):
            ref, mag = ref_operand(m, kind, bs, uvec)
            if kind == "value_grad":
                want = np.concatenate([expected("value", grad(xq), u(xq)), expected("grad", grad(xq), u(xq))], axis=2)
            elif kind == "detF":          # expected() takes np.linalg.det, which has no long double
                want = ref_det(grad(xq) + np.eye(m.gdim))
            elif kind == "eps":           # expected() scales the shear slots by the float64 sqrt(2) / 2
                want = expected("eps", grad(xq), None)
                want[..., 3:] *= (np.sqrt(LD(2)) / 2) / (np.sqrt(2.0) * 0.5)
            else:
                want = expected(kind, grad(xq), u(xq))
            assert want.dtype == LD and want.shape == ref.shape
            r = worst_ratio(want, ref, mag) * 2.0 ** -53 / 2.0 ** -64
            print(f"{cell} degree {degree} bs {bs} {kind}: {r:.2f} * 2^-64 * mag")
            assert r <= 64.0, (kind, bs, r)


def ref_det(F):
    G = F.shape[-1]
    if G == 2:
        return (F[..., 0, 0] * F[..., 1, 1] - F[..., 0, 1] * F[..., 1, 0])[..., None]
    return (F[..., 0, 0] * (F[..., 1, 1] * F[..., 2, 2] - F[..., 1, 2] * F[..., 2, 1])
            - F[..., 0, 1] * (F[..., 1, 0] * F[..., 2, 2] - F[..., 1, 2] * F[..., 2, 0])
            + F[..., 0, 2] * (F[..., 1, 0] * F[..., 2, 1] - F[..., 1, 1] * F[..., 2, 0]))[..., None]


# ------------------------------------------------------------------------------------------------ lists and facets name rows
@pytest.mark.parametrize("cell", list(SIZES))
def test_entity_lists_and_facets_name_rows_of_the_all_cells_result(cell):
    """ref_operand through an entity list returns the rows of its all-cells result bit for bit (value and mag; repeats, one cell, the
    empty list's shape), ref_coordinate likewise, and ref_operand_facets returns, for a pair (cell, f), the cell's row of the
    all-cells result of the mesh tabulated at local facet f's points. This is what lets the GPU file index one reference."""
    case = resolution_case(cell)
    m = build_mesh(case)
    tabs = facet_tabs(m)
    G = m.gdim
    for bs in (G, 5):
        u = fields(case, m, bs)["rough"]
        for kind in kinds_of(G, bs):
            ref, mag = ref_operand(m, kind, bs, u)
            assert ref.shape == mag.shape == (m.num_cells, m.nq, value_size(kind, bs, G)) and ref.dtype == LD
            for name, cells in entity_lists(m).items():
                sub, sub_mag = ref_operand(m, kind, bs, u, cells)
                assert sub.shape == (len(cells), m.nq, ref.shape[2]), name
                assert np.array_equal(sub, ref[cells]) and np.array_equal(sub_mag, mag[cells]), (kind, bs, name)
            per_facet = [ref_operand(dataclasses.replace(m, phi=tabs[0][f], dphi=tabs[1][f], dpsi=tabs[2][f]), kind, bs, u) for f in range(len(tabs[0]))]
            for name, ents in facet_lists(m).items():
                got, got_mag = ref_operand_facets(m, kind, bs, u, *tabs, ents)
                assert got.shape == (len(ents), tabs[0].shape[1], ref.shape[2])
                for row, (c, f) in enumerate(ents):
                    assert np.array_equal(got[row], per_facet[f][0][c]) and np.array_equal(got_mag[row], per_facet[f][1][c]), (kind, bs, name, row)
    xq, xmag = ref_coordinate(m)
    for name, cells in entity_lists(m).items():
        sub, sub_mag = ref_coordinate(m, cells)
        assert sub.shape == (len(cells), m.nq, G) and np.array_equal(sub, xq[cells]) and np.array_equal(sub_mag, xmag[cells])
    assert ref_operand_facets(m, "grad", 1, np.zeros(m.node_x.shape[0]), *tabs, np.empty((0, 2), dtype=np.int32))[0].shape == (0, tabs[0].shape[1], G)
    # entries whose mag is 0 are exact zeros: the zz slot of 2-D eps
    if G == 2:
        e, e_mag = ref_operand(m, "eps", 2, fields(case, m, 2)["offset"])
        assert np.all(e[..., 2] == 0) and np.all(e_mag[..., 2] == 0) and np.all(e_mag[..., [0, 1, 3]] > 0)


# ------------------------------------------------------------------------------------------------ what the bound resolves
@functools.lru_cache(maxsize=None)
def scaled_cell_miss(cell, kind, p):
    """-> (miss, old_ok): the float64 oracle fed the field "rough" with the dofs of cell 0's nodes scaled by 1 + 10^-p, against the
    reference of the unscaled field: its worst ratio as a multiple of MARGIN * C_REF[kind], and whether it still meets
    max|got - ref| <= 1e-13 max|ref| (test_operand_eval.py's criterion)."""
    case = resolution_case(cell)
    m = build_mesh(case)
    u = fields(case, m, m.gdim)["rough"]
    ref, mag = ref_operand(m, kind, m.gdim, u)
    got = eval_operand(KIND_ID[kind], m.gdim, scale_one_cell(m, u, m.gdim, p), m.dofmap, m.geom_dofmap, m.x, m.phi, m.dphi, m.dpsi)
    ref64 = ref.astype(np.float64)
    return worst_ratio(got, ref, mag) / (MARGIN * C_REF[kind]), bool(np.abs(got - ref64).max() <= 1e-13 * np.abs(ref64).max())


@pytest.mark.parametrize("kind", CELL_KINDS)
def test_resolves_is_the_finest_relative_error_in_one_cell_that_misses_the_bound(kind):
    """operand_cases.RESOLVES[kind] = p: with one cell's dofs scaled by 1 + 10^-p the float64 oracle misses MARGIN * C_REF[kind] on
    each of the four quadratic size-b meshes, and with 1 + 10^-(p + 1) it is back inside on at least one of them. Wherever p >= 13
    the same result still passes the max-norm criterion of test_operand_eval.py: the gap the componentwise bound closes."""
    p = RESOLVES[kind]
    at_p = {cell: scaled_cell_miss(cell, kind, p) for cell in SIZES}
    finer = {cell: scaled_cell_miss(cell, kind, p + 1) for cell in SIZES}
    print(kind, "p =", p, {c: round(v[0], 2) for c, v in at_p.items()}, "p + 1:", {c: round(v[0], 2) for c, v in finer.items()})
    assert all(miss > 1.0 for miss, _ in at_p.values())
    assert any(miss <= 1.0 for miss, _ in finer.values())
    if p >= 13:
        assert all(old_ok for _, old_ok in at_p.values())
    assert set(RESOLVES) == set(CELL_KINDS) and set(itertools.chain(CELL_KINDS, ["x"])) == {k for k in C_REF if "@" not in k}
