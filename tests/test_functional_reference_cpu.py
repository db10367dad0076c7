"""What the bound of tests/test_functional_gpu.py rests on, checked without a GPU: the constants C_REF and RESOLVES of
tests/functional_cases.py against what the float64 NumPy twin of the long-double reference shows, the lists that straddle the
boundaries of the two passes, closed forms of the reference itself, and the host arithmetic of examples/device_functionals.py."""
import functools
import importlib.util
import math
import pathlib

import numpy as np
import pytest

import facet_reference_cases as FC
import functional_cases as F
from functional_cases import C_REF, RESOLVES, allowed, worst_ratio
from tools.synthetic import structured_mesh

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _seed(*k):
    return tuple(int(x) for x in k)


def twin_ratios():
    """Yields (entry, ratio, where): the float64 twin against the long-double reference, in units of 2^-53 * mag at the worst output
    entry, for every case, list and input of functional_cases."""
    for ic, case in enumerate(F.CELL_CASES):
        m = F.cell_mesh(case)
        for il, (name, cells) in enumerate(F.cell_lists(case).items()):
            il = 0 if name == "arange" else il          # arange gets the inputs of NULL (list 0): the two must agree bit for bit
            where = f"{F.cell_case_id(case)}, {name}"
            n = m.num_cells if cells is None else len(cells)
            ld, f64 = F.ref_cell_measure(m, cells), F.ref_cell_measure(m, cells, np.float64)
            yield "measure", worst_ratio(f64[0], *ld), where
            for item in F.integrate_items(n, m.nq, _seed(1, ic, il)):
                ref, mag = F.ref_integrate(m, item.f, item.g, cells, measure=ld)
                got, _ = F.ref_integrate(m, item.f, item.g, cells, np.float64, measure=f64)
                yield item.entry, worst_ratio(got, ref, mag), f"{where}, {F.item_id(item)}"
            for item in F.moment_items(m, _seed(2, ic, il)):
                ref, mag = F.ref_operand_moments(m, item.kind, item.bs, item.u, cells, measure=ld)
                got, _ = F.ref_operand_moments(m, item.kind, item.bs, item.u, cells, np.float64, measure=f64)
                yield item.entry, worst_ratio(got, ref, mag), f"{where}, {F.item_id(item)}"
    for ic, case in enumerate(F.FACET_CASES):
        m = FC.mesh_of(case)
        tabs, geom, _ = FC.rule_tables(case)
        for il, (name, ents) in enumerate(F.facet_lists(case).items()):
            if len(ents) == 0:
                continue
            where = f"{FC.case_id(case)}, {name}"
            ld, f64 = F.ref_facet_measure(m, tabs, geom, ents), F.ref_facet_measure(m, tabs, geom, ents, np.float64)
            for item in F.integrate_items(len(ents), geom[0].size, _seed(3, ic, il)):
                ref, mag = F.ref_facet_integrate(m, tabs, geom, ents, item.f, item.g, measure=ld)
                got, _ = F.ref_facet_integrate(m, tabs, geom, ents, item.f, item.g, np.float64, measure=f64)
                yield "facet_" + item.entry, worst_ratio(got, ref, mag), f"{where}, {F.item_id(item)}"


@functools.lru_cache(maxsize=None)
def measured_c_ref():
    worst = {}
    for entry, ratio, where in twin_ratios():
        if ratio > worst.get(entry, (-1.0, ""))[0]:
            worst[entry] = (ratio, where)
    return worst


def test_c_ref_holds_and_is_not_padded():
    """C_REF[entry] >= what the float64 twin loses at its worst entry over all cases, and no more than twice that."""
    worst = measured_c_ref()
    for entry, (ratio, where) in sorted(worst.items()):
        print(f"{entry:18s} measured {ratio:6.2f}  C_REF {C_REF.get(entry)}   at {where}")
    assert set(worst) == set(C_REF)
    for entry, (ratio, where) in worst.items():
        assert math.isfinite(ratio), (entry, where)
        assert ratio <= C_REF[entry] <= 2.0 * ratio, (entry, ratio, C_REF[entry], where)


SIZE_B = [c for c in F.CELL_CASES if c[0] == "cells" and c[1][1] == 2 and c[1][4] == "b"]
FACET_SIZE_B = [c for c in F.FACET_CASES if c[1] == 2 and c[2] == "b" and not c[3] and c[4] == "deg2"]


def scaled_twin_ratios(p):
    """Yields (entry, mesh, ratio): the float64 twin fed f (u) scaled by 1 + 10^-p on cell / entity 0 (the dofs of cell 0), against the
    reference of the unscaled input; quadratic size-b meshes, all cells / the whole boundary, the plain inputs."""
    s = 1.0 + 10.0 ** -p
    for ic, case in enumerate(SIZE_B):
        m = F.cell_mesh(case)
        ld, f64 = F.ref_cell_measure(m), F.ref_cell_measure(m, None, np.float64)
        for item in F.integrate_items(m.num_cells, m.nq, _seed(4, ic)):
            if item.variant:
                continue
            f = item.f.copy()
            f[0] *= s
            ref, mag = F.ref_integrate(m, item.f, item.g, measure=ld)
            got, _ = F.ref_integrate(m, f, item.g, None, np.float64, measure=f64)
            yield item.entry, ic, worst_ratio(got, ref, mag)
        for item in F.moment_items(m, _seed(5, ic)):
            if item.variant:
                continue
            u = item.u.reshape(-1, item.bs).copy()
            u[m.dofmap[0]] *= s
            ref, mag = F.ref_operand_moments(m, item.kind, item.bs, item.u, measure=ld)
            got, _ = F.ref_operand_moments(m, item.kind, item.bs, u.reshape(-1), None, np.float64, measure=f64)
            yield item.entry, ic, worst_ratio(got, ref, mag)
    for ic, case in enumerate(FACET_SIZE_B):
        m = FC.mesh_of(case)
        tabs, geom, _ = FC.rule_tables(case)
        ents = F.facet_lists(case)["exterior"]
        ld, f64 = F.ref_facet_measure(m, tabs, geom, ents), F.ref_facet_measure(m, tabs, geom, ents, np.float64)
        for item in F.integrate_items(len(ents), geom[0].size, _seed(6, ic)):
            if item.variant:
                continue
            f = item.f.copy()
            f[0] *= s
            ref, mag = F.ref_facet_integrate(m, tabs, geom, ents, item.f, item.g, measure=ld)
            got, _ = F.ref_facet_integrate(m, tabs, geom, ents, f, item.g, np.float64, measure=f64)
            yield "facet_" + item.entry, ic, worst_ratio(got, ref, mag)


@functools.lru_cache(maxsize=None)
def misses_at(p):
    """entry -> True where EVERY call of the entry on EVERY size-b mesh misses its bound at scaling 1 + 10^-p."""
    out = {}
    for entry, _, ratio in scaled_twin_ratios(p):
        out[entry] = out.get(entry, True) and ratio > allowed(entry)
    return out


def measured_resolves():
    found = {}
    for p in range(16, 5, -1):
        for entry, miss in misses_at(p).items():
            if miss and entry not in found:
                found[entry] = p
    return found


def test_the_bound_resolves_a_relative_error_in_one_cell():
    """RESOLVES[entry] is the largest p at which the twin with one scaled cell / entity still misses the bound on all four meshes."""
    assert len(SIZE_B) == 4 and len(FACET_SIZE_B) == 4
    found = measured_resolves()
    print(found)
    assert found == RESOLVES
    assert set(RESOLVES) == set(C_REF) - {"measure"}


def test_the_lists_straddle_the_pass_boundaries():
    for line in F.check_groups():
        print(line)


@pytest.mark.parametrize("cell", ["triangle", "quadrilateral", "tetrahedron", "hexahedron"])
def test_known_answers_of_the_reference(cell):
    """What the GPU test asks of the kernels, first asked of the long-double reference: int 1 dx is the volume of the structured
    domain (the unit square / cube, distorted inside, its boundary kept), int 1 ds its perimeter / surface, and on undistorted
    meshes the divergence theorem for a quadratic field: int div u dx = int u . n ds."""
    case = next(c for c in FC.ALL_CASES if c[0] == cell and c[1] == 2 and c[2] == "b" and not c[3] and c[4] == "deg2")
    m, (tabs, geom, _) = FC.mesh_of(case), FC.rule_tables(case)         # the distorted size-b quadratic mesh
    G = m.gdim
    vol, _ = F.ref_integrate(m, np.ones((m.num_cells, m.nq, 1)))
    assert abs(float(vol[0]) - 1.0) < 1e-15
    ents = FC.entity_lists(case)["exterior"]
    surf, _ = F.ref_facet_integrate(m, tabs, geom, ents, np.ones((len(ents), geom[0].size, 1)))
    assert abs(float(surf[0]) - 2.0 * G) < 1e-15
    lhs, rhs, bound = divergence_sides(cell, 2)
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


def quadratic_field(x):
    """u_i = sum_j A_ij x_j + x^T Q_i x on the nodes x (n, G): a field the quadratic elements hold exactly."""
    G = x.shape[1]
    rng = np.random.Generator(np.random.PCG64(5))
    A, Q = rng.normal(size=(G, G)), rng.normal(size=(G, G, G))
    return (x @ A.T + np.einsum("nj,ijk,nk->ni", x, Q, x)).reshape(-1)


def divergence_case(cell):
    """(mesh, tabs, geom, ents) of the undistorted size-b quadratic mesh: P1 geometry is affine per cell on simplices, and with
    distort = 0 on quadrilaterals and hexahedra too, so the degree-2 rules integrate both sides exactly."""
    case = next(c for c in FC.ALL_CASES if c[0] == cell and c[1] == 2 and c[2] == "b" and not c[3] and c[4] == "deg2")
    m = structured_mesh(cell, F.CC.SIZES[cell]["b"], 2, distort=0.0, seed=6)
    tabs, geom, _ = FC.rule_tables(case)
    return m, tabs, geom, FC.entity_list(m, "exterior")


def divergence_sides(cell, degree, dtype=F.LD):
    """-> (int div u dx, int u . n ds, the sum of the two sides' bounds) from the long-double reference."""
    from oracle.facet_reference import ref_facet_geometry
    from oracle.operand_reference import ref_operand_facets

    m, tabs, geom, ents = divergence_case(cell)
    G = m.gdim
    u = quadratic_field(m.node_x[:, :G])
    lhs, lmag = F.ref_operand_moments(m, "div", G, u, dtype=dtype)
    val, vmag = ref_operand_facets(m, "value", G, u, *tabs, ents, dtype)
    nrm, nmag, dS, dSm = ref_facet_geometry(m, tabs, geom, ents, dtype)
    rhs = np.einsum("eq,eqi,eqi->", dS, val, nrm)
    rmag = np.einsum("eq,eqi,eqi->", dSm, vmag, nmag)
    eps = F.LD(2.0) ** -53
    return F.LD(lhs[0]), F.LD(rhs), eps * (allowed("moments:div") * lmag[0] + allowed("facet_pair") * rmag)


def test_the_examples_host_arithmetic_matches_the_closed_forms():
    """examples/device_functionals.py compares the device with NumPy quadrature on the host; that quadrature against the closed
    forms of u = x + y on the unit square, at what the rule and the 5 x 5 mesh allow (the degree-2 rule is exact for polynomials of
    degree 2, so int 3 u^2 dx over the cells with x <= 0.2 is exact to rounding; u^3 and cos / sin carry the rule's error)."""
    spec = importlib.util.spec_from_file_location("device_functionals", ROOT / "examples" / "device_functionals.py")
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    host = ex.host_side()
    # over the strip 0 <= x <= 0.2, 0 <= y <= 1 with u = x + y:  int 3 u^2 = (1.2^4 - 1 - 0.2^4) / 4,  int u^3 = (1.2^5 - 1 - 0.2^5) / 20
    assert abs(host["int_3u2_dx"] - (1.2 ** 4 - 1.0 - 0.2 ** 4) / 4.0) < 1e-14
    assert abs(host["int_u3_dx"] - (1.2 ** 5 - 1.0 - 0.2 ** 5) / 20.0) < 2e-4       # f(u^2) = u^3 for u >= 0: degree 3, h = 0.2
    # the boundary of the unit square: int cos(x + y) ds = 2 sin 1 + 2 (sin 2 - sin 1), int sin(x + y) ds = 2 (1 - cos 1) + 2 (cos 1 - cos 2)
    # two Gauss points on an edge of length h: error <= h^5 / 4320 max|g| per edge, 4 / h edges, |g| <= 1
    gauss2 = 4.0 * 0.2 ** 4 / 4320.0
    assert abs(host["int_cos_ds"] - 2.0 * math.sin(2.0)) <= gauss2
    assert abs(host["int_sin_ds"] - 2.0 * (1.0 - math.cos(2.0))) <= gauss2
    assert abs(host["l2_error_sq"] - ex.L2_ERROR_SQ_EXACT) < 1e-14
    assert abs(host["deformed_volume"] - ex.DEFORMED_VOLUME_EXACT) < 1e-14
