"""Meshes, facet rules, entity lists, inputs and bounds shared by tests/test_facet_reference_cpu.py and
tests/test_facet_reference_gpu.py (not a test module).

The bound of both files is componentwise: |got[k] - ref[k]| <= c * 2^-53 * mag[k] for EVERY entry k of a facet result, with ref and
mag from oracle/facet_reference.py (long double); entries with mag = 0 must be exact. c is not tuned on the kernels: C_REF below is
what float64 NumPy itself loses against long double on these meshes, rules, lists and inputs (measured and asserted in
test_facet_reference_cpu.py), and the kernels get MARGIN = 8 times that, as in consumer_cases.py.

Workgroup rounds (csrc/facet_form.hip). The vector kernels (facet_element in its four modes) take DXO_BLOCK / nq entities per
workgroup and round, facet_assemble_elem min(DXO_BLOCK / nq, FB_LDS_DOUBLES / (nq * PS)) with PS = (bs * bs * NZ) | 1 parked doubles
per point; vector_epb / assembly_epb restate the two formulas and check_rounds() asserts, for every (rule, trial, bs), that the case
list holds a list shorter than a round, one longer than a round with a ragged tail, and one that is a whole number (> 1) of rounds.
Where a mesh has fewer entities than that, the list `all` is repeated cyclically (a repeated entity is legal); no larger mesh is built.
"""
import contextlib
import functools
import types

import numpy as np

import facet_bilinear_cases
import test_facet_oracle_cpu
from consumer_cases import MARGIN, SIZES, build_mesh  # noqa: F401  (MARGIN: shared with the test modules)
from facet_bilinear_cases import entity_list, trial_cases, value_size
from oracle import facet_reference as R
from tools.synthetic import (LagrangeElement, facet_geometry, facet_points_in_cell, facet_quadrature_degree2,
                             gauss_tensor_rule)

DXO_BLOCK, FB_LDS_DOUBLES = 256, 64 * 1024 // 8
RULES = ("deg2", "gauss3", "gauss3x3", "strang6")


# ------------------------------------------------------------------------------------------------ cases: (cell, degree, size, mirror, rule)
def _cases():
    out = [(cell, degree, s, False, "deg2") for cell in SIZES for degree in (1, 2) for s in "abd"]
    out += [(cell, degree, "b", True, "deg2") for cell in SIZES for degree in (1, 2)]                 # det J < 0 in every cell
    out += [(cell, degree, "b", False, "gauss3") for cell in ("triangle", "quadrilateral") for degree in (1, 2)]
    out += [("hexahedron", degree, "b", False, "gauss3x3") for degree in (1, 2)]
    out += [("tetrahedron", degree, "b", False, "strang6") for degree in (1, 2)]
    return out


ALL_CASES = _cases()


def case_id(case):
    cell, degree, size, mirror, rule = case
    return f"{cell}-{'PQ'[cell in ('quadrilateral', 'hexahedron')]}{degree}-{size}{'x'.join(map(str, SIZES[cell][size]))}" + \
        ("-mirrored" if mirror else "") + (f"-{rule}" if rule != "deg2" else "")


@functools.lru_cache(maxsize=None)
def mesh_of(case):
    cell, degree, size, mirror, _ = case
    m = build_mesh((cell, degree, SIZES[cell][size], None, size))
    return test_facet_oracle_cpu.mirrored(m) if mirror else m


def strang_fix_6():
    """The 6-point rule of degree 4 on the reference triangle (Strang and Fix; Dunavant's table), in closed form: two orbits
    (t, t), (t, 1 - 2t), (1 - 2t, t) with t = (8 - sqrt 10 +- sqrt(38 - 44 sqrt(2/5))) / 18 and the weights
    (620 +- sqrt(213125 - 53320 sqrt 10)) / 7440 (reference area 1/2). test_facet_reference_cpu.py checks every monomial up to degree 4."""
    s10, root = np.sqrt(10.0), np.sqrt(38.0 - 44.0 * np.sqrt(0.4))
    wroot = np.sqrt(213125.0 - 53320.0 * s10)
    pts, w = [], []
    for t, wt in (((8.0 - s10 + root) / 18.0, (620.0 + wroot) / 7440.0), ((8.0 - s10 - root) / 18.0, (620.0 - wroot) / 7440.0)):
        pts += [[t, t], [t, 1.0 - 2.0 * t], [1.0 - 2.0 * t, t]]
        w += [wt] * 3
    return np.array(pts), np.array(w)


def facet_rule(cell, rule):
    """(points on the reference facet (nq, tdim - 1), weights (nq,))."""
    if rule == "deg2":
        return facet_quadrature_degree2(cell)
    if rule == "gauss3":                       # 3 points on an edge: 85 entities per round, lane 255 idle
        assert cell in ("triangle", "quadrilateral")
        t, w = np.polynomial.legendre.leggauss(3)
        return (0.5 * (t + 1.0))[:, None], 0.5 * w
    if rule == "gauss3x3":                     # 9 points on a hexahedron face: 28 entities per round, four idle lanes
        assert cell == "hexahedron"
        return gauss_tensor_rule("quadrilateral", 3)
    if rule == "strang6":                      # 6 points on a tetrahedron face: 42 entities per round, four idle lanes
        assert cell == "tetrahedron"
        return strang_fix_6()
    raise ValueError(rule)


@functools.lru_cache(maxsize=None)
def rule_tables(case):
    """-> (tabs, geom, ref_points): tabs = (phi_f, dphi_f, dpsi_f) and geom = (weights, ref_normals, ref_jacobians) as
    DeviceMesh.set_facet_tables / set_facet_geometry take them, for the case's element at the case's facet rule."""
    cell, degree, _, _, rule = case
    fpts, w = facet_rule(cell, rule)
    pts = facet_points_in_cell(cell, fpts)
    fe, geo = LagrangeElement(cell, degree), LagrangeElement(cell, 1)
    tabs = [fe.tabulate(p) for p in pts]
    _, nref, jref = facet_geometry(cell)
    out = ((np.array([t[0] for t in tabs]), np.array([t[1] for t in tabs]), np.array([geo.tabulate(p)[1] for p in pts])),
           (np.ascontiguousarray(w), nref, jref), pts)
    for group in out[:2]:
        for a in group:
            a.setflags(write=False)
    return out


@contextlib.contextmanager
def float64_oracles_at(case):
    """The float64 facet oracles (tests/test_facet_oracle_cpu.py, tests/facet_bilinear_cases.py) look their tables up by name, at the
    degree-2 rule; inside this block the names give the case's rule, so that the same oracles serve every rule."""
    tabs, geom, pts = rule_tables(case)
    saved = (test_facet_oracle_cpu.facet_tables, test_facet_oracle_cpu.facet_geometry, facet_bilinear_cases.facet_tables)
    test_facet_oracle_cpu.facet_tables = facet_bilinear_cases.facet_tables = lambda m: tabs + (pts,)
    test_facet_oracle_cpu.facet_geometry = lambda cell: geom
    try:
        yield
    finally:
        test_facet_oracle_cpu.facet_tables, test_facet_oracle_cpu.facet_geometry, facet_bilinear_cases.facet_tables = saved


# ------------------------------------------------------------------------------------------------ workgroup rounds
def vector_epb(nq):
    """Entities per workgroup and round of facet_element (every mode): epb = DXO_BLOCK / nqf."""
    return DXO_BLOCK // nq


def assembly_epb(nq, G, trial, bs):
    """The same of facet_assemble_elem: min(DXO_BLOCK / nqf, FB_LDS_DOUBLES / (nqf * ps)), ps = fb_block_stride = (BS * BS * NZ) | 1,
    NZ = facet_nz = one value slot where the kind has a value, G gradient slots where it has a gradient ("F" runs as "grad")."""
    nz = (1 if trial in ("value", "value_grad") else 0) + (G if trial != "value" else 0)
    return min(DXO_BLOCK // nq, FB_LDS_DOUBLES // (nq * ((bs * bs * nz) | 1)))


def nq_of(case):
    return rule_tables(case)[1][0].size


def round_sizes(case):
    """Every entities-per-round figure a kernel takes on this case, ascending."""
    G, nq = mesh_of(case).gdim, nq_of(case)
    return sorted({vector_epb(nq)} | {assembly_epb(nq, G, trial, bs) for trial, bs in trial_cases(G)})


def carries_round_lists(case):
    """The mesh that carries the lists sized by the rounds: size d for the degree-2 rule, the size-b mesh of every other rule."""
    return not case[3] and (case[2] == "d" if case[4] == "deg2" else True)


def _cycled(ents, n):
    return np.ascontiguousarray(ents[np.arange(n) % len(ents)])


@functools.lru_cache(maxsize=None)
def entity_lists(case):
    """name -> (n, 2) int32 (cell, local facet): the whole boundary; a shuffled two thirds of it; every local facet of every cell (a
    cell carries several entities, interior nodes are touched from both sides); a list with one entity three times; one entity; the
    empty list; and, on the mesh that carries them, `all` cut or repeated cyclically to 2 * epb (whole rounds) and epb + 3 (a ragged
    second round) entities for every epb of round_sizes."""
    m = mesh_of(case)
    ext, everything = entity_list(m, "exterior"), entity_list(m, "all")
    rep = np.concatenate([ext[:4], ext[1:2], ext[-1:], ext[1:2]])
    out = {"exterior": ext, "subset": entity_list(m, "subset"), "all": everything, "repeated": np.ascontiguousarray(rep),
           "single": np.ascontiguousarray(ext[len(ext) // 2:len(ext) // 2 + 1]), "empty": np.zeros((0, 2), dtype=np.int32)}
    if carries_round_lists(case):
        for epb in round_sizes(case):
            for n in (2 * epb, epb + 3):
                out[f"all{n}"] = _cycled(everything, n)
    for a in out.values():
        a.setflags(write=False)
    return out


def check_rounds():
    """-> report lines; asserts what the module docstring promises, per (cell, rule, trial, bs) and kernel family, over ALL_CASES."""
    lines = []
    for cell, rule in sorted({(c[0], c[4]) for c in ALL_CASES}):
        cases = [c for c in ALL_CASES if c[0] == cell and c[4] == rule]
        lengths = sorted({len(e) for c in cases for e in entity_lists(c).values() if len(e)})
        G, nq = mesh_of(cases[0]).gdim, nq_of(cases[0])
        families = {("vector", "*", 0): vector_epb(nq)}
        families.update({("assembly", trial, bs): assembly_epb(nq, G, trial, bs) for trial, bs in trial_cases(G)})
        for (family, trial, bs), epb in families.items():
            below = [n for n in lengths if n < epb]
            ragged = [n for n in lengths if n > epb and n % epb]
            whole = [n for n in lengths if n > epb and n % epb == 0]
            assert below and ragged and whole, (cell, rule, family, trial, bs, epb, lengths)
            lines.append(f"{cell:13s} {rule:8s} nq {nq} {family:8s} {trial:10s} bs {bs} epb {epb:3d}: below {below[-1]}, ragged {ragged[0]}"
                         f" .. {ragged[-1]}, whole {whole}")
    return lines


# ------------------------------------------------------------------------------------------------ inputs
def _rng(case, list_name, salt):
    return np.random.Generator(np.random.PCG64([ALL_CASES.index(case), sorted(entity_lists(case)).index(list_name), salt]))


def rows_scaled(C):
    """C with row i of every point's block scaled by 10^(3 i): small entries beside large ones."""
    return C * (10.0 ** (3 * np.arange(C.shape[2])))[None, None, :, None]


def work_items(case, list_name):
    """The calls of one (case, entity list), each a namespace (entry, what, kind, bs, variant, arrays...):
      geometry                  what = "geometry"
      pressure                  variants "p" (scale 1), "p=NULL", "scale" (p, scale = -2.5)
      adjoint:<kind>            every kind with every block size it takes, S ~ N(0, 1)
      apply:<trial>             variants "" (C, v ~ N(0, 1)), "rows" (rows of C scaled by 10^(3 i)), "offset" (v + 1e6: the gradient kinds
                                cancel terms of size 1e6 / h, and mag grows with them)
      diag:<trial>, matrix:<trial>   variants "" and "rows"; no matrix on the list `all` of size d (500 to 650 entities, up to 3.3
                                million element-matrix entries to scatter in long double per call: the lists of 2 * epb and epb + 3
                                entities put the same mesh through whole and ragged rounds)
    and r0 ~ N(0, 1), what the output holds before the call. All seeded by (case, list, call)."""
    m = mesh_of(case)
    G, nn, nq = m.gdim, m.node_x.shape[0], nq_of(case)
    ents = entity_lists(case)[list_name]
    n = len(ents)
    ns = types.SimpleNamespace
    items = [ns(entry="geometry", what="geometry", kind=None, bs=0, variant="")]
    rng = _rng(case, list_name, 1)
    p, r0 = rng.normal(size=(n, nq)), rng.normal(size=nn * G)
    items += [ns(entry="pressure", what="pressure", kind=None, bs=G, variant="p", p=p, scale=1.0, r0=r0),
              ns(entry="pressure", what="pressure", kind=None, bs=G, variant="p=NULL", p=None, scale=1.0, r0=r0),
              ns(entry="pressure", what="pressure", kind=None, bs=G, variant="scale", p=p, scale=-2.5, r0=r0)]
    for k, (kind, bs) in enumerate(trial_cases(G)):
        rng = _rng(case, list_name, 10 + k)
        D = value_size(kind, G, bs)
        S, C, v, r0 = rng.normal(size=(n, nq, D)), rng.normal(size=(n, nq, bs, D)), rng.normal(size=nn * bs), rng.normal(size=nn * bs)
        items.append(ns(entry=f"adjoint:{kind}", what="adjoint", kind=kind, bs=bs, variant="", S=S, r0=r0))
        Cr = rows_scaled(C)
        items += [ns(entry=f"apply:{kind}", what="apply", kind=kind, bs=bs, variant="", C=C, v=v, r0=r0),
                  ns(entry=f"apply:{kind}", what="apply", kind=kind, bs=bs, variant="rows", C=Cr, v=v, r0=r0),
                  ns(entry=f"apply:{kind}", what="apply", kind=kind, bs=bs, variant="offset", C=C, v=v + 1e6, r0=r0)]
        for what in ("diag", "matrix"):
            if what == "matrix" and case[2] == "d" and list_name == "all":
                continue
            items += [ns(entry=f"{what}:{kind}", what=what, kind=kind, bs=bs, variant="", C=C, r0=r0),
                      ns(entry=f"{what}:{kind}", what=what, kind=kind, bs=bs, variant="rows", C=Cr, r0=r0)]
    return items


def item_id(item):
    return f"{item.entry}" + (f" bs {item.bs}" if item.kind else "") + (f" [{item.variant}]" if item.variant else "")


# ------------------------------------------------------------------------------------------------ the two sides on the CPU
def reference(case, ents, item, dtype=R.LD):
    """-> {entry: (ref, mag)} of one work item from oracle.facet_reference; "matrix:<trial>" gives the ELEMENT matrices (n, nd * bs,
    nd * bs), which the caller scatters (R.scatter_dense, R.scatter_csr)."""
    m = mesh_of(case)
    tabs, geom, _ = rule_tables(case)
    if item.what == "geometry":
        n, n_mag, dS, dS_mag = R.ref_facet_geometry(m, tabs, geom, ents, dtype)
        return {"normal": (n, n_mag), "dS": (dS, dS_mag)}
    if item.what == "pressure":
        return {item.entry: R.ref_facet_pressure(m, tabs, geom, ents, item.p, item.scale, dtype)}
    if item.what == "adjoint":
        return {item.entry: R.ref_facet_adjoint(m, tabs, geom, ents, item.kind, item.bs, item.S, dtype)}
    if item.what == "apply":
        return {item.entry: R.ref_facet_bilinear_apply(m, tabs, geom, ents, item.kind, item.bs, item.C, item.v, dtype)}
    if item.what == "diag":
        return {item.entry: R.ref_facet_bilinear_diagonal(m, tabs, geom, ents, item.kind, item.bs, item.C, dtype)}
    if item.what == "matrix":
        return {item.entry: R.ref_facet_bilinear_elements(m, tabs, geom, ents, item.kind, item.bs, item.C, dtype)}
    raise ValueError(item.what)


@functools.lru_cache(maxsize=None)
def pattern_of(case, bs):
    """(indptr, indices, rows, indices) of the mesh's blocked CSR pattern as oracle.form_oracle.pattern_ref states it (the device
    pattern is compared with it in tests/test_assemble_gpu.py); rows = the row of every entry."""
    from oracle.form_oracle import pattern_ref

    indptr, indices = pattern_ref(mesh_of(case), bs)
    return indptr, indices, np.repeat(np.arange(indptr.size - 1), np.diff(indptr)), indices


def on_pattern(case, ents, bs, Ke):
    """Element matrices (or their mags) scattered into the entries of pattern_of(case, bs)."""
    return R.scatter_csr(mesh_of(case), ents, bs, Ke, *pattern_of(case, bs)[:2])


def float64_side(case, ents, item):
    """-> {entry: float64 result} of the same work item from the float64 oracles the suite already trusts (see C_REF below);
    "matrix:<trial>" gives the values on the entries of pattern_of (the dense oracle's matrix must vanish outside them)."""
    m = mesh_of(case)
    KIND = facet_bilinear_cases.KIND_ID
    with float64_oracles_at(case):
        if item.what == "geometry":
            n, dS = test_facet_oracle_cpu.facet_geometry_ref(m, ents)
            return {"normal": n, "dS": dS}
        if item.what == "pressure":
            return {item.entry: test_facet_oracle_cpu.facet_pressure_ref(m, ents, item.p, item.scale)}
        if item.what == "adjoint":
            return {item.entry: test_facet_oracle_cpu.facet_adjoint_ref(m, ents, KIND[item.kind], item.bs, item.S)}
        if item.what == "apply":
            return {item.entry: facet_bilinear_cases.facet_bilinear_apply_ref(m, ents, item.kind, item.bs, item.C, item.v)}
        if item.what == "matrix" and len(ents) <= DENSE_ORACLE_LIMIT:
            K = facet_bilinear_cases.facet_bilinear_dense_ref(m, ents, item.kind, item.bs, item.C)
            rows, indices = pattern_of(case, item.bs)[2:]
            values = K[rows, indices]
            assert np.count_nonzero(K) == np.count_nonzero(values), "the dense oracle has an entry outside the pattern"
            return {item.entry: values}
    twin = reference(case, ents, item, dtype=np.float64)[item.entry][0]
    return {item.entry: on_pattern(case, ents, item.bs, twin) if item.what == "matrix" else twin}


def old_criterion(got, ref):
    """max|got - ref| <= 1e-12 max|ref|: what tests/test_facet_form_gpu.py and tests/test_facet_bilinear_gpu.py ask."""
    ref = np.asarray(ref, dtype=np.float64)
    return bool(np.abs(np.asarray(got, dtype=np.float64) - ref).max() <= 1e-12 * np.abs(ref).max())


# ------------------------------------------------------------------------------------------------ bounds
# What float64 NumPy loses against oracle.facet_reference, in units of 2^-53 * mag[k], at the worst entry over every case of
# ALL_CASES, every entity list and every input variant above; rounded up from the figures test_facet_reference_cpu.py measures, which
# asserts that they still hold and that none is more than twice what is measured. The float64 side is the existing oracle:
#   normal, dS   facet_geometry_ref;  pressure  facet_pressure_ref;  adjoint:<kind>  facet_adjoint_ref   (tests/test_facet_oracle_cpu.py)
#   apply:<trial>  facet_bilinear_apply_ref;  matrix:<trial>  facet_bilinear_dense_ref, every entry of the pattern
#                  (tests/facet_bilinear_cases.py; lists of more than DENSE_ORACLE_LIMIT entities: the float64 twin of
#                  ref_facet_bilinear_elements scattered by scatter_csr, because the dense oracle forms one operand evaluation per column)
#   diag:<trial>   the float64 twin of ref_facet_bilinear_diagonal (no float64 oracle of the diagonal exists)
# and in every entry the float64 twin of the reference is held to the same figure.
DENSE_ORACLE_LIMIT = 40
# Measured (x86-64 long double) and the case that gives each figure. The value kinds carry no K; the gradient kinds' mag contains
# K_mag = |K| + |K| J_mag |K| (oracle/facet_reference.py), which is why their figures are near or below 1.
#   normal  1.04  P1 tetrahedra 3x3x3, all        dS  2.19  Q1 quadrilaterals 6x3 gauss3, exterior      pressure  4.10  Q2 hexahedra 7x4x3, subset
#                adjoint                      apply                          diag                         matrix
#   value        8.74  Q2 hex 7x4x3 exterior  7.18  Q1 hex 7x4x3 subset      9.79  Q2 hex 7x4x3 subset    11.71  Q2 hex 7x4x3 subset
#   grad         3.06  Q2 hex 7x4x3 subset    1.19  Q2 quad 6x3 gauss3 all   1.29  Q1 quad 13x12 all256    5.95  Q2 hex 7x4x3 exterior
#   value_grad   2.35  Q1 hex 7x4x3 subset    1.02  Q2 quad 6x3 gauss3 ext.  1.93  Q2 quad 6x3 all         5.96  Q2 hex 7x4x3 exterior
#   eps          3.59  Q2 hex 7x4x3 subset    1.09  Q2 quad 1x1 subset       1.38  P2 tet 3x3x3 all76      5.25  Q2 hex 7x4x3 exterior
#   div          2.52  Q2 hex 7x4x3 subset    1.18  Q2 quad 6x3 gauss3 sub.  1.82  P2 tri 10x10 subset     5.34  Q2 hex 7x4x3 exterior
#   F            2.89  Q2 hex 7x4x3 exterior  0.99  Q2 quad 13x12 all        1.34  P2 tri 10x10 repeated  21.51  Q2 hex 1x1x1 single
# matrix:F is the dense oracle's: it evaluates F = I + grad e_c and subtracts I again, which costs 2^-53 of 1 where the entry is small.
C_REF = {"normal": 1.1, "dS": 2.3, "pressure": 4.2,
         "adjoint:value": 8.8, "adjoint:grad": 3.2, "adjoint:value_grad": 2.4, "adjoint:eps": 3.7, "adjoint:div": 2.6, "adjoint:F": 3.0,
         "apply:value": 7.3, "apply:grad": 1.3, "apply:value_grad": 1.1, "apply:eps": 1.2, "apply:div": 1.3, "apply:F": 1.1,
         "diag:value": 9.9, "diag:grad": 1.4, "diag:value_grad": 2.0, "diag:eps": 1.5, "diag:div": 1.9, "diag:F": 1.4,
         "matrix:value": 11.8, "matrix:grad": 6.0, "matrix:value_grad": 6.1, "matrix:eps": 5.3, "matrix:div": 5.4, "matrix:F": 21.6}
# The finest relative error in one entity that the bound resolves: the largest integer p for which the float64 oracle, fed S / C / p
# whose values on entity 0 are scaled by 1 + 10^-p, still misses MARGIN * C_REF[entry] against the reference of the unscaled input on
# every one of the four quadratic size-b meshes (the whole boundary, bs = gdim, the plain inputs). Measured in
# test_facet_reference_cpu.py: at p = 13 every entry misses by a factor 1.15 (apply:div, tetrahedra) to 27.8 (apply:value_grad,
# triangles); at 14 only adjoint:div (1.28 to 2.17), matrix:eps (1.07 to 1.11) and matrix:div (1.05 to 1.09) still miss on all four. At
# that p every result still meets max|got - ref| <= 1e-12 max|ref|, the criterion of the older facet tests.
RESOLVES = {k: 13 for k in C_REF if k not in ("normal", "dS")}
RESOLVES.update({"adjoint:div": 14, "matrix:eps": 14, "matrix:div": 14})
