"""Meshes, fields, entity lists and bounds shared by tests/test_operand_reference_cpu.py and tests/test_operand_reference_gpu.py (not a
test module).

The bound of both files is componentwise: |got[k] - ref[k]| <= c * 2^-53 * mag[k] for EVERY entry k of an operand array, with ref and
mag from oracle/operand_reference.py (long double); entries with mag = 0 must be exact. c is not tuned on the kernels: C_REF below is
what float64 NumPy itself loses against long double on these meshes, lists and fields (measured and asserted in
test_operand_reference_cpu.py), and the kernels get MARGIN = 8 times that, as in consumer_cases.py.
"""
import numpy as np

from consumer_cases import MARGIN, OTHER_RULES, SIZES, build_mesh, case_id, element_name  # noqa: F401  (shared with the test modules)
from tools.synthetic import FACETS, exterior_facets, facet_tables

# The size letters of consumer_cases.SIZES mean the same here (a wave of operand_eval owns the same 64 // nq cells). Size e is for the
# lane = cell strain kernel of operand_cell.h, whose wave group is 64 CELLS: 8 x 8 quadrilaterals are exactly one group, 8 x 8 boxes of
# two triangles exactly two; sizes b and d (24 / 200 triangles, 18 / 156 quadrilaterals) are its partial and ragged cases.
SIZE_E = {"triangle": (8, 8), "quadrilateral": (8, 8)}
MUST_SERVE = [(cell, degree, SIZES[cell][s], None, s) for cell in SIZES for degree in (1, 2) for s in "abcd"] + \
             [(cell, degree, SIZE_E[cell], None, "e") for cell in SIZE_E for degree in (1, 2)]
ALL_CASES = MUST_SERVE + OTHER_RULES

CELL_KINDS = ("value", "grad", "eps", "F", "value_grad", "C", "I1", "detF", "div")
COMPONENT_KINDS = ("value", "grad", "value_grad")          # defined for a field of any block size, one scalar launch per component


def block_sizes(gdim):
    """Dense kernels: bs = 1 and bs = gdim. Per-component launches (out_stride, u_stride): a bs that is neither."""
    return (1, gdim, 3 if gdim == 2 else 2, 5)


def kinds_of(gdim, bs):
    return CELL_KINDS if bs == gdim else COMPONENT_KINDS


def fields(case, mesh, bs, seed=None):
    """Seeded field vectors of one (case, block size), name -> u (num_field_nodes * bs):
      rough   N(0, 1) * 0.3 * (node spacing), so that grad u = O(1) and F = I + grad u is far from the identity;
      offset  rough + 1e6, a rigid offset: the gradient is a cancellation of terms of size 1e6 / h, and mag grows with them;
      det     size b, bs = gdim only: (A - I) x + rough with A = diag(0.05, 1[, 1]), so that det F = 0.05 + O(1) noise passes through
              zero and is negative in some cells (asserted in test_operand_reference_cpu.py).
    seed: for a case outside ALL_CASES (trip_cases.py), whose place in that list otherwise seeds the draw."""
    nn, G = mesh.node_x.shape[0], mesh.gdim
    rng = np.random.Generator(np.random.PCG64((1000 + 10 * ALL_CASES.index(case) if seed is None else seed) + bs))
    h = 1.0 / (max(case[2]) * case[1])
    rough = rng.normal(size=(nn, bs)) * (0.3 * h)
    out = {"rough": rough.reshape(-1), "offset": (rough + 1e6).reshape(-1)}
    if case[4] == "b" and bs == G:
        A = np.eye(G)
        A[0, 0] = 0.05
        out["det"] = (mesh.node_x @ (A - np.eye(G)).T + rough).reshape(-1)
    return out


def entity_lists(mesh):
    """name -> int32 cell list: the reversed full list, a list with repeats of length cells-per-wave + 1 (a full group and one cell),
    the last cell alone, and the empty list (shape-only result)."""
    nc, cpw = mesh.num_cells, 64 // mesh.nq
    rng = np.random.Generator(np.random.PCG64(77 + nc))
    rep = rng.integers(0, nc, cpw + 1)
    rep[1], rep[-1] = rep[0], rep[0]
    return {"reversed": np.arange(nc - 1, -1, -1, dtype=np.int32), "repeats": rep.astype(np.int32),
            "last": np.array([nc - 1], dtype=np.int32), "empty": np.empty(0, dtype=np.int32)}


def facet_lists(mesh):
    """name -> (n, 2) int32 (cell, local facet): all exterior facets; every local facet of cell 0 and of the last cell, one repeated."""
    nf, last = len(FACETS[mesh.cell]), mesh.num_cells - 1
    local = [(0, f) for f in range(nf)] + [(last, f) for f in range(nf)] + [(last, nf - 1)]
    return {"exterior": exterior_facets(mesh), "local": np.array(local, dtype=np.int32)}


def facet_tabs(mesh):
    """(phi_f, dphi_f, dpsi_f) of the mesh's element at the degree-2 facet rule (tools.synthetic.facet_tables)."""
    return facet_tables(mesh)[:3]


def resolution_case(cell):
    """Quadratic element, size b: where the resolution check of both test files runs."""
    return next(c for c in ALL_CASES if c[0] == cell and c[1] == 2 and c[4] == "b")


def scale_one_cell(mesh, u, bs, p, cell=0):
    """u with the dofs of `cell`'s nodes scaled by 1 + 10^-p."""
    v = np.array(u, dtype=np.float64).reshape(-1, bs)
    v[mesh.dofmap[cell]] *= 1.0 + 10.0 ** -p
    return v.reshape(-1)


# What float64 NumPy loses against oracle.operand_reference, in units of 2^-53 * mag[k], at the worst entry over every mesh of
# ALL_CASES, every block size, field, entity list and facet list above; rounded up from the figures test_operand_reference_cpu.py
# measures, which asserts that they still hold and that none is more than twice what is measured. Cell kinds:
# oracle.operand_oracle.eval_operand; "<kind>@facet": eval_operand_facets; "x": the float64 twin of ref_coordinate.
# Measured (x86-64 long double), cells / facets, and the case that gives the cell figure:
#   value        4.31 /  4.04   Q2 hexahedra gauss3 5x1x1, bs = 5          C      14.78 /  7.41   Q1 quadrilaterals 13x12
#   grad        44.59 / 31.92   Q2 hexahedra gauss3 5x1x1, bs = 3          I1      8.26 /  5.75   Q1 quadrilaterals 13x12
#   value_grad  44.59 / 31.92   the same                                   detF    9.39 /  3.79   Q2 quadrilaterals 13x12
#   eps         44.59 / 24.87   the same                                   div    20.39 /  8.57   Q2 quadrilaterals 13x12
#   F           36.71 / 26.64   the same                                   x       3.1004         Q1 hexahedra 7x4x3
# The facet figures of the gradient kinds come from the 13 x 12 quadrilaterals. As in consumer_cases.py the large figures are the
# rounding of J, a difference of coordinates of size 1 at a spacing of 1 / 13 (or 1 / 5 in one direction of five long hexahedra), which
# mag does not contain and every float64 evaluation, the kernels' included, loses alike; simplices stay below 4.6 (per element: the
# docstring of test_float64_oracle_stays_within_c_ref_of_the_long_double_reference).
C_REF = {"value": 4.4, "grad": 44.6, "value_grad": 44.6, "eps": 44.6, "F": 36.8, "C": 14.8, "I1": 8.3, "detF": 9.4, "div": 20.4, "x": 3.2,
         "value@facet": 4.1, "grad@facet": 32.0, "value_grad@facet": 32.0, "eps@facet": 24.9, "F@facet": 26.7, "C@facet": 7.5,
         "I1@facet": 5.8, "detF@facet": 3.8, "div@facet": 8.6}
# The finest relative error in one cell that the bound resolves: the largest integer p for which the float64 oracle, fed a field whose
# dofs on the nodes of cell 0 are scaled by 1 + 10^-p, still misses MARGIN * C_REF[kind] against the reference of the unscaled field
# on every one of the four quadratic size-b meshes (field "rough", bs = gdim). Measured in test_operand_reference_cpu.py.
# Measured miss at that p, as a multiple of the bound, least of the four meshes (at p + 1 every mesh is back inside the bound):
#   value 1.12 (p = 14; 11.3 at 13)   grad 1.96   eps 1.89   F 2.18   value_grad 1.96   C 4.09   I1 3.84   detF 1.72   div 2.03
# At p = 13 the float64 oracle still meets max|got - ref| <= 1e-13 max|ref|, the criterion of test_operand_eval.py, for every kind.
RESOLVES = {"value": 14, "grad": 13, "eps": 13, "F": 13, "value_grad": 13, "C": 13, "I1": 13, "detF": 13, "div": 13}
