"""Reference, meshes, lists, inputs and bounds shared by tests/test_functional_reference_cpu.py and tests/test_functional_gpu.py (not a
test module): the scalar functionals of csrc/functional.hip (dxo_eval_cell_measure, dxo_integrate, dxo_facet_integrate,
dxo_operand_moments).

Reference. Long double, composed from what oracle/ exports: oracle.operand_reference.ref_operand (the operand and its mag),
oracle.consumer_reference.inverse_and_det (det J), oracle.facet_reference.ref_facet_geometry (dS and its mag). Every function returns
(ref, mag), mag the same sum with the absolute value of every term: |f_k|, |g_k|, the operand's mag, dS_mag, and for the cell measure
dx_mag = |w| * sum over the permutations of prod |J_i,p(i)| (every term of det J's expansion taken positive, as the det F operand's mag
is formed). dtype = np.float64 gives the float64 twin of the same statements.

Bound, for EVERY output entry k: |got[k] - ref[k]| <= c * 2^-53 * mag[k]; entries with mag = 0 must be exact. c is not tuned on the
kernels: C_REF below is what the float64 twin loses against long double over all cases (measured and asserted in
test_functional_reference_cpu.py), and the kernels get c = MARGIN * max(C_REF[entry], 1) with MARGIN = 8 of consumer_cases.py — the
floor 1 because one rounding of the result already costs a unit.

Groups and passes (csrc/functional.hip). A cell kernel's wave takes cpw = 64 // nq consecutive cells of the list per trip, the facet
kernel's epw = 64 // nq_facet entities; one partial per group; fn_final adds them with W = FN_FINAL = 256 lanes, lane t taking groups
t, t + W, ... . The persistent kernels launch at most BLOCKS_PER_CU * compute_units workgroups of 4 waves (wave_group_grid /
capped_grid, form_host.h), so a list of more than 4 * 8 * compute_units groups sends some wave on a second trip. cell_lists() /
facet_lists() hold lists around W groups, made by cutting or repeating a mesh's list cyclically, big_cells() / big_entities() the
list past the cap; check_groups() asserts that they straddle the boundaries they are meant for.
"""
import functools
import itertools
import types

import numpy as np

import consumer_cases as CC
import facet_reference_cases as FC
from consumer_cases import MARGIN  # noqa: F401  (shared with the test modules)
from oracle.consumer_reference import LD, inverse_and_det, worst_ratio  # noqa: F401
from oracle.facet_reference import ref_facet_geometry
from oracle.operand_reference import ref_operand, value_size

FN_FINAL = 256            # W: lanes of fn_final
FN_WAVES = 4              # waves per workgroup = groups per workgroup and trip
FN_BLOCKS_PER_CU = 8      # cap of both grids
MI355X_COMPUTE_UNITS = 256
INTEGRATE_SIZES = (1, 2, 3, 4, 6, 9)          # D of the per-component form
PAIR_SIZES = (1, 3, 5, 6, 13)                 # D of the pairing: served sizes (compile-time divisor) and others (run time)
# every kind with every block size the fused form takes on gdim G
KINDS_SCALAR = ("value", "grad", "value_grad")
KINDS_VECTOR = ("eps", "F", "C", "I1", "detF", "div")


def moment_cases(G):
    return [(k, bs) for k in KINDS_SCALAR for bs in (1, G)] + [(k, G) for k in KINDS_VECTOR]


# ------------------------------------------------------------------------------------------------ reference
def _perm_abs(J):
    """(..., G, G) -> sum over permutations p of prod_i |J[i, p(i)]|: det J with every term taken positive."""
    G = J.shape[-1]
    A = np.abs(J)
    out = np.zeros(J.shape[:-2], dtype=J.dtype)
    for p in itertools.permutations(range(G)):
        term = np.ones(J.shape[:-2], dtype=J.dtype)
        for i in range(G):
            term = term * A[..., i, p[i]]
        out = out + term
    return out


def _cells(mesh, cells):
    return np.arange(mesh.num_cells) if cells is None else np.asarray(cells, dtype=np.int64).reshape(-1)


def ref_cell_measure(mesh, cells=None, dtype=LD):
    """-> (dx, mag), each (n_cells, nq): dx = w |det J| at the quadrature points of the listed cells."""
    G = mesh.gdim
    uniq, inv = np.unique(_cells(mesh, cells), return_inverse=True)          # a repeated cell is formed once and indexed
    X = np.asarray(mesh.x, dtype=dtype)[:, :G][mesh.geom_dofmap[uniq]]
    J = np.einsum("cvj,qvk->cqjk", X, np.asarray(mesh.dpsi, dtype=dtype))
    if J.shape[0] == 0:
        return np.zeros(J.shape[:2], dtype=dtype), np.zeros(J.shape[:2], dtype=dtype)
    _, det = inverse_and_det(J)
    w = np.asarray(mesh.weights, dtype=dtype)
    return (w[None, :] * np.abs(det))[inv], (np.abs(w)[None, :] * _perm_abs(J))[inv]


def _reduce(meas, meas_mag, f, g, dtype):
    """The two forms on a point measure (n, nq): -> (ref, mag), (D,) without g, (1,) with."""
    f = np.asarray(f, dtype=dtype)
    f = f.reshape(meas.shape + (f.shape[-1] if f.size == 0 else -1,))          # f (0, nq, D): the functional over nothing
    if g is None:
        return np.einsum("cq,cqk->k", meas, f), np.einsum("cq,cqk->k", meas_mag, np.abs(f))
    g = np.asarray(g, dtype=dtype).reshape(f.shape)
    return (np.einsum("cq,cqk,cqk->", meas, f, g).reshape(1), np.einsum("cq,cqk,cqk->", meas_mag, np.abs(f), np.abs(g)).reshape(1))


def ref_integrate(mesh, f, g=None, cells=None, dtype=LD, measure=None):
    """-> (ref, mag) of dxo_integrate: f (n_cells, nq, D) by position in the list. measure: ref_cell_measure of the same list and
    dtype, where the caller has it already."""
    return _reduce(*(measure or ref_cell_measure(mesh, cells, dtype)), f, g, dtype)


def ref_facet_measure(mesh, tabs, geom, ents, dtype=LD):
    """-> (dS, mag), each (n_entities, nq_facet)."""
    return ref_facet_geometry(mesh, tabs, geom, ents, dtype)[2:]


def ref_facet_integrate(mesh, tabs, geom, ents, f, g=None, dtype=LD, measure=None):
    """-> (ref, mag) of dxo_facet_integrate over (cell, local facet) pairs with the tables of facet_reference_cases.rule_tables."""
    ents = np.asarray(ents).reshape(-1, 2)
    if len(ents) == 0:                                       # f (0, nq, D): the functional over nothing
        n_out = np.asarray(f).shape[-1] if g is None else 1
        return np.zeros(n_out, dtype), np.zeros(n_out, dtype)
    return _reduce(*(measure or ref_facet_measure(mesh, tabs, geom, ents, dtype)), f, g, dtype)


def ref_operand_moments(mesh, kind, bs, u, cells=None, dtype=LD, measure=None):
    """-> (ref, mag), each (D + 1,): [int operand_k dx, k < D; int |operand|^2 dx]."""
    dx, dxm = measure or ref_cell_measure(mesh, cells, dtype)
    D = value_size(kind, bs, mesh.gdim)
    if dx.shape[0] == 0:
        return np.zeros(D + 1, dtype), np.zeros(D + 1, dtype)
    uniq, inv = np.unique(_cells(mesh, cells), return_inverse=True)
    o, om = (a[inv] for a in ref_operand(mesh, kind, bs, u, uniq, dtype))
    ref = np.concatenate([np.einsum("cq,cqk->k", dx, o), np.einsum("cq,cqk,cqk->", dx, o, o).reshape(1)])
    mag = np.concatenate([np.einsum("cq,cqk->k", dxm, om), np.einsum("cq,cqk,cqk->", dxm, om, om).reshape(1)])
    return ref, mag


# ------------------------------------------------------------------------------------------------ cell cases
# ("cells", consumer case) for consumer_cases.ALL_CASES; ("mirrored", facet case) for the mirrored size-b meshes (det J < 0)
MIRRORED = [c for c in FC.ALL_CASES if c[3]]
CELL_CASES = [("cells", c) for c in CC.ALL_CASES] + [("mirrored", c) for c in MIRRORED]
FACET_CASES = FC.ALL_CASES


def cell_case_id(case):
    return CC.case_id(case[1]) if case[0] == "cells" else FC.case_id(case[1])


@functools.lru_cache(maxsize=None)
def cell_mesh(case):
    return CC.build_mesh(case[1]) if case[0] == "cells" else FC.mesh_of(case[1])


def is_size(case, cell, degree, size):
    """The unmirrored mesh of that cell type, degree and size letter at the degree-2 rule."""
    return case[0] == "cells" and case[1][0] == cell and case[1][1] == degree and case[1][4] == size


GROUP_CELLS = ("triangle", "hexahedron")       # one simplex and one tensor cell type carry the lists sized by W and by the cap


def carries_group_lists(case):
    return any(is_size(case, cell, 2, "d") for cell in GROUP_CELLS)


def _cycled(a, n):
    return np.ascontiguousarray(a[np.arange(n) % len(a)])


def group_lengths(per_group):
    """Lists of (W - 1) groups and one cell, exactly W groups, and (2 W + 3) groups and one cell."""
    W = FN_FINAL
    return ((W - 1) * per_group + 1, W * per_group, (2 * W + 3) * per_group + 1)


@functools.lru_cache(maxsize=None)
def cell_lists(case):
    """name -> int32 cell list or None: NULL (all cells), arange (must equal NULL bit for bit), a shuffled two thirds, one cell three
    times among others, a single cell, the empty list; on the meshes of carries_group_lists the lists of group_lengths."""
    m = cell_mesh(case)
    nc, cpw = m.num_cells, 64 // m.nq
    rng = np.random.Generator(np.random.PCG64([41, CELL_CASES.index(case)]))
    perm = rng.permutation(nc).astype(np.int32)
    some = perm[:min(nc, 5)]
    rep = np.concatenate([some, some[:1], perm[-1:], some[:1]]).astype(np.int32)
    out = {"all": None, "arange": np.arange(nc, dtype=np.int32), "shuffled": np.ascontiguousarray(perm[:max(1, nc * 2 // 3)]),
           "repeated": rep, "single": np.array([nc // 2], dtype=np.int32), "empty": np.zeros(0, dtype=np.int32)}
    if carries_group_lists(case):
        for n in group_lengths(cpw):
            out[f"cycled{n}"] = _cycled(np.arange(nc, dtype=np.int32), n)
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


def cap_groups(compute_units):
    """Groups one trip of a persistent kernel covers at most: 4 waves * 8 workgroups per compute unit."""
    return FN_WAVES * FN_BLOCKS_PER_CU * compute_units


def big_cells(case, compute_units):
    """(4 * 8 * compute_units + 5) * cpw cells, the mesh's cells repeated cyclically: past the cap of wave_group_grid."""
    m = cell_mesh(case)
    return _cycled(np.arange(m.num_cells, dtype=np.int32), (cap_groups(compute_units) + 5) * (64 // m.nq))


# ------------------------------------------------------------------------------------------------ facet lists
def facet_epw(nq):
    """Entities per group of fn_facet: floor(64 / nq_facet), one for a rule of 64 points or more."""
    return 1 if nq >= 64 else 64 // nq


def carries_facet_group_lists(case):
    return case[0] in GROUP_CELLS and case[1] == 2 and case[2] == "d" and not case[3] and case[4] == "deg2"


@functools.lru_cache(maxsize=None)
def facet_lists(case):
    """The lists of facet_reference_cases.entity_lists (exterior, subset, all, repeated, single, empty, whole and ragged rounds), and on
    the size-d quadratic triangles and hexahedra `all` cut or repeated to the lengths of group_lengths."""
    out = dict(FC.entity_lists(case))
    if carries_facet_group_lists(case):
        for n in group_lengths(facet_epw(FC.nq_of(case))):
            out[f"cycled{n}"] = _cycled(out["all"], n)
            out[f"cycled{n}"].setflags(write=False)
    return out


def big_entities(case, compute_units):
    return _cycled(FC.entity_lists(case)["all"], (cap_groups(compute_units) + 5) * facet_epw(FC.nq_of(case)))


def check_groups(compute_units=MI355X_COMPUTE_UNITS):
    """-> report lines; asserts what the module docstring promises about the lists and the two boundaries."""
    W, lines = FN_FINAL, []
    for case in CELL_CASES:
        if not carries_group_lists(case):
            continue
        m = cell_mesh(case)
        cpw = 64 // m.nq
        groups = sorted(-(-len(a) // cpw) for name, a in cell_lists(case).items() if name.startswith("cycled"))
        assert groups == [W, W, 2 * W + 4], groups          # W - 1 full groups and a ragged one; exactly W; two full strides and a tail
        assert [len(a) % cpw for name, a in cell_lists(case).items() if name.startswith("cycled")] == [1, 0, 1]
        big = -(-len(big_cells(case, compute_units)) // cpw)
        assert big > cap_groups(compute_units) and big % 8 != 0, big     # a second trip for some waves, uneven XCD slices
        lines.append(f"{cell_case_id(case):28s} cpw {cpw:2d}: groups {groups}, past the cap {big} > {cap_groups(compute_units)}")
    assert len(lines) == len(GROUP_CELLS)
    n_facet = 0
    for cell, rule in sorted({(c[0], c[4]) for c in FACET_CASES}):                   # per (cell type, facet rule), as FC.check_rounds
        cases = [c for c in FACET_CASES if c[0] == cell and c[4] == rule]
        epw = facet_epw(FC.nq_of(cases[0]))
        lengths = sorted({len(a) for c in cases for a in facet_lists(c).values() if len(a)})
        assert any(n < epw for n in lengths), (cell, rule, epw, lengths)                     # a partial group
        assert any(n > epw and n % epw for n in lengths), (cell, rule, epw, lengths)         # full groups and a ragged one
    for case in FACET_CASES:
        epw = facet_epw(FC.nq_of(case))
        if carries_facet_group_lists(case):
            groups = sorted(-(-len(a) // epw) for name, a in facet_lists(case).items() if name.startswith("cycled"))
            assert groups == [W, W, 2 * W + 4], groups
            big = -(-len(big_entities(case, compute_units)) // epw)
            assert big > cap_groups(compute_units), big
            lines.append(f"{FC.case_id(case):28s} epw {epw:2d}: groups {groups}, past the cap {big} > {cap_groups(compute_units)}")
            n_facet += 1
    assert n_facet == len(GROUP_CELLS)
    return lines


# ------------------------------------------------------------------------------------------------ inputs
VARIANTS = ("", "scaled", "offset")


def _variant(a, variant):
    """"": N(0, 1) as drawn; "scaled": component k times 10^(3 k); "offset": + 10^6 (large cancellation, and mag grows with it)."""
    if variant == "scaled":
        return a * (10.0 ** (3 * np.arange(a.shape[-1])))
    if variant == "offset":
        return a + 1e6
    return a


def integrate_items(n, nq, seed):
    """The calls on one list of n cells or entities: namespaces (entry, D, variant, f, g). Per-component form: every D of
    INTEGRATE_SIZES in every variant. Pairing: every D of PAIR_SIZES in every variant, and g aliased to f ("alias", g is f)."""
    ns, items = types.SimpleNamespace, []
    for D in sorted(set(INTEGRATE_SIZES) | set(PAIR_SIZES)):
        rng = np.random.Generator(np.random.PCG64(list(seed) + [D]))
        f0, g0 = rng.normal(size=(n, nq, D)), rng.normal(size=(n, nq, D))
        for v in VARIANTS:
            f, g = _variant(f0, v), _variant(g0, v)
            if D in INTEGRATE_SIZES:
                items.append(ns(entry="integrate", D=D, variant=v, f=f, g=None))
            if D in PAIR_SIZES:
                items.append(ns(entry="pair", D=D, variant=v, f=f, g=g))
        if D in PAIR_SIZES:
            items.append(ns(entry="pair", D=D, variant="alias", f=f0, g=f0))
    return items


def moment_items(mesh, seed):
    """namespaces (entry "moments:<kind>", kind, bs, variant, u): u ~ N(0, 1) and u + 10^6, every kind with every block size."""
    ns, items, nn = types.SimpleNamespace, [], mesh.node_x.shape[0]
    for i, (kind, bs) in enumerate(moment_cases(mesh.gdim)):
        u = np.random.Generator(np.random.PCG64(list(seed) + [i])).normal(size=nn * bs)
        items += [ns(entry=f"moments:{kind}", kind=kind, bs=bs, variant="", u=u), ns(entry=f"moments:{kind}", kind=kind, bs=bs, variant="offset", u=u + 1e6)]
    return items


def item_id(item):
    return item.entry + (f" D {item.D}" if hasattr(item, "D") else f" bs {item.bs}") + (f" [{item.variant}]" if item.variant else "")


# ------------------------------------------------------------------------------------------------ bounds
# What the float64 twin of the reference loses against long double, in units of 2^-53 * mag[k], at the worst output entry over every
# case, list and input above (x86-64 long double); rounded up from what test_functional_reference_cpu.py measures, which asserts that
# the figures hold and that none is more than twice what is measured. Measured figure and the case that gives it:
#   measure          27.51  Q1 quadrilaterals 13x12, all cells (J is a difference of coordinates of size 1 at a spacing of 1 / 13, which mag
#                           does not see and every float64 evaluation loses alike: consumer_cases.py)
#   integrate       105.02  P2 triangles 10x10, 10816 cycled cells, D 9, f + 10^6        pair      53.96  Q2 quadrilaterals 13x12, arange, D 13, g = f
#   facet_integrate   4.68  P2 triangles 10x10, 16481 cycled entities, D 9, f + 10^6     facet_pair 6.29  P2 tetrahedra 3x2x2 strang6, all72, D 13, g = f
#   moments: value 299.45, value_grad 214.53, C 62.74 (P2 triangles 10x10, 10816 cycled cells, bs 2; the first two with u + 10^6)
#            grad 17.47 (P1 tetrahedra 3x3x3, all)   F 15.14, div 3.41 (Q2 hexahedra 7x4x3, 4121 cycled cells)   I1 4.71 (P2 triangles, 5376 cells)
#            eps 4.81 (Q2 hexahedra 5x1x1 gauss3, repeated)   detF 0.67 (Q1 quadrilateral 1x1)
# The figures above 50 are np.einsum's: on the cycled lists it adds 10^4 to 10^5 terms of one sign (f + 10^6, |f|^2, u + 10^6) in sequence,
# and a sequential sum of n equal terms loses about n / 2 roundings of its result in the worst case. The kernels' tree does not, but the
# rule of this file is that c comes from the twin, so those entries' bounds are as loose as the twin is.
C_REF = {"measure": 27.6, "integrate": 105.1, "pair": 54.0, "facet_integrate": 4.7, "facet_pair": 6.3,
         "moments:value": 299.5, "moments:grad": 17.5, "moments:value_grad": 214.6, "moments:eps": 4.9, "moments:F": 15.2,
         "moments:C": 62.8, "moments:I1": 4.8, "moments:detF": 0.7, "moments:div": 3.5}
# The finest relative error in one cell (or entity) that the bound resolves: the largest integer p for which the float64 twin, fed f (u
# for the moments) whose values on cell / entity 0 (the dofs of cell 0) are scaled by 1 + 10^-p, still misses c = MARGIN *
# max(C_REF[entry], 1) against the reference of the unscaled input on every one of the four quadratic size-b meshes (all cells or the
# whole boundary, the plain inputs, every D or block size). Measured in test_functional_reference_cpu.py.
# At p + 1 at least one call of the entry on one of the four meshes meets its bound.
RESOLVES = {"integrate": 8, "pair": 10, "facet_integrate": 10, "facet_pair": 9, "moments:value": 10, "moments:grad": 11, "moments:value_grad": 11,
            "moments:eps": 12, "moments:F": 12, "moments:C": 11, "moments:I1": 12, "moments:detF": 11, "moments:div": 12}


def allowed(entry):
    return MARGIN * max(C_REF[entry], 1.0)
