"""The NumPy / SciPy yardstick of dxo_amg_create_transfer (csrc/amg.hip): a p-coarsening first level for quadratic elements.

vertex_transfer_ref is the nodal interpolation W from the degree-1 space on the same cells, cell by cell from the two dofmaps and the
coordinate element tabulated at the field element's nodes. amg_ref(first_transfer=(W, coarse_to_fine)) is the hierarchy: level 0 keeps
Dinv, rho and omega of any level; its P is kron(W, I_bs) with the rows of constrained fine dofs and the columns of the coarse dofs
constrained at their own node zero; A_1 = P^T A P on the symbolic pattern of the product; the levels below are the hierarchy of A_1
with the constraints of the coarse nodes (and the rows of the zeroed B at those nodes). Both are in oracle/amg_oracle.py.

The iteration counts pinned here are the experiment the feature was specified with: CG to rtol 1e-8 on eps / eps isotropic elasticity,
bottom clamped, distort 0.1, seed 2, coarse_rows 60, a PCG64(1) normal right-hand side."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle.amg_oracle import (amg_ref, cg_with_cycle, expand_pattern, node_graph, operator_complexity, power_rho_ref,
                               rigid_body_modes_ref, transfer_patterns, vertex_transfer_ref)
from oracle.form_oracle import apply_bcs, dense_ref, pattern_ref
from oracle.krylov_oracle import bottom_dofs, elastic_C, elastic_C3, to_pattern_csr
from solver_cases import COARSE_ROWS
from tools.synthetic import coordinate_element_at_nodes, gauss_tensor_rule, structured_mesh, with_rule


# ---- the systems of the experiment
CASES = {                # cell, boxes per side, block size, 27-point rule
    "p2_tri14": ("triangle", (14, 14), 2, False),
    "q2_hex3": ("hexahedron", (3, 3, 3), 3, True),
    "q2_hex5": ("hexahedron", (5, 5, 5), 3, True),
    "p2_tet3": ("tetrahedron", (3, 3, 3), 3, False),
}
_CACHE = {}


def elasticity(cell, n, bs, rule27=False, degree=2, distort=0.1, seed=2, extra=()):
    """(mesh, S on the device pattern, constrained dofs): eps / eps with the isotropic C, the bottom clamped (and `extra` dofs)."""
    m = structured_mesh(cell, n, degree, distort=distort, seed=seed)
    if rule27:
        m = with_rule(m, *gauss_tensor_rule(cell, 3))
    C = elastic_C(m) if bs == 2 else elastic_C3(m.num_cells * m.nq)
    dofs = np.unique(np.concatenate([bottom_dofs(m, bs), np.asarray(extra, dtype=np.int64)]))
    return m, to_pattern_csr(m, apply_bcs(dense_ref(m, "eps", "eps", bs, C), dofs, 1.0), bs), dofs


def case(name):
    if name not in _CACHE:
        cell, n, bs, rule27 = CASES[name]
        m, S, dofs = elasticity(cell, n, bs, rule27)
        W, ctf = vertex_transfer_ref(m)
        b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
        _CACHE[name] = (m, S, bs, dofs, W, ctf, b)
    return _CACHE[name]


VARIANTS = {
    "jacobi": dict(smoother="jacobi", rho="inf-norm"),
    "cheby": dict(smoother="chebyshev", degree=2, rho="power"),
    "cheby_rbm": dict(smoother="chebyshev", degree=2, rho="power"),
}
# iterations (plain hierarchy, with the p level), rows per level and operator complexity of both: the figures of the experiment
TABLE = {
    ("p2_tri14", "jacobi"): (97, 41), ("p2_tri14", "cheby"): (39, 20), ("p2_tri14", "cheby_rbm"): (20, 13),
    ("q2_hex3", "jacobi"): (68, 39), ("q2_hex3", "cheby"): (24, 15), ("q2_hex3", "cheby_rbm"): (15, 12),
    ("q2_hex5", "jacobi"): (105, 43), ("q2_hex5", "cheby"): (30, 16), ("q2_hex5", "cheby_rbm"): (16, 10),
    ("p2_tet3", "cheby"): (32, 19), ("p2_tet3", "cheby_rbm"): (19, 15),
}
ROWS = {"p2_tri14": ([1682, 112, 8], [1682, 450, 50]), "q2_hex3": ([1029, 24], [1029, 192, 12]),
        "q2_hex5": ([3993, 81, 3], [3993, 648, 24]), "p2_tet3": ([1029, 24], [1029, 192, 12])}
COMPLEXITY = {"p2_tri14": (1.10, 1.18), "q2_hex3": (1.00, 1.07), "q2_hex5": (1.01, 1.06), "p2_tet3": (1.01, 1.09)}


def hierarchies(name, variant):
    m, S, bs, dofs, W, ctf, _ = case(name)
    kw = dict(VARIANTS[variant], coarse_rows=COARSE_ROWS)
    if variant == "cheby_rbm":
        kw["near_nullspace"] = rigid_body_modes_ref(m.node_x)
    return amg_ref(S, bs, dofs, **kw), amg_ref(S, bs, dofs, first_transfer=(W, ctf), **kw)


# ---- tests
MESHES = [("triangle", (4, 3)), ("quadrilateral", (3, 4)), ("tetrahedron", (2, 2, 3)), ("hexahedron", (2, 3, 2))]


@pytest.mark.parametrize("cell,n", MESHES)
def test_weights_are_binary_fractions_and_rows_interpolate(cell, n):
    m = structured_mesh(cell, n, 2, distort=0.1, seed=2)
    W, ctf = vertex_transfer_ref(m)
    # simplices: a vertex or the midpoint of an edge; tensor cells: the centre of a sub-cell of dimension j <= gdim has weight 2^-j
    allowed = {1.0, 0.5} if cell in ("triangle", "tetrahedron") else {2.0 ** -j for j in range(m.gdim + 1)}
    assert set(W.data.tolist()) == allowed
    counts = np.diff(W.indptr)
    assert counts.min() == 1 and counts.max() == (2 if cell in ("triangle", "tetrahedron") else 2 ** m.gdim)
    assert np.array_equal(np.asarray(W.sum(axis=1)).ravel(), np.ones(W.shape[0]))          # exactly: sums of binary fractions
    assert np.abs(W @ m.x - m.node_x).max() <= 4 * 2.0 ** -53                                # the field nodes are images of the vertices
    assert np.unique(ctf).size == W.shape[1] and np.array_equal(m.node_x[ctf], m.x)
    for v, i in enumerate(ctf):
        assert W.indptr[i + 1] - W.indptr[i] == 1 and W.indices[W.indptr[i]] == v and W.data[W.indptr[i]] == 1.0


@pytest.mark.parametrize("cell,n", MESHES)
def test_library_vertex_transfer_is_the_oracle(cell, n):
    from dolfinx_external_operator_amd.operand_eval import vertex_transfer

    m = structured_mesh(cell, n, 2, distort=0.1, seed=2)
    W, ctf = vertex_transfer_ref(m)
    t = vertex_transfer(m.dofmap, m.geom_dofmap, coordinate_element_at_nodes(cell, 2), m.node_x.shape[0])
    assert t.n_coarse == W.shape[1]
    assert np.array_equal(t.ptr, W.indptr) and np.array_equal(t.col, W.indices) and np.array_equal(t.w, W.data)
    assert np.array_equal(t.coarse_to_fine, ctf)
    assert t.ptr.dtype == np.int64 and t.col.dtype == np.int32 and t.coarse_to_fine.dtype == np.int32
    m1 = structured_mesh(cell, n, 1)
    with pytest.raises(ValueError, match="degree 1"):
        vertex_transfer(m1.dofmap, m1.geom_dofmap, coordinate_element_at_nodes(cell, 1))
    bad = coordinate_element_at_nodes(cell, 2).copy()
    bad[-1] = bad[-1][::-1] * 0.75 + 0.01                     # the last local node, shared between cells, gets cell-dependent weights
    with pytest.raises(ValueError):
        vertex_transfer(m.dofmap, m.geom_dofmap, bad, m.node_x.shape[0])


@pytest.mark.parametrize("cell,n", MESHES)
@pytest.mark.parametrize("bs", [1, 0])
def test_galerkin_pattern_is_the_pattern_of_the_degree_one_mesh(cell, n, bs):
    m = structured_mesh(cell, n, 2, distort=0.1, seed=2)
    bs = bs or m.gdim
    W, _ = vertex_transfer_ref(m)
    indptr, indices = pattern_ref(m, bs)
    ptr, nb = node_graph(indptr, indices, bs)
    Pp, APp, Cp = transfer_patterns(ptr, nb, W)
    cptr, cidx = expand_pattern(Cp, bs)
    m1 = structured_mesh(cell, n, 1, distort=0.1, seed=2)
    assert np.array_equal(m1.geom_dofmap, m.geom_dofmap) and np.array_equal(m1.x, m.x)
    rptr, ridx = pattern_ref(m1, bs)
    assert np.array_equal(cptr, rptr) and np.array_equal(cidx, ridx)                       # no fill
    # and a generic product has no zero inside it: the pattern is not merely an upper bound
    rng = np.random.Generator(np.random.PCG64(4))
    G = sp.csr_matrix((rng.uniform(1.0, 2.0, nb.size), nb, ptr), shape=(ptr.size - 1,) * 2)
    C = (W.T @ G @ W).tocsr()
    C.sort_indices()
    assert np.array_equal(C.indptr, Cp.indptr) and np.array_equal(C.indices, Cp.indices)


def test_masked_transfer_and_level_one_constraints():
    """Rollers on one side: partly constrained nodes. Rows of constrained fine dofs and columns of coarse dofs constrained at their own
    node are zero, A_1 gets unit diagonal entries there, and level 1 is the hierarchy of A_1 with that set."""
    m0 = structured_mesh("triangle", (6, 5), 2, distort=0.1, seed=2)
    left = np.flatnonzero(np.abs(m0.node_x[:, 0]) < 1e-12) * 2               # the horizontal component on x = 0
    m, S, dofs = elasticity("triangle", (6, 5), 2, extra=left)
    W, ctf = vertex_transfer_ref(m)
    levels = amg_ref(S, 2, dofs, first_transfer=(W, ctf), coarse_rows=COARSE_ROWS)
    L0, L1 = levels[0], levels[1]
    mask = np.zeros(S.shape[0], dtype=bool)
    mask[dofs] = True
    mask1 = mask.reshape(-1, 2)[ctf].reshape(-1)
    assert mask1.reshape(-1, 2).any(axis=1).sum() > mask1.reshape(-1, 2).all(axis=1).sum() > 0      # both kinds of node
    assert not abs(L0.P[np.flatnonzero(mask)]).sum() and not abs(L0.P[:, np.flatnonzero(mask1)]).sum()
    assert set(np.unique(L0.p_diag).tolist()) == {0.0, 0.5, 1.0}
    d = L1.A.diagonal()
    assert (d[mask1] == 1.0).all() and not abs(L1.A[np.flatnonzero(mask1)]).sum() - mask1.sum()
    assert np.array_equal(L1.mask, mask1)
    direct = amg_ref(L1.A, 2, np.flatnonzero(mask1), coarse_rows=COARSE_ROWS)
    assert len(direct) == len(levels) - 1
    for a, b in zip(direct, levels[1:]):
        assert np.array_equal(a.A.toarray(), b.A.toarray())
    # a degree-1 displacement field that satisfies the constraints is reproduced by P
    u1 = np.random.Generator(np.random.PCG64(3)).normal(size=(m.x.shape[0], 2))
    u1.reshape(-1)[mask1] = 0.0
    u2 = (W @ u1).reshape(-1)
    free = ~mask
    assert np.abs((L0.P @ u1.reshape(-1))[free] - u2[free]).max() <= 1e-15


def test_rigid_body_modes_of_level_one_are_those_of_its_nodes():
    m, S, bs, dofs, W, ctf, _ = case("p2_tri14")
    B = rigid_body_modes_ref(m.node_x)
    levels = amg_ref(S, bs, dofs, first_transfer=(W, ctf), near_nullspace=B, coarse_rows=COARSE_ROWS)
    B1 = rigid_body_modes_ref(m.x)
    on = np.zeros(S.shape[0], dtype=bool)
    on[dofs] = True
    B1[on.reshape(-1, bs)[ctf].reshape(-1)] = 0.0
    assert np.array_equal(levels[1].B, B1)
    # degree-1 functions reproduce them, wherever no constrained coarse node takes part in the interpolation
    inner = np.repeat(np.asarray(W @ on.reshape(-1, bs)[ctf].any(axis=1).astype(float)).ravel() == 0.0, bs) & ~on
    assert inner.sum() > 0.8 * inner.size
    assert np.abs((levels[0].P @ B1)[inner] - B[inner]).max() <= 4 * 2.0 ** -53 * np.abs(B).max()


@pytest.mark.parametrize("name,variant", sorted(TABLE))
def test_iteration_table(name, variant):
    _, S, _, _, _, _, b = case(name)
    plain, with_p = hierarchies(name, variant)
    its = []
    for levels in (plain, with_p):
        x, n, conv = cg_with_cycle(S, b, levels, rtol=1e-8, maxiter=600)
        assert conv and np.linalg.norm(b - S @ x) <= 1.01e-8 * np.linalg.norm(b)
        its.append(n)
    rows = [[L.n_rows for L in h] for h in (plain, with_p)]
    cx = [operator_complexity(h) for h in (plain, with_p)]
    print(f"{name} {variant}: CG iterations {its[0]} -> {its[1]}, rows {rows[0]} -> {rows[1]}, complexity {cx[0]:.3f} -> {cx[1]:.3f}")
    assert abs(its[0] - TABLE[name, variant][0]) <= 2 and abs(its[1] - TABLE[name, variant][1]) <= 2, (its, TABLE[name, variant])
    assert its[1] < its[0]
    if variant != "cheby_rbm":                                   # with the modes the coarse block size, and so the rows, differ
        assert (rows[0], rows[1]) == tuple(ROWS[name])
        assert abs(cx[0] - COMPLEXITY[name][0]) <= 0.006 and abs(cx[1] - COMPLEXITY[name][1]) <= 0.006


def test_the_p_level_gives_the_iterations_of_the_degree_one_problem():
    """With the true rho on level 0 (Chebyshev 2, power iteration) the Q2 system with the p level takes what Q1 takes on its own."""
    for name, q1_its in (("q2_hex3", 28), ("q2_hex5", 40)):
        cell, n, bs, _ = CASES[name]
        m1, S1, dofs1 = elasticity(cell, n, bs, degree=1)
        b1 = np.random.Generator(np.random.PCG64(1)).normal(size=S1.shape[0])
        _, its1, conv = cg_with_cycle(S1, b1, amg_ref(S1, bs, dofs1, **VARIANTS["jacobi"], coarse_rows=COARSE_ROWS), rtol=1e-8, maxiter=600)
        assert conv and abs(its1 - q1_its) <= 2, (name, its1)
        _, S, _, _, _, _, b = case(name)
        lv = hierarchies(name, "jacobi")[1]
        lv[0].rho = power_rho_ref(lv[0].A, lv[0].Dinv, 10, 1.1)  # the true rho on level 0 alone
        lv[0].omega = (4.0 / 3.0) / lv[0].rho
        _, its2, conv = cg_with_cycle(S, b, lv, rtol=1e-8, maxiter=600)
        print(f"{name}: Q1 alone {its1}, Q2 with the p level and the power rho on level 0 {its2}")
        assert conv and abs(its2 - its1) <= 3, (name, its1, its2)


def test_the_eight_point_rule_under_integrates_the_q2_hexahedron():
    """Q2 hexahedra under quadrature_degree2 (8 points: 48 strain values against 81 dofs per cell) carry spurious zero-energy modes: CG
    does not converge in 600 iterations under any of the cycles. Under the 27-point rule the same hierarchies converge."""
    m8, S8, dofs = elasticity("hexahedron", (3, 3, 3), 3, rule27=False)
    assert m8.nq == 8
    W, ctf = vertex_transfer_ref(m8)
    b = np.random.Generator(np.random.PCG64(1)).normal(size=S8.shape[0])
    for kw in (VARIANTS["jacobi"], VARIANTS["cheby"]):
        for levels in (amg_ref(S8, 3, dofs, coarse_rows=COARSE_ROWS, **kw), amg_ref(S8, 3, dofs, first_transfer=(W, ctf), coarse_rows=COARSE_ROWS, **kw)):
            _, its, conv = cg_with_cycle(S8, b, levels, rtol=1e-8, maxiter=600)
            assert not conv and its == 600
    _, S27, _, dofs27, _, _, b27 = case("q2_hex3")
    assert np.array_equal(dofs27, dofs)
    _, its, conv = cg_with_cycle(S27, b27, hierarchies("q2_hex3", "jacobi")[0], rtol=1e-8, maxiter=600)
    assert conv and abs(its - 68) <= 2
    # the cause, not only the symptom: the free-free 8-point matrix has more zero-energy modes than the 6 rigid-body modes
    m = structured_mesh("hexahedron", (1, 1, 1), 2)
    for rule, nullity in ((None, None), (gauss_tensor_rule("hexahedron", 3), 6)):
        mm = m if rule is None else with_rule(m, *rule)
        ev = np.linalg.eigvalsh(dense_ref(mm, "eps", "eps", 3, elastic_C3(mm.nq)))
        zero = int((np.abs(ev) <= 1e-10 * ev.max()).sum())
        assert zero == 6 if nullity else zero >= 81 - 48
