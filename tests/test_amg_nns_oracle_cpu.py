"""The NumPy / SciPy yardstick of dxo_amg_create_nns (csrc/amg.hip): smoothed aggregation with a near-null space, pinned on the CPU.

amg_nns_ref restates the device algorithm on top of the oracle of test_amg_oracle_cpu.py: today's aggregates; per level and aggregate
the rows of B of its nodes in ascending node order, orthonormalised by Gram-Schmidt in column order with a second pass (a column with
|v| <= rank_tol |v0| after the projections is dead: Q column zero, R diagonal zero); T carries the Q blocks (bs_l x k), the next B the
R factors; P = T - omega Dinv A T and A_c = P^T A P on today's block patterns expanded with bs_l rows and k columns. Every coarse level
has block size k. The level objects carry what vcycle_ref of test_amg_oracle_cpu.py reads, so the cycle is that function."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg

import test_krylov_oracle_cpu as kro
from test_amg_oracle_cpu import (MAX_DENSE, U, Level, active_nodes, aggregate_ref, amg_ref, block_patterns, cg_with_cycle, coarse_ref,
                                 gmres_with_cycle, node_graph, on_pattern, operator_complexity, prolongator_ref, rho_ref, vcycle_ref)
from test_assemble_oracle_cpu import apply_bcs, dense_ref, pattern_ref
from test_krylov_oracle_cpu import block_jacobi_ref, bottom_dofs, elastic_C, eps_matrix, to_pattern_csr
from tools.synthetic import structured_mesh

RANK_TOL = 1e-10


def rigid_body_modes_ref(x):
    """B [n_nodes * gdim][k]: the gdim translations, then (-y, x) in 2-D and (-y, x, 0), (0, -z, y), (z, 0, -x) in 3-D."""
    x = np.asarray(x, dtype=np.float64)
    n, g = x.shape
    k = 3 if g == 2 else 6
    B = np.zeros((n, g, k))
    for d in range(g):
        B[:, d, d] = 1.0
    if g == 2:
        B[:, 0, 2], B[:, 1, 2] = -x[:, 1], x[:, 0]
    else:
        B[:, 0, 3], B[:, 1, 3] = -x[:, 1], x[:, 0]
        B[:, 1, 4], B[:, 2, 4] = -x[:, 2], x[:, 1]
        B[:, 0, 5], B[:, 2, 5] = x[:, 2], -x[:, 0]
    return B.reshape(n * g, k)


def translations_ref(n_nodes, bs):
    return np.tile(np.eye(bs), (n_nodes, 1))


def qr_aggregate(Ba, rank_tol=RANK_TOL):
    """(Q, R, dead) of the m x k rows of one aggregate: Gram-Schmidt in column order with a second pass."""
    m, k = Ba.shape
    Q, R = np.zeros((m, k)), np.zeros((k, k))
    dead = np.zeros(k, dtype=bool)
    for j in range(k):
        v = Ba[:, j].copy()
        n0 = np.sqrt(v @ v)
        for _ in range(2):
            c = Q[:, :j].T @ v
            v -= Q[:, :j] @ c
            R[:j, j] += c
        nv = np.sqrt(v @ v)
        if n0 == 0.0 or nv <= rank_tol * n0:
            dead[j] = True
        else:
            R[j, j] = nv
            Q[:, j] = v / nv
    return Q, R, dead


def tentative_nns_ref(agg, na, B, bs, rank_tol=RANK_TOL):
    """(T scipy CSR [n_nodes * bs][na * k] with explicit zeros of the whole Q blocks, B_next [na * k][k], dead columns)."""
    k = B.shape[1]
    n = agg.size
    Bn = np.zeros((na * k, k))
    blocks = np.zeros((n, bs, k))
    dead = 0
    for a in range(na):
        nodes = np.flatnonzero(agg == a)
        rows = (nodes[:, None] * bs + np.arange(bs)).reshape(-1)
        Q, R, d = qr_aggregate(B[rows], rank_tol)
        blocks[nodes] = Q.reshape(nodes.size, bs, k)
        Bn[a * k:(a + 1) * k] = R
        dead += int(d.sum())
    on = np.flatnonzero(agg >= 0)
    T = sp.bsr_matrix((blocks[on], agg[on], np.concatenate([[0], np.cumsum(agg >= 0)])), shape=(n * bs, na * k)).tocsr()
    return T, Bn, dead


def expand_rect(Bp, bsr, bsc):
    M = sp.kron(Bp, np.ones((bsr, bsc), dtype=np.int64), format="csr")
    M.sort_indices()
    return M.indptr.astype(np.int64), M.indices.astype(np.int32)


def amg_nns_ref(S, bs, constrained, B, max_levels=10, coarse_rows=512, sweeps=1, rank_tol=RANK_TOL):
    """The hierarchy with the near-null space B [n_rows][k]: a list of Level as amg_ref makes them, with bs per level, bs_coarse = k,
    B, T, dead (dead columns of the level's T) and P on the pattern Pp expanded to bs x k blocks."""
    levels = []
    A = S.tocsr()
    k = B.shape[1]
    indptr, indices = A.indptr.astype(np.int64), A.indices.astype(np.int32)
    mask, active = active_nodes(A.shape[0], bs, constrained)
    B = np.array(B, dtype=np.float64)
    B[mask] = 0.0
    while True:
        L = Level()
        L.A, L.indptr, L.indices, L.bs, L.sweeps, L.B = A, indptr, indices, bs, sweeps, B
        L.n_rows = A.shape[0]
        levels.append(L)
        last = L.n_rows <= coarse_rows or len(levels) >= max_levels
        if not last:
            ptr, nb = node_graph(indptr, indices, bs)
            agg, na = aggregate_ref(ptr, nb, active)
            last = na == 0 or na * k > 0.8 * L.n_rows
        if last:
            break
        L.agg, L.n_agg, L.bs_coarse = agg, na, k
        L.Pp, L.APp, L.Cp = block_patterns(ptr, nb, agg, na)
        L.Dinv = block_jacobi_ref(A, bs)
        L.rho, _ = rho_ref(A, L.Dinv)
        L.omega = (4.0 / 3.0) / L.rho
        L.T, B, L.dead = tentative_nns_ref(agg, na, B, bs, rank_tol)
        pptr, pidx = expand_rect(L.Pp, bs, k)
        L.P = on_pattern(prolongator_ref(A, L.Dinv, L.omega, L.T), pptr, pidx, (L.n_rows, na * k))
        indptr, indices = expand_rect(L.Cp, k, k)
        A = on_pattern(coarse_ref(A, L.P), indptr, indices, (na * k, na * k))
        bs = k
        active = np.ones(na, dtype=bool)
    if levels[-1].n_rows > MAX_DENSE:
        raise ValueError("coarsest level too large for the dense solve")
    levels[-1].dense_inverse = np.linalg.inv(levels[-1].A.toarray())
    return levels


def qr_bounds(Ba, Q, R):
    """Entrywise bounds on |Q^T Q - I_live| and |Q R - B_a| for the Gram-Schmidt above.

    A column product is a sum of m_a terms and a column is built from at most 2 k projections of m_a-term products plus a
    normalisation, so an entry of Q^T Q is a sum of m_a products of numbers that each carry at most (2 k + 2) roundings of sums of
    m_a terms: c = 4 (2 k + 2) in c k m_a u S, with the factor 4 of forward_bound for the products and fused multiply-adds. S is the
    sum over absolute values: |Q|^T |Q| and |Q| |R| + |B_a|. The second pass makes the loss of orthogonality of the first
    (u cond(B_a)) a second-order term as long as u cond(B_a) << 1, which rank_tol = 1e-10 enforces: a live column keeps more than
    1e-10 of its norm."""
    m, k = Ba.shape
    c = 4.0 * (2 * k + 2)
    return c * k * m * U * (np.abs(Q).T @ np.abs(Q)), c * k * m * U * (np.abs(Q) @ np.abs(R) + np.abs(Ba))


def check_tentative(agg, na, B, T, Bn, bs):
    """Property 1 of one level on given T (dense or sparse) and B_next; returns the number of dead columns seen."""
    k = B.shape[1]
    T = T.toarray() if sp.issparse(T) else T
    dead = 0
    for a in range(na):
        nodes = np.flatnonzero(agg == a)
        rows = (nodes[:, None] * bs + np.arange(bs)).reshape(-1)
        Q, R = T[rows][:, a * k:(a + 1) * k], Bn[a * k:(a + 1) * k]
        live = np.diag(R) != 0.0
        dead += int((~live).sum())
        bq, bb = qr_bounds(B[rows], Q, R)
        G = Q.T @ Q
        assert (np.abs(G - np.diag(live.astype(float))) <= bq + 4 * U).all(), (a, np.abs(G - np.diag(live.astype(float))).max())
        assert not Q[:, ~live].any()
        assert (np.abs(Q @ R - B[rows]) <= bb).all(), (a, np.abs(Q @ R - B[rows]).max())
        assert not np.tril(R, -1).any()
    outside = np.ones(T.shape, dtype=bool)                  # nothing outside the node's own aggregate
    for i in np.flatnonzero(agg >= 0):
        outside[i * bs:(i + 1) * bs, agg[i] * k:(agg[i] + 1) * k] = False
    assert not T[outside].any()
    return dead


def eps_spd(n, degree=2, clamp="bottom", distort=0.15, seed=5):
    """(mesh, S on the device pattern, constrained dofs): eps/eps with the isotropic C on triangles, SPD."""
    m = structured_mesh("triangle", n, degree, distort=distort, seed=seed)
    if clamp == "bottom":
        dofs = bottom_dofs(m, 2)
    else:                                                  # the left edge: a cantilever
        on = np.flatnonzero(np.abs(m.node_x[:, 0] - m.node_x[:, 0].min()) < 1e-12)
        dofs = (on[:, None] * 2 + np.arange(2)).reshape(-1)
    A = apply_bcs(dense_ref(m, "eps", "eps", 2, elastic_C(m)), dofs, 1.0)
    return m, to_pattern_csr(m, A, 2), dofs


def elastic_C3(n_points):
    lam, mu = 1.0, 0.7
    Ce = np.zeros((6, 6))
    Ce[:3, :3] = lam
    Ce[np.arange(6), np.arange(6)] += 2 * mu
    return np.broadcast_to(Ce, (n_points, 6, 6)).copy()


def hex_spd(n=(4, 4, 4)):
    m = structured_mesh("hexahedron", n, 1, distort=0.1, seed=2)
    dofs = bottom_dofs(m, 3)
    A = apply_bcs(dense_ref(m, "eps", "eps", 3, elastic_C3(m.num_cells * m.nq)), dofs, 1.0)
    return m, to_pattern_csr(m, A, 3), dofs


# the dead-column case: P1 triangles 6 x 5, rollers (the vertical component) on the bottom, the horizontal component held on the left
# edge, and the neighbours of one interior node clamped. Rollers alone cannot give a singleton: a partly constrained node stays active,
# so the aggregates are those of the unconstrained mesh, and these structured meshes have no singleton aggregate
# (test_dead_column_case_has_a_singleton checks the sizes 3..8 per side). Clamped neighbours leave the node alone in the graph, so it
# founds an aggregate of one node: 2 rows, 3 vectors, the rotation is dead.
DEAD_CASE = (6, 5)
DEAD_NODE = 14


def dead_case():
    m = structured_mesh("triangle", DEAD_CASE, 1, distort=0.1, seed=2)
    indptr, indices = pattern_ref(m, 2)
    ptr, nb = node_graph(indptr, indices, 2)
    ring = nb[ptr[DEAD_NODE]:ptr[DEAD_NODE + 1]]
    ring = ring[ring != DEAD_NODE]
    rollers = bottom_dofs(m, 2)[1::2]
    left = np.flatnonzero(np.abs(m.node_x[:, 0] - m.node_x[:, 0].min()) < 1e-12) * 2
    dofs = np.unique(np.concatenate([rollers, left, (ring[:, None] * 2 + np.arange(2)).reshape(-1)]))
    A = dense_ref(m, "eps", "eps", 2, elastic_C(m))
    return m, to_pattern_csr(m, apply_bcs(A, dofs, 1.0), 2), dofs


# ---- tests
def test_rigid_body_modes_are_in_the_kernel_of_the_free_operator():
    for cell, n, bs in (("triangle", (4, 3), 2), ("hexahedron", (2, 2, 2), 3)):
        m = structured_mesh(cell, n, 1, distort=0.1, seed=1)
        C = elastic_C(m) if bs == 2 else elastic_C3(m.num_cells * m.nq)
        A = dense_ref(m, "eps", "eps", bs, C)
        B = rigid_body_modes_ref(m.node_x)
        assert B.shape == (m.node_x.shape[0] * bs, 3 if bs == 2 else 6)
        assert np.abs(A @ B).max() <= 1e-12 * np.abs(A).max() * np.abs(B).max()
        assert np.linalg.matrix_rank(B) == B.shape[1]


@pytest.mark.parametrize("case", ["eps2d", "hex"])
def test_q_is_orthonormal_and_t_reproduces_b(case):
    if case == "eps2d":
        m, S, dofs = eps_spd((8, 8))
        bs = 2
    else:
        m, S, dofs = hex_spd((3, 3, 3))
        bs = 3
    levels = amg_nns_ref(S, bs, dofs, rigid_body_modes_ref(m.node_x), coarse_rows=20)
    assert len(levels) >= (3 if case == "eps2d" else 2)
    k = levels[0].B.shape[1]
    mask, _ = active_nodes(S.shape[0], bs, dofs)
    for l, (L, C) in enumerate(zip(levels[:-1], levels[1:])):
        assert L.bs == (bs if l == 0 else k) and C.bs == k and L.bs_coarse == k
        dead = check_tentative(L.agg, L.n_agg, L.B, L.T, C.B, L.bs)
        assert dead == L.dead
        free = np.repeat(L.agg >= 0, L.bs)
        if l == 0:
            free &= ~mask
            assert not L.B[mask].any()
        S_TB = abs(L.T) @ np.abs(C.B) + np.abs(L.B)
        m_max = int(np.bincount(L.agg[L.agg >= 0]).max()) * L.bs
        assert (np.abs(L.T @ C.B - L.B)[free] <= (4.0 * (2 * k + 2)) * k * m_max * U * S_TB[free]).all()
        exact = prolongator_ref(L.A, L.Dinv, L.omega, L.T)
        assert abs(exact).sum() == abs(L.P).sum()                              # nothing outside the symbolic pattern of P
        assert C.n_rows == L.n_agg * k


def test_translations_only_two_levels_equal_the_pinned_cycle():
    """Q is T with its columns scaled per aggregate: the same coarse space, an exact coarse solve, so the same cycle. The two dense
    inverses are of A_c and D A_c D (D the scaling); their errors are bounded by n_c u cond, which is the tolerance."""
    rng = np.random.Generator(np.random.PCG64(4))
    for (m, A), bs, dofs_of in ((eps_matrix((8, 7)), 2, bottom_dofs), (kro.heat_matrix(14), 1, kro.boundary_dofs)):
        S = to_pattern_csr(m, A, bs)
        dofs = dofs_of(m, bs)
        old = amg_ref(S, bs, dofs, max_levels=2, coarse_rows=1)
        new = amg_nns_ref(S, bs, dofs, translations_ref(S.shape[0] // bs, bs), max_levels=2, coarse_rows=1)
        assert len(old) == len(new) == 2 and old[1].n_rows == new[1].n_rows
        assert np.array_equal(old[0].agg, new[0].agg) and old[0].omega == new[0].omega
        nc = old[1].n_rows
        tol = 8 * nc * U * (np.linalg.cond(old[1].A.toarray()) + np.linalg.cond(new[1].A.toarray()))
        for _ in range(3):
            r = rng.normal(size=S.shape[0])
            z0, z1 = vcycle_ref(old, r), vcycle_ref(new, r)
            dev = np.linalg.norm(z1 - z0) / np.linalg.norm(z0)
            print(f"bs {bs}: two-level cycles differ by {dev:.3e} |z| (bound {tol:.3e})")
            assert dev <= tol


def _singletons(agg, na):
    return np.flatnonzero(np.bincount(agg[agg >= 0], minlength=na) == 1)


def test_dead_column_case_has_a_singleton():
    m, S, dofs = dead_case()
    ptr, nb = node_graph(S.indptr, S.indices, 2)
    on_boundary = np.any((np.abs(m.node_x - m.node_x.min(axis=0)) < 1e-12) | (np.abs(m.node_x - m.node_x.max(axis=0)) < 1e-12), axis=1)
    assert not on_boundary[nb[ptr[DEAD_NODE]:ptr[DEAD_NODE + 1]]].any()        # the node and its ring are interior
    _, active = active_nodes(S.shape[0], 2, dofs)
    agg, na = aggregate_ref(ptr, nb, active)
    single = _singletons(agg, na)
    assert single.size == 1 and agg[DEAD_NODE] == single[0]
    for nx in range(3, 9):                                                     # rollers alone: no singleton at these sizes
        for ny in range(3, 9):
            mm = structured_mesh("triangle", (nx, ny), 1, distort=0.1, seed=2)
            indptr, indices = pattern_ref(mm, 2)
            p2, n2 = node_graph(indptr, indices, 2)
            _, act = active_nodes(indptr.size - 1, 2, bottom_dofs(mm, 2)[1::2])
            assert act.all() and not _singletons(*aggregate_ref(p2, n2, act)).size


def test_a_dead_column_stays_dead_and_the_cycle_is_regular():
    m, S, dofs = dead_case()
    levels = amg_nns_ref(S, 2, dofs, rigid_body_modes_ref(m.node_x), coarse_rows=8)
    assert len(levels) >= 3
    L0 = levels[0]
    single = _singletons(L0.agg, L0.n_agg)
    assert single.size >= 1 and L0.dead >= single.size
    for l, (L, C) in enumerate(zip(levels[:-1], levels[1:])):
        check_tentative(L.agg, L.n_agg, L.B, L.T, C.B, L.bs)
        zero_rows = np.flatnonzero(~C.B.any(axis=1))                           # the dead columns of this level's T
        assert zero_rows.size == L.dead
        d = C.A.diagonal()
        assert (d[zero_rows] == 1.0).all() and (d != 0.0).all()
        if l + 2 < len(levels):                                                # dead on every coarser level too: its row of the
            Tn = levels[l + 1].T.toarray()                                     # next T is zero, nothing is interpolated to it
            assert not Tn[zero_rows].any()
    a = single[0]
    assert not levels[1].B[a * 3 + 2].any()                                    # 2 rows, 3 vectors: the rotation is the dead one
    b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
    assert np.isfinite(vcycle_ref(levels, b)).all()
    x, its, conv = cg_with_cycle(S, b, levels, rtol=1e-8, maxiter=500)
    assert conv and np.linalg.norm(b - S @ x) <= 1e-8 * np.linalg.norm(b) * (1 + 1e-6)


def _counts(S, bs, dofs, B, solver, coarse_rows=60):
    b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
    out = []
    for levels in (amg_ref(S, bs, dofs, coarse_rows=coarse_rows), amg_nns_ref(S, bs, dofs, B, coarse_rows=coarse_rows)):
        if solver == "cg":
            _, its, conv = cg_with_cycle(S, b, levels, rtol=1e-8, maxiter=3000)
        else:
            _, its, conv, _ = gmres_with_cycle(S, b, levels, m=30, rtol=1e-8, maxiter=3000)
        assert conv
        out.append((its, [L.n_rows for L in levels], operator_complexity(levels)))
    return out


@pytest.mark.parametrize("case", ["eps_p2_8", "eps_p2_14", "eps_p1_16", "cantilever_32x4", "eps_nonsym_14"])
def test_rigid_body_modes_lower_the_iteration_counts(case):
    if case == "eps_nonsym_14":
        m, A = eps_matrix((14, 14))
        S, dofs, solver = to_pattern_csr(m, A, 2), bottom_dofs(m, 2), "gmres"
    else:
        n, degree, clamp = {"eps_p2_8": ((8, 8), 2, "bottom"), "eps_p2_14": ((14, 14), 2, "bottom"), "eps_p1_16": ((16, 16), 1, "bottom"),
                            "cantilever_32x4": ((32, 4), 2, "left")}[case]
        m, S, dofs = eps_spd(n, degree, clamp)
        solver = "cg"
    (t_its, t_rows, t_c), (r_its, r_rows, r_c) = _counts(S, 2, dofs, rigid_body_modes_ref(m.node_x), solver)
    print(f"{case}: dofs {S.shape[0]}, translations {t_its} its ({t_rows}, c {t_c:.2f}), rigid-body modes {r_its} its ({r_rows}, c {r_c:.2f})")
    assert r_its < t_its, (case, r_its, t_its)


def test_hexahedra_3d():
    """P1 hexahedra 4 x 4 x 4, eps/eps SPD, bottom clamped, 375 dofs, coarse_rows = 60, CG to rtol 1e-8, right-hand side seed 1:
    translations only 30 iterations (rows 375 / 24, complexity 1.03), rigid-body modes 18 (rows 375 / 48, complexity 1.12)."""
    m, S, dofs = hex_spd((4, 4, 4))
    (t_its, t_rows, t_c), (r_its, r_rows, r_c) = _counts(S, 3, dofs, rigid_body_modes_ref(m.node_x), "cg")
    print(f"hex 4^3: dofs {S.shape[0]}, translations {t_its} its ({t_rows}, c {t_c:.2f}), rigid-body modes {r_its} its ({r_rows}, c {r_c:.2f})")
    levels = amg_nns_ref(S, 3, dofs, rigid_body_modes_ref(m.node_x), coarse_rows=60)
    assert len(levels) >= 2 and levels[0].bs == 3 and all(L.bs == 6 for L in levels[1:])
    assert r_its < t_its, (r_its, t_its)
