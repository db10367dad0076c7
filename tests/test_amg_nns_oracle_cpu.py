"""The NumPy / SciPy yardstick of dxo_amg_create_nns (csrc/amg.hip): smoothed aggregation with a near-null space, pinned on the CPU.

amg_ref(near_nullspace=B) of oracle/amg_oracle.py restates the device algorithm: today's aggregates; per level and aggregate
the rows of B of its nodes in ascending node order, orthonormalised by Gram-Schmidt in column order with a second pass (a column with
|v| <= rank_tol |v0| after the projections is dead: Q column zero, R diagonal zero); T carries the Q blocks (bs_l x k), the next B the
R factors; P = T - omega Dinv A T and A_c = P^T A P on today's block patterns expanded with bs_l rows and k columns. Every coarse level
has block size k."""
import numpy as np
import pytest

from oracle.amg_oracle import (U, active_nodes, aggregate_ref, amg_ref, cg_with_cycle, check_tentative, cycle_ref, gmres_with_cycle,
                               node_graph, operator_complexity, prolongator_ref, rigid_body_modes_ref)
from oracle.form_oracle import apply_bcs, dense_ref, pattern_ref
from oracle.krylov_oracle import bottom_dofs, boundary_dofs, elastic_C, elastic_C3, eps_matrix, heat_matrix, to_pattern_csr
from solver_cases import DEAD_NODE, dead_case, eps_spd
from tools.synthetic import structured_mesh


def translations_ref(n_nodes, bs):
    return np.tile(np.eye(bs), (n_nodes, 1))


def hex_spd(n=(4, 4, 4)):
    m = structured_mesh("hexahedron", n, 1, distort=0.1, seed=2)
    dofs = bottom_dofs(m, 3)
    A = apply_bcs(dense_ref(m, "eps", "eps", 3, elastic_C3(m.num_cells * m.nq)), dofs, 1.0)
    return m, to_pattern_csr(m, A, 3), dofs


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
    levels = amg_ref(S, bs, dofs, near_nullspace=rigid_body_modes_ref(m.node_x), coarse_rows=20)
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
    for (m, A), bs, dofs_of in ((eps_matrix((8, 7)), 2, bottom_dofs), (heat_matrix(14), 1, boundary_dofs)):
        S = to_pattern_csr(m, A, bs)
        dofs = dofs_of(m, bs)
        old = amg_ref(S, bs, dofs, max_levels=2, coarse_rows=1)
        new = amg_ref(S, bs, dofs, near_nullspace=translations_ref(S.shape[0] // bs, bs), max_levels=2, coarse_rows=1)
        assert len(old) == len(new) == 2 and old[1].n_rows == new[1].n_rows
        assert np.array_equal(old[0].agg, new[0].agg) and old[0].omega == new[0].omega
        nc = old[1].n_rows
        tol = 8 * nc * U * (np.linalg.cond(old[1].A.toarray()) + np.linalg.cond(new[1].A.toarray()))
        for _ in range(3):
            r = rng.normal(size=S.shape[0])
            z0, z1 = cycle_ref(old, r), cycle_ref(new, r)
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
    levels = amg_ref(S, 2, dofs, near_nullspace=rigid_body_modes_ref(m.node_x), coarse_rows=8)
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
    assert np.isfinite(cycle_ref(levels, b)).all()
    x, its, conv = cg_with_cycle(S, b, levels, rtol=1e-8, maxiter=500)
    assert conv and np.linalg.norm(b - S @ x) <= 1e-8 * np.linalg.norm(b) * (1 + 1e-6)


def _counts(S, bs, dofs, B, solver, coarse_rows=60):
    b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
    out = []
    for levels in (amg_ref(S, bs, dofs, coarse_rows=coarse_rows), amg_ref(S, bs, dofs, near_nullspace=B, coarse_rows=coarse_rows)):
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
    levels = amg_ref(S, 3, dofs, near_nullspace=rigid_body_modes_ref(m.node_x), coarse_rows=60)
    assert len(levels) >= 2 and levels[0].bs == 3 and all(L.bs == 6 for L in levels[1:])
    assert r_its < t_its, (r_its, t_its)
