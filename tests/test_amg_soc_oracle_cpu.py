"""The NumPy / SciPy yardstick of dxo_amg_create_soc (csrc/amg.hip): strength-of-connection coarsening and filtered prolongator
smoothing, pinned on the CPU (oracle/amg_oracle.py).

strength_ref: block (i, j), i != j, is strong when |A_ij|_F^2 >= theta^2 |A_ii|_F |A_jj|_F or the same holds for (j, i); diagonal
blocks are strong. The squares are formed on entries scaled by a power of two, so the mask does not depend on the scale of A.
amg_ref(strength=theta): today's three passes on the strong graph, P on the pattern (strong graph) x (aggregates), A P and
P^T A P on the full graph, P = T - omega_F Dinv_F A^F T with A^F the matrix without its weak blocks, each added onto the diagonal
block of its row, Dinv_F the inverses of the lumped blocks (A_ii's where the lumped block fails Hadamard's test, zero for a node
without a strong neighbour) and omega_F = (4/3) / rho_F from the selected estimate of Dinv_F A^F. The sweeps keep A, Dinv and rho, so
the cycle is cycle_ref. `frozen` takes the masks and aggregates of an earlier hierarchy, as dxo_amg_setup does.

Measured here (CG, rtol 1e-8, coarse_rows 60, theta 0.25, one Jacobi sweep, C = diag(1, 1e-3), 625 dofs); the figures are printed by
test_iteration_counts_on_the_anisotropic_systems:
    P1 quadrilaterals 24^2:           107 iterations without strength (rows 625 / 64 / 9, complexity 1.10), 18 with
                                      (625 / 184 / 69 / 46, 1.41); smoothing with the unfiltered matrix 20 (2.17)
    P1 triangles 24^2, distort 0.1:    80 iterations without strength (625 / 64 / 8, 1.14), 12 with (625 / 184 / 69, 1.47);
                                      smoothing with the unfiltered matrix 11 (2.93)"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph

from oracle.amg_oracle import (U, amg_ref, cg_with_cycle, cycle_ref, filtered_ref, lumped_inverse_ref, node_graph, on_pattern, ones_pattern,
                               operator_complexity, rigid_body_modes_ref, same_csr, strength_ref, strength_unscaled_ref)
from oracle.form_oracle import apply_bcs, dense_ref
from oracle.krylov_oracle import bottom_dofs, boundary_dofs, elastic_C, elastic_C3, to_pattern_csr
from solver_cases import GPU_THETAS, THETA, cached_aniso
from tools.synthetic import structured_mesh


# ---- the systems
def isotropic_q1_system(n=20):
    """Q1 on uniform squares with C = I: every neighbour at a_ii / 8, so theta = 0.25 leaves nothing strong; (n - 1)^2 interior nodes
    of (n + 1)^2 are more than 0.8 of the rows from n = 18 on."""
    m = structured_mesh("quadrilateral", (n, n), 1)
    C = np.broadcast_to(np.eye(2), (m.num_cells * m.nq, 2, 2)).copy()
    dofs = boundary_dofs(m, 1)
    return m, to_pattern_csr(m, apply_bcs(dense_ref(m, "grad", "grad", 1, C), dofs, 1.0), 1), dofs


def eps_rbm_system(cell="triangle", n=(6, 5), degree=2):
    """(mesh, S, constrained dofs, rigid-body modes): eps/eps with the isotropic C, clamped at the bottom."""
    m = structured_mesh(cell, n, degree, distort=0.1, seed=2)
    g = m.gdim
    dofs = bottom_dofs(m, g)
    C = elastic_C(m) if g == 2 else elastic_C3(m.num_cells * m.nq)
    S = to_pattern_csr(m, apply_bcs(dense_ref(m, "eps", "eps", g, C), dofs, 1.0), g)
    return m, S, dofs, rigid_body_modes_ref(m.node_x)


# ---- tests
def test_theta_zero_is_the_hierarchy_of_today():
    m, S, dofs = cached_aniso("triangle", 12)
    for ref, soc in ((amg_ref(S, 1, dofs, coarse_rows=6), amg_ref(S, 1, dofs, strength=0.0, filtered=True, coarse_rows=6)),):
        assert len(ref) == len(soc) >= 3
        for a, b in zip(ref, soc):
            assert same_csr(a.A, b.A)
        for a, b in zip(ref[:-1], soc[:-1]):
            assert b.strong.all() and np.array_equal(a.agg, b.agg) and same_csr(a.P, b.P) and a.omega == b.omega_f
    m, S, dofs, B = eps_rbm_system()
    ref = amg_ref(S, 2, dofs, near_nullspace=B, coarse_rows=20)
    soc = amg_ref(S, 2, dofs, near_nullspace=B, strength=0.0, filtered=True, coarse_rows=20)
    assert len(ref) == len(soc) >= 2
    for a, b in zip(ref, soc):
        assert same_csr(a.A, b.A)
    for a, b in zip(ref[:-1], soc[:-1]):
        assert np.array_equal(a.agg, b.agg) and same_csr(a.P, b.P) and same_csr(a.T, b.T)


@pytest.mark.parametrize("theta", [0.05, 0.25, 0.6])
def test_mask_is_symmetric_with_a_strong_diagonal(theta):
    for _, S, bs, dofs, B in _systems():
        levels = amg_ref(S, bs, dofs, near_nullspace=B, strength=theta, coarse_rows=20)
        for L in levels[:-1]:
            ptr, nb = node_graph(L.indptr, L.indices, L.bs)
            n = ptr.size - 1
            M = sp.csr_matrix((L.strong.astype(np.int64), nb, ptr), shape=(n, n))
            assert (M != M.T).nnz == 0                                  # the patterns are structurally symmetric
            assert (M.diagonal() == 1).all()


def test_mask_on_the_uniform_stencils():
    """Q1 on unit squares: the anisotropic stencil has x-neighbours at 0.5 a_ii, y-neighbours at 0.2493 a_ii and corners at 0.125 a_ii;
    the isotropic one has every neighbour at a_ii / 8. theta = 0.25 keeps the x-neighbours alone, and nothing."""
    m, S, dofs = cached_aniso("quadrilateral")
    strong, closest = strength_ref(S, S.indptr, S.indices, 1, THETA)
    free = np.ones(S.shape[0], dtype=bool)
    free[dofs] = False
    ptr, nb = node_graph(S.indptr, S.indices, 1)
    row = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    dx = m.node_x[nb] - m.node_x[row]
    h = 1.0 / 24
    x_nb = (np.abs(np.abs(dx[:, 0]) - h) < 1e-12) & (np.abs(dx[:, 1]) < 1e-12)
    inner = free[row] & free[nb]
    assert np.array_equal(strong[inner], (x_nb | (row == nb))[inner])
    assert not strong[~inner & (row != nb)].any()                       # a zeroed coupling to a Dirichlet node is weak
    assert closest > 1e-3
    m, S, dofs = isotropic_q1_system()
    strong, _ = strength_ref(S, S.indptr, S.indices, 1, THETA)
    ptr, nb = node_graph(S.indptr, S.indices, 1)
    assert np.array_equal(strong, np.repeat(np.arange(ptr.size - 1), np.diff(ptr)) == nb)
    levels = amg_ref(S, 1, dofs, strength=THETA, coarse_rows=10)
    assert len(levels) == 1                                              # every node alone, 361 of 441: the 0.8 rule stops at once
    r = np.arange(S.shape[0], dtype=float)
    assert np.allclose(S @ cycle_ref(levels, r), r, atol=1e-9 * np.abs(r).max())


def _systems():
    m, S, dofs = cached_aniso("triangle")
    yield "aniso", S, 1, dofs, None
    m, S, dofs, B = eps_rbm_system()
    yield "eps_rbm", S, 2, dofs, B


def test_filtered_matrix_keeps_the_row_sums_and_the_strong_pattern():
    for name, S, bs, dofs, B in _systems():
        for L in amg_ref(S, bs, dofs, near_nullspace=B, strength=THETA, coarse_rows=20)[:-1]:
            b = L.bs
            n = L.n_rows // b
            E = sp.kron(np.ones((n, 1)), np.eye(b), format="csr")            # block row sums, component by component
            sa, sf = (L.A @ E).toarray(), (L.AF @ E).toarray()
            scale = (abs(L.A) @ E).toarray()
            assert (np.abs(sa - sf) <= 64 * U * scale).all(), name
            ptr, nb = node_graph(L.indptr, L.indices, b)
            Gs = sp.csr_matrix((L.strong.astype(np.int64), nb, ptr), shape=(n, n))
            Gs.eliminate_zeros()
            pat = sp.kron(Gs, np.ones((b, b)), format="csr")
            assert abs(L.AF).multiply(pat).sum() == abs(L.AF).sum(), name     # nothing outside the strong graph
            assert (L.Pp != ones_pattern(Gs @ ones_pattern(sp.csr_matrix((np.ones((L.agg >= 0).sum()), (np.flatnonzero(L.agg >= 0), L.agg[L.agg >= 0])),
                                                             shape=(n, L.n_agg))))).nnz == 0


def test_a_node_without_a_strong_neighbour_keeps_its_row_of_t():
    """One interior node of the anisotropic quadrilateral system gets a diagonal entry 100 times larger: every coupling of it is weak
    (0.5 / 10 < 0.25), it founds an aggregate of its own among strong neighbours, and its row of P is its row of T."""
    m, S, dofs = cached_aniso("quadrilateral", 12)
    S = S.copy()
    free = np.setdiff1d(np.arange(S.shape[0]), dofs)
    lone = free[free.size // 2]
    d = S.indptr[lone] + np.flatnonzero(S.indices[S.indptr[lone]:S.indptr[lone + 1]] == lone)[0]
    S.data[d] *= 100.0
    levels = amg_ref(S, 1, dofs, strength=THETA, coarse_rows=20)
    L = levels[0]
    assert L.n_strong_off[lone] == 0 and (L.agg == L.agg[lone]).sum() == 1
    assert not L.Dinv_f[lone].any() and not L.fell[lone]
    assert same_csr(L.P[lone].tocsr(), on_pattern(L.T, L.P.indptr, L.P.indices, L.P.shape)[lone].tocsr()) and L.P[lone].sum() == 1.0
    assert (L.n_strong_off[free] > 0).sum() >= free.size - 1 - 2 * 11           # the others are smoothed (but for rows next to it)
    x, its, conv = cg_with_cycle(S, np.ones(S.shape[0]), levels, rtol=1e-8)
    assert conv and np.isfinite(x).all()


def test_a_near_singular_lumped_block_falls_back_and_is_counted():
    """bs 2, three nodes in a chain: node 1 couples strongly to node 0 and weakly to node 2, and its diagonal block is chosen so
    that the lumped block A_11 + A_12 has dependent rows: it fails Hadamard's test, Dinv_F takes the inverse of A_11, and the node
    is counted."""
    D = np.array([[2.0, 0.5], [0.5, 1.0]])
    W = np.array([[1.0, 0.0], [0.0, -1.0]]) * 1e-3                          # small: weak at theta 0.25
    A = np.zeros((6, 6))
    for i in range(3):
        A[2 * i:2 * i + 2, 2 * i:2 * i + 2] = D
    A[0:2, 2:4] = A[2:4, 0:2] = -0.6 * np.eye(2)
    A[2:4, 4:6] = W
    A[4:6, 2:4] = W.T
    # make the lumped block of node 1 singular: A_11 + W must have dependent rows
    A[2:4, 2:4] = np.array([[2.0, 0.5], [1.0, 0.25]]) - W
    S = sp.csr_matrix(np.where(np.kron(np.array([[1, 1, 0], [1, 1, 1], [0, 1, 1]]), np.ones((2, 2))) > 0, 1.0, 0.0))
    S.data = A[S.nonzero()]
    mask, _ = strength_ref(S, S.indptr, S.indices, 2, THETA)
    ptr, nb = node_graph(S.indptr, S.indices, 2)
    assert mask.tolist() == [True, True, True, True, False, False, True]
    AF, lumped, diag, n_strong = filtered_ref(S, S.indptr, S.indices, 2, mask)
    assert abs(np.linalg.det(lumped[1])) <= 1e-14
    Dinv_f, fell = lumped_inverse_ref(lumped, diag, n_strong)
    assert fell.tolist() == [False, True, False]
    assert np.allclose(Dinv_f[1], np.linalg.inv(diag[1])) and np.isfinite(Dinv_f).all()
    assert not Dinv_f[2].any()                                              # node 2 has no strong neighbour
    assert np.allclose(Dinv_f[0], np.linalg.inv(D))


def test_every_aggregate_is_connected_in_the_strong_graph():
    for name, S, bs, dofs, B in _systems():
        for theta in (0.1, THETA):
            for L in amg_ref(S, bs, dofs, near_nullspace=B, strength=theta, coarse_rows=20)[:-1]:
                ptr, nb = node_graph(L.indptr, L.indices, L.bs)
                n = ptr.size - 1
                Gs = sp.csr_matrix((L.strong.astype(np.int64), nb, ptr), shape=(n, n))
                for a in range(L.n_agg):
                    members = np.flatnonzero(L.agg == a)
                    ncomp, _ = scipy.sparse.csgraph.connected_components(Gs[members][:, members], directed=False)
                    assert ncomp == 1, (name, theta, a)


def test_frozen_masks_reproduce_the_hierarchy_and_survive_new_values():
    m, S, dofs = cached_aniso("triangle", 12)
    first = amg_ref(S, 1, dofs, strength=THETA, coarse_rows=6)
    again = amg_ref(S, 1, dofs, strength=THETA, coarse_rows=6, frozen=first)
    assert len(first) == len(again) >= 3
    for a, b in zip(first[:-1], again[:-1]):
        assert same_csr(a.P, b.P) and same_csr(a.A, b.A)
    S2 = S.copy()
    S2.data = S.data * (1.0 + 0.05 * np.cos(np.arange(S.data.size)))
    other = amg_ref(S2, 1, dofs, strength=THETA, coarse_rows=6, frozen=first)
    for a, b in zip(first[:-1], other[:-1]):
        assert np.array_equal(a.agg, b.agg) and np.array_equal(a.strong, b.strong) and np.array_equal(a.P.indices, b.P.indices)
        assert not np.array_equal(a.P.data, b.P.data)


def gpu_system_ref(which):
    """(mesh, S, bs, constrained dofs, rigid-body modes or None) of the systems of tests/test_amg_soc_gpu.py."""
    if which in ("aniso_quad", "aniso_tri"):
        m, S, dofs = cached_aniso("quadrilateral" if which == "aniso_quad" else "triangle")
        return m, S, 1, dofs, None
    if which == "p2_tri_rbm":
        m, S, dofs, B = eps_rbm_system("triangle", (6, 5), 2)
        return m, S, 2, dofs, B
    m, S, dofs, B = eps_rbm_system("hexahedron", (3, 2, 3), 1)
    return m, S, 3, dofs, B


@pytest.mark.parametrize("which", sorted(GPU_THETAS))
def test_no_block_of_the_gpu_systems_lies_at_the_threshold(which):
    """The condition under which the device mask must equal the oracle's exactly: no test value within 4 K u of its threshold, K the
    bs^2 terms of a block norm (far from it: the closest is printed)."""
    m, S, bs, dofs, B = gpu_system_ref(which)
    levels = amg_ref(S, bs, dofs, near_nullspace=B, strength=GPU_THETAS[which], coarse_rows=60 if bs == 1 else 20)
    assert len(levels) >= 2
    for l, L in enumerate(levels[:-1]):
        print(f"{which} level {l}: closest test value {L.closest:.3e} of its threshold away, {int(L.strong.sum())} of {L.strong.size} strong")
        assert L.closest > 1e3 * 4 * L.bs * L.bs * U, (which, l, L.closest)
        assert not L.strong.all() or l > 0, which


SCALE_EXPONENTS = (996, -900, 520, -540)      # near both ends of double; where the unscaled squares first overflow / underflow


@pytest.mark.parametrize("which", sorted(GPU_THETAS))
def test_masks_do_not_depend_on_the_scale_of_the_matrix(which):
    """Every level of the GPU systems: the range-safe masks at scale 1 are those of the unscaled arithmetic (same `closest` too: the
    two sides of a comparison are scaled by the same power of two), and the masks of 2^e A are the masks of A for the four
    exponents. The unscaled arithmetic loses the mask of level 0 at every one of them (asserted, so that the exponents stay meaningful)."""
    m, S, bs, dofs, B = gpu_system_ref(which)
    theta = GPU_THETAS[which]
    levels = amg_ref(S, bs, dofs, near_nullspace=B, strength=theta, coarse_rows=60 if bs == 1 else 20)
    assert len(levels) >= 2
    for l, L in enumerate(levels[:-1]):
        old, old_closest = strength_unscaled_ref(L.A, L.indptr, L.indices, L.bs, theta)
        new, new_closest = strength_ref(L.A, L.indptr, L.indices, L.bs, theta)
        assert np.array_equal(new, old) and np.array_equal(new, L.strong) and new_closest == old_closest, (which, l)
        assert not new.all() or l > 0
        for e in SCALE_EXPONENTS:
            As = L.A.copy()
            As.data = np.ldexp(L.A.data, e)
            assert np.isfinite(As.data).all() and np.array_equal(np.ldexp(As.data, -e), L.A.data)
            scaled, closest = strength_ref(As, L.indptr, L.indices, L.bs, theta)
            assert np.array_equal(scaled, new) and closest == new_closest, (which, l, e)
            with np.errstate(over="ignore", invalid="ignore"):            # inf >= inf and 0 >= 0 are what it is kept for
                lost, _ = strength_unscaled_ref(As, L.indptr, L.indices, L.bs, theta)
            print(f"{which} level {l} scale 2^{e}: {int(new.sum())} strong of {new.size}; unscaled arithmetic {int(lost.sum())}")
            assert l > 0 or not np.array_equal(lost, new), (which, l, e)


def test_iteration_counts_on_the_anisotropic_systems():
    for cell in ("quadrilateral", "triangle"):
        m, S, dofs = cached_aniso(cell)
        b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
        plain = amg_ref(S, 1, dofs, coarse_rows=60)
        soc = amg_ref(S, 1, dofs, strength=THETA, coarse_rows=60)
        full = amg_ref(S, 1, dofs, strength=THETA, coarse_rows=60, filtered=False)
        _, its0, conv0 = cg_with_cycle(S, b, plain, rtol=1e-8)
        x, its1, conv1 = cg_with_cycle(S, b, soc, rtol=1e-8)
        _, its2, conv2 = cg_with_cycle(S, b, full, rtol=1e-8)
        print(f"{cell}: no strength {its0} its, rows {[L.n_rows for L in plain]}, complexity {operator_complexity(plain):.2f}; "
              f"theta {THETA} filtered {its1} its, rows {[L.n_rows for L in soc]}, complexity {operator_complexity(soc):.2f}; "
              f"unfiltered {its2} its, complexity {operator_complexity(full):.2f}")
        assert conv0 and conv1 and conv2
        assert 2 * its1 <= its0, (cell, its1, its0)
        assert operator_complexity(soc) < operator_complexity(full), cell
        assert np.linalg.norm(S @ x - b) <= 1e-7 * np.linalg.norm(b)


def test_chebyshev_and_power_iteration_on_a_strength_hierarchy():
    m, S, dofs = cached_aniso("triangle")
    b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
    levels = amg_ref(S, 1, dofs, strength=THETA, smoother="chebyshev", rho="power", degree=2, coarse_rows=60)
    jac = amg_ref(S, 1, dofs, strength=THETA, coarse_rows=60)
    for a, c in zip(jac[:-1], levels[:-1]):
        assert np.array_equal(a.strong, c.strong) and np.array_equal(a.agg, c.agg)
        assert 0.0 < c.rho_f != a.rho_f and c.omega_f == (4.0 / 3.0) / c.rho_f  # omega_F follows the selected estimate
    x, its, conv = cg_with_cycle(S, b, levels, rtol=1e-8)
    _, its_j, _ = cg_with_cycle(S, b, jac, rtol=1e-8)
    assert conv and its <= its_j
