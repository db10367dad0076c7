"""The NumPy / SciPy yardstick of dxo_amg_* (csrc/amg.hip), pinned on the CPU.

amg_ref restates the device algorithm: the node graph of the block pattern without the fully constrained nodes, aggregation in three
passes in ascending node order, the tentative prolongator T (a bs x bs identity per node, the rows of masked dofs zero),
P = T - omega Dinv A T with omega = (4/3) / |Dinv A|_inf, A_c = P^T A P on the symbolic pattern (an exactly zero diagonal entry
becomes 1), recursion until a level is small, stagnates or max_levels is reached, a dense inverse on the coarsest level. cycle_ref is
the cycle: `sweeps` damped block-Jacobi sweeps (the first from zero), restriction by P^T, recursion, prolongation, `sweeps` sweeps.
Both are in oracle/amg_oracle.py; the defaults of amg_ref are checked here against mathematics and scipy.sparse.linalg.spsolve."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph
import scipy.sparse.linalg

from oracle.amg_oracle import (active_nodes, aggregate_ref, amg_ref, cg_with_cycle, cycle_ref, gmres_with_cycle, node_graph,
                               operator_complexity, prolongator_ref)
from oracle.form_oracle import apply_bcs, pattern_ref
from oracle.krylov_oracle import (block_jacobi_ref, bottom_dofs, boundary_dofs, cg_ref, eps_matrix, gmres_ref, heat_matrix,
                                  to_pattern_csr)
from tools.synthetic import structured_mesh


# ---- tests
MESHES = [("triangle", (7, 6)), ("quadrilateral", (6, 6)), ("tetrahedron", (3, 3, 2)), ("hexahedron", (3, 2, 3))]


@pytest.mark.parametrize("cell,n", MESHES)
@pytest.mark.parametrize("degree", [1, 2])
def test_aggregates_partition_the_active_nodes(cell, n, degree):
    m = structured_mesh(cell, n, degree, distort=0.1, seed=2)
    for bs, dofs in ((1, boundary_dofs(m, 1)), (m.gdim, bottom_dofs(m, m.gdim)), (m.gdim, bottom_dofs(m, m.gdim)[::m.gdim]), (1, [])):
        indptr, indices = pattern_ref(m, bs)
        ptr, nb = node_graph(indptr, indices, bs)
        mask, active = active_nodes(indptr.size - 1, bs, dofs)
        agg, na = aggregate_ref(ptr, nb, active)
        assert (agg[~active] == -1).all() and (agg[active] >= 0).all()        # every active node in exactly one aggregate
        assert np.array_equal(np.unique(agg[active]), np.arange(na))
        if len(dofs) and len(dofs) % bs == 0 and bs * np.unique(np.asarray(dofs) // bs).size == len(dofs):
            assert (~active).sum() == len(dofs) // bs
        else:
            assert active.all()                                                # partly constrained nodes stay active
        G = sp.csr_matrix((np.ones(nb.size), nb, ptr), shape=(agg.size, agg.size))
        for a in range(na):                                                    # every aggregate is connected in the graph
            members = np.flatnonzero(agg == a)
            ncomp, _ = scipy.sparse.csgraph.connected_components(G[members][:, members], directed=False)
            assert ncomp == 1, (cell, degree, a)
        again, na2 = aggregate_ref(ptr.copy(), nb.copy(), active.copy())       # a function of the pattern and the list alone
        assert na2 == na and np.array_equal(again, agg)
        assert na < 0.5 * active.sum()                                         # it coarsens


def _cases():
    m, A = heat_matrix(20)
    yield "heat", to_pattern_csr(m, A, 1), 1, boundary_dofs(m, 1)
    m, A = eps_matrix((8, 7))
    yield "eps", to_pattern_csr(m, A, 2), 2, bottom_dofs(m, 2)


def test_transfer_and_coarse_matrices():
    for name, S, bs, dofs in _cases():
        levels = amg_ref(S, bs, dofs, coarse_rows=10)
        assert len(levels) >= 3, name
        for L, C in zip(levels[:-1], levels[1:]):
            free = ~L.mask & (np.repeat(L.agg, bs) >= 0)
            sums = np.asarray(L.T.sum(axis=1)).ravel()
            assert np.array_equal(sums[free], np.ones(free.sum())) and not sums[~free].any()
            exact = prolongator_ref(L.A, L.Dinv, L.omega, L.T)
            assert abs(exact).sum() == abs(L.P).sum()                          # nothing outside the symbolic pattern of P
            Ac = (L.P.T @ L.A @ L.P).toarray()
            d = np.flatnonzero(np.diag(Ac) == 0.0)
            Ac[d, d] = 1.0
            assert np.abs(C.A.toarray() - Ac).max() <= 1e-13 * np.abs(Ac).max(), name
            # the csr.h layout: the rows of a node share their columns, runs m*bs + j, sorted, diagonal present
            ptr, idx = C.indptr, C.indices
            for node in range(C.n_rows // bs):
                cols = idx[ptr[node * bs]:ptr[node * bs + 1]]
                assert (np.diff(cols) > 0).all() and cols.size % bs == 0
                assert np.array_equal(cols.reshape(-1, bs), cols[::bs, None] + np.arange(bs)) and (cols[::bs] % bs == 0).all()
                assert node * bs in cols
                for i in range(1, bs):
                    assert np.array_equal(idx[ptr[node * bs + i]:ptr[node * bs + i + 1]], cols)
            assert 0.0 < L.omega and L.rho >= 1.0 - 1e-12                      # a Dirichlet row alone gives |Dinv A| = 1
        assert 1.0 < operator_complexity(levels) < 2.0, name


def test_a_fully_constrained_aggregate_column_gets_a_unit_diagonal():
    m, A = eps_matrix((6, 5))
    rollers = bottom_dofs(m, 2)[1::2]                     # the vertical component only: the nodes stay active
    S = to_pattern_csr(m, apply_bcs(A, rollers, 1.0), 2)
    levels = amg_ref(S, 2, rollers, coarse_rows=10)
    for L in levels[:-1]:
        assert not np.asarray(abs(L.P[np.flatnonzero(L.mask)]).sum(axis=1)).any()      # masked rows of P are zero
    d = levels[1].A.diagonal()
    assert (d != 0.0).all()
    x = cycle_ref(levels, np.ones(S.shape[0]))
    assert np.isfinite(x).all()


def test_cycle_is_linear_and_symmetric_for_an_spd_matrix():
    rng = np.random.Generator(np.random.PCG64(11))
    m, A = eps_matrix(nonsym_seed=None)                   # the matrix of test_cg_oracle_on_an_spd_elastic_matrix
    S = to_pattern_csr(m, A, 2)
    for sweeps in (1, 2):
        levels = amg_ref(S, 2, bottom_dofs(m, 2), coarse_rows=30, sweeps=sweeps)
        assert len(levels) >= 2
        r1, r2 = rng.normal(size=(2, S.shape[0]))
        z1, z2 = cycle_ref(levels, r1), cycle_ref(levels, r2)
        z = cycle_ref(levels, 2.5 * r1 + r2)
        assert np.linalg.norm(z - (2.5 * z1 + z2)) <= 1e-13 * np.linalg.norm(z)
        assert abs(r2 @ z1 - r1 @ z2) <= 1e-12 * (np.linalg.norm(r1) * np.linalg.norm(z2))
        assert r1 @ z1 > 0 and r2 @ z2 > 0
        x, its, conv = cg_with_cycle(S, r1, levels, rtol=1e-10)
        _, its_bj, _ = cg_ref(S, r1, inv=block_jacobi_ref(S, 2), rtol=1e-10)
        assert conv and its < its_bj
        assert np.linalg.norm(x - scipy.sparse.linalg.spsolve(S.tocsc(), r1)) <= 1e-8 * np.linalg.norm(x)


def test_gmres_with_the_cycle_beats_block_jacobi_and_scales():
    counts = {}
    for name, (m, A), bs, dofs_of in (("heat32", heat_matrix(32), 1, boundary_dofs), ("heat64", heat_matrix(64), 1, boundary_dofs),
                                      ("eps14", eps_matrix((14, 14)), 2, bottom_dofs)):
        S = to_pattern_csr(m, A, bs)
        b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
        ref = scipy.sparse.linalg.spsolve(S.tocsc(), b)
        levels = amg_ref(S, bs, dofs_of(m, bs), coarse_rows=300)
        assert len(levels) >= 2
        x, its, conv, res = gmres_with_cycle(S, b, levels, m=30, rtol=1e-8, maxiter=3000)
        assert conv and res <= 1e-8, name
        assert np.linalg.norm(x - ref) <= 1e-6 * np.linalg.norm(ref), name
        _, its_bj, _, _ = gmres_ref(S, b, inv=block_jacobi_ref(S, bs), m=30, rtol=1e-8, maxiter=3000)
        print(f"{name}: dofs {S.shape[0]}, level rows {[L.n_rows for L in levels]}, complexity {operator_complexity(levels):.3f}, "
              f"block Jacobi {its_bj} its, V(1,1) {its} its")
        assert its < its_bj, (name, its, its_bj)
        counts[name] = (its, its_bj)
    assert counts["heat64"][0] - counts["heat32"][0] < counts["heat64"][1] - counts["heat32"][1]


def test_stagnation_and_size_rules():
    m, A = heat_matrix(12)
    S = to_pattern_csr(m, A, 1)
    assert len(amg_ref(S, 1, boundary_dofs(m, 1), max_levels=1)) == 1
    assert len(amg_ref(S, 1, boundary_dofs(m, 1), coarse_rows=10 ** 6)) == 1
    assert len(amg_ref(S, 1, boundary_dofs(m, 1), max_levels=2, coarse_rows=1)) == 2
    # without the rule for constrained nodes nothing changes on a matrix without constraints: every node is active
    levels = amg_ref(S, 1, [], coarse_rows=10)
    rows = [L.n_rows for L in levels]
    assert all(b <= 0.8 * a for a, b in zip(rows, rows[1:]))
    one = amg_ref(S, 1, boundary_dofs(m, 1), max_levels=1)
    r = np.arange(S.shape[0], dtype=float)
    assert np.allclose(S @ cycle_ref(one, r), r, atol=1e-9 * np.abs(r).max())          # a single level is the direct solve
