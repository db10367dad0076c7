"""The NumPy / SciPy yardstick of dxo_amg_* (csrc/amg.hip), pinned on the CPU.

amg_ref restates the device algorithm: the node graph of the block pattern without the fully constrained nodes, aggregation in three
passes in ascending node order, the tentative prolongator T (a bs x bs identity per node, the rows of masked dofs zero),
P = T - omega Dinv A T with omega = (4/3) / |Dinv A|_inf, A_c = P^T A P on the symbolic pattern (an exactly zero diagonal entry
becomes 1), recursion until a level is small, stagnates or max_levels is reached, a dense inverse on the coarsest level. vcycle_ref is
the cycle: `sweeps` damped block-Jacobi sweeps (the first from zero), restriction by P^T, recursion, prolongation, `sweeps` sweeps.
The patterns come from integer sparse products, not from the loops the library runs, and the numbers from scipy.sparse products.
Checked here against mathematics and scipy.sparse.linalg.spsolve."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph
import scipy.sparse.linalg

import test_krylov_oracle_cpu as kro
from test_assemble_oracle_cpu import pattern_ref
from test_krylov_oracle_cpu import (block_jacobi_ref, bottom_dofs, boundary_dofs, cg_ref, eps_matrix, gmres_ref, heat_matrix,
                                    to_pattern_csr)
from tools.synthetic import structured_mesh

U = 2.0 ** -53
MAX_DENSE = 4096


# ---- symbolic phase
def node_graph(indptr, indices, bs):
    """(ptr, nb): sorted neighbour nodes of every node of a csr.h pattern, the node itself included."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n_nodes = (indptr.size - 1) // bs
    starts = indptr[0:-1:bs]
    counts = (indptr[1::bs] - starts) // bs
    ptr = np.concatenate([[0], np.cumsum(counts)])
    nb = np.concatenate([indices[s:s + c * bs:bs] // bs for s, c in zip(starts, counts)]) if n_nodes else np.zeros(0, dtype=np.int64)
    return ptr, nb.astype(np.int64)


def active_nodes(n_rows, bs, constrained):
    mask = np.zeros(n_rows, dtype=bool)
    c = np.asarray(constrained, dtype=np.int64).reshape(-1)
    mask[c[(c >= 0) & (c < n_rows)]] = True
    return mask, ~mask.reshape(-1, bs).all(axis=1)


def aggregate_ref(ptr, nb, active):
    """Aggregate of every node (-1: inactive) and the number of aggregates; three passes in ascending node order."""
    n = ptr.size - 1
    agg = -np.ones(n, dtype=np.int64)
    na = 0
    nbs = [nb[ptr[i]:ptr[i + 1]][active[nb[ptr[i]:ptr[i + 1]]]] for i in range(n)]
    for i in range(n):
        if active[i] and (agg[nbs[i]] < 0).all():
            agg[nbs[i]] = na
            na += 1
    first = agg.copy()
    for i in range(n):
        if active[i] and first[i] < 0:
            cand = first[nbs[i]]
            cand = cand[cand >= 0]
            if cand.size:
                agg[i] = cand.min()
    for i in range(n):
        if active[i] and agg[i] < 0:
            free = nbs[i][agg[nbs[i]] < 0]
            agg[free] = na
            na += 1
    return agg, na


def block_patterns(ptr, nb, agg, na):
    """Block patterns (scipy CSR of ones, sorted) of P, A P and P^T A P from integer products of the graph and the aggregates."""
    n = ptr.size - 1
    G = sp.csr_matrix((np.ones(nb.size, dtype=np.int64), nb, ptr), shape=(n, n))
    on = np.flatnonzero(agg >= 0)
    Tg = sp.csr_matrix((np.ones(on.size, dtype=np.int64), (on, agg[on])), shape=(n, na))
    out = []
    Pp = G @ Tg
    APp = G @ _ones(Pp)
    Cp = _ones(Pp).T @ _ones(APp) + sp.identity(na, dtype=np.int64, format="csr")
    for M in (Pp, APp, Cp):
        M = _ones(M.tocsr())
        M.sort_indices()
        out.append(M)
    return out


def _ones(M):
    M = M.tocsr().copy()
    M.data = np.ones_like(M.data)
    return M


def expand_pattern(Bp, bs):
    """csr.h layout of a block pattern: (indptr int64, indices int32)."""
    M = sp.kron(Bp, np.ones((bs, bs), dtype=np.int64), format="csr")
    M.sort_indices()
    return M.indptr.astype(np.int64), M.indices.astype(np.int32)


def on_pattern(M, indptr, indices, shape):
    """The entries of M at the pattern's positions as a CSR matrix that keeps explicit zeros."""
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    vals = np.asarray(M.tocsr()[rows, indices]).ravel() if indices.size else np.zeros(0)
    return sp.csr_matrix((vals, indices, indptr), shape=shape)


# ---- numeric phase
def block_diag(D):
    return sp.block_diag(list(D), format="csr") if len(D) else sp.csr_matrix((0, 0))


def rho_ref(A, Dinv):
    """|Dinv A|_inf and, per row, the same sum over absolute values of the factors (the S of its forward bound)."""
    B = block_diag(Dinv) @ A
    rows = np.asarray(abs(B).sum(axis=1)).ravel()
    S = np.asarray((abs(block_diag(Dinv)) @ abs(A)).sum(axis=1)).ravel()
    return rows.max(), S.max()


def tentative_ref(agg, mask, bs, na):
    n = agg.size
    dofs = np.arange(n * bs)
    node, comp = dofs // bs, dofs % bs
    keep = (agg[node] >= 0) & ~mask
    return sp.csr_matrix((np.ones(keep.sum()), (dofs[keep], agg[node[keep]] * bs + comp[keep])), shape=(n * bs, na * bs))


def prolongator_ref(A, Dinv, omega, T):
    return (T - omega * (block_diag(Dinv) @ (A @ T))).tocsr()


def coarse_ref(A, P):
    Ac = (P.T @ A @ P).tolil()
    d = Ac.diagonal()
    for k in np.flatnonzero(d == 0.0):
        Ac[k, k] = 1.0
    return Ac.tocsr()


def coarse_mask_ref(Ac):
    off = Ac.tocsr().copy()
    off.setdiag(0.0)
    return np.asarray(abs(off).sum(axis=1)).ravel() == 0.0


class Level:
    pass


def amg_ref(S, bs, constrained=(), max_levels=10, coarse_rows=512, sweeps=1):
    """The hierarchy of `S` (a scipy CSR on a csr.h pattern, explicit zeros kept): a list of Level with A, indptr, indices and, but
    for the last, agg, n_agg, mask, Dinv, rho, omega, T, P (CSR on the block pattern Pp), APp; `.dense_inverse` on the last."""
    levels = []
    A = S.tocsr()
    indptr, indices = A.indptr.astype(np.int64), A.indices.astype(np.int32)
    mask, active = active_nodes(A.shape[0], bs, constrained)
    while True:
        L = Level()
        L.A, L.indptr, L.indices, L.bs, L.mask, L.sweeps = A, indptr, indices, bs, mask, sweeps
        L.n_rows = A.shape[0]
        levels.append(L)
        last = L.n_rows <= coarse_rows or len(levels) >= max_levels
        if not last:
            ptr, nb = node_graph(indptr, indices, bs)
            agg, na = aggregate_ref(ptr, nb, active)
            last = na == 0 or na * bs > 0.8 * L.n_rows
        if last:
            break
        L.agg, L.n_agg = agg, na
        L.Pp, L.APp, L.Cp = block_patterns(ptr, nb, agg, na)
        L.Dinv = block_jacobi_ref(A, bs)
        L.rho, _ = rho_ref(A, L.Dinv)
        L.omega = (4.0 / 3.0) / L.rho
        L.T = tentative_ref(agg, mask, bs, na)
        pptr, pidx = expand_pattern(L.Pp, bs)
        L.P = on_pattern(prolongator_ref(A, L.Dinv, L.omega, L.T), pptr, pidx, (L.n_rows, na * bs))
        indptr, indices = expand_pattern(L.Cp, bs)
        A = on_pattern(coarse_ref(A, L.P), indptr, indices, (na * bs, na * bs))
        mask = coarse_mask_ref(A)
        active = np.ones(na, dtype=bool)
    if levels[-1].n_rows > MAX_DENSE:
        raise ValueError("coarsest level too large for the dense solve")
    levels[-1].dense_inverse = np.linalg.inv(levels[-1].A.toarray())
    return levels


def apply_block(Dinv, v):
    return np.einsum("nij,nj->ni", Dinv, v.reshape(Dinv.shape[0], -1)).reshape(-1)


def vcycle_ref(levels, r, l=0):
    L = levels[l]
    if l == len(levels) - 1:
        return L.dense_inverse @ r
    x = L.omega * apply_block(L.Dinv, r)
    for _ in range(1, L.sweeps):
        x = x + L.omega * apply_block(L.Dinv, r - L.A @ x)
    x = x + L.P @ vcycle_ref(levels, L.P.T @ (r - L.A @ x), l + 1)
    for _ in range(L.sweeps):
        x = x + L.omega * apply_block(L.Dinv, r - L.A @ x)
    return x


def operator_complexity(levels):
    return sum(L.indices.size for L in levels) / levels[0].indices.size


@contextlib.contextmanager
def callable_preconditioners():
    """Inside, gmres_ref / cg_ref of test_krylov_oracle_cpu take a callable r -> z as `inv` (e.g. the oracle cycle)."""
    plain = kro.apply_pc
    kro.apply_pc = lambda inv, r: inv(r) if callable(inv) else plain(inv, r)
    try:
        yield
    finally:
        kro.apply_pc = plain


def gmres_with_cycle(S, b, levels, **kw):
    with callable_preconditioners():
        return gmres_ref(S, b, inv=lambda r: vcycle_ref(levels, r), **kw)


def cg_with_cycle(S, b, levels, **kw):
    with callable_preconditioners():
        return cg_ref(S, b, inv=lambda r: vcycle_ref(levels, r), **kw)


def forward_bound(K, S):
    """|computed - exact| of a sum of K terms in any order, S the same sum over absolute values (with a factor 4 for the products
    and the fused multiply-adds inside the terms)."""
    return 4.0 * K * U * S


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
    S = to_pattern_csr(m, kro.apply_bcs(A, rollers, 1.0), 2)
    levels = amg_ref(S, 2, rollers, coarse_rows=10)
    for L in levels[:-1]:
        assert not np.asarray(abs(L.P[np.flatnonzero(L.mask)]).sum(axis=1)).any()      # masked rows of P are zero
    d = levels[1].A.diagonal()
    assert (d != 0.0).all()
    x = vcycle_ref(levels, np.ones(S.shape[0]))
    assert np.isfinite(x).all()


def test_cycle_is_linear_and_symmetric_for_an_spd_matrix():
    rng = np.random.Generator(np.random.PCG64(11))
    m, A = eps_matrix(nonsym_seed=None)                   # the matrix of test_cg_oracle_on_an_spd_elastic_matrix
    S = to_pattern_csr(m, A, 2)
    for sweeps in (1, 2):
        levels = amg_ref(S, 2, bottom_dofs(m, 2), coarse_rows=30, sweeps=sweeps)
        assert len(levels) >= 2
        r1, r2 = rng.normal(size=(2, S.shape[0]))
        z1, z2 = vcycle_ref(levels, r1), vcycle_ref(levels, r2)
        z = vcycle_ref(levels, 2.5 * r1 + r2)
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
    assert np.allclose(S @ vcycle_ref(one, r), r, atol=1e-9 * np.abs(r).max())          # a single level is the direct solve
