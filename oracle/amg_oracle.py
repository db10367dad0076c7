"""The NumPy / SciPy yardstick of dxo_amg_* (csrc/amg.hip): one hierarchy, one relaxation and one cycle that take the keywords of
dolfinx_external_operator_amd.krylov.AMG. Pinned by the tests/test_amg_*_oracle_cpu.py files and tests/test_fgmres_kcycle_oracle_cpu.py.

amg_ref restates the device algorithm: the node graph of the block pattern without the fully constrained nodes, aggregation in three
passes in ascending node order, the tentative prolongator T, P = T - omega Dinv A T with omega = (4/3) / rho, A_c = P^T A P on the
symbolic pattern (an exactly zero diagonal entry becomes 1), recursion until a level is small, stagnates or max_levels is reached, a
dense inverse on the coarsest level. The patterns come from integer sparse products, not from the loops the library runs, and the
numbers from scipy.sparse products. Its options:
  near_nullspace  B [n_rows][k]: per level and aggregate the rows of B of its nodes in ascending node order, orthonormalised by
                  Gram-Schmidt in column order with a second pass (a column with |v| <= rank_tol |v0| after the projections is dead:
                  Q column zero, R diagonal zero); T carries the Q blocks (bs_l x k), the next B the R factors; every coarse level
                  has block size k (dxo_amg_create_nns).
  strength        theta: block (i, j), i != j, is strong when |A_ij|_F^2 >= theta^2 |A_ii|_F |A_jj|_F or the same holds for (j, i);
                  diagonal blocks are strong. The aggregates are made on the strong graph, P on the pattern (strong graph) x
                  (aggregates), A P and P^T A P on the full graph, P = T - omega_F Dinv_F A^F T with A^F the matrix without its weak
                  blocks, each added onto the diagonal block of its row, Dinv_F the inverses of the lumped blocks (A_ii's where the
                  lumped block fails Hadamard's test, zero for a node without a strong neighbour) and omega_F = (4/3) / rho_F. The
                  sweeps keep A, Dinv and rho (dxo_amg_create_soc).
  first_transfer  (W, coarse_to_fine) of vertex_transfer_ref: level 0 keeps Dinv, rho and omega; its P is kron(W, I_bs) with the
                  rows of constrained fine dofs and the columns of the coarse dofs constrained at their own node zero; the
                  aggregation, the near-null space and the strength start on level 1 with the constraints of the coarse nodes
                  (dxo_amg_create_transfer).
  smoother, degree, rho, rho_iters, lower, safety
                  the relaxation (dxo_amg_set_smoother): rho "inf-norm" is |Dinv A|_inf, "power" is safety |w_m| after m steps
                  w_k = Dinv A (w_{k-1} / |w_{k-1}|) from the fixed start vector w_0[i] = 0.5 + ((uint32)(i * 2654435761) >> 8) * 2^-24,
                  which is exact in float64; "chebyshev" is the polynomial of `degree` in Dinv A on [lower rho, rho], by the
                  recurrence of the device.
cycle_ref walks a hierarchy given as SciPy matrices (the Level list of amg_ref, or one read back from the device). "V": `sweeps`
damped block-Jacobi sweeps or the Chebyshev polynomial, restriction by P^T, recursion, prolongation, the relaxation again. "K": every
level between the finest and the coarsest solves A_l x = r by the two GCR steps of gcr2_ref preconditioned by the body of that
level, with the two guards of the device (dxo_amg_set_cycle). "fp32": A, Dinv, P and every vector of every level but the coarsest in
numpy.float32; omega and the Chebyshev pairs are made in double and narrowed once; the coarsest level widens its right-hand side,
multiplies by the float64 dense inverse and narrows the result. The hierarchy itself is the float64 one: only the cycle is narrowed,
as on the device (dxo_amg_set_precision)."""
import numpy as np
import scipy.sparse as sp

from oracle.krylov_oracle import block_jacobi_ref, cg_ref, fgmres_ref, gmres_ref
from tools.synthetic import coordinate_element_at_nodes

U = 2.0 ** -53
MAX_DENSE = 4096
RANK_TOL = 1e-10
RHO_ITERS, LOWER, SAFETY = 10, 0.1, 1.1        # the customary rule (PETSc's), the defaults of the library
K_DEPENDENT = 1e-14      # rho2 <= K_DEPENDENT beta: the second direction depends on the first (the rule of a singular diagonal block)


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


def ones_pattern(M):
    M = M.tocsr().copy()
    M.data = np.ones_like(M.data)
    return M


def block_patterns(ptr, nb, agg, na):
    """Block patterns (scipy CSR of ones, sorted) of P, A P and P^T A P from integer products of the graph and the aggregates."""
    n = ptr.size - 1
    G = sp.csr_matrix((np.ones(nb.size, dtype=np.int64), nb, ptr), shape=(n, n))
    on = np.flatnonzero(agg >= 0)
    Tg = sp.csr_matrix((np.ones(on.size, dtype=np.int64), (on, agg[on])), shape=(n, na))
    out = []
    Pp = G @ Tg
    APp = G @ ones_pattern(Pp)
    Cp = ones_pattern(Pp).T @ ones_pattern(APp) + sp.identity(na, dtype=np.int64, format="csr")
    for M in (Pp, APp, Cp):
        M = ones_pattern(M.tocsr())
        M.sort_indices()
        out.append(M)
    return out


def soc_patterns(ptr, nb, mask, agg, na):
    """Block patterns of P (strong graph x aggregates), A P and P^T A P (full graph) from integer products."""
    n = ptr.size - 1
    G = sp.csr_matrix((np.ones(nb.size, dtype=np.int64), nb, ptr), shape=(n, n))
    Gs = sp.csr_matrix((mask.astype(np.int64), nb, ptr), shape=(n, n))
    Gs.eliminate_zeros()
    on = np.flatnonzero(agg >= 0)
    Tg = sp.csr_matrix((np.ones(on.size, dtype=np.int64), (on, agg[on])), shape=(n, na))
    Pp = ones_pattern(Gs @ Tg)
    APp = ones_pattern(G @ Pp)
    Cp = ones_pattern(Pp.T @ APp + sp.identity(na, dtype=np.int64, format="csr"))
    out = []
    for M in (Pp, APp, Cp):
        M = M.tocsr()
        M.sort_indices()
        out.append(M)
    return out


def transfer_patterns(ptr, nb, W):
    """Block patterns of P (that of W), A P and P^T A P + I from integer products."""
    n = ptr.size - 1
    G = sp.csr_matrix((np.ones(nb.size, dtype=np.int64), nb, ptr), shape=(n, n))
    Pp = ones_pattern(W).astype(np.int64)
    APp = ones_pattern(G @ Pp)
    Cp = ones_pattern(Pp.T @ APp + sp.identity(W.shape[1], dtype=np.int64, format="csr"))
    for M in (Pp, APp, Cp):
        M.sort_indices()
    return Pp, APp, Cp


def strong_graph_ref(ptr, nb, mask):
    n = ptr.size - 1
    row = np.repeat(np.arange(n), np.diff(ptr))
    return np.concatenate([[0], np.cumsum(np.bincount(row[mask], minlength=n))]), nb[mask]


def expand_rect(Bp, bsr, bsc):
    """csr.h layout of a block pattern with bsr x bsc blocks: (indptr int64, indices int32)."""
    M = sp.kron(Bp, np.ones((bsr, bsc), dtype=np.int64), format="csr")
    M.sort_indices()
    return M.indptr.astype(np.int64), M.indices.astype(np.int32)


def expand_pattern(Bp, bs):
    return expand_rect(Bp, bs, bs)


def on_pattern(M, indptr, indices, shape):
    """The entries of M at the pattern's positions as a CSR matrix that keeps explicit zeros."""
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    vals = np.asarray(M.tocsr()[rows, indices]).ravel() if indices.size else np.zeros(0)
    return sp.csr_matrix((vals, indices, indptr), shape=shape)


def same_csr(A, B):
    return A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data)


# ---- the spectral radius and the relaxation
def block_diag(D):
    return sp.block_diag(list(D), format="csr") if len(D) else sp.csr_matrix((0, 0))


def apply_block(Dinv, v):
    return np.einsum("nij,nj->ni", Dinv, v.reshape(Dinv.shape[0], -1)).reshape(-1)


def rho_ref(A, Dinv):
    """|Dinv A|_inf and, per row, the same sum over absolute values of the factors (the S of its forward bound)."""
    B = block_diag(Dinv) @ A
    rows = np.asarray(abs(B).sum(axis=1)).ravel()
    S = np.asarray((abs(block_diag(Dinv)) @ abs(A)).sum(axis=1)).ravel()
    return rows.max(), S.max()


def start_vector(n):
    i = np.arange(n, dtype=np.uint64)
    return 0.5 + (((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def power_rho_ref(A, Dinv, iters=RHO_ITERS, safety=SAFETY):
    """safety |w_iters|; 0 for a zero matrix."""
    w = start_vector(A.shape[0])
    lam = np.sqrt(w @ w)
    for _ in range(iters):
        s = 1.0 / lam if lam > 0.0 else 0.0
        w = apply_block(Dinv, A @ (s * w))
        lam = np.sqrt(w @ w)
    return safety * lam


def cheby_pairs(rho, lower, degree):
    """(c1, c2) of the steps d = c1 d + c2 Dinv (r - A x), x += d."""
    if not rho > 0.0:
        return [(0.0, 0.0)] * degree
    a = lower * rho
    theta, delta = 0.5 * (a + rho), 0.5 * (rho - a)
    sigma = theta / delta
    r0 = 1.0 / sigma
    out = [(0.0, 1.0 / theta)]
    for _ in range(1, degree):
        r1 = 1.0 / (2.0 * sigma - r0)
        out.append((r1 * r0, 2.0 * r1 / delta))
        r0 = r1
    return out


def cheby_ref(A, Dinv, rho, lower, degree, r, x=None, dtype=np.float64):
    """x after the Chebyshev polynomial of `degree` in Dinv A on [lower rho, rho], started from x (None: zero). dtype: what the pairs,
    made in double, are narrowed to (A, Dinv and r are the caller's)."""
    x = np.zeros_like(r) if x is None else x.copy()
    d = np.zeros_like(r)
    for c1, c2 in cheby_pairs(rho, lower, degree):
        d = dtype(c1) * d + dtype(c2) * apply_block(Dinv, r - A @ x)
        x = x + d
    return x


# ---- numeric phase
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


# ---- the near-null space
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


# ---- the strength of connection
def block_values(A, indptr, indices, bs):
    """(blocks [nnzb][bs][bs], node of every block, its column node) of a matrix on a csr.h pattern, in the order of the pattern."""
    ptr, nb = node_graph(indptr, indices, bs)
    n = ptr.size - 1
    row = np.repeat(np.arange(n), np.diff(ptr))
    k = np.arange(nb.size) - ptr[row]
    base = np.asarray(indptr, dtype=np.int64)[row * bs]
    ln = np.asarray(indptr, dtype=np.int64)[row * bs + 1] - base
    r, c = np.arange(bs)[None, :, None], np.arange(bs)[None, None, :]
    idx = base[:, None, None] + r * ln[:, None, None] + k[:, None, None] * bs + c
    return A.data[idx], row, nb


def pow2_down(m):
    """2^-e, e the exponent of m (frexp) held in +-1000; 1 for a zero, NaN or infinite m: amg_pow2_down of the device."""
    m = np.asarray(m, dtype=np.float64)
    ok = (m > 0.0) & np.isfinite(m)
    e = np.where(ok, np.frexp(np.where(ok, m, 1.0))[1], 0)
    return np.ldexp(1.0, -np.clip(e, -1000, 1000))


def _norm2(blocks, s):
    """The sum of the squares of s[b] blocks[b], entry by entry in row-major order."""
    n2 = np.zeros(blocks.shape[0])
    for v in blocks.reshape(blocks.shape[0], -1).T:
        v = v * s
        n2 = n2 + v * v
    return n2


def _decide(A, indptr, indices, bs, theta, n2, bound):
    """(mask, closest) from the squared norms and the thresholds of every block, both in the scaling of the block."""
    blocks, row, colnode = block_values(A, indptr, indices, bs)
    ptr, nb = node_graph(indptr, indices, bs)
    n = ptr.size - 1
    N2 = sp.csr_matrix((n2, nb, ptr), shape=(n, n))
    has = sp.csr_matrix((np.ones(nb.size), nb, ptr), shape=(n, n))
    n2t = np.asarray(N2.T.tocsr()[row, colnode]).ravel() if nb.size else np.zeros(0)
    present = np.asarray(has.T.tocsr()[row, colnode]).ravel() > 0 if nb.size else np.zeros(0, dtype=bool)
    mask = (n2 >= bound) | (present & (n2t >= bound)) | (row == colnode)
    off = (row != colnode) & (bound > 0.0)
    closest = np.inf
    if off.any():
        closest = min(np.abs(n2[off] / bound[off] - 1.0).min(), np.abs(n2t[off & present] / bound[off & present] - 1.0).min(initial=np.inf))
    return mask, closest


def strength_ref(A, indptr, indices, bs, theta):
    """(mask per block, closest): the strong blocks, and the smallest |value / threshold - 1| over the tests that decided them.
    The device's range-safe arithmetic: |A_ii|_F from the block times 2^-e of its largest entry, divided by it again; block (i, j)
    compared as |s A_ij|_F^2 >= theta^2 (s |A_ii|_F) (s |A_jj|_F) with s = 2^-e of the larger norm, the same s for (j, i)."""
    blocks, row, colnode = block_values(A, indptr, indices, bs)
    n = (np.asarray(indptr).size - 1) // bs
    on = row == colnode
    sd = pow2_down(np.abs(blocks[on]).reshape(-1, bs * bs).max(axis=1))
    dn = np.zeros(n)
    dn[row[on]] = np.sqrt(_norm2(blocks[on], sd)) / sd
    s = pow2_down(np.maximum(dn[row], dn[colnode]))
    bound = theta * theta * ((dn[row] * s) * (dn[colnode] * s))
    return _decide(A, indptr, indices, bs, theta, _norm2(blocks, s), bound)


def strength_unscaled_ref(A, indptr, indices, bs, theta):
    """strength_ref in the arithmetic of earlier versions, which squares the entries as they are: |A_ij|_F^2 >= theta^2 |A_ii|_F
    |A_jj|_F. Kept as what the range-safe form is compared against inside the range where these squares are normal numbers."""
    blocks, row, colnode = block_values(A, indptr, indices, bs)
    n = (np.asarray(indptr).size - 1) // bs
    n2 = _norm2(blocks, 1.0)
    dn = np.zeros(n)
    dn[row[row == colnode]] = np.sqrt(n2[row == colnode])
    return _decide(A, indptr, indices, bs, theta, n2, theta * theta * (dn[row] * dn[colnode]))


def filtered_ref(A, indptr, indices, bs, mask):
    """(A^F as CSR, the lumped diagonal blocks [n][bs][bs], A's own [n][bs][bs], strong off-diagonal blocks per node)."""
    blocks, row, colnode = block_values(A, indptr, indices, bs)
    n = (np.asarray(indptr).size - 1) // bs
    diag = np.zeros((n, bs, bs))
    diag[row[row == colnode]] = blocks[row == colnode]
    lumped = diag.copy()
    weak = ~mask
    np.add.at(lumped, row[weak], blocks[weak])                    # in the order of the pattern: ascending column
    n_strong = np.bincount(row[mask & (row != colnode)], minlength=n)
    keep = mask & (row != colnode)
    AF = sp.bsr_matrix((blocks[keep], colnode[keep], np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=n))])),
                       shape=A.shape).tocsr() + block_diag(lumped)
    return AF.tocsr(), lumped, diag, n_strong


def lumped_inverse_ref(lumped, diag, n_strong):
    """(Dinv_F [n][bs][bs], nodes that fell back to A_ii): Hadamard's test of dxo_csr_block_jacobi on the lumped blocks."""
    n = lumped.shape[0]
    out = np.zeros_like(lumped)
    fell = np.zeros(n, dtype=bool)
    for i in np.flatnonzero(n_strong > 0):
        had = np.prod(np.sqrt((lumped[i] ** 2).sum(axis=1)))
        ok = abs(np.linalg.det(lumped[i])) > 1e-14 * had
        out[i] = np.linalg.inv(lumped[i] if ok else diag[i])
        fell[i] = not ok
    return out, fell


# ---- the p level
def vertex_transfer_ref(m):
    """(W scipy CSR [field nodes][geometry nodes] with sorted rows, coarse_to_fine) of a SyntheticMesh, entry by entry: the nodal
    interpolation from the degree-1 space on the same cells, cell by cell from the two dofmaps and the coordinate element tabulated at
    the field element's nodes."""
    psi = coordinate_element_at_nodes(m.cell, m.degree)
    n, nc = m.node_x.shape[0], m.x.shape[0]
    rows = [dict() for _ in range(n)]
    for cell in range(m.num_cells):
        for a, i in enumerate(m.dofmap[cell]):
            for v, g in enumerate(m.geom_dofmap[cell]):
                if abs(psi[a, v]) > 1e-14:
                    assert rows[i].setdefault(int(g), psi[a, v]) == psi[a, v]        # the cells that share a node agree
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    col = np.array([g for r in rows for g in sorted(r)], dtype=np.int32)
    w = np.array([r[g] for r in rows for g in sorted(r)])
    W = sp.csr_matrix((w, col, ptr), shape=(n, nc))
    ctf = -np.ones(nc, dtype=np.int64)
    for i, r in enumerate(rows):
        if len(r) == 1 and next(iter(r.values())) == 1.0:
            ctf[next(iter(r))] = i
    assert (ctf >= 0).all()
    return W, ctf.astype(np.int32)


def p_diag_ref(W, ctf, mask, bs):
    """[blocks of W][bs]: w_iv keep(i, c) keep(coarse_to_fine[v], c)."""
    keep = ~np.asarray(mask, dtype=bool).reshape(-1, bs)
    rows = np.repeat(np.arange(W.shape[0]), np.diff(W.indptr))
    return W.data[:, None] * keep[rows] * keep[ctf[W.indices]]


# ---- the hierarchy
class Level:
    """One level: A, indptr, indices, bs, mask, sweeps, smoother, degree, lower, n_rows (B with a near-null space) and, but for the
    last, agg, n_agg, bs_coarse, Pp, APp, Cp, Dinv, rho, omega, P (CSR on the pattern Pp expanded to bs x bs_coarse blocks); T (and
    dead, the dead columns of T, with a near-null space) below an aggregation, p_diag below a transfer; with a strength strong (mask
    per block), closest, AF, lumped, Dinv_f, fell (nodes that fell back to A_ii), n_strong_off, rho_f and omega_f. `.dense_inverse`
    on the last."""


def amg_ref(S, bs, constrained=(), *, near_nullspace=None, strength=0.0, first_transfer=None, smoother="jacobi", degree=None,
            rho="inf-norm", rho_iters=RHO_ITERS, lower=LOWER, safety=SAFETY, max_levels=10, coarse_rows=512, sweeps=1,
            rank_tol=RANK_TOL, filtered=None, frozen=None):
    """The hierarchy of `S` (a scipy CSR on a csr.h pattern, explicit zeros kept) under the keywords of AMG(...): a list of Level.
    Oracle-only: rank_tol; filtered (None: the device's rule, the filtered matrix smooths P when strength > 0; True at strength 0: the
    same formulas with every block strong; False: the aggregates of the strong graph with P smoothed by the full matrix); frozen (the
    levels of an earlier call whose masks and aggregates are reused, as dxo_amg_setup reuses those of the creation).
    A matrix that is its own coarsest level is one level, with or without first_transfer."""
    soc = strength > 0.0 or filtered is not None
    if soc and frozen is None and rho != "inf-norm":
        # the device coarsens with the default relaxation at construction; the selected one is applied on those masks and aggregates
        frozen = amg_ref(S, bs, constrained, near_nullspace=near_nullspace, strength=strength, first_transfer=first_transfer,
                         max_levels=max_levels, coarse_rows=coarse_rows, sweeps=sweeps, rank_tol=rank_tol, filtered=filtered)
    if rho == "power":
        def estimate(A, Dinv):
            return power_rho_ref(A, Dinv, rho_iters, safety)
    else:
        def estimate(A, Dinv):
            return rho_ref(A, Dinv)[0]
    levels = []
    A = S.tocsr()
    indptr, indices = A.indptr.astype(np.int64), A.indices.astype(np.int32)
    mask, active = active_nodes(A.shape[0], bs, constrained)
    k = 0 if near_nullspace is None else near_nullspace.shape[1]
    if k:
        B = np.array(near_nullspace, dtype=np.float64)
        B[mask] = 0.0
    while True:
        L = Level()
        L.A, L.indptr, L.indices, L.bs, L.mask, L.sweeps = A, indptr, indices, bs, mask, sweeps
        L.smoother, L.degree, L.lower = smoother, (sweeps if degree is None else degree), lower
        L.n_rows = A.shape[0]
        if k:
            L.B = B
        levels.append(L)
        p_level = first_transfer is not None and len(levels) == 1
        bsc = k if k and not p_level else bs
        last = L.n_rows <= coarse_rows or len(levels) >= max_levels
        if frozen is not None:
            last = len(levels) == len(frozen)
        strong = closest = None
        if not last:
            ptr, nb = node_graph(indptr, indices, bs)
            if p_level:
                W, ctf = first_transfer
                agg, na = None, W.shape[1]
            elif frozen is not None:
                F = frozen[len(levels) - 1]
                strong, closest, agg, na = F.strong, F.closest, F.agg, F.n_agg
            else:
                if soc:
                    strong, closest = strength_ref(A, indptr, indices, bs, strength)
                    agg, na = aggregate_ref(*strong_graph_ref(ptr, nb, strong), active)
                else:
                    agg, na = aggregate_ref(ptr, nb, active)
                last = na == 0 or na * bsc > 0.8 * L.n_rows
        if last:
            break
        L.strong, L.closest, L.agg, L.n_agg, L.bs_coarse = strong, closest, agg, na, bsc
        L.Dinv = block_jacobi_ref(A, bs)
        L.rho = estimate(A, L.Dinv)
        L.omega = (4.0 / 3.0) / L.rho
        if p_level:
            L.Pp, L.APp, L.Cp = transfer_patterns(ptr, nb, W)
            L.p_diag = p_diag_ref(W, ctf, mask, bs)
            L.P = sp.bsr_matrix((L.p_diag[:, :, None] * np.eye(bs)[None], W.indices, W.indptr), shape=(L.n_rows, na * bs)).tocsr()
        else:
            if soc:
                L.Pp, L.APp, L.Cp = soc_patterns(ptr, nb, strong if filtered is not False else np.ones_like(strong), agg, na)
                L.AF, L.lumped, diag, L.n_strong_off = filtered_ref(A, indptr, indices, bs, strong)
                L.Dinv_f, L.fell = lumped_inverse_ref(L.lumped, diag, L.n_strong_off)
                L.rho_f = estimate(L.AF, L.Dinv_f)
                L.omega_f = (4.0 / 3.0) / L.rho_f if L.rho_f > 0.0 else 0.0
            else:
                L.Pp, L.APp, L.Cp = block_patterns(ptr, nb, agg, na)
            if k:
                L.T, B, L.dead = tentative_nns_ref(agg, na, B, bs, rank_tol)
            else:
                L.T = tentative_ref(agg, mask, bs, na)
            if soc and filtered is not False:
                exact = prolongator_ref(L.AF, L.Dinv_f, L.omega_f, L.T)
            else:
                exact = prolongator_ref(A, L.Dinv, L.omega, L.T)
            pptr, pidx = expand_rect(L.Pp, bs, bsc)
            L.P = on_pattern(exact, pptr, pidx, (L.n_rows, na * bsc))
        indptr, indices = expand_rect(L.Cp, bsc, bsc)
        A = on_pattern(coarse_ref(A, L.P), indptr, indices, (na * bsc, na * bsc))
        if p_level:                      # level 1 starts like a finest level, with the constraints of the coarse nodes
            mask = mask.reshape(-1, bs)[ctf].reshape(-1)
            active = ~mask.reshape(-1, bs).all(axis=1)
            if k:
                B = B.reshape(-1, bs, k)[ctf].reshape(-1, k)
        else:
            mask = coarse_mask_ref(A)
            active = np.ones(na, dtype=bool)
        bs = bsc
    if levels[-1].n_rows > MAX_DENSE:
        raise ValueError("coarsest level too large for the dense solve")
    levels[-1].dense_inverse = np.linalg.inv(levels[-1].A.toarray())
    return levels


def operator_complexity(levels):
    return sum(L.indices.size for L in levels) / levels[0].indices.size


def forward_bound(K, S):
    """|computed - exact| of a sum of K terms in any order, S the same sum over absolute values (with a factor 4 for the products
    and the fused multiply-adds inside the terms)."""
    return 4.0 * K * U * S


# ---- the cycle
_F32 = {}      # id(level) -> (level, A, Dinv, P, P^T) in float32: the levels themselves stay untouched


def _operators(L, dtype):
    """(A, Dinv, P, P^T) of a level in the cycle's precision."""
    if dtype is np.float64:
        return L.A, L.Dinv, L.P, L.P.T
    hit = _F32.get(id(L))
    if hit is None or hit[0] is not L:
        P = sp.csr_matrix(L.P).astype(np.float32)
        hit = _F32[id(L)] = (L, sp.csr_matrix(L.A).astype(np.float32), np.asarray(L.Dinv).astype(np.float32), P, sp.csr_matrix(P.T))
    return hit[1:]


def smooth_ref(L, r, x=None, dtype=np.float64):
    """The relaxation of a level from x (None: zero): the Chebyshev polynomial or `sweeps` damped block-Jacobi sweeps. dtype
    numpy.float32: on the narrowed A and Dinv, the coefficients made in double and narrowed once."""
    A, Dinv, _, _ = _operators(L, dtype)
    if L.smoother == "chebyshev":
        return cheby_ref(A, Dinv, L.rho, L.lower, L.degree, r, x, dtype)
    x = np.zeros_like(r) if x is None else x
    om = dtype(L.omega)
    for _ in range(L.sweeps):
        x = x + om * apply_block(Dinv, r - A @ x)
    return x


def gcr2_ref(A, B, r, trace=None):
    """Two GCR steps on A x = r preconditioned by the callable B, with the guards of the device: rho1 == 0 gives x = 0; rho2 not
    finite or <= 1e-14 beta gives x = (a1 / rho1) c1. trace (a list) receives (r, x after one step, x, the guard that was hit)."""
    c1 = B(r)
    v1 = A @ c1
    rho1, a1 = v1 @ v1, v1 @ r
    if rho1 == 0.0:
        x = np.zeros_like(r)
        if trace is not None:
            trace.append((r, x, x, "rho1"))
        return x
    alpha1 = a1 / rho1
    r1 = r - alpha1 * v1
    c2 = B(r1)
    v2 = A @ c2
    g, beta, a2 = v2 @ v1, v2 @ v2, v2 @ r1
    gr = g / rho1                                          # ratios only: no product of two dot products (a fourth power of |r|)
    rho2 = beta - g * gr
    x1 = alpha1 * c1
    if not np.isfinite(rho2) or rho2 <= K_DEPENDENT * beta:
        x, hit = x1, "rho2"
    else:
        x2 = a2 / rho2
        x, hit = (alpha1 - gr * x2) * c1 + x2 * c2, None
    if trace is not None:
        trace.append((r, x1, x, hit))
    return x


def cycle_ref(levels, r, cycle="V", precision="fp64", trace=None, visits=None):
    """z = M(r), one cycle from zero. cycle "K": trace, a dict level -> list of gcr2_ref records. visits: a list per level, counted
    up at every visit. precision "fp32": r is narrowed on entry and the result is float32; not with "K", as on the device."""
    if cycle == "K" and precision != "fp64":
        raise ValueError("the K-cycle runs in fp64 only")
    dtype = np.float64 if precision == "fp64" else np.float32
    last = len(levels) - 1

    def solve(rc, l):
        if l == last:
            if visits is not None:
                visits[l] += 1
            return (levels[l].dense_inverse @ rc.astype(np.float64)).astype(dtype)
        if cycle == "K" and l > 0:
            return gcr2_ref(levels[l].A, lambda q: body(q, l), rc, None if trace is None else trace.setdefault(l, []))
        return body(rc, l)

    def body(q, l):
        L = levels[l]
        if visits is not None:
            visits[l] += 1
        A, _, P, PT = _operators(L, dtype)
        x = smooth_ref(L, q, None, dtype)
        x = x + P @ solve(PT @ (q - A @ x), l + 1)
        x = smooth_ref(L, q, x, dtype)
        assert x.dtype == dtype, x.dtype
        return x

    return solve(np.asarray(r).astype(dtype), 0)


def k_visits(n_levels):
    """Level visits of one K-cycle: 2^l on level l but the coarsest, which is visited as often as the level above it."""
    if n_levels == 1:
        return 1
    return sum(2 ** l for l in range(n_levels - 1)) + 2 ** (n_levels - 2)


def gmres_with_cycle(S, b, levels, cycle="V", precision="fp64", **kw):
    return gmres_ref(S, b, inv=lambda r: cycle_ref(levels, r, cycle, precision), **kw)


def cg_with_cycle(S, b, levels, cycle="V", precision="fp64", **kw):
    return cg_ref(S, b, inv=lambda r: cycle_ref(levels, r, cycle, precision), **kw)


def fgmres_with_cycle(S, b, levels, cycle="V", precision="fp64", **kw):
    return fgmres_ref(S, b, M=lambda r, j: cycle_ref(levels, r, cycle, precision), **kw)
