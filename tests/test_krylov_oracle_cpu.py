"""The NumPy yardstick of dxo_krylov_gmres / dxo_krylov_cg / dxo_csr_block_jacobi, pinned on the CPU.

gmres_ref restates the device algorithm step for step: restarted GMRES(m) with right preconditioning, classical Gram-Schmidt with
one reorthogonalisation pass, Givens rotations, the first step whose estimate |g_{j+1}| met max(rtol |b|, atol) as the cycle's
length, the true residual b - A x at every restart. block_jacobi_ref inverts the bs x bs diagonal blocks. Both are checked against
scipy.sparse.linalg.spsolve / numpy.linalg.inv on the assembled matrices the device makes: the heat Jacobian of the heat demo
(non-symmetric, bs = 1), an (eps, eps) matrix with a random non-symmetric C (bs = 2) and an SPD elastic matrix (CG), each with
Dirichlet rows."""
import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.linalg

from test_assemble_oracle_cpu import apply_bcs, dense_ref, heat_setting, pattern_ref
from tools.synthetic import structured_mesh


# ---- the oracles
def diagonal_blocks(A, bs):
    """(n/bs, bs, bs) diagonal blocks of a scipy matrix."""
    n = A.shape[0]
    D = np.zeros((n // bs, bs, bs))
    A = A.tocsr()
    for i in range(bs):
        for j in range(bs):
            D[:, i, j] = np.asarray(A[np.arange(i, n, bs), np.arange(j, n, bs)]).ravel()
    return D


def block_jacobi_ref(A, bs):
    """Inverses of the diagonal blocks (n/bs, bs, bs); a singular block raises."""
    D = diagonal_blocks(A, bs)
    return np.linalg.inv(D)


def apply_pc(inv, r):
    """z = inv r per block; inv None: identity."""
    if inv is None:
        return r.copy()
    nb, bs, _ = inv.shape
    return np.einsum("nij,nj->ni", inv, r.reshape(nb, bs)).reshape(-1)


def gmres_ref(A, b, x0=None, inv=None, m=30, rtol=1e-10, atol=0.0, maxiter=1000, reorth=True):
    """(x, iterations, converged, true relative residual) of the device's restarted GMRES(m)."""
    n = b.size
    x = np.zeros(n) if x0 is None else x0.astype(float).copy()
    bnorm = np.linalg.norm(b)
    if bnorm == 0.0:
        return np.zeros(n), 0, True, 0.0
    tol = max(rtol * bnorm, atol)
    total, breakdown = 0, False
    while True:
        r = b - A @ x
        beta = np.linalg.norm(r)
        if beta <= tol:
            return x, total, True, beta / bnorm
        if total >= maxiter or breakdown:
            return x, total, False, beta / bnorm
        V = np.zeros((m + 1, n))
        H = np.zeros((m + 1, m))
        cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        V[0] = r / beta
        g[0] = beta
        k = 0
        for j in range(m):
            if total + j >= maxiter:
                break
            w = A @ apply_pc(inv, V[j])
            h = V[: j + 1] @ w
            w = w - V[: j + 1].T @ h
            if reorth:
                c = V[: j + 1] @ w
                w = w - V[: j + 1].T @ c
                h = h + c
            hn = np.linalg.norm(w)
            V[j + 1] = w / hn if hn > 0 else 0.0
            col = np.concatenate([h, [hn]])
            for i in range(j):
                t = cs[i] * col[i] + sn[i] * col[i + 1]
                col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1]
                col[i] = t
            rr = np.hypot(col[j], hn)
            cs[j], sn[j] = (col[j] / rr, hn / rr) if rr > 0 else (1.0, 0.0)
            col[j], col[j + 1] = rr, 0.0
            H[: j + 2, j] = col
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            k = j + 1
            if not hn > 0:
                breakdown = True
            if abs(g[j + 1]) <= tol or not hn > 0:
                break
        if k == 0:
            return x, total, False, beta / bnorm
        y = np.zeros(k)
        for i in range(k - 1, -1, -1):
            s = g[i] - H[i, i + 1: k] @ y[i + 1:]
            y[i] = s / H[i, i] if H[i, i] != 0 else 0.0
        x = x + apply_pc(inv, V[:k].T @ y)
        total += k


def cg_ref(A, b, inv=None, rtol=1e-10, atol=0.0, maxiter=1000):
    """(x, iterations, converged) of preconditioned CG from x = 0."""
    bnorm = np.linalg.norm(b)
    tol = max(rtol * bnorm, atol)
    x = np.zeros_like(b)
    r = b.copy()
    z = apply_pc(inv, r)
    p = z.copy()
    rz = r @ z
    for it in range(1, maxiter + 1):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        if np.linalg.norm(r) <= tol:
            return x, it, True
        z = apply_pc(inv, r)
        rzn = r @ z
        p = z + (rzn / rz) * p
        rz = rzn
    return x, maxiter, False


# ---- the test matrices (the layouts the device assembles)
def boundary_dofs(m, bs):
    x = m.node_x
    lo, hi = x.min(axis=0), x.max(axis=0)
    on = np.any((np.abs(x - lo) < 1e-12) | (np.abs(x - hi) < 1e-12), axis=1)
    return (np.flatnonzero(on)[:, None] * bs + np.arange(bs)).reshape(-1)


def bottom_dofs(m, bs):
    on = np.abs(m.node_x[:, 1] - m.node_x[:, 1].min()) < 1e-12
    return (np.flatnonzero(on)[:, None] * bs + np.arange(bs)).reshape(-1)


def heat_matrix(nx=6):
    """The heat demo's Jacobian (grad, value_grad), bs = 1, with identity rows on the boundary nodes."""
    m, dqdT, dqds, _ = heat_setting(nx)
    C = np.concatenate([dqdT[..., None], dqds], axis=-1).reshape(m.num_cells * m.nq, 2, 3)
    A = -dense_ref(m, "grad", "value_grad", 1, C)         # J = inner(-(dq/dT T^ + dq/dsigma grad T^), grad T~)
    return m, apply_bcs(A, boundary_dofs(m, 1), 1.0)


def elastic_C(m, nonsym_seed=None):
    """Per-point Mandel blocks (n, 4, 4): plane-strain isotropic elasticity, plus a random non-symmetric part with a seed."""
    lam, mu = 1.0, 0.7
    Ce = np.zeros((4, 4))
    Ce[:3, :3] = lam
    Ce[np.arange(4), np.arange(4)] += 2 * mu
    C = np.broadcast_to(Ce, (m.num_cells * m.nq, 4, 4)).copy()
    if nonsym_seed is not None:
        rng = np.random.Generator(np.random.PCG64(nonsym_seed))
        C += 0.3 * rng.normal(size=C.shape)
    return C


def eps_matrix(n=(5, 4), nonsym_seed=3, degree=2):
    m = structured_mesh("triangle", n, degree, distort=0.15, seed=5)
    A = dense_ref(m, "eps", "eps", 2, elastic_C(m, nonsym_seed))
    return m, apply_bcs(A, bottom_dofs(m, 2), 1.0)


def to_pattern_csr(m, A, bs):
    """scipy CSR on the device pattern (explicit zeros kept), as dxo_bilinear_assemble lays it out."""
    indptr, indices = pattern_ref(m, bs)
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    return scipy.sparse.csr_matrix((A[rows, indices], indices, indptr), shape=A.shape)


# ---- tests
@pytest.mark.parametrize("case", ["heat", "eps"])
def test_gmres_oracle_matches_spsolve(case):
    m, A = heat_matrix() if case == "heat" else eps_matrix()
    bs = 1 if case == "heat" else 2
    S = to_pattern_csr(m, A, bs)
    assert abs(S - S.T).max() > 1e-3                       # not symmetric: CG does not apply
    b = np.random.Generator(np.random.PCG64(1)).normal(size=A.shape[0])
    ref = scipy.sparse.linalg.spsolve(S.tocsc(), b)
    for inv in (None, block_jacobi_ref(S, bs)):
        x, its, conv, res = gmres_ref(S, b, inv=inv, m=30, rtol=1e-12)
        assert conv and res <= 1e-12 and 0 < its
        assert np.linalg.norm(x - ref) <= 1e-8 * np.linalg.norm(ref)
        assert np.linalg.norm(b - S @ x) <= 1e-12 * np.linalg.norm(b) * (1 + 1e-9)


def test_gmres_oracle_restarts_and_early_exits():
    m, A = eps_matrix()
    S = to_pattern_csr(m, A, 2)
    b = np.random.Generator(np.random.PCG64(2)).normal(size=A.shape[0])
    ref = scipy.sparse.linalg.spsolve(S.tocsc(), b)
    x, its, conv, _ = gmres_ref(S, b, inv=block_jacobi_ref(S, 2), m=5, rtol=1e-10, maxiter=5000)
    assert conv and its > 5                                   # several cycles
    assert np.linalg.norm(x - ref) <= 1e-7 * np.linalg.norm(ref)
    x, its, conv, res = gmres_ref(S, np.zeros_like(b))
    assert its == 0 and conv and not x.any()
    x, its, conv, res = gmres_ref(S, b, m=30, maxiter=3)
    assert its == 3 and not conv and res < 1.0
    # a single pass of Gram-Schmidt solves it as well here
    x, its1, conv, _ = gmres_ref(S, b, inv=block_jacobi_ref(S, 2), m=30, reorth=False)
    assert conv and np.linalg.norm(x - ref) <= 1e-7 * np.linalg.norm(ref)


def test_cg_oracle_on_an_spd_elastic_matrix():
    m, A = eps_matrix(nonsym_seed=None)
    S = to_pattern_csr(m, A, 2)
    assert abs(S - S.T).max() <= 1e-14 * abs(S).max() and np.linalg.eigvalsh(0.5 * (A + A.T)).min() > 0
    b = np.random.Generator(np.random.PCG64(4)).normal(size=A.shape[0])
    ref = scipy.sparse.linalg.spsolve(S.tocsc(), b)
    for inv in (None, block_jacobi_ref(S, 2)):
        x, its, conv = cg_ref(S, b, inv=inv, rtol=1e-12)
        assert conv and np.linalg.norm(x - ref) <= 1e-8 * np.linalg.norm(ref)
    xg, _, conv, _ = gmres_ref(S, b, inv=block_jacobi_ref(S, 2), rtol=1e-12)
    assert conv and np.linalg.norm(xg - ref) <= 1e-8 * np.linalg.norm(ref)


@pytest.mark.parametrize("case", ["heat", "eps"])
def test_block_inverses_are_the_inverses_of_the_blocks(case):
    m, A = heat_matrix() if case == "heat" else eps_matrix()
    bs = 1 if case == "heat" else 2
    S = to_pattern_csr(m, A, bs)
    inv = block_jacobi_ref(S, bs)
    D = np.stack([A[k * bs:(k + 1) * bs, k * bs:(k + 1) * bs] for k in range(A.shape[0] // bs)])
    assert np.allclose(inv, np.linalg.inv(D), rtol=0, atol=1e-12 * np.abs(inv).max())
    assert np.allclose(np.einsum("nij,njk->nik", inv, D), np.eye(bs), atol=1e-12)
    # a Dirichlet component keeps its block invertible: its row and column are the unit vector
    dofs = bottom_dofs(m, bs) if case == "eps" else boundary_dofs(m, bs)
    k = dofs[0] // bs
    assert np.allclose(D[k][dofs[0] % bs], np.eye(bs)[dofs[0] % bs])
