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
    """z = inv r per block, or entry by entry for a 1-D inv; inv None: identity."""
    if inv is None:
        return r.copy()
    if inv.ndim == 1:                                     # an inverse diagonal (DXO_PC_JACOBI)
        return inv * r
    nb, bs, _ = inv.shape
    return np.einsum("nij,nj->ni", inv, r.reshape(nb, bs)).reshape(-1)


class FnOperator:
    """A callable v -> A v behind the `A @ v` the oracles use (the matrix-free operators of the known-answer families)."""

    def __init__(self, fn):
        self.fn = fn

    def __matmul__(self, v):
        return self.fn(v)


def gmres_ref(A, b, x0=None, inv=None, m=30, rtol=1e-10, atol=0.0, maxiter=1000, reorth=True, full=False, dtype=float):
    """(x, iterations, converged, true relative residual) of the device's restarted GMRES(m); with full=True also
    (..., breakdown, cycles started), the device's info.breakdown and info.restarts. dtype: the arithmetic (np.longdouble: the
    same algorithm as a referee of the float64 run)."""
    n = b.size
    b = b.astype(dtype)
    x = np.zeros(n, dtype) if x0 is None else x0.astype(dtype).copy()
    bnorm = np.linalg.norm(b)
    total, breakdown, cycles = 0, False, 0

    def result(x, conv, res):
        return (x, total, conv, res, breakdown, cycles) if full else (x, total, conv, res)

    if bnorm == 0.0:
        return result(np.zeros(n, dtype), True, 0.0)
    tol = max(rtol * bnorm, atol)
    while True:
        r = b - A @ x
        beta = np.linalg.norm(r)
        if beta <= tol:
            return result(x, True, beta / bnorm)
        if total >= maxiter or breakdown:
            return result(x, False, beta / bnorm)
        cycles += 1
        V = np.zeros((m + 1, n), dtype)
        H = np.zeros((m + 1, m), dtype)
        cs, sn, g = np.zeros(m, dtype), np.zeros(m, dtype), np.zeros(m + 1, dtype)
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
            return result(x, False, beta / bnorm)
        y = np.zeros(k, dtype)
        for i in range(k - 1, -1, -1):
            s = g[i] - H[i, i + 1: k] @ y[i + 1:]
            y[i] = s / H[i, i] if H[i, i] != 0 else 0.0
        x = x + apply_pc(inv, V[:k].T @ y)
        total += k


def cg_ref(A, b, inv=None, rtol=1e-10, atol=0.0, maxiter=1000, full=False):
    """(x, iterations, converged) of preconditioned CG from x = 0; with full=True
    (x, iterations, converged, true relative residual, breakdown, cycles started) as the device reports them: (p, q) = 0 or not
    finite is a breakdown, which keeps the iterate of the step before."""
    bnorm = np.linalg.norm(b)
    tol = max(rtol * bnorm, atol)
    x = np.zeros_like(b)

    def result(it, conv, breakdown):
        if not full:
            return x, it, conv
        res = np.linalg.norm(b - A @ x)
        return x, it, bool(res <= tol), res / bnorm if bnorm > 0 else 0.0, breakdown, int(bnorm > tol and maxiter > 0)

    r = b.copy()
    if bnorm <= tol:
        return result(0, True, False)
    z = apply_pc(inv, r)
    p = z.copy()
    rz = r @ z
    for it in range(1, maxiter + 1):
        q = A @ p
        pq = p @ q
        if full and not (pq != 0.0 and np.isfinite(pq)):
            return result(it - 1, False, True)
        alpha = rz / pq
        x += alpha * p
        r -= alpha * q
        if np.linalg.norm(r) <= tol:
            return result(it, True, False)
        z = apply_pc(inv, r)
        rzn = r @ z
        p = z + (rzn / rz) * p
        rz = rzn
    return result(maxiter, False, False)


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


# ---- known answers: operators whose GMRES / CG history is known in closed form (tests/test_krylov_known_answers_gpu.py runs the
# same families on the device)
U = float(np.finfo(float).eps) / 2                       # unit roundoff of float64
SHIFT_D = (1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)      # both sides of every KMAX switch of kr_kmax (4 / 8 / 16 / 32 / 64)
F2_C, F2_S, F2_D = 1.0, 0.8, 80                         # A = c I + s P on cycles longer than the longest restart
GRID_CAP_256CU = 256 * 4 * 256                          # rows one trip of the row kernels covers on 256 compute units
# (q, t) of the F2 sizes: n = 80 q + t = 80, 2480, 255, 256, 257, 70 003 (more than 256 partials), just above the grid cap of 256
# compute units and more than twice that cap with a ragged tail
F2_SIZES = ((1, 0), (31, 0), (3, 15), (3, 16), (3, 17), (875, 3), (GRID_CAP_256CU // F2_D + 1, 7), (2 * GRID_CAP_256CU // F2_D + 1, 13))
F2_MAIN = (37, 5)                                       # n = 2965: every k in 1..64
# The float64 oracle's own deviation, measured here by test_cyclic_shift_terminates_at_step_d_and_stagnates_below (F1) and
# test_reference_deviation_of_the_shifted_shift (F2), which print it (-s):
#   F1, |x - P^T b| / max|b| and the residual at termination: 4.5e-16 and 3.6e-16;
#   F2, residual against the long-double closed form, relative: 6.5e-16 over k = 1..64, all sizes, preconditioned, one pass, short restarts;
#   F2, x_k against the same algorithm in long double, max|dx| / max|x|: 5.2e-16.
# The constants are round upper bounds of these; the device is held to 100 x them (the margin of CYCLE_TOL in test_amg_gpu.py).
REF_F1_X, REF_F1_RES = 6e-16, 4e-16
REF_F2_RES, REF_F2_X = 1e-15, 1e-15
MARGIN = 100


def cyclic_shift_src(d, q, t):
    """src of the permutation (P v)[i] = v[src[i]] on n = t + d q entries: t fixed points first, then q cycles of length d that
    move every entry one place up (the last of a cycle to its first)."""
    src = np.arange(t + d * q)
    src[t:] = t + np.roll(np.arange(d * q).reshape(q, d), 1, axis=1).reshape(-1)
    return src


def cycle_rhs(d, q, t, seed=0):
    """b: non-zero (0.5 <= |b_i| < 1.5, random sign) on the first entry of each cycle, zero elsewhere."""
    rng = np.random.Generator(np.random.PCG64(seed))
    b = np.zeros(t + d * q)
    b[t + d * np.arange(q)] = rng.uniform(0.5, 1.5, q) * rng.choice([-1.0, 1.0], q)
    return b


def shift_op(src):
    return FnOperator(lambda v: v[src])


def shifted_op(src, c=F2_C, s=F2_S, D=None):
    """c I + s P, or (c I + s P) diag(D)."""
    def fn(v):
        v = v if D is None else D * v
        return c * v + s * v[src]
    return FnOperator(fn)


def shift_solution(src, b):
    """P^T b, the solution of P x = b."""
    x = np.zeros_like(b)
    x[src] = b
    return x


def shifted_residual(k, c=F2_C, s=F2_S):
    """|b - A x_k| / |b| of GMRES on c I + s P after k < d steps, in long double: 1 / sqrt(sum_{i <= k} (c/s)^(2i))."""
    rho2 = (np.longdouble(c) / np.longdouble(s)) ** 2
    return 1 / np.sqrt(np.sum(rho2 ** np.arange(k + 1, dtype=np.longdouble)))


def shifted_atol(k, bnorm, c=F2_C, s=F2_S):
    """The absolute tolerance between the residuals of steps k - 1 and k (their geometric mean): a factor >= sqrt(c/s) from both."""
    return float(bnorm * np.sqrt(shifted_residual(k - 1, c, s) * shifted_residual(k, c, s)))


def precond_diagonal(n, seed=1):
    return np.random.Generator(np.random.PCG64(seed)).uniform(0.5, 2.0, n)


def nilpotent_op(n):
    def fn(v):
        out = np.zeros_like(v)
        out[1:] = v[:-1]
        return out
    return FnOperator(fn)


def exact_breakdown_rhs(n):
    """Entries +-1 on n a power of 4: |b| = 2^k and b / |b| are exact, (v, v) = 1 exactly, so A = I breaks down with hn == 0."""
    assert n >= 1 and 4 ** round(np.log(n) / np.log(4)) == n
    return np.where(np.arange(n) % 3 == 0, -1.0, 1.0)


def xdev(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def test_cyclic_shift_terminates_at_step_d_and_stagnates_below():
    worst_x = worst_r = 0.0
    for d in SHIFT_D:
        for q, t in ((1, 0), (31, 0), (3, 2)):
            src, b = cyclic_shift_src(d, q, t), cycle_rhs(d, q, t, seed=d)
            P, xs = shift_op(src), shift_solution(src, b)
            assert np.array_equal(P @ xs, b)
            for m, reorth in ((64, True), (d, True), (64, False)):
                x, its, conv, res, _, cycles = gmres_ref(P, b, m=m, rtol=1e-10, reorth=reorth, full=True)
                assert (its, conv, cycles) == (d, True, 1), (d, q, t, m, its)
                worst_x, worst_r = max(worst_x, np.abs(x - xs).max() / np.abs(b).max()), max(worst_r, res)
            if d == 1:
                continue                                      # no step before the first, no restart length 0
            x, its, conv, res, brk, cycles = gmres_ref(P, b, m=64, rtol=1e-10, maxiter=d - 1, full=True)
            assert (its, conv, brk, cycles) == (d - 1, False, False, 1) and abs(res - 1) <= 4 * U and not x.any()      # no progress before d
            x, its, conv, res, brk, cycles = gmres_ref(P, b, m=d - 1, rtol=1e-10, maxiter=3 * (d - 1), full=True)
            assert (its, conv, brk, cycles) == (3 * (d - 1), False, False, 3), (d, its, cycles)
            assert res == 1.0 and not x.any()
    print(f"F1 reference deviation: x {worst_x:.2e} max|b|, residual {worst_r:.2e}")
    assert worst_x <= REF_F1_X and worst_r <= REF_F1_RES
    # x0 already the solution: nothing runs
    src, b = cyclic_shift_src(9, 5, 3), cycle_rhs(9, 5, 3)
    xs = shift_solution(src, b)
    x, its, conv, res, brk, cycles = gmres_ref(shift_op(src), b, x0=xs, m=64, full=True)
    assert (its, conv, brk, cycles, res) == (0, True, False, 0, 0.0) and np.array_equal(x, xs)


def _f2(q, t, D=None):
    src, b = cyclic_shift_src(F2_D, q, t), cycle_rhs(F2_D, q, t, seed=q)
    return src, b, shifted_op(src, D=D)


def test_reference_deviation_of_the_shifted_shift():
    """The oracle against the closed form (residual) and against itself in long double (x_k): what REF_F2_* bound."""
    worst_r = worst_x = 0.0
    L = np.longdouble

    def check(q, t, k, m=64, reorth=True, precond=False, closed=True, referee=True):
        nonlocal worst_r, worst_x
        D = precond_diagonal(t + F2_D * q) if precond else None
        src, b, A = _f2(q, t, D)
        inv = None if D is None else 1.0 / D
        x, its, conv, res, brk, cycles = gmres_ref(A, b, inv=inv, m=m, rtol=0.0, maxiter=k, reorth=reorth, full=True)
        assert (its, conv, brk, cycles) == (k, False, False, -(-k // m)), (q, t, k, m)
        if not referee:                                       # the residual against the formula alone
            worst_r = max(worst_r, float(abs(res - shifted_residual(k)) / shifted_residual(k)))
            return
        xl, _, _, resl = gmres_ref(shifted_op(src), b.astype(L), m=m, rtol=0.0, maxiter=k, dtype=L)
        assert xl.dtype == L
        if closed:
            f = shifted_residual(k)
            assert abs(resl - f) <= 1e-17 * f                 # the long-double run confirms the formula
        else:
            f = resl
        worst_r = max(worst_r, float(abs(res - f) / f))
        worst_x = max(worst_x, xdev(x, (xl if D is None else xl / D).astype(float)))

    for k in range(1, 65):
        check(*F2_MAIN, k)
    for q, t in F2_SIZES:
        for k in (1, 33, 64):
            check(q, t, k, referee=k == 64 or q < 1000)       # the long-double run of the two largest sizes at k = 64 only: it is slow
    for k in (1, 2, 5, 17, 33, 64):
        check(*F2_MAIN, k, reorth=False)
        check(*F2_MAIN, k, precond=True)
    for m in (1, 2, 3, 7):
        check(*F2_MAIN, 20, m=m, closed=False)
    print(f"F2 reference deviation: residual {worst_r:.2e} relative, x {worst_x:.2e} max|x|")
    assert worst_r <= REF_F2_RES and worst_x <= REF_F2_X
    assert MARGIN * max(REF_F2_RES, REF_F2_X, REF_F1_X, REF_F1_RES) <= 1e-11


def test_shifted_shift_stops_on_atol_at_step_k():
    src, b, A = _f2(*F2_MAIN)
    bnorm = np.linalg.norm(b)
    for k in (1, 2, 5, 17, 33, 64):
        lo, hi = float(shifted_residual(k)), float(shifted_residual(k - 1))
        atol = shifted_atol(k, bnorm)
        assert lo * np.sqrt(F2_C / F2_S) <= atol / bnorm <= hi / np.sqrt(F2_C / F2_S)        # never near a tie
        x, its, conv, res, brk, cycles = gmres_ref(A, b, m=64, rtol=0.0, atol=atol, full=True)
        assert (its, conv, brk, cycles) == (k, True, False, 1) and abs(res - lo) <= REF_F2_RES * lo


def test_breakdowns_of_the_oracle():
    I = FnOperator(lambda v: v.copy())
    x, its, conv, res, brk, cycles = gmres_ref(I, np.array([-4.0]), m=64, full=True)
    assert (its, conv, brk, cycles, res) == (1, True, True, 1, 0.0) and x[0] == -4.0
    for n in (4, 16, 64, 256, 1024, 4096, 65536):
        b = exact_breakdown_rhs(n)
        x, its, conv, res, brk, _ = gmres_ref(I, b, m=64, full=True)
        assert (its, conv, brk) == (1, True, True) and np.array_equal(x, b), n
    for n in (2, 3, 31, 257, 1000):                           # any b: one step, breakdown or not
        b = cycle_rhs(1, n, 0, seed=n)
        x, its, conv, res, _, _ = gmres_ref(I, b, m=64, full=True)
        assert (its, conv) == (1, True) and np.abs(x - b).max() <= 4 * U * np.abs(b).max()
    for n in (2, 33, 300):                                    # singular A, A b = 0: nothing to gain, reported as a breakdown
        b = np.zeros(n)
        b[-1] = 3.0
        for x0 in (None, 7.0 * b):                            # A x0 = 0 as well: x0 comes back untouched
            x, its, conv, res, brk, cycles = gmres_ref(nilpotent_op(n), b, x0=x0, m=64, full=True)
            assert (its, conv, brk, cycles) == (1, False, True, 1) and res == 1.0 and np.isfinite(x).all()
            assert np.array_equal(x, np.zeros(n) if x0 is None else x0)
    # a step that met the tolerance with hn > 0 is no breakdown, whatever a later step would find
    b = np.array([-4.0, 0.0, 0.0])
    x, its, conv, res, brk, cycles = gmres_ref(late_zero_op(), b, m=64, rtol=0.1, full=True)
    eps = 2.0 ** -10
    assert (its, conv, brk, cycles) == (1, True, False, 1) and abs(res - eps / np.hypot(1, eps)) <= 16 * U * eps


def late_zero_op(eps=2.0 ** -10):
    """A e0 = e0 + eps e1, A e1 = A e2 = 0 on n = 3: from b = -4 e0 the first step meets rtol = 0.1 with hn = eps > 0, all in
    exact arithmetic; the second step finds A v1 = 0."""
    def fn(v):
        out = np.zeros_like(v)
        out[0], out[1] = v[0], eps * v[0]
        return out
    return FnOperator(fn)


def alternating_diag(n):
    return np.where(np.arange(n) % 2 == 0, 1.0, -1.0)


def repeated_diag(d, n):
    return 1.0 + np.arange(n) % d


def test_cg_breakdown_and_exact_termination():
    for n in (2, 64, 1000):
        dg = alternating_diag(n)
        x, its, conv, res, brk, cycles = cg_ref(FnOperator(lambda v: dg * v), np.ones(n), full=True)
        assert (its, conv, brk, cycles) == (0, False, True, 1) and res == 1.0 and not x.any()
    for d in range(1, 9):
        n = 37 * d + 3
        dg = repeated_diag(d, n)
        A = FnOperator(lambda v: dg * v)
        x, its, conv, res, brk, _ = cg_ref(A, np.ones(n), full=True)
        assert (its, conv, brk) == (d, True, False), (d, its)
        assert np.abs(x - 1 / dg).max() <= 1e-10
        if d > 1:
            _, its1, conv1 = cg_ref(A, np.ones(n), maxiter=d - 1)
            assert its1 == d - 1 and not conv1
        x, its, conv, res, brk, _ = cg_ref(A, np.ones(n), inv=1 / dg, full=True)
        assert (its, conv, brk) == (1, True, False)
