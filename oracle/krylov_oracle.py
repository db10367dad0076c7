"""The NumPy yardstick of dxo_krylov_gmres / dxo_krylov_fgmres / dxo_krylov_cg / dxo_csr_block_jacobi. Pinned by
tests/test_krylov_oracle_cpu.py, tests/test_krylov_fp32_basis_oracle_cpu.py and tests/test_fgmres_kcycle_oracle_cpu.py.

gmres_ref restates the device algorithm step for step: restarted GMRES(m) with right preconditioning, classical Gram-Schmidt with
one reorthogonalisation pass, Givens rotations, the first step whose estimate |g_{j+1}| met max(rtol |b|, atol) as the cycle's
length, the true residual b - A x at every restart. gmres_cb_ref is gmres_ref with every stored basis vector passed through float32
(DXO_KRYLOV_BASIS_FP32): the vector is rounded once, the rounded vector is what is stored, what the preconditioner and the operator
are given at the next step and what the update combines; everything else stays float64. fgmres_ref is gmres_ref with the
preconditioned vectors z_j = M_j v_j kept: w = A z_j, and x += Z^T y at the end of a cycle with no further call of M.
block_jacobi_ref inverts the bs x bs diagonal blocks. The test matrices are the assembled matrices the device makes: the heat Jacobian
of the heat demo (non-symmetric, bs = 1), an (eps, eps) matrix with a random non-symmetric C (bs = 2) and an SPD elastic matrix
(CG), each with Dirichlet rows."""
import numpy as np
import scipy.sparse

from oracle.form_oracle import apply_bcs, dense_ref, heat_setting, pattern_ref
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
    """z = inv r per block, or entry by entry for a 1-D inv; inv None: identity; a callable r -> z (a multigrid cycle) is called."""
    if inv is None:
        return r.copy()
    if callable(inv):
        return inv(r)
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


def gmres_ref(A, b, x0=None, inv=None, m=30, rtol=1e-10, atol=0.0, maxiter=1000, reorth=True, full=False, dtype=float, stored=None,
              basis=None):
    """(x, iterations, converged, true relative residual) of the device's restarted GMRES(m); with full=True also
    (..., breakdown, cycles started), the device's info.breakdown and info.restarts. dtype: the arithmetic (np.longdouble: the
    same algorithm as a referee of the float64 run). stored: what a basis vector becomes when it is stored (None: itself);
    basis: a list that receives the stored rows of the last cycle as float32."""
    n = b.size
    stored = stored or (lambda v: v)
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
        V[0] = stored(r / beta)
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
            V[j + 1] = stored(w / hn) if hn > 0 else 0.0
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
        if basis is not None:
            basis[:] = [V.astype(np.float32)]
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


def f32(v):
    """v rounded to float32 (nearest even) and widened again."""
    return v.astype(np.float32).astype(np.float64)


# gmres_cb_ref against the long-double answers of F2 (n = 2965, restart 64, k = 1..64), measured by
# test_reference_deviation_of_the_compressed_basis of tests/test_krylov_fp32_basis_oracle_cpu.py, which prints them (-s): the residual
# against the closed form, relative, 2.2e-3 (at k = 64); x_k against gmres_ref in long double, max|dx| / max|x|, 5.8e-8. Both are the
# rounding of v_0: the cycle solves for beta v_0 with v_0 = fl32(r / beta), so the part beta (r / beta - v_0) of the residual, about
# 2^-24 |r|, is not touched by this cycle. At k = 64 the closed form has fallen to 3.8e-7 of |r| and that part is a visible share of
# it: this is the "seven digits per cycle" of the option, seen on a known answer. The constants are round upper bounds.
REF_CB_F2_RES, REF_CB_F2_X = 3e-3, 1e-7


def gmres_cb_ref(A, b, **kw):
    """gmres_ref (float64) with the basis stored in float32."""
    return gmres_ref(A, b, stored=f32, **kw)


def fgmres_ref(A, b, M=None, x0=None, m=30, rtol=1e-10, atol=0.0, maxiter=1000, reorth=True):
    """(x, iterations, converged, true relative residual, breakdown, cycles started, calls of M) of the device's flexible GMRES(m).
    M: None or a callable (r, j) -> z with j the number of earlier calls."""
    n = b.size
    x = np.zeros(n) if x0 is None else x0.astype(float).copy()
    bnorm = np.linalg.norm(b)
    total, breakdown, cycles, calls = 0, False, 0, 0
    if bnorm == 0.0:
        return np.zeros(n), 0, True, 0.0, False, 0, 0
    tol = max(rtol * bnorm, atol)
    while True:
        r = b - A @ x
        beta = np.linalg.norm(r)
        if beta <= tol:
            return x, total, True, beta / bnorm, breakdown, cycles, calls
        if total >= maxiter or breakdown:
            return x, total, False, beta / bnorm, breakdown, cycles, calls
        cycles += 1
        V, Z, H = np.zeros((m + 1, n)), np.zeros((m, n)), np.zeros((m + 1, m))
        cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        V[0] = r / beta
        g[0] = beta
        k = 0
        for j in range(m):
            if total + j >= maxiter:
                break
            Z[j] = V[j].copy() if M is None else M(V[j], calls)
            calls += M is not None
            w = A @ Z[j]
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
            return x, total, False, beta / bnorm, breakdown, cycles, calls
        y = np.zeros(k)
        for i in range(k - 1, -1, -1):
            s = g[i] - H[i, i + 1: k] @ y[i + 1:]
            y[i] = s / H[i, i] if H[i, i] != 0 else 0.0
        x = x + Z[:k].T @ y                                # no call of M here
        total += k


def same(a, b):
    """Two results of the oracles, bit for bit."""
    return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(a, b)) and len(a) == len(b)


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


def elastic_C3(n_points, nonsym_seed=None):
    """Per-point Mandel blocks (n, 6, 6) of isotropic elasticity in 3-D, plus a random non-symmetric part with a seed."""
    lam, mu = 1.0, 0.7
    Ce = np.zeros((6, 6))
    Ce[:3, :3] = lam
    Ce[np.arange(6), np.arange(6)] += 2 * mu
    C = np.broadcast_to(Ce, (n_points, 6, 6)).copy()
    if nonsym_seed is not None:
        C += 0.3 * np.random.Generator(np.random.PCG64(nonsym_seed)).normal(size=C.shape)
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


def f2_problem(q, t, D=None):
    """(src, b, operator) of the F2 family on n = 80 q + t entries."""
    src, b = cyclic_shift_src(F2_D, q, t), cycle_rhs(F2_D, q, t, seed=q)
    return src, b, shifted_op(src, D=D)


def unit_rhs(n, s):
    """0.25 e_s: |b| and b / |b| are exact, and so is every basis vector of a permutation."""
    b = np.zeros(n)
    b[s] = 0.25
    return b


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
