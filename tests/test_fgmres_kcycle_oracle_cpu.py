"""NumPy oracle of flexible GMRES (dxo_krylov_fgmres) and of the K-cycle (dxo_amg_set_cycle), built on the oracles of
test_krylov_oracle_cpu.py and of the multigrid modules (imported, not edited), and what they promise (not gpu).

fgmres_ref is gmres_ref with the preconditioned vectors z_j = M_j v_j kept: w = A z_j, and x += Z^T y at the end of a cycle with no
further call of M. M is a callable (r, j) -> z, j the number of calls before this one, so a test can make it vary.

kcycle_ref walks a hierarchy given as SciPy matrices (the Level lists of amg_ref, amg_nns_ref, amg_soc_ref, amg_cheby_ref, or one read
back from the device): level 0 runs one cycle body, the coarsest its dense solve, and every level between them solves A_l x = r by the
two GCR steps of gcr2_ref preconditioned by the body of that level, with the two guards of the device.

Iterations x level visits, measured here (test_fgmres_with_the_k_cycle_against_gmres_with_the_v_cycle, rtol 1e-8, right-hand side seed 1,
GMRES(30) + V against FGMRES(30) + K; visits per apply V / K):

    P2 eps/eps 14 x 14, rigid-body modes, coarse_rows 20   rows 1682 / 168 / 12       V  59 its x 3 = 177, K  52 its x  5 = 260
    P1 heat 16 x 16, coarse_rows 10                        rows 289 / 25 / 4          V  16 its x 3 =  48, K  16 its x  5 =  80
    eps_matrix((14, 14)) non-symmetric, coarse_rows 20     rows 1682 / 112 / 8        V 136 its x 3 = 408, K 123 its x  5 = 615
    anisotropic 24 x 24 quadrilaterals, strength 0.25, 10  rows 625 / 184 / 69 / 46   V  18 its x 4 =  72, K  18 its x 11 = 198

K never needs more iterations than V and saves at most 12 %; by iterations x level visits it loses on every one of these systems.
The hierarchies coarsen so fast that the two-grid step of level 0 limits the cycle, not the accuracy of the coarse solves, which
is all the K-cycle improves. It stays opt-in; see DESIGN 9.5."""
import numpy as np
import pytest

import test_amg_cheby_oracle_cpu as cheby_oracle
import test_amg_nns_oracle_cpu as nns_oracle
import test_amg_soc_oracle_cpu as soc_oracle
from test_amg_oracle_cpu import U, amg_ref, apply_block, callable_preconditioners, vcycle_ref
from test_krylov_oracle_cpu import (block_jacobi_ref, bottom_dofs, boundary_dofs, eps_matrix, gmres_ref, heat_matrix, to_pattern_csr)

K_DEPENDENT = 1e-14      # rho2 <= K_DEPENDENT beta: the second direction depends on the first (the rule of a singular diagonal block)


# ---- flexible GMRES
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


# ---- the K-cycle
def smooth_ref(L, r, x=None):
    """The relaxation of a level: the Chebyshev polynomial of the levels of amg_cheby_ref, damped block-Jacobi sweeps otherwise."""
    if getattr(L, "smoother", "jacobi") == "chebyshev":
        return cheby_oracle.cheby_ref(L.A, L.Dinv, L.rho, L.lower, L.degree, r, x)
    x = np.zeros_like(r) if x is None else x
    for _ in range(L.sweeps):
        x = x + L.omega * apply_block(L.Dinv, r - L.A @ x)
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


def kcycle_ref(levels, r, trace=None, visits=None):
    """z = K(r). trace: a dict level -> list of gcr2_ref records; visits: a list per level, counted up at every visit."""
    last = len(levels) - 1

    def solve(rc, l):
        if l == last:
            if visits is not None:
                visits[l] += 1
            return levels[l].dense_inverse @ rc
        return gcr2_ref(levels[l].A, lambda q: body(q, l), rc, None if trace is None else trace.setdefault(l, []))

    def body(q, l):
        L = levels[l]
        if visits is not None:
            visits[l] += 1
        x = smooth_ref(L, q)
        x = x + L.P @ solve(L.P.T @ (q - L.A @ x), l + 1)
        return smooth_ref(L, q, x)

    if last == 0:
        return solve(r, 0)
    return body(r, 0)


def k_visits(n_levels):
    """Level visits of one K-cycle: 2^l on level l but the coarsest, which is visited as often as the level above it."""
    if n_levels == 1:
        return 1
    return sum(2 ** l for l in range(n_levels - 1)) + 2 ** (n_levels - 2)


def vcycle_any_ref(levels, r, l=0):
    """The V-cycle of a hierarchy with either relaxation (vcycle_ref / vcycle_cheby_ref in one)."""
    L = levels[l]
    if l == len(levels) - 1:
        return L.dense_inverse @ r
    x = smooth_ref(L, r)
    x = x + L.P @ vcycle_any_ref(levels, L.P.T @ (r - L.A @ x), l + 1)
    return smooth_ref(L, r, x)


def fgmres_with_kcycle(S, b, levels, **kw):
    return fgmres_ref(S, b, M=lambda r, j: kcycle_ref(levels, r), **kw)


# ---- the systems of the earlier oracle tests, coarsened far enough for three levels and more
_CACHE = {}


def system(which):
    """(S, b, levels): "p2_rbm" P2 eps/eps 14 x 14 with rigid-body modes, "heat" the P1 heat Jacobian 16 x 16, "nonsym" the
    non-symmetric eps_matrix((14, 14)), "aniso" the anisotropic 24 x 24 quadrilaterals with strength 0.25, "heat48" the scalar P1
    system of 2401 rows on four levels."""
    if which not in _CACHE:
        if which == "p2_rbm":
            m, S, dofs = nns_oracle.eps_spd((14, 14))
            levels = nns_oracle.amg_nns_ref(S, 2, dofs, nns_oracle.rigid_body_modes_ref(m.node_x), coarse_rows=20)
        elif which in ("heat", "heat48"):
            m, A = heat_matrix(16 if which == "heat" else 48)
            S = to_pattern_csr(m, A, 1)
            levels = amg_ref(S, 1, boundary_dofs(m, 1), coarse_rows=10)
        elif which == "nonsym":
            m, A = eps_matrix((14, 14))
            S = to_pattern_csr(m, A, 2)
            levels = amg_ref(S, 2, bottom_dofs(m, 2), coarse_rows=20)
        else:
            m, S, dofs = soc_oracle.cached_aniso("quadrilateral")
            levels = soc_oracle.amg_soc_ref(S, 1, dofs, soc_oracle.THETA, coarse_rows=10)
        b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
        _CACHE[which] = (S, b, levels)
    return _CACHE[which]


# ---- tests
@pytest.mark.parametrize("which", ["heat", "nonsym"])
def test_fgmres_with_a_fixed_preconditioner_is_gmres(which):
    """With a fixed linear M the two methods build the same Krylov space: x_k = x_0 + M V_k y against x_0 + (M V_k) y, the same vector
    but for the rounding of one more application of M. The true relative residuals after k steps therefore differ by a few
    u |A| |M| |V_k y| / |b|, far below 1e-10 on these systems (condition numbers of some 1e3); the counts are equal."""
    S, b, levels = system(which)
    if which == "heat":
        inv = block_jacobi_ref(S, 1)

        def M(r, j):
            return apply_block(inv, r)
    else:                                                  # the V-cycle: a fixed linear operator too
        def inv(r):
            return vcycle_ref(levels, r)

        def M(r, j):
            return vcycle_ref(levels, r)

    with callable_preconditioners():
        return _fixed_preconditioner(which, S, b, inv, M)


def _fixed_preconditioner(which, S, b, inv, M):
    _, its_g, conv_g, res_g = gmres_ref(S, b, inv=inv, m=30, rtol=1e-10, maxiter=3000)
    xf, its_f, conv_f, res_f, _, cycles, calls = fgmres_ref(S, b, M=M, m=30, rtol=1e-10, maxiter=3000)
    assert conv_g and conv_f and its_f == its_g and calls == its_f and cycles > 1, (its_f, its_g, calls, cycles)
    assert np.linalg.norm(b - S @ xf) <= 1e-10 * np.linalg.norm(b) * (1 + 1e-6)
    worst = 0.0
    for k in list(range(1, 35)) + [its_g - 1]:
        _, ig, _, rg = gmres_ref(S, b, inv=inv, m=30, rtol=1e-10, maxiter=k)
        _, i_f, _, rf, *_ = fgmres_ref(S, b, M=M, m=30, rtol=1e-10, maxiter=k)
        assert ig == i_f == k
        worst = max(worst, abs(rf - rg))
    print(f"{which}: {its_g} iterations, largest difference of the residual histories {worst:.2e}")
    assert worst <= 1e-10


def test_k_on_two_levels_is_the_pinned_v_cycle():
    m, A = heat_matrix(16)
    S = to_pattern_csr(m, A, 1)
    levels = amg_ref(S, 1, boundary_dofs(m, 1), coarse_rows=60)
    assert len(levels) == 2 and k_visits(2) == 2 and k_visits(1) == 1
    rng = np.random.Generator(np.random.PCG64(3))
    for _ in range(3):
        r = rng.normal(size=S.shape[0])
        assert np.array_equal(kcycle_ref(levels, r), vcycle_ref(levels, r))
    one = amg_ref(S, 1, boundary_dofs(m, 1), coarse_rows=400)
    assert len(one) == 1 and np.array_equal(kcycle_ref(one, r), vcycle_ref(one, r))


@pytest.mark.parametrize("which", ["heat48", "aniso"])
def test_every_gcr_solve_minimises_the_residual(which):
    """|r - A x| <= |r - (a1 / rho1) A c1| <= |r| on every intermediate level: each GCR step minimises the residual over its
    direction(s). In floating point up to a few u |A| |x| per evaluated residual (8 u (| |A| |x| | + |r|) here)."""
    S, _, levels = system(which)
    assert len(levels) >= 4, [L.n_rows for L in levels]
    visits, trace = [0] * len(levels), {}
    rng = np.random.Generator(np.random.PCG64(5))
    for _ in range(2):
        z = kcycle_ref(levels, rng.normal(size=S.shape[0]), trace, visits)
        assert np.isfinite(z).all()
    assert sorted(trace) == list(range(1, len(levels) - 1))
    assert visits == [2 * v for v in [2 ** l for l in range(len(levels) - 1)] + [2 ** (len(levels) - 2)]] and sum(visits) == 2 * k_visits(len(levels))
    for l, records in trace.items():
        A = levels[l].A
        assert len(records) == 2 * 2 ** (l - 1)
        for r, x1, x, hit in records:
            assert hit is None
            n0, n1, n2 = np.linalg.norm(r), np.linalg.norm(r - A @ x1), np.linalg.norm(r - A @ x)
            slack = 8 * U * (np.linalg.norm(abs(A) @ abs(x)) + np.linalg.norm(abs(A) @ abs(x1)) + n0)
            assert n2 <= n1 + slack and n1 <= n0 + slack, (which, l, n0, n1, n2)
        print(f"{which} rows {[L.n_rows for L in levels]} level {l}: |r| {n0:.3e} -> one step {n1:.3e} -> two steps {n2:.3e}")


def test_guards():
    S, _, levels = system("heat")
    A = levels[1].A
    n = A.shape[0]
    rng = np.random.Generator(np.random.PCG64(7))
    # r = 0: c1 = 0, rho1 = 0, x = 0 exactly
    trace = []
    x = gcr2_ref(A, lambda q: levels[1].omega * apply_block(levels[1].Dinv, q), np.zeros(n), trace)
    assert not x.any() and trace[-1][3] == "rho1"
    z = kcycle_ref(levels, np.zeros(S.shape[0]))
    assert not z.any() and np.isfinite(z).all()
    # B of rank one: c2 is a multiple of c1, rho2 is rounding noise of beta, x = (a1 / rho1) c1
    u, w, r = rng.normal(size=n), rng.normal(size=n), rng.normal(size=n)
    x = gcr2_ref(A, lambda q: u * (w @ q), r, trace)
    c1 = u * (w @ r)
    v1 = A @ c1
    assert trace[-1][3] == "rho2" and np.array_equal(x, ((v1 @ r) / (v1 @ v1)) * c1) and np.array_equal(x, trace[-1][1])
    # and a B that answers NaN in the second call only: rho2 is not finite
    calls = []

    def B(q):
        calls.append(1)
        return u * (w @ q) if len(calls) == 1 else np.full(n, np.nan)

    x = gcr2_ref(A, B, r, trace)
    assert trace[-1][3] == "rho2" and np.array_equal(x, ((v1 @ r) / (v1 @ v1)) * c1)


@pytest.mark.parametrize("which", ["heat48", "aniso", "p2_rbm"])
def test_the_k_cycle_is_homogeneous_in_r(which):
    """K(2^e r) == 2^e K(r) bit for bit, finite, and without a guard at |e| up to 480: the K-cycle is not linear, but its
    coefficients are ratios of dot products, homogeneous of degree 0, and every other step is linear. The dot products are second
    powers of |r| (2^+-960 here, inside double); the products of two of them that earlier versions formed are not."""
    S, _, levels = system(which)
    assert len(levels) >= 3
    r = np.random.Generator(np.random.PCG64(9)).normal(size=S.shape[0])
    trace = {}
    z = kcycle_ref(levels, r, trace)
    assert np.isfinite(z).all() and all(rec[3] is None for recs in trace.values() for rec in recs)
    for e in (300, -300, 400, -400, 480, -480):
        trace = {}
        ze = kcycle_ref(levels, np.ldexp(r, e), trace)
        assert np.isfinite(ze).all(), (which, e)
        assert all(rec[3] is None for recs in trace.values() for rec in recs), (which, e)
        assert np.array_equal(ze, np.ldexp(z, e)), (which, e, np.abs(np.ldexp(ze, -e) - z).max())


MEASURED = {"p2_rbm": (59, 52), "heat": (16, 16), "nonsym": (136, 123), "aniso": (18, 18)}


@pytest.mark.parametrize("which", sorted(MEASURED))
def test_fgmres_with_the_k_cycle_against_gmres_with_the_v_cycle(which):
    """Iterations of GMRES(30) + V and of FGMRES(30) + K to rtol 1e-8 and the level visits of one apply, printed; the table of the
    module docstring and of DESIGN 9.5. Asserted: both converge to the tolerance, the counts are the recorded ones +- 2 (they are
    integers that depend on rounding near the tolerance), and K does not need more iterations than V (measured first: it needs fewer
    on all four)."""
    S, b, levels = system(which)
    assert len(levels) >= 3
    with callable_preconditioners():
        xv, its_v, conv_v, _ = gmres_ref(S, b, inv=lambda r: vcycle_any_ref(levels, r), m=30, rtol=1e-8, maxiter=2000)
    xk, its_k, conv_k, res_k, _, _, calls = fgmres_with_kcycle(S, b, levels, m=30, rtol=1e-8, maxiter=2000)
    nv, nk = len(levels), k_visits(len(levels))
    print(f"{which}: rows {[L.n_rows for L in levels]}; GMRES(30) + V {its_v} its x {nv} visits = {its_v * nv}; "
          f"FGMRES(30) + K {its_k} its x {nk} visits = {its_k * nk}")
    assert conv_v and conv_k and calls == its_k
    for x in (xv, xk):
        assert np.linalg.norm(b - S @ x) <= 1e-8 * np.linalg.norm(b) * (1 + 1e-6)
    assert abs(its_v - MEASURED[which][0]) <= 2 and abs(its_k - MEASURED[which][1]) <= 2, (which, its_v, its_k)
    assert its_k <= its_v
