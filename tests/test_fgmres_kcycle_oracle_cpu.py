"""NumPy oracle of flexible GMRES (dxo_krylov_fgmres, fgmres_ref of oracle/krylov_oracle.py) and of the K-cycle (dxo_amg_set_cycle,
cycle_ref of oracle/amg_oracle.py with cycle="K"), and what they promise (not gpu).

fgmres_ref is gmres_ref with the preconditioned vectors z_j = M_j v_j kept: w = A z_j, and x += Z^T y at the end of a cycle with no
further call of M. M is a callable (r, j) -> z, j the number of calls before this one, so a test can make it vary.

The K-cycle walks a hierarchy given as SciPy matrices (the Level list of amg_ref under any of its keywords, or one read
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

from oracle.amg_oracle import U, amg_ref, apply_block, cycle_ref, fgmres_with_cycle, gcr2_ref, k_visits
from oracle.krylov_oracle import block_jacobi_ref, boundary_dofs, fgmres_ref, gmres_ref, heat_matrix, to_pattern_csr
from solver_cases import system


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
            return cycle_ref(levels, r)

        def M(r, j):
            return cycle_ref(levels, r)

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
        assert np.array_equal(cycle_ref(levels, r, "K"), cycle_ref(levels, r))
    one = amg_ref(S, 1, boundary_dofs(m, 1), coarse_rows=400)
    assert len(one) == 1 and np.array_equal(cycle_ref(one, r, "K"), cycle_ref(one, r))


@pytest.mark.parametrize("which", ["heat48", "aniso"])
def test_every_gcr_solve_minimises_the_residual(which):
    """|r - A x| <= |r - (a1 / rho1) A c1| <= |r| on every intermediate level: each GCR step minimises the residual over its
    direction(s). In floating point up to a few u |A| |x| per evaluated residual (8 u (| |A| |x| | + |r|) here)."""
    S, _, levels = system(which)
    assert len(levels) >= 4, [L.n_rows for L in levels]
    visits, trace = [0] * len(levels), {}
    rng = np.random.Generator(np.random.PCG64(5))
    for _ in range(2):
        z = cycle_ref(levels, rng.normal(size=S.shape[0]), "K", trace=trace, visits=visits)
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
    z = cycle_ref(levels, np.zeros(S.shape[0]), "K")
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
    z = cycle_ref(levels, r, "K", trace=trace)
    assert np.isfinite(z).all() and all(rec[3] is None for recs in trace.values() for rec in recs)
    for e in (300, -300, 400, -400, 480, -480):
        trace = {}
        ze = cycle_ref(levels, np.ldexp(r, e), "K", trace=trace)
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
    xv, its_v, conv_v, _ = gmres_ref(S, b, inv=lambda r: cycle_ref(levels, r), m=30, rtol=1e-8, maxiter=2000)
    xk, its_k, conv_k, res_k, _, _, calls = fgmres_with_cycle(S, b, levels, "K", m=30, rtol=1e-8, maxiter=2000)
    nv, nk = len(levels), k_visits(len(levels))
    print(f"{which}: rows {[L.n_rows for L in levels]}; GMRES(30) + V {its_v} its x {nv} visits = {its_v * nv}; "
          f"FGMRES(30) + K {its_k} its x {nk} visits = {its_k * nk}")
    assert conv_v and conv_k and calls == its_k
    for x in (xv, xk):
        assert np.linalg.norm(b - S @ x) <= 1e-8 * np.linalg.norm(b) * (1 + 1e-6)
    assert abs(its_v - MEASURED[which][0]) <= 2 and abs(its_k - MEASURED[which][1]) <= 2, (which, its_v, its_k)
    assert its_k <= its_v
