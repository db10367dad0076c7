"""The NumPy yardstick of dxo_krylov_gmres / dxo_krylov_cg / dxo_csr_block_jacobi (oracle/krylov_oracle.py), pinned on the CPU.

gmres_ref and block_jacobi_ref are checked against scipy.sparse.linalg.spsolve / numpy.linalg.inv on the assembled matrices the
device makes: the heat Jacobian of the heat demo (non-symmetric, bs = 1), an (eps, eps) matrix with a random non-symmetric C (bs = 2)
and an SPD elastic matrix (CG), each with Dirichlet rows; and on the known-answer families, operators whose GMRES / CG history is
known in closed form (tests/test_krylov_known_answers_gpu.py runs the same families on the device)."""
import numpy as np
import pytest
import scipy.sparse.linalg

from oracle.krylov_oracle import (F2_C, F2_D, F2_MAIN, F2_S, F2_SIZES, MARGIN, REF_F1_RES, REF_F1_X, REF_F2_RES, REF_F2_X, SHIFT_D, U,
                                  FnOperator, alternating_diag, block_jacobi_ref, bottom_dofs, boundary_dofs, cg_ref, cycle_rhs,
                                  cyclic_shift_src, eps_matrix, exact_breakdown_rhs, f2_problem, gmres_ref, heat_matrix, late_zero_op,
                                  nilpotent_op, precond_diagonal, repeated_diag, shift_op, shift_solution, shifted_atol, shifted_op,
                                  shifted_residual, to_pattern_csr, xdev)


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


def test_reference_deviation_of_the_shifted_shift():
    """The oracle against the closed form (residual) and against itself in long double (x_k): what REF_F2_* bound."""
    worst_r = worst_x = 0.0
    L = np.longdouble

    def check(q, t, k, m=64, reorth=True, precond=False, closed=True, referee=True):
        nonlocal worst_r, worst_x
        D = precond_diagonal(t + F2_D * q) if precond else None
        src, b, A = f2_problem(q, t, D)
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
    src, b, A = f2_problem(*F2_MAIN)
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
