"""dxo_krylov_gmres / dxo_krylov_cg against operators whose history is known in closed form, step by step, at every restart length
and at the sizes where the row kernels change shape. The operators are callbacks (one torch indexing call); the families, their
closed forms and the reference's own deviation (REF_*) are pinned on the CPU in tests/test_krylov_oracle_cpu.py.

F1: a cyclic shift of period d makes no progress for d - 1 steps and terminates at step d. F2: c I + s P has a bidiagonal
Hessenberg matrix and the residual 1 / sqrt(sum_{i <= k} (c/s)^(2i)) after k steps. F3: breakdowns and exact termination.
Counts and flags are exact; iterates and residuals are held to MARGIN = 100 x the float64 oracle's own deviation from the
long-double answers. F1 leaves `breakdown` unasserted at termination: there hn is rounding noise of w - v0 (v0, w), zero or not
by the order of the sums. Nothing else of the families is left out."""
import numpy as np
import pytest

from oracle.krylov_oracle import (F2_D, F2_MAIN, MARGIN, SHIFT_D, U, FnOperator, alternating_diag, block_jacobi_ref, cg_ref, cycle_rhs,
                                  cyclic_shift_src, exact_breakdown_rhs, gmres_ref, late_zero_op, nilpotent_op, repeated_diag,
                                  shift_solution, shifted_atol, shifted_op, shifted_residual, xdev)
from solver_cases import (F1_RES_TOL, F1_X_TOL, F2_RES_TOL, F2_X_TOL, _cuda, _f2, _grid_cap, _krylov_system, _reorth, _shift, _torch,
                          meshes)  # noqa: F401  (meshes: the fixture of the CSR cross-check)

pytestmark = pytest.mark.gpu


# ---- F1
def _f1_sizes(d, cap):
    """(q, t): n = 1 or d (one cycle), 31 d, and per d one of the edges: 255 / 256 / 257 rows, more than 256 partials, one trip
    of the grid and more than two trips with a ragged tail."""
    sizes = [(1, 0), (31, 0)]
    if d == 17:
        sizes += [(15, 0), (15, 1), (15, 2)]
    if d == 33:
        sizes += [(2122, 0)]
    if d == 64:
        sizes += [(cap // d + 1, 5), (2 * cap // d + 1, 13)]
    return sizes


@pytest.mark.parametrize("d", SHIFT_D)
def test_cyclic_shift_terminates_at_step_d(ctx, d):
    from dolfinx_external_operator_amd import gmres

    torch = _torch(ctx)
    cap = _grid_cap(torch)
    worst_x = worst_r = 0.0
    ns = []
    for q, t in _f1_sizes(d, cap):
        src, b = cyclic_shift_src(d, q, t), cycle_rhs(d, q, t, seed=d)
        ns.append(b.size)
        P, bd, xs = _shift(torch, src), _cuda(b), shift_solution(src, b)
        for restart in sorted({64, d}):
            for reorth in (1, 0):
                with _reorth(ctx, reorth):
                    out = gmres(P, bd, restart=restart, rtol=1e-10, ctx=ctx)
                what = (d, b.size, restart, reorth, out)
                assert out.iterations == d and out.converged and out.restarts == 1, what
                dx = float(np.abs(out.x.cpu().numpy() - xs).max() / np.abs(b).max())
                worst_x, worst_r = max(worst_x, dx), max(worst_r, out.residual)
                assert dx <= F1_X_TOL and out.residual <= F1_RES_TOL, what
        # the solution as the initial guess: nothing runs, x is not written
        x0 = _cuda(xs)
        out = gmres(P, bd, x=x0, restart=64, ctx=ctx)
        assert (out.iterations, out.restarts, out.converged, out.breakdown) == (0, 0, True, False) and out.x is x0
        assert np.array_equal(x0.cpu().numpy(), xs), (d, b.size)
        if d == 1:
            continue                                          # no restart length 0: dxo_krylov_create refuses it
        # restart = d - 1: every cycle ends one step short, g = (0, ..., 0, +-beta), y = 0
        out = gmres(P, bd, restart=d - 1, rtol=1e-10, maxiter=3 * (d - 1), ctx=ctx)
        what = (d, b.size, out)
        assert (out.iterations, out.restarts, out.converged, out.breakdown) == (3 * (d - 1), 3, False, False), what
        assert abs(out.residual - 1.0) <= 4 * U and not out.x.any(), what
        # and within one long cycle the residual is still 1 after d - 1 steps
        out = gmres(P, bd, restart=64, rtol=1e-10, maxiter=d - 1, ctx=ctx)
        assert (out.iterations, out.restarts, out.converged, out.breakdown) == (d - 1, 1, False, False), what
        assert abs(out.residual - 1.0) <= 4 * U and not out.x.any(), what
    if d == 64:
        assert ns[-2] > cap and ns[-1] > 2 * cap and ns[-1] % 256 != 0, (ns, cap)     # the second and third trip of the grid-stride loops
    if d == 33:
        assert -(-ns[-1] // 256) > 256                        # kr_reduce adds more partials than it has threads
    print(f"F1 d = {d}, n = {ns}: x {worst_x:.2e} max|b|, residual {worst_r:.2e}")


# ---- F2
def _f2_step(gmres, ctx, dev, src, b, D, k, restart=64, closed=True, worst=None):
    """k steps on the device against the oracle's k steps (x_k) and the closed form (residual)."""
    torch = _torch(ctx)
    inv = None if D is None else 1.0 / D
    out = gmres(dev, _cuda(b), M=None if D is None else _cuda(inv), restart=restart, rtol=0.0, maxiter=k, ctx=ctx)
    x, its, conv, res, brk, cycles = gmres_ref(shifted_op(src, D=D), b, inv=inv, m=restart, rtol=0.0, maxiter=k, full=True)
    what = (b.size, k, restart, D is not None, out)
    assert (out.iterations, out.restarts, out.converged, out.breakdown) == (k, -(-k // restart), False, False) == (its, cycles, conv, brk), what
    f = float(shifted_residual(k)) if closed else res
    dr, dx = abs(out.residual - f) / f, xdev(out.x.cpu().numpy(), x)
    if worst is not None:
        worst[0], worst[1] = max(worst[0], dr), max(worst[1], dx)
    assert dr <= F2_RES_TOL and dx <= F2_X_TOL, (what, dr, dx)
    return out


def test_shifted_shift_residual_and_iterate_at_every_step(ctx):
    from dolfinx_external_operator_amd import gmres

    torch = _torch(ctx)
    src, b, D, dev = _f2(torch, *F2_MAIN)
    worst = [0.0, 0.0]
    for k in range(1, 65):
        _f2_step(gmres, ctx, dev, src, b, D, k, worst=worst)
    print(f"F2 n = {b.size}, k = 1..64: residual {worst[0]:.2e} relative, x_k {worst[1]:.2e} max|x|")
    worst = [0.0, 0.0]
    with _reorth(ctx, 0):                                     # the basis is orthogonal by construction: one pass, the same history
        for k in (1, 2, 5, 17, 33, 64):
            _f2_step(gmres, ctx, dev, src, b, D, k, worst=worst)
    print(f"F2 one Gram-Schmidt pass: residual {worst[0]:.2e} relative, x_k {worst[1]:.2e} max|x|")


def test_shifted_shift_at_the_sizes_where_the_row_kernels_change_shape(ctx):
    from dolfinx_external_operator_amd import gmres

    torch = _torch(ctx)
    cap = _grid_cap(torch)
    sizes = [(1, 0), (31, 0), (3, 15), (3, 16), (3, 17), (875, 3), (cap // F2_D + 1, 7), (2 * cap // F2_D + 1, 13)]
    ns = [t + F2_D * q for q, t in sizes]
    assert ns[:6] == [80, 2480, 255, 256, 257, 70003] and -(-ns[5] // 256) > 256
    assert ns[6] > cap and ns[7] > 2 * cap and ns[7] % 256 != 0, (ns, cap)
    for q, t in sizes:
        src, b, D, dev = _f2(torch, q, t)
        worst = [0.0, 0.0]
        for k in (1, 33, 64):
            _f2_step(gmres, ctx, dev, src, b, D, k, worst=worst)
        print(f"F2 n = {b.size}: residual {worst[0]:.2e} relative, x_k {worst[1]:.2e} max|x|")


def test_shifted_shift_right_preconditioned_by_an_inverse_diagonal(ctx):
    """(c I + s P) D with M = 1 / D: the history of c I + s P, and x_k = D^-1 (its x_k)."""
    from dolfinx_external_operator_amd import gmres

    torch = _torch(ctx)
    src, b, D, dev = _f2(torch, *F2_MAIN, precond=True)
    worst = [0.0, 0.0]
    for k in (1, 2, 5, 17, 33, 64):
        out = _f2_step(gmres, ctx, dev, src, b, D, k, worst=worst)
        plain, *_ = gmres_ref(shifted_op(src), b, m=64, rtol=0.0, maxiter=k)
        assert xdev(out.x.cpu().numpy(), plain / D) <= F2_X_TOL, k
    print(f"F2 preconditioned: residual {worst[0]:.2e} relative, x_k {worst[1]:.2e} max|x|")


@pytest.mark.parametrize("restart", [1, 2, 3, 7])
def test_shifted_shift_short_restarts_follow_the_oracle(ctx, restart):
    from dolfinx_external_operator_amd import gmres

    torch = _torch(ctx)
    src, b, D, dev = _f2(torch, *F2_MAIN)
    worst = [0.0, 0.0]
    for maxiter in (20, 21):                                  # the last cycle full and cut short
        _f2_step(gmres, ctx, dev, src, b, D, maxiter, restart=restart, closed=False, worst=worst)
    print(f"F2 restart = {restart}: residual {worst[0]:.2e} relative, x {worst[1]:.2e} max|x|")


def test_shifted_shift_stops_on_atol_at_step_k_for_every_check_every(ctx):
    from dolfinx_external_operator_amd import gmres

    torch = _torch(ctx)
    src, b, D, dev = _f2(torch, *F2_MAIN)
    bd, bnorm = _cuda(b), np.linalg.norm(b)
    for k in (1, 2, 5, 17, 33, 64):
        atol, f = shifted_atol(k, bnorm), float(shifted_residual(k))
        runs = [gmres(dev, bd, restart=64, rtol=0.0, atol=atol, check_every=ce, ctx=ctx) for ce in (1, 8, 64)]
        for out in runs:
            assert (out.iterations, out.restarts, out.converged, out.breakdown) == (k, 1, True, False), (k, out)
            assert abs(out.residual - f) <= F2_RES_TOL * f, (k, out)
            assert torch.allclose(out.x, runs[0].x, rtol=0, atol=1e-14 * float(runs[0].x.abs().max())), k


# ---- F3
def test_gmres_happy_breakdown_on_the_identity(ctx):
    from dolfinx_external_operator_amd import gmres

    torch = _torch(ctx)

    def identity(v, out):
        out.copy_(v)

    for ce in (1, 8):
        out = gmres(identity, _cuda(np.array([-4.0])), restart=64, check_every=ce, ctx=ctx)       # exact arithmetic
        assert (out.iterations, out.restarts, out.converged, out.breakdown) == (1, 1, True, True) and out.x.item() == -4.0, out
        for n in (4, 16, 64, 256, 1024, 4096, 65536):         # hn == 0 exactly (checked on the oracle)
            b = exact_breakdown_rhs(n)
            out = gmres(identity, _cuda(b), restart=64, check_every=ce, ctx=ctx)
            assert (out.iterations, out.restarts, out.converged, out.breakdown) == (1, 1, True, True), (n, out)
            assert np.array_equal(out.x.cpu().numpy(), b) and out.residual == 0.0, n
        for n in (2, 3, 31, 257, 1000, 70001):                # any b: hn is zero or rounding noise
            b = cycle_rhs(1, n, 0, seed=n)
            out = gmres(identity, _cuda(b), restart=64, check_every=ce, ctx=ctx)
            assert (out.iterations, out.restarts, out.converged) == (1, 1, True), (n, out)
            assert np.abs(out.x.cpu().numpy() - b).max() <= 4 * U * np.abs(b).max(), n


def test_gmres_on_a_singular_operator_reports_the_breakdown(ctx):
    from dolfinx_external_operator_amd import gmres

    torch = _torch(ctx)

    def nilpotent(v, out):
        out[1:].copy_(v[:-1])
        out[:1].zero_()

    for n in (2, 33, 300, 70001):
        b = np.zeros(n)
        b[-1] = 3.0
        ref = gmres_ref(nilpotent_op(n), b, m=64, full=True)
        assert ref[1:] == (1, False, 1.0, True, 1)
        for x0 in (None, 7.0 * b):                            # A x0 = 0 as well
            for ce in (1, 8):
                x = None if x0 is None else _cuda(x0)
                out = gmres(nilpotent, _cuda(b), x=x, restart=64, check_every=ce, ctx=ctx)
                assert (out.iterations, out.restarts, out.converged, out.breakdown) == (1, 1, False, True), (n, out)
                assert abs(out.residual - 1.0) <= 4 * U
                assert np.array_equal(out.x.cpu().numpy(), np.zeros(n) if x0 is None else x0), n


def test_a_zero_vector_after_the_converged_step_is_no_breakdown(ctx):
    """The first step meets rtol = 0.1 with hn = 2^-10 > 0, in exact arithmetic; A v1 = 0, so a step run past it (check_every > 1)
    finds hn == 0. That step is not part of the solve: no breakdown, as with check_every = 1 and on the oracle."""
    from dolfinx_external_operator_amd import gmres

    torch = _torch(ctx)
    eps = 2.0 ** -10

    def late_zero(v, out):
        out.zero_()
        out[:1].copy_(v[:1])
        out[1:2].copy_(v[:1] * eps)

    b = np.array([-4.0, 0.0, 0.0])
    x, its, conv, res, brk, cycles = gmres_ref(late_zero_op(eps), b, m=64, rtol=0.1, full=True)
    assert (its, conv, brk, cycles) == (1, True, False, 1)
    for ce in (1, 8):
        out = gmres(late_zero, _cuda(b), restart=64, rtol=0.1, check_every=ce, ctx=ctx)
        assert (out.iterations, out.restarts, out.converged, out.breakdown) == (1, 1, True, False), (ce, out)
        assert abs(out.residual - res) <= 16 * U * res and np.abs(out.x.cpu().numpy() - x).max() <= 16 * U * 4.0


def test_cg_breaks_down_on_an_indefinite_diagonal(ctx):
    from dolfinx_external_operator_amd import cg

    torch = _torch(ctx)
    for n in (2, 64, 1000, 70000):
        dg = _cuda(alternating_diag(n))
        for ce in (1, 8):
            out = cg(lambda v, o: torch.mul(v, dg, out=o), _cuda(np.ones(n)), check_every=ce, ctx=ctx)       # (p, q) = 0 at the first step
            assert (out.iterations, out.restarts, out.converged, out.breakdown) == (0, 1, False, True), (n, out)
            assert abs(out.residual - 1.0) <= 4 * U and not out.x.any()


@pytest.mark.parametrize("d", range(1, 9))
def test_cg_terminates_after_as_many_steps_as_eigenvalues(ctx, d):
    from dolfinx_external_operator_amd import cg

    torch = _torch(ctx)
    for n in (37 * d + 3, 70003):
        dg = repeated_diag(d, n)
        dgd, inv = _cuda(dg), _cuda(1.0 / dg)

        def A(v, o):
            torch.mul(v, dgd, out=o)

        _, its, conv, _, brk, _ = cg_ref(FnOperator(lambda v: dg * v), np.ones(n), full=True)
        assert (its, conv, brk) == (d, True, False)
        for ce in (1, 8):
            out = cg(A, _cuda(np.ones(n)), check_every=ce, ctx=ctx)
            assert (out.iterations, out.restarts, out.converged, out.breakdown) == (d, 1, True, False), (d, n, out)
            assert np.abs(out.x.cpu().numpy() - 1.0 / dg).max() <= 1e-10
            out = cg(A, _cuda(np.ones(n)), M=inv, check_every=ce, ctx=ctx)
            assert (out.iterations, out.restarts, out.converged, out.breakdown) == (1, 1, True, False), (d, n, out)


# ---- the callback path tied to the matrix path
def test_csr_gmres_follows_the_oracle_step_by_step(ctx, meshes):  # noqa: F811
    """k steps of GMRES(64) on an assembled matrix with its block Jacobi: counts exact, residual and x_k within MARGIN x the
    deviation of the float64 oracle from its own long-double run on this matrix (measured here, on the host). The residual
    |b - A x_k| / |b| is compared absolutely: by k = 64 it is so small on this matrix that its rounding, of size u (|b| + |A| |x|) / |b|
    on either side, is 1e-4 of it."""
    from dolfinx_external_operator_amd import gmres

    A, bs = _krylov_system(ctx, meshes, "hex_eps")
    S = A.to_scipy()
    b = np.random.Generator(np.random.PCG64(8)).normal(size=S.shape[0])
    inv = block_jacobi_ref(S, bs)
    L = np.longdouble
    dense = S.toarray().astype(L)
    runs, ref_r, ref_x = [], 0.0, 0.0
    for k in (1, 31, 32, 33, 64):
        x, its, conv, res, brk, cycles = gmres_ref(S, b, inv=inv, m=64, rtol=0.0, maxiter=k, full=True)
        xl, _, _, resl = gmres_ref(dense, b, inv=inv.astype(L), m=64, rtol=0.0, maxiter=k, dtype=L)
        assert (its, conv, brk, cycles) == (k, False, False, 1) and xl.dtype == L
        ref_r, ref_x = max(ref_r, float(abs(res - resl))), max(ref_x, xdev(x, xl.astype(float)))
        runs.append((k, x, res))
    assert MARGIN * max(ref_r, ref_x) <= 1e-11, (ref_r, ref_x)
    M = A.block_jacobi()
    worst_r = worst_x = 0.0
    for k, x, res in runs:
        out = gmres(A, _cuda(b), M=M, restart=64, rtol=0.0, maxiter=k)
        assert (out.iterations, out.restarts, out.converged, out.breakdown) == (k, 1, False, False), (k, out)
        dr, dx = abs(out.residual - res), xdev(out.x.cpu().numpy(), x)
        worst_r, worst_x = max(worst_r, dr), max(worst_x, dx)
        assert dr <= MARGIN * ref_r and dx <= MARGIN * ref_x, (k, dr, dx, ref_r, ref_x)
    print(f"CSR hex_eps n = {b.size}: oracle against long double: residual {ref_r:.2e}, x_k {ref_x:.2e}; device against oracle: "
          f"residual {worst_r:.2e}, x_k {worst_x:.2e}")
