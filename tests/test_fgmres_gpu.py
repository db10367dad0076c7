"""dxo_krylov_fgmres, the callback preconditioner DXO_PC_CALLBACK and the multigrid on a callable operator, against closed forms in
the manner of test_krylov_known_answers_gpu.py: the cyclic shift of period d makes no progress for d - 1 steps and terminates at
step d with x = P^T b, with M = None and with a preconditioner that changes at every call, M_j(r) = (j + 1) r (the Krylov
directions only change their lengths, so flexible GMRES still terminates at step d; M is called d times, never at the update).
With a fixed preconditioner fgmres takes the iterations of gmres. Tolerances: those of the known-answer tests (F1_X_TOL,
F1_RES_TOL: 100 x the float64 oracle's own deviation from the closed form)."""
import numpy as np
import pytest

from oracle.krylov_oracle import U, cycle_rhs, cyclic_shift_src, precond_diagonal, shift_solution
from solver_cases import F1_RES_TOL, F1_X_TOL, _assembled_system, _cuda, _shift, _torch, meshes  # noqa: F401  (meshes is a fixture)

pytestmark = pytest.mark.gpu

SHIFT_D = (1, 2, 5, 33, 64)
# (q, t), n = t + d q: one cycle (n = d: 1, 2, 5 < 32) and 257 rows (more than one workgroup, a ragged tail)
SIZES = {1: ((1, 0), (257, 0)), 2: ((1, 0), (128, 1)), 5: ((1, 0), (51, 2)), 33: ((1, 0), (7, 26)), 64: ((1, 0), (4, 1))}


def _cases(d):
    for q, t in SIZES[d]:
        src, b = cyclic_shift_src(d, q, t), cycle_rhs(d, q, t, seed=d)
        assert b.size in (d, 257)
        yield src, b, shift_solution(src, b)


@pytest.mark.parametrize("d", SHIFT_D)
def test_cyclic_shift_terminates_at_step_d(ctx, d):
    from dolfinx_external_operator_amd import fgmres

    torch = _torch(ctx)
    for src, b, xs in _cases(d):
        P, bd = _shift(torch, src), _cuda(b)
        for ce in (1, 8):
            out = fgmres(P, bd, restart=64, rtol=1e-10, check_every=ce, ctx=ctx)
            what = (d, b.size, ce, out)
            assert out.iterations == d and out.converged and out.restarts == 1, what
            dx = float(np.abs(out.x.cpu().numpy() - xs).max() / np.abs(b).max())
            print(f"d = {d}, n = {b.size}, check_every {ce}: x {dx:.2e} max|b|, residual {out.residual:.2e}")
            assert dx <= F1_X_TOL and out.residual <= F1_RES_TOL, what
            if d > 1:                                         # no progress for d - 1 steps
                out = fgmres(P, bd, restart=64, rtol=1e-10, maxiter=d - 1, check_every=ce, ctx=ctx)
                assert (out.iterations, out.restarts, out.converged, out.breakdown) == (d - 1, 1, False, False), what
                assert abs(out.residual - 1.0) <= 4 * U and not out.x.any(), what


@pytest.mark.parametrize("d", SHIFT_D)
def test_a_preconditioner_that_changes_at_every_call(ctx, d):
    from dolfinx_external_operator_amd import fgmres

    torch = _torch(ctx)
    for src, b, xs in _cases(d):
        P, bd = _shift(torch, src), _cuda(b)
        for ce in (1, 8):
            calls = []

            def M(r, out):
                calls.append(1)
                torch.mul(r, float(len(calls)), out=out)      # M_j = (j + 1) I, j the calls before this one

            out = fgmres(P, bd, M=M, restart=64, rtol=1e-10, check_every=ce, ctx=ctx)
            what = (d, b.size, ce, len(calls), out)
            # steps run past the converged one before the host looks (check_every 8) call M too; none is called at the update
            ran = d if ce == 1 else min(-(-d // 8) * 8, 64)
            assert out.iterations == d and out.converged and out.restarts == 1 and len(calls) == ran, what
            dx = float(np.abs(out.x.cpu().numpy() - xs).max() / np.abs(b).max())
            print(f"varying M, d = {d}, n = {b.size}, check_every {ce}: x {dx:.2e} max|b|, residual {out.residual:.2e}, calls {len(calls)}")
            assert dx <= F1_X_TOL and out.residual <= F1_RES_TOL, what


def test_fixed_preconditioners_take_the_iterations_of_gmres(ctx, meshes):  # noqa: F811
    from dolfinx_external_operator_amd import fgmres, gmres

    torch = _torch(ctx)
    A, bs, bcs = _assembled_system(ctx, meshes, "heat")
    S = A.to_scipy()
    b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
    bd = _cuda(b)
    for name, M in (("block Jacobi", A.block_jacobi()), ("AMG V", A.amg(bcs, coarse_rows=40))):
        for ce in (1, 8):
            f = fgmres(A, bd, M=M, restart=30, rtol=1e-10, check_every=ce)
            g = gmres(A, bd, M=M, restart=30, rtol=1e-10, check_every=ce)
            print(f"{name}, check_every {ce}: fgmres {f.iterations} iterations (residual {f.residual:.2e}), gmres {g.iterations} ({g.residual:.2e})")
            assert f.converged and g.converged and f.iterations == g.iterations and f.restarts == g.restarts, (name, f, g)
            for out in (f, g):
                assert np.linalg.norm(b - S @ out.x.cpu().numpy()) <= 1e-10 * np.linalg.norm(b) * (1 + 1e-6), (name, out)
        # two solves are bit-identical
        assert torch.equal(fgmres(A, bd, M=M, restart=30).x, fgmres(A, bd, M=M, restart=30).x)
    # restart = 1: the second basis has one row
    M = A.block_jacobi()
    f, g = fgmres(A, bd, M=M, restart=1, maxiter=40), gmres(A, bd, M=M, restart=1, maxiter=40)
    assert (f.iterations, f.restarts, f.converged) == (g.iterations, g.restarts, g.converged) == (40, 40, False), (f, g)
    assert abs(f.residual - g.residual) <= 1e-12 and f.residual < 1.0


def test_multigrid_on_a_callable_operator(ctx, meshes):  # noqa: F811
    """The matrix-free action preconditioned by the multigrid of the assembled matrix: the same kernels in the same order, so the
    count of the DeviceCSR call (and here its bits)."""
    from dolfinx_external_operator_amd import cg, fgmres, gmres

    torch = _torch(ctx)
    A, bs, bcs = _assembled_system(ctx, meshes, "spd_quad")
    amg = A.amg(bcs, coarse_rows=40)
    bd = _cuda(np.random.Generator(np.random.PCG64(2)).normal(size=A.shape[0]))

    def op(v, out):
        A.matvec(v, out)

    for solve in (fgmres, gmres, cg):
        direct = solve(A, bd, M=amg, rtol=1e-10)
        free = solve(op, bd, M=amg, rtol=1e-10, ctx=ctx)
        assert direct.converged and free.converged and free.iterations == direct.iterations, (solve.__name__, direct, free)
        assert torch.equal(free.x, direct.x)
    with pytest.raises(ValueError, match="multigrid preconditioner covers"):
        fgmres(op, bd[:-2].contiguous(), M=amg, ctx=ctx)                      # the sizes are still checked


def test_a_callable_preconditioner_in_cg_and_gmres(ctx):
    from dolfinx_external_operator_amd import cg, gmres

    torch = _torch(ctx)
    for n in (1, 19, 257):
        dg = precond_diagonal(n)
        dgd, inv = _cuda(dg), _cuda(1.0 / dg)
        bd = _cuda(np.ones(n))

        def A(v, o):
            torch.mul(v, dgd, out=o)

        def M(r, o):
            torch.mul(r, inv, out=o)

        for solve in (cg, gmres):
            tensor = solve(A, bd, M=inv, ctx=ctx)
            out = solve(A, bd, M=M, ctx=ctx)
            assert (out.iterations, out.restarts, out.converged) == (tensor.iterations, tensor.restarts, tensor.converged) == (1, 1, True), (n, out)
            assert np.abs(out.x.cpu().numpy() * dg - 1.0).max() <= 32 * U, (n, solve.__name__)      # a dozen roundings and the norm of b


def test_an_exception_in_the_preconditioner_is_raised_again(ctx):
    from dolfinx_external_operator_amd import cg, fgmres, gmres

    torch = _torch(ctx)
    bd = _cuda(np.ones(50))

    def A(v, o):
        torch.mul(v, 2.0, out=o)

    def M(r, o):
        raise KeyError("from the preconditioner")

    for solve in (fgmres, gmres, cg):
        with pytest.raises(KeyError, match="from the preconditioner"):
            solve(A, bd, M=M, ctx=ctx)
        assert solve(A, bd, ctx=ctx).converged                               # and the context is usable afterwards
    with pytest.raises(TypeError, match="M must be"):
        fgmres(A, bd, M="jacobi", ctx=ctx)


def test_c_abi_of_the_callback_kind(ctx, hip_library):
    import ctypes as C

    from dolfinx_external_operator_amd._lib import KRYLOV_APPLY_FN, KrylovCallback, KrylovInfo, KrylovOp, KrylovPc, _CudaArrayView

    torch = _torch(ctx)
    lib, h, n = hip_library, ctx._h, 64
    b, x = _cuda(np.ones(n)), _cuda(np.zeros(n))

    def view(ptr):
        return torch.as_tensor(_CudaArrayView(ctx, ptr, n, "<f8"), device="cuda")

    @KRYLOV_APPLY_FN
    def identity(_user, v, out):
        view(out).copy_(view(v))
        return 0

    @KRYLOV_APPLY_FN
    def failing(_user, v, out):
        return 7

    def pc(kind, rows, cb):
        return C.byref(KrylovPc(kind, 1, rows, None if cb is None else C.cast(C.pointer(cb), C.c_void_p)))

    ws = C.c_void_p()
    assert lib.dxo_krylov_create(h, n, 8, C.byref(ws)) == 0
    try:
        info = KrylovInfo()
        op = KrylovOp(n, None, None, identity, None)
        args = (C.c_void_p(b.data_ptr()), C.c_void_p(x.data_ptr()), 1e-8, 0.0, 10, 1, C.byref(info))
        empty, bad, good = KrylovCallback(KRYLOV_APPLY_FN(), None), KrylovCallback(failing, None), KrylovCallback(identity, None)
        for fn in (lib.dxo_krylov_fgmres, lib.dxo_krylov_gmres, lib.dxo_krylov_cg):
            x.fill_(0.5)
            assert fn(h, ws, C.byref(op), pc(4, n, None), *args) == -1                 # DXO_E_NULL: no struct
            assert fn(h, ws, C.byref(op), pc(4, n, empty), *args) == -1                # DXO_E_NULL: no function
            assert fn(h, ws, C.byref(op), pc(4, n + 1, good), *args) == -3             # DXO_E_SIZE
            assert fn(h, ws, C.byref(op), pc(5, n, good), *args) == -6                 # DXO_E_OPTION: an unknown kind
            assert fn(h, ws, C.byref(op), pc(4, n, bad), *args) == -6                  # a positive return of the callback: DXO_E_OPTION
            assert b"preconditioner callback returned 7" in (lib.dxo_last_error(h) or b"")
            assert fn(h, ws, C.byref(op), pc(4, n, good), *args) == 0 and info.converged == 1 and info.iterations == 1
            assert torch.equal(x, b)
        assert lib.dxo_krylov_fgmres(None, ws, C.byref(op), None, *args) == -1
    finally:
        lib.dxo_krylov_destroy(h, ws)


def _drop_workspace(ctx, n, restart):
    ws = ctx.__dict__.get("_krylov_ws", {}).pop((n, restart), None)
    if ws is not None:
        ws.close()


def test_one_workspace_serves_gmres_and_fgmres_in_either_order(ctx, meshes):  # noqa: F811
    """The second basis comes with the first flexible solve on a workspace: before or after a gmres on it, the results are those of
    a workspace of their own, bit for bit."""
    from dolfinx_external_operator_amd import fgmres, gmres

    torch = _torch(ctx)
    A, bs, bcs = _assembled_system(ctx, meshes, "heat")
    n, restart = A.shape[0], 17
    M = A.block_jacobi()
    bd = _cuda(np.random.Generator(np.random.PCG64(4)).normal(size=n))
    _drop_workspace(ctx, n, restart)
    g_first = gmres(A, bd, M=M, restart=restart).x.clone()
    f_second = fgmres(A, bd, M=M, restart=restart).x.clone()
    g_third = gmres(A, bd, M=M, restart=restart).x.clone()
    _drop_workspace(ctx, n, restart)
    f_first = fgmres(A, bd, M=M, restart=restart).x.clone()
    g_second = gmres(A, bd, M=M, restart=restart).x.clone()
    assert torch.equal(g_first, g_second) and torch.equal(g_first, g_third) and torch.equal(f_first, f_second)
    assert len([k for k in ctx.__dict__["_krylov_ws"] if k == (n, restart)]) == 1
