"""Adjoint solves on the device: A x = b and A^T lambda = g on the non-symmetric systems of tests/solver_cases.py, the transposed
solve on the transposed matrix, on the callable transposed product and behind a multigrid re-setup after an in-place transpose.

The check is the duality g.x - lambda.b = r_lambda.x - lambda.r_x, exact for r_x = b - A x and r_lambda = g - A^T lambda. So
|g.x - lambda.b| <= |r_lambda| |x| + |lambda| |r_x| + 1e-13 sum |g_i x_i| with the residuals formed on the host in float64 from
to_scipy(): a derived bound (the last term covers the rounding of the two dot products), not a tuned one. The identity holds for any
pair (x, lambda), so the bound is small only if the host residual of the adjoint equation is: that is asserted too, against the
solver's tolerance plus the rounding of the host product (1e-13 | |A|^T |lambda| |, rows of at most 81 entries at 1.1e-16 each)."""
import numpy as np
import pytest

from solver_cases import _assembled_system, _cuda, _torch, meshes  # noqa: F401 (meshes: a fixture)

pytestmark = pytest.mark.gpu


RTOL = 1e-12


def _duality_gap_and_bound(S, St, x, lam, b, g):
    """St: the operator of the adjoint equation (S.T; S itself to show what a missing transpose does)."""
    r_x, r_l = b - S @ x, g - St @ lam
    assert np.linalg.norm(r_l) <= RTOL * np.linalg.norm(g) + 1e-13 * np.linalg.norm(abs(St) @ np.abs(lam))
    gap = abs(g @ x - lam @ b)
    bound = np.linalg.norm(r_l) * np.linalg.norm(x) + np.linalg.norm(lam) * np.linalg.norm(r_x) + 1e-13 * np.abs(g * x).sum()
    return gap, bound


@pytest.mark.parametrize("which", ["heat", "hex_eps"])
def test_adjoint_solves_satisfy_the_duality(ctx, meshes, which):
    from dolfinx_external_operator_amd.krylov import gmres

    torch = _torch(ctx)
    A, bs, bcs = _assembled_system(ctx, meshes, which)
    S = A.to_scipy()
    n = S.shape[0]
    assert abs(S - S.T).max() >= 1e-3 * abs(S).max()
    rng = np.random.Generator(np.random.PCG64(23))
    b, g = rng.normal(size=n), rng.normal(size=n)
    bd, gd = _cuda(b), _cuda(g)
    kw = dict(restart=30, rtol=RTOL, maxiter=2000)

    fwd = gmres(A, bd, M=A.block_jacobi(), **kw)
    assert fwd.converged
    x = fwd.x.cpu().numpy()

    T = A.transpose()
    MT = T.block_jacobi()
    solves = {"transposed matrix": gmres(T, gd, M=MT, **kw),
              "callable": gmres(lambda v, out: A.matvec(v, out, transpose=True), gd, M=MT, ctx=ctx, **kw)}
    # without the transpose the assertion fails: A mu = g in the place of A^T lambda = g
    wrong = gmres(A, gd, M=A.block_jacobi(), **kw)
    assert wrong.converged
    if which == "heat":      # the hierarchy's symbolic phase reused: transpose in place, setup() again
        amg = A.amg(bcs, coarse_rows=10)
        assert A.transpose(out=A.values) is A
        amg.setup()
        solves["amg after an in-place transpose"] = gmres(A, gd, M=amg, **kw)
        torch.cuda.synchronize()
        assert torch.equal(A.values, T.values)
    for name, res in solves.items():
        assert res.converged, name
        gap, bound = _duality_gap_and_bound(S, S.T, x, res.x.cpu().numpy(), b, g)
        print(f"{which}, {name}: |g.x - lambda.b| = {gap:.3e}, bound {bound:.3e}, {res.iterations} iterations")
        assert gap <= bound, (name, gap, bound)
    # the roles reversed: mu solves A mu = g to the same tolerance, and the duality does not hold for it
    gap, bound = _duality_gap_and_bound(S, S, x, wrong.x.cpu().numpy(), b, g)
    print(f"{which}, no transpose: |g.x - mu.b| = {gap:.3e}, bound {bound:.3e}")
    assert gap > bound
