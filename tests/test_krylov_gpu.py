"""dxo_csr_spmv / dxo_csr_block_jacobi / dxo_krylov_gmres / dxo_krylov_cg on the device, against scipy and the NumPy oracles of
tests/test_krylov_oracle_cpu.py, on the matrices dxo_bilinear_assemble makes."""
import ctypes as C

import numpy as np
import pytest

from oracle.krylov_oracle import block_jacobi_ref, bottom_dofs, cg_ref, elastic_C, elastic_C3, gmres_ref
from solver_cases import CELLS, _assemble, _cuda, _krylov_system, _torch, _value_size, meshes  # noqa: F401  (meshes is a fixture)
from tools.synthetic import structured_mesh

pytestmark = pytest.mark.gpu


# ---- SpMV
@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("degree", [1, 2])
def test_spmv_matches_scipy(ctx, meshes, cell, degree):
    m = structured_mesh(cell, CELLS[cell], degree, distort=0.2, seed=7)
    dm = meshes(m)
    torch = _torch(ctx)
    rng = np.random.Generator(np.random.PCG64(3))
    G = m.gdim
    for test, trial, bs in (("grad", "value_grad", 1), ("grad", "grad", G)):
        Cb = rng.normal(size=(m.num_cells * m.nq, _value_size(test, G, bs), _value_size(trial, G, bs)))
        A = _assemble(ctx, dm, test, trial, bs, Cb)
        S = A.to_scipy()
        n = S.shape[0]
        x, y0 = rng.normal(size=n), rng.normal(size=n)
        scale = np.linalg.norm(abs(S) @ abs(x)) + np.linalg.norm(y0)
        for alpha, beta in ((1.0, 0.0), (2.5, -0.5), (-1.0, 1.0), (0.0, 3.0)):
            y = _cuda(y0)
            A.matvec(_cuda(x), y, alpha, beta)
            ref = alpha * (S @ x) + beta * y0
            assert np.linalg.norm(y.cpu().numpy() - ref) <= 1e-14 * (abs(alpha) + abs(beta)) * scale, (cell, degree, bs, alpha, beta)
        y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")      # beta = 0: y is not read
        A.matvec(_cuda(x), y, 1.5, 0.0)
        first = y.cpu().numpy()
        assert np.isfinite(first).all() and np.linalg.norm(first - 1.5 * (S @ x)) <= 1e-14 * 1.5 * scale
        for _ in range(2):
            assert np.array_equal(A.matvec(_cuda(x), alpha=1.5).cpu().numpy(), first)       # bitwise repeatable
        for lanes in (8, 16, 32, 64):
            ctx.set_option("spmv_lanes", lanes)
            try:
                got = A.matvec(_cuda(x)).cpu().numpy()
            finally:
                ctx.set_option("spmv_lanes", 0)
            assert np.linalg.norm(got - S @ x) <= 1e-14 * scale


# ---- block Jacobi
@pytest.mark.parametrize("cell,n", [("triangle", (6, 5)), ("tetrahedron", (2, 2, 2)), ("quadrilateral", (5, 5))])
def test_block_jacobi_matches_numpy(ctx, meshes, cell, n):
    m = structured_mesh(cell, n, 2, distort=0.15, seed=5)
    dm = meshes(m)
    G = m.gdim
    for bs, Cb, pair in ((G, elastic_C(m, 3) if G == 2 else elastic_C3(m.num_cells * m.nq, 3), ("eps", "eps")),
                         (1, np.random.Generator(np.random.PCG64(2)).normal(size=(m.num_cells * m.nq, G, 1 + G)), ("grad", "value_grad"))):
        bcs = bottom_dofs(m, bs)
        A = _assemble(ctx, dm, *pair, bs, Cb, bcs=bcs)
        got = A.block_jacobi().inv.cpu().numpy().reshape(-1, bs, bs)
        ref = block_jacobi_ref(A.to_scipy(), bs)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
        k, i = divmod(int(bcs[0]), bs)
        assert np.allclose(got[k][i], np.eye(bs)[i]) and np.allclose(got[k][:, i], np.eye(bs)[:, i])   # Dirichlet: unit row / column


def test_zeroed_block_is_singular(ctx, meshes):
    m = structured_mesh("triangle", (4, 4), 2)
    dm = meshes(m)
    torch = _torch(ctx)
    A = _assemble(ctx, dm, "eps", "eps", 2, elastic_C(m))
    indptr, indices = A.pattern.indptr.cpu().numpy(), A.pattern.indices.cpu().numpy()
    node = 7
    for r in (2 * node, 2 * node + 1):
        cols = np.arange(indptr[r], indptr[r + 1])
        A.values[torch.from_numpy(cols[(indices[cols] // 2) == node]).cuda()] = 0.0
    with pytest.raises(ValueError, match="DXO_E_SINGULAR"):
        A.block_jacobi()


@pytest.mark.parametrize("which", ["heat", "hyperelastic", "hex_eps"])
def test_gmres_on_assembled_systems(ctx, meshes, which):
    import scipy.sparse.linalg

    from dolfinx_external_operator_amd import gmres

    A, bs = _krylov_system(ctx, meshes, which)
    S = A.to_scipy()
    b = np.random.Generator(np.random.PCG64(8)).normal(size=S.shape[0])
    ref = scipy.sparse.linalg.spsolve(S.tocsc(), b)
    rtol = 1e-12
    out = gmres(A, _cuda(b), M=A.block_jacobi(), restart=30, rtol=rtol, maxiter=5000)
    x = out.x.cpu().numpy()
    assert out.converged and not out.breakdown, which
    assert np.linalg.norm(x - ref) <= 1e-8 * np.linalg.norm(ref), which
    assert np.linalg.norm(b - S @ x) <= rtol * np.linalg.norm(b) * (1 + 1e-6)
    assert abs(out.residual - np.linalg.norm(b - S @ x) / np.linalg.norm(b)) <= 1e-3 * rtol
    _, its, conv, _ = gmres_ref(S, b, inv=block_jacobi_ref(S, bs), m=30, rtol=rtol, maxiter=5000)
    assert conv and abs(out.iterations - its) <= 2, (which, out.iterations, its)
    # one Gram-Schmidt pass (option krylov_reorth = 0) solves it too
    ctx.set_option("krylov_reorth", 0)
    try:
        one = gmres(A, _cuda(b), M=A.block_jacobi(), rtol=1e-10, maxiter=5000)
    finally:
        ctx.set_option("krylov_reorth", 1)
    assert one.converged and np.linalg.norm(one.x.cpu().numpy() - ref) <= 1e-6 * np.linalg.norm(ref)


def test_cg_on_an_spd_system(ctx, meshes):
    import scipy.sparse.linalg

    from dolfinx_external_operator_amd import cg, gmres

    m = structured_mesh("quadrilateral", (12, 10), 2, distort=0.1, seed=1)
    A = _assemble(ctx, meshes(m), "eps", "eps", 2, elastic_C(m), bcs=bottom_dofs(m, 2))
    S = A.to_scipy()
    b = np.random.Generator(np.random.PCG64(9)).normal(size=S.shape[0])
    ref = scipy.sparse.linalg.spsolve(S.tocsc(), b)
    M = A.block_jacobi()
    out = cg(A, _cuda(b), M=M, rtol=1e-12, maxiter=5000)
    assert out.converged and np.linalg.norm(out.x.cpu().numpy() - ref) <= 1e-8 * np.linalg.norm(ref)
    _, its, _ = cg_ref(S, b, inv=block_jacobi_ref(S, 2), rtol=1e-12, maxiter=5000)
    assert abs(out.iterations - its) <= 2, (out.iterations, its)
    g = gmres(A, _cuda(b), M=M, rtol=1e-12, maxiter=5000)
    assert np.linalg.norm(g.x.cpu().numpy() - out.x.cpu().numpy()) <= 1e-8 * np.linalg.norm(ref)
    # check_every changes nothing: steps past the converged one leave x alone
    again = cg(A, _cuda(b), M=M, rtol=1e-12, maxiter=5000, check_every=1)
    assert again.iterations == out.iterations and np.array_equal(again.x.cpu().numpy(), out.x.cpu().numpy())


def test_fp64_basis_ignores_krylov_basis_width(ctx, meshes):
    """The row kernels of a double basis are launched through the dispatch of the float ones and take one row per thread there,
    whatever the option krylov_basis_width says: a width that leaked into them would regroup a thread's rows, the sums would change
    their order and the bits below would differ. n = 257 is one full workgroup and a ragged tail. The operator is the leading
    257 x 257 block of the matrix of test_cg_on_an_spd_system (symmetric positive definite like it), applied by a callback."""
    from dolfinx_external_operator_amd import cg, gmres

    torch = _torch(ctx)
    m = structured_mesh("quadrilateral", (12, 10), 2, distort=0.1, seed=1)
    A = _assemble(ctx, meshes(m), "eps", "eps", 2, elastic_C(m), bcs=bottom_dofs(m, 2))
    n = 257
    Ad = _cuda(A.to_scipy().tocsr()[:n, :n].toarray()).view(n, n)
    b = _cuda(np.random.Generator(np.random.PCG64(10)).normal(size=n))

    def apply(v, out):
        torch.sum(Ad * v, dim=1, out=out)

    saved = ctx.get_option("krylov_basis_width")
    runs = []
    try:
        for width in (1, 2, 4):
            ctx.set_option("krylov_basis_width", width)
            g = gmres(apply, b, restart=8, rtol=1e-10, maxiter=400, ctx=ctx)
            c = cg(apply, b, rtol=1e-10, maxiter=400, ctx=ctx)
            assert g.basis == "fp64" and g.iterations > 8 and c.iterations > 1, (width, g.iterations, c.iterations)
            runs.append((g, c))
    finally:
        ctx.set_option("krylov_basis_width", saved)
    for pair in runs[1:]:
        for r, first in zip(pair, runs[0]):
            assert (r.iterations, r.restarts, r.residual, r.converged) == (first.iterations, first.restarts, first.residual, first.converged)
            assert torch.equal(r.x, first.x)


def test_matrix_free_operator_agrees_with_the_csr_path(ctx, meshes):
    """A callback that re-enters the library (dxo_bilinear_apply on the same context) as the operator."""
    from dolfinx_external_operator_amd import gmres

    torch = _torch(ctx)
    m = structured_mesh("triangle", (10, 8), 2, distort=0.1, seed=4)
    dm = meshes(m)
    Cb = elastic_C(m, 6)
    Cd = _cuda(Cb)
    fixed_np = bottom_dofs(m, 2)
    A = _assemble(ctx, dm, "eps", "eps", 2, Cb, bcs=fixed_np)
    n = A.shape[0]
    free = torch.ones(n, dtype=torch.float64, device="cuda")
    free[torch.from_numpy(fixed_np).cuda()] = 0.0
    fixed = 1.0 - free
    tmp = torch.empty(n, dtype=torch.float64, device="cuda")
    calls = []

    def apply(v, out):                                    # the Dirichlet matrix: A (free v) on free rows, v on fixed rows
        torch.mul(v, free, out=tmp)
        out.zero_()
        dm.bilinear_apply("eps", "eps", 2, Cd.data_ptr(), tmp.data_ptr(), out.data_ptr())
        out.mul_(free).add_(v * fixed)
        calls.append(1)

    diag = torch.zeros(n, dtype=torch.float64, device="cuda")
    dm.bilinear_diagonal("eps", "eps", 2, Cd.data_ptr(), diag.data_ptr())
    inv_diag = 1.0 / (diag * free + fixed)
    b = _cuda(np.random.Generator(np.random.PCG64(5)).normal(size=n)) * free
    mf = gmres(apply, b, M=inv_diag, rtol=1e-12, maxiter=5000, ctx=ctx)
    csr = gmres(A, b, M=inv_diag, rtol=1e-12, maxiter=5000)
    assert mf.converged and csr.converged and len(calls) >= mf.iterations
    ref = csr.x.cpu().numpy()
    assert np.linalg.norm(mf.x.cpu().numpy() - ref) <= 1e-9 * np.linalg.norm(ref)
    assert abs(mf.iterations - csr.iterations) <= max(2, csr.iterations // 10)


def test_reproducible_early_exits_and_overshoot(ctx, meshes):
    from dolfinx_external_operator_amd import gmres

    torch = _torch(ctx)
    A, bs = _krylov_system(ctx, meshes, "hyperelastic")
    M = A.block_jacobi()
    b = _cuda(np.random.Generator(np.random.PCG64(6)).normal(size=A.shape[0]))
    x0 = _cuda(np.random.Generator(np.random.PCG64(7)).normal(size=A.shape[0]))
    r1 = gmres(A, b, x=x0.clone(), M=M, rtol=1e-10, maxiter=5000)
    r2 = gmres(A, b, x=x0.clone(), M=M, rtol=1e-10, maxiter=5000)
    assert r1.converged and r1.iterations == r2.iterations and torch.equal(r1.x, r2.x)        # bit-reproducible
    r8 = gmres(A, b, x=x0.clone(), M=M, rtol=1e-10, maxiter=5000, check_every=8)
    r1c = gmres(A, b, x=x0.clone(), M=M, rtol=1e-10, maxiter=5000, check_every=1)
    assert r8.iterations == r1c.iterations
    assert torch.allclose(r8.x, r1c.x, rtol=0, atol=1e-14 * float(r1c.x.abs().max()))
    z = gmres(A, torch.zeros_like(b), x=x0.clone(), M=M)
    assert z.iterations == 0 and z.converged and not z.x.any()
    short = gmres(A, b, M=M, maxiter=3)
    assert not short.converged and short.iterations == 3 and 0 < short.residual < 1


def test_graph_capture_replays_bitwise(ctx, meshes):
    torch = _torch(ctx)
    m = structured_mesh("triangle", (8, 8), 2)
    A = _assemble(ctx, meshes(m), "eps", "eps", 2, elastic_C(m, 1), bcs=bottom_dofs(m, 2))
    M = A.block_jacobi()
    x = _cuda(np.random.Generator(np.random.PCG64(1)).normal(size=A.shape[0]))
    y, z = torch.empty_like(x), torch.empty_like(x)
    A.matvec(x, y)
    M.apply(y, z)
    eager_y, eager_z = y.clone(), z.clone()
    y.zero_()
    z.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ctx.set_stream(s.cuda_stream)
            A.matvec(x, y)
            M.apply(y, z)
    torch.cuda.current_stream().wait_stream(s)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        y.zero_()
        z.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager_y) and torch.equal(z, eager_z)


def test_argument_errors(ctx, meshes, hip_library):
    from dolfinx_external_operator_amd._lib import KRYLOV_APPLY_FN, KrylovInfo, KrylovOp, KrylovPc

    torch = _torch(ctx)
    lib, h = hip_library, ctx._h
    m = structured_mesh("triangle", (4, 4), 2)
    A = _assemble(ctx, meshes(m), "eps", "eps", 2, elastic_C(m), bcs=bottom_dofs(m, 2))
    n = A.shape[0]
    vals = C.c_void_p(A.values.data_ptr())
    b, x = _cuda(np.ones(n)), torch.zeros(n, dtype=torch.float64, device="cuda")
    inv = A.block_jacobi().inv
    ws = C.c_void_p()
    assert lib.dxo_krylov_create(h, n, 0, C.byref(ws)) == -3
    assert lib.dxo_krylov_create(h, n, 65, C.byref(ws)) == -3
    assert lib.dxo_krylov_create(h, n, 10, None) == -1
    assert lib.dxo_krylov_create(h, n, 10, C.byref(ws)) == 0
    small = C.c_void_p()
    assert lib.dxo_krylov_create(h, n - 2, 10, C.byref(small)) == 0
    try:
        info = KrylovInfo()
        op = KrylovOp(n, A.pattern._h, vals, KRYLOV_APPLY_FN(), None)
        pc = KrylovPc(2, 2, n, C.c_void_p(inv.data_ptr()))
        bp, xp = C.c_void_p(b.data_ptr()), C.c_void_p(x.data_ptr())
        for fn in (lib.dxo_krylov_gmres, lib.dxo_krylov_cg):
            assert fn(h, ws, C.byref(op), C.byref(pc), bp, xp, 1e-8, 0.0, 100, 8, C.byref(info)) == 0
            assert fn(h, None, C.byref(op), C.byref(pc), bp, xp, 1e-8, 0.0, 100, 8, C.byref(info)) == -1           # NULL
            assert fn(h, ws, C.byref(op), C.byref(pc), None, xp, 1e-8, 0.0, 100, 8, C.byref(info)) == -1
            assert fn(h, small, C.byref(op), C.byref(pc), bp, xp, 1e-8, 0.0, 100, 8, C.byref(info)) == -3          # sizes
            assert fn(h, ws, C.byref(KrylovOp(n - 2, A.pattern._h, vals, KRYLOV_APPLY_FN(), None)), C.byref(pc), bp, xp, 1e-8, 0.0, 100, 8,
                      C.byref(info)) == -3
            assert fn(h, ws, C.byref(op), C.byref(KrylovPc(2, 3, n, C.c_void_p(inv.data_ptr()))), bp, xp, 1e-8, 0.0, 100, 8,
                      C.byref(info)) == -2                                                                       # block size
            assert fn(h, ws, C.byref(op), C.byref(KrylovPc(2, 2, n - 2, C.c_void_p(inv.data_ptr()))), bp, xp, 1e-8, 0.0, 100, 8,
                      C.byref(info)) == -3                                                  # preconditioner of another size
            assert fn(h, ws, C.byref(op), C.byref(KrylovPc(1, 1, n + 2, C.c_void_p(inv.data_ptr()))), bp, xp, 1e-8, 0.0, 100, 8,
                      C.byref(info)) == -3
            assert fn(h, ws, C.byref(op), C.byref(pc), C.c_void_p(b.data_ptr() + 4), xp, 1e-8, 0.0, 100, 8, C.byref(info)) == -5
            assert fn(h, ws, C.byref(op), C.byref(pc), bp, xp, 1e-8, 0.0, 100, 0, C.byref(info)) == -3
            assert fn(h, ws, C.byref(op), C.byref(pc), bp, xp, -1.0, 0.0, 100, 8, C.byref(info)) == -6
            assert fn(h, ws, C.byref(KrylovOp(n, None, None, KRYLOV_APPLY_FN(), None)), C.byref(pc), bp, xp, 1e-8, 0.0, 100, 8,
                      C.byref(info)) == -1
        assert lib.dxo_csr_spmv(h, A.pattern._h, vals, 1.0, None, 0.0, xp) == -1
        assert lib.dxo_csr_spmv(h, A.pattern._h, vals, 1.0, C.c_void_p(b.data_ptr() + 4), 0.0, xp) == -5
        assert lib.dxo_csr_block_jacobi(h, A.pattern._h, vals, None) == -1
        assert lib.dxo_block_jacobi_apply(h, 4, n, C.c_void_p(inv.data_ptr()), bp, xp) == -2
        assert lib.dxo_block_jacobi_apply(h, 2, n + 1, C.c_void_p(inv.data_ptr()), bp, xp) == -3
    finally:
        lib.dxo_krylov_destroy(h, ws)
        lib.dxo_krylov_destroy(h, small)
    for key, bad in (("krylov_reorth", 2), ("spmv_lanes", 12)):
        with pytest.raises(ValueError, match="DXO_E_OPTION"):
            ctx.set_option(key, bad)
    from dolfinx_external_operator_amd import gmres

    m2 = structured_mesh("triangle", (3, 3), 2)
    small_M = _assemble(ctx, meshes(m2), "eps", "eps", 2, elastic_C(m2), bcs=bottom_dofs(m2, 2)).block_jacobi()
    with pytest.raises(ValueError, match="preconditioner covers"):
        gmres(A, b, M=small_M)
    with pytest.raises(ValueError, match="must be a float64"):
        gmres(lambda v, out: None, [1.0, 2.0], ctx=ctx)
    with pytest.raises(RuntimeError, match="boom"):
        gmres(lambda v, out: (_ for _ in ()).throw(RuntimeError("boom")), b, ctx=ctx)


def test_slope_example_matches_its_lu_run():
    import pathlib
    import sys

    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1] / "examples"))
    import device_mohr_coulomb_slope as ex

    g = ex.main(12, steps=10, solver="gmres", verbose=False)
    lu = ex.main(12, steps=10, solver="lu", verbose=False)
    assert g["failed"] is None and lu["failed"] is None, (g["failed"], lu["failed"])
    assert len(g["steps"]) == len(lu["steps"]) == 10
    for sg, sl in zip(g["steps"], lu["steps"]):
        assert abs(sg["newton"] - sl["newton"]) <= 1 and sg["newton"] < 100
        assert sg["residuals"][-1] <= max(1e-8, 1e-8 * sg["residuals"][0])
        ug, ul = np.array(sg["u_corner"]), np.array(sl["u_corner"])
        assert np.abs(ug - ul).max() <= 1e-6 * np.abs(ul).max()
    assert np.abs(g["u"] - lu["u"]).max() <= 1e-6 * np.abs(lu["u"]).max()
