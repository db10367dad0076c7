"""gmres / fgmres with basis="fp32" (dxo_krylov_create_basis, DXO_KRYLOV_BASIS_FP32) on the device: bit for bit the fp64 basis where
every basis vector is a unit vector, against gmres_cb_ref and the closed forms of F2 at every step, restart length and size where
the row kernels change shape (every width of the float-basis kernels, option krylov_basis_width), the stored rows themselves,
assembled and multigrid-preconditioned systems on the true residual, the range of b, reproducibility and the errors.

Tolerances: counts and flags are exact. F2 residuals and iterates are held to MARGIN = 100 x REF_CB_F2_RES / REF_CB_F2_X, the
deviation of gmres_cb_ref itself from the long-double answers (tests/test_krylov_fp32_basis_oracle_cpu.py): 100 x 3e-3 relative on
the residual against the closed form, 100 x 1e-7 max|x| on x_k against gmres_cb_ref. One wrong rotation, stride or tail changes
either by O(1)."""
import ctypes as C

import numpy as np
import pytest

from oracle.krylov_oracle import (F2_D, F2_MAIN, MARGIN, REF_CB_F2_RES, REF_CB_F2_X, cyclic_shift_src, gmres_cb_ref, shifted_op,
                                  shifted_residual, unit_rhs, xdev)
from solver_cases import (_case_hierarchy, _cuda, _f2, _grid_cap, _krylov_system, _reorth, _shift, _torch,
                          meshes)  # noqa: F401  (meshes is a fixture)

pytestmark = pytest.mark.gpu

CB_RES_TOL, CB_X_TOL = MARGIN * REF_CB_F2_RES, MARGIN * REF_CB_F2_X
WIDTHS = (1, 2, 4)
EXACT_D = (1, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)        # both sides of every KMAX switch of the multi-dot (4 / 8 / 16 / 32 / 64)


class _width:
    """The rows of the float basis a thread owns, for the solves inside the scope."""

    def __init__(self, ctx, value):
        self.ctx, self.value = ctx, value

    def __enter__(self):
        self.default = self.ctx.get_option("krylov_basis_width")
        self.ctx.set_option("krylov_basis_width", self.value)

    def __exit__(self, *exc):
        self.ctx.set_option("krylov_basis_width", self.default)


def _flags(out):
    return out.iterations, out.restarts, out.converged, out.breakdown


def _rows(ctx, n, restart):
    from dolfinx_external_operator_amd import krylov_basis_rows

    rows = krylov_basis_rows(ctx, n, restart, "fp32")
    ld = max(64, -(-n // 64) * 64)
    assert rows.dtype == np.float32 and rows.shape == (restart + 1, ld), (rows.dtype, rows.shape, n)
    assert not rows[:, n:].any()                              # the padding of a row is never written
    return rows


# ---- 1. the exact family
def _exact_sizes(d, cap):
    """(q, t) with n = t + d q: n = d and 31 d, and per d the ragged sizes: below any width (n = 1, 2, 3, 5), 255 / 256 / 257,
    1023 / 1025, one trip of the grid and more than two with a ragged tail."""
    sizes = [(1, 0), (31, 0)]
    if d == 1:
        sizes += [(2, 0), (3, 0), (5, 0)]
    if d == 4:
        sizes += [(1, 1)]                                     # n = 5 with a cycle of 4
    if d == 17:
        sizes += [(15, 0), (15, 1), (15, 2)]                  # 255, 256, 257
    if d == 33:
        sizes += [(31, 2)]                                    # 1025 (31 d = 1023)
    if d == 64:
        sizes += [((cap + 5) // d, (cap + 5) % d), ((2 * cap + 13) // d, (2 * cap + 13) % d)]
    return sizes


@pytest.mark.parametrize("d", EXACT_D)
def test_unit_vector_bases_are_bitwise_the_fp64_basis(ctx, d):
    from dolfinx_external_operator_amd import gmres

    torch = _torch(ctx)
    cap = _grid_cap(torch)
    ns = []
    for q, t in _exact_sizes(d, cap):
        src = cyclic_shift_src(d, q, t)
        n = src.size
        ns.append(n)
        P = _shift(torch, src)
        nxt = np.empty(n, np.int64)
        nxt[src] = np.arange(n)                               # P e_p = e_{nxt[p]}
        for s in sorted({t, n - 1}):                          # on the first cycle and on the last one
            bd = _cuda(unit_rhs(n, s))
            for restart in sorted({64, d}):
                ref = gmres(P, bd, restart=restart, rtol=1e-10, ctx=ctx)
                assert _flags(ref)[:3] == (d, 1, True) and ref.residual == 0.0 and ref.basis == "fp64", (d, n, s, ref)
                for width in WIDTHS:
                    with _width(ctx, width):
                        out = gmres(P, bd, restart=restart, rtol=1e-10, ctx=ctx, basis="fp32")
                    what = (d, n, s, restart, width, out)
                    assert _flags(out) == _flags(ref) and out.residual == ref.residual and out.basis == "fp32", what
                    assert torch.equal(out.x, ref.x), what
                    rows = _rows(ctx, n, restart)
                    assert out.basis_bytes == rows.size * 4 and ref.basis_bytes == (restart + 1) * max(32, -(-n // 32) * 32) * 8, what
                    pos = s
                    for j in range(d):                        # row j is e_{P^j s}, exactly
                        hot = np.flatnonzero(rows[j])
                        assert hot.tolist() == [pos] and rows[j, pos] == np.float32(1.0), (what, j, hot[:4])
                        pos = int(nxt[pos])
    if d == 64:
        assert ns[-2] == cap + 5 and ns[-1] == 2 * cap + 13


# ---- 2. and 3. F2 against gmres_cb_ref and the closed form
def _cb_step(gmres, ctx, dev, src, b, k, restart=64, closed=True, reorth=True, worst=None, ref=None, **kw):
    """k steps on the device against k steps of gmres_cb_ref (counts, flags, x_k) and the closed form (residual)."""
    if ref is None:
        ref = gmres_cb_ref(shifted_op(src), b, m=restart, rtol=0.0, maxiter=k, reorth=reorth, full=True)
    x, its, conv, res, brk, cycles = ref
    out = gmres(dev, _cuda(b), restart=restart, rtol=0.0, maxiter=k, ctx=ctx, basis="fp32", **kw)
    what = (b.size, k, restart, out)
    assert _flags(out) == (k, -(-k // restart), False, False) == (its, cycles, conv, brk), what
    f = float(shifted_residual(k)) if closed else res
    dr, dx = abs(out.residual - f) / f, xdev(out.x.cpu().numpy(), x)
    if worst is not None:
        worst[0], worst[1] = max(worst[0], dr), max(worst[1], dx)
    assert dr <= CB_RES_TOL and dx <= CB_X_TOL, (what, dr, dx)
    return ref


def test_shifted_shift_at_the_sizes_where_the_row_kernels_change_shape(ctx):
    from dolfinx_external_operator_amd import gmres

    torch = _torch(ctx)
    cap = _grid_cap(torch)
    ns = [255, 256, 257, 1023, 1025, cap + 5, 2 * cap + 13]
    for n in ns:
        q, t = divmod(n, F2_D)
        src, b, D, dev = _f2(torch, q, t)
        assert b.size == n
        worst = [0.0, 0.0]
        for k in (1, 33, 64):
            ref = None
            for width in WIDTHS:
                with _width(ctx, width):
                    ref = _cb_step(gmres, ctx, dev, src, b, k, worst=worst, ref=ref)
        print(f"F2 fp32 basis n = {n}: residual {worst[0]:.2e} relative to the closed form, x_k {worst[1]:.2e} max|x| from gmres_cb_ref")


def test_shifted_shift_residual_and_iterate_at_every_step(ctx):
    from dolfinx_external_operator_amd import gmres

    torch = _torch(ctx)
    src, b, D, dev = _f2(torch, *F2_MAIN)
    worst = [0.0, 0.0]
    for k in range(1, 65):
        _cb_step(gmres, ctx, dev, src, b, k, worst=worst)
    print(f"F2 fp32 basis n = {b.size}, k = 1..64: residual {worst[0]:.2e} relative, x_k {worst[1]:.2e} max|x|")
    worst = [0.0, 0.0]
    with _reorth(ctx, 0):
        for k in (1, 2, 5, 17, 33, 64):
            _cb_step(gmres, ctx, dev, src, b, k, reorth=False, worst=worst)
    print(f"F2 fp32 basis, one Gram-Schmidt pass: residual {worst[0]:.2e} relative, x_k {worst[1]:.2e} max|x|")


@pytest.mark.parametrize("restart", [1, 2, 3, 7])
def test_shifted_shift_short_restarts_follow_the_oracle(ctx, restart):
    from dolfinx_external_operator_amd import gmres

    torch = _torch(ctx)
    src, b, D, dev = _f2(torch, *F2_MAIN)
    worst = [0.0, 0.0]
    for maxiter in (20, 21):                                  # the last cycle full and cut short
        _cb_step(gmres, ctx, dev, src, b, maxiter, restart=restart, closed=False, worst=worst)
    print(f"F2 fp32 basis restart = {restart}: residual {worst[0]:.2e} relative, x {worst[1]:.2e} max|x|")


# ---- 4. the stored basis
def _check_stored(ctx, out, n, restart, k):
    ws = ctx._krylov_ws[(n, restart, "fp32")]
    kind, nbytes, ptr, ld = ws.basis_info()
    assert kind == "fp32" and ptr and nbytes == (restart + 1) * ld * 4 == out.basis_bytes and ld % 64 == 0 and ld >= n
    V = _rows(ctx, n, restart)[: k + 1, :n].astype(np.float64)
    G = V @ V.T
    norms, off = np.sqrt(np.diag(G)), np.abs(G - np.diag(np.diag(G))).max()
    print(f"stored basis n = {n}, k = {k}: max | |v_j| - 1 | {np.abs(norms - 1).max():.2e}, max |(v_i, v_j)| {off:.2e}")
    assert np.abs(norms - 1).max() <= 2.0 ** -23
    assert off <= k * 2.0 ** -23


def test_the_stored_basis_is_normalised_and_orthogonal_to_float_rounding(ctx, meshes):  # noqa: F811
    from dolfinx_external_operator_amd import fgmres, gmres

    torch = _torch(ctx)
    src, b, D, dev = _f2(torch, *F2_MAIN)
    for k in (5, 64):
        out = gmres(dev, _cuda(b), restart=64, rtol=0.0, maxiter=k, ctx=ctx, basis="fp32")
        assert _flags(out) == (k, 1, False, False)
        _check_stored(ctx, out, b.size, 64, k)
    A, bs = _krylov_system(ctx, meshes, "hex_eps")
    rhs = _cuda(np.random.Generator(np.random.PCG64(8)).normal(size=A.shape[0]))
    for solve in (gmres, fgmres):
        out = solve(A, rhs.clone(), M=A.block_jacobi(), restart=30, rtol=0.0, maxiter=30, basis="fp32")
        assert _flags(out) == (30, 1, False, False)
        _check_stored(ctx, out, A.shape[0], 30, 30)


# ---- 5. assembled systems
def _true_residual(A, b, x):
    from dolfinx_external_operator_amd.krylov import csr_matvec

    return float((b - csr_matvec(A, x)).norm() / b.norm())


def _both_bases(solve, A, b, M, which, restart=30, rtol=1e-10):
    out64 = solve(A, b, M=M, restart=restart, rtol=rtol, maxiter=5000)
    out32 = solve(A, b, M=M, restart=restart, rtol=rtol, maxiter=5000, basis="fp32")
    r64, r32 = _true_residual(A, b, out64.x), _true_residual(A, b, out32.x)
    print(f"{which} {solve.__name__}({restart}): iterations fp32 / fp64 basis {out32.iterations} / {out64.iterations}, cycles "
          f"{out32.restarts} / {out64.restarts}, |b - A x| / |b| {r32:.3e} / {r64:.3e}, basis bytes {out32.basis_bytes} / {out64.basis_bytes}")
    assert out64.converged and out32.converged and not out32.breakdown, (which, out32)
    assert r32 <= rtol and r64 <= rtol, (which, r32, r64)     # the iterates are compared through their residuals
    assert out32.iterations <= out64.iterations + restart, (which, out32.iterations, out64.iterations)
    n = A.shape[0]
    assert out32.basis_bytes == (restart + 1) * max(64, -(-n // 64) * 64) * 4 and out64.basis_bytes == (restart + 1) * max(32, -(-n // 32) * 32) * 8
    return out32, out64


@pytest.mark.parametrize("which", ["heat", "hyperelastic", "hex_eps"])
def test_assembled_systems_converge_on_the_true_residual(ctx, meshes, which):  # noqa: F811
    from dolfinx_external_operator_amd import fgmres, gmres

    _torch(ctx)
    A, bs = _krylov_system(ctx, meshes, which)
    b = _cuda(np.random.Generator(np.random.PCG64(8)).normal(size=A.shape[0]))
    M = A.block_jacobi()
    _both_bases(gmres, A, b, M, which)
    _both_bases(fgmres, A, b, M, which)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_multigrid_preconditioned_solves_converge_on_the_true_residual(ctx, meshes, precision):  # noqa: F811
    from dolfinx_external_operator_amd import fgmres, gmres

    _torch(ctx)
    A, amg = _case_hierarchy(ctx, meshes, "heat48", precision=precision)
    b = _cuda(np.random.Generator(np.random.PCG64(1)).normal(size=A.shape[0]))
    for solve in (gmres, fgmres):
        _both_bases(solve, A, b, amg, f"heat48 AMG {precision}")


# ---- 6. range
def test_the_basis_sees_normalised_vectors_whatever_the_scale_of_b(ctx, meshes):  # noqa: F811
    from dolfinx_external_operator_amd import fgmres, gmres

    torch = _torch(ctx)
    src, b, D, dev = _f2(torch, *F2_MAIN)
    A, bs = _krylov_system(ctx, meshes, "heat")
    rhs = np.random.Generator(np.random.PCG64(8)).normal(size=A.shape[0])
    cases = (("F2", lambda v, **kw: gmres(dev, v, restart=30, ctx=ctx, **kw), b),
             ("heat gmres", lambda v, **kw: gmres(A, v, M=A.block_jacobi(), **kw), rhs),
             ("heat fgmres", lambda v, **kw: fgmres(A, v, M=A.block_jacobi(), **kw), rhs))
    for name, solve, vec in cases:
        one = solve(_cuda(vec), basis="fp32")
        assert one.converged and one.iterations > 5, (name, one)
        for e in (300, -300):
            s = 2.0 ** e
            out = solve(_cuda(vec * s), basis="fp32")
            assert _flags(out) == _flags(one) and out.residual == one.residual, (name, e, out, one)
            assert torch.equal(out.x, one.x * s), (name, e)


# ---- 7. reproducibility
def test_two_solves_are_bit_identical(ctx, meshes):  # noqa: F811
    from dolfinx_external_operator_amd import fgmres, gmres

    torch = _torch(ctx)
    A, bs = _krylov_system(ctx, meshes, "hyperelastic")              # 41 cycles: a long history to repeat bit for bit
    M = A.block_jacobi()
    b = _cuda(np.random.Generator(np.random.PCG64(6)).normal(size=A.shape[0]))
    for solve in (gmres, fgmres):
        for width in WIDTHS:
            with _width(ctx, width):
                first = solve(A, b, M=M, rtol=1e-10, maxiter=5000, basis="fp32")
                x1 = first.x.clone()
                other = gmres(A, b, M=M, restart=7, rtol=1e-3, basis="fp32")       # another workspace in between
                again = solve(A, b, M=M, rtol=1e-10, maxiter=5000, basis="fp32")
            assert other.converged and first.converged and _flags(again) == _flags(first) and again.residual == first.residual
            assert torch.equal(again.x, x1), (solve.__name__, width)


@pytest.mark.parametrize("which", ["heat", "hex_eps"])
def test_fgmres_takes_the_iterations_of_gmres_with_a_fixed_preconditioner(ctx, meshes, which):  # noqa: F811
    """x += M (V y) and x += sum y_j (M v_j) are the same vector rounded differently, so the two histories agree step for step
    only while that rounding cannot decide a step: on solves of a few cycles. (The 41-cycle hyperelastic solve of the test above
    ends at 1208 and 1207 iterations on an MI355X, 1216 both with the fp64 basis.)"""
    from dolfinx_external_operator_amd import fgmres, gmres

    _torch(ctx)
    A, bs = _krylov_system(ctx, meshes, which)
    M = A.block_jacobi()
    b = _cuda(np.random.Generator(np.random.PCG64(8)).normal(size=A.shape[0]))
    g, f = gmres(A, b, M=M, rtol=1e-10, basis="fp32"), fgmres(A, b, M=M, rtol=1e-10, basis="fp32")
    print(f"{which}: gmres {g.iterations} iterations in {g.restarts} cycles, fgmres {f.iterations} in {f.restarts}")
    assert g.converged and f.converged and g.restarts <= 5
    assert (f.iterations, f.restarts) == (g.iterations, g.restarts), (which, f, g)


# ---- 8. errors
def test_errors(ctx, meshes, hip_library):  # noqa: F811
    from dolfinx_external_operator_amd import cg, fgmres, gmres, krylov_basis_rows
    from dolfinx_external_operator_amd._lib import KrylovInfo

    torch = _torch(ctx)
    lib, h = hip_library, ctx._h
    b = _cuda(np.ones(4))                                      # |b| = 2: b / |b| is exact in float

    def identity(v, out):
        out.copy_(v)

    for bad in ("fp16", "FP32", None, 32):
        for solve in (gmres, fgmres):
            with pytest.raises(ValueError, match="basis must be one of"):
                solve(identity, b, ctx=ctx, basis=bad)
    with pytest.raises(TypeError):
        cg(identity, b, ctx=ctx, basis="fp32")
    with pytest.raises(ValueError, match="no solve"):
        krylov_basis_rows(ctx, 12345, 3, "fp32")
    with pytest.raises(ValueError, match="DXO_E_OPTION"):
        ctx.set_option("krylov_basis_width", 3)
    ws = C.c_void_p()
    for kind in (2, -1, 64):
        assert lib.dxo_krylov_create_basis(h, 10, 5, kind, C.byref(ws)) == -6 and not ws.value
    assert b"DXO_KRYLOV_BASIS_FP32" in lib.dxo_last_error(h)
    for restart in (0, 65):                                   # the bounds of dxo_krylov_create
        assert lib.dxo_krylov_create_basis(h, 10, restart, 1, C.byref(ws)) == lib.dxo_krylov_create(h, 10, restart, C.byref(ws)) == -3
    assert lib.dxo_krylov_create_basis(h, -1, 5, 1, C.byref(ws)) == -3
    assert lib.dxo_krylov_create_basis(h, 10, 5, 1, None) == -1
    plain = C.c_void_p()
    assert lib.dxo_krylov_create_basis(h, 10, 5, 1, C.byref(ws)) == 0 and lib.dxo_krylov_create(h, 10, 5, C.byref(plain)) == 0
    try:
        assert lib.dxo_krylov_basis_info(h, None, None, None, None, None) == -1
        assert lib.dxo_krylov_basis_info(h, ws, None, None, None, None) == 0
        kind, nbytes, rows, ld = C.c_int(-1), C.c_int64(-1), C.c_void_p(), C.c_int64(-1)
        assert lib.dxo_krylov_basis_info(h, ws, C.byref(kind), None, None, C.byref(ld)) == 0 and (kind.value, ld.value) == (1, 64)
        assert lib.dxo_krylov_basis_info(h, ws, C.byref(kind), C.byref(nbytes), C.byref(rows), C.byref(ld)) == 0
        assert (kind.value, nbytes.value, ld.value) == (1, 6 * 64 * 4, 64) and rows.value
        assert lib.dxo_krylov_basis_info(h, plain, C.byref(kind), C.byref(nbytes), C.byref(rows), C.byref(ld)) == 0
        assert (kind.value, nbytes.value, ld.value) == (0, 6 * 32 * 8, 32) and rows.value
        info = KrylovInfo()
        assert lib.dxo_krylov_cg(h, ws, None, None, None, None, 1e-8, 0.0, 10, 8, C.byref(info)) == -6       # CG keeps no basis
        assert b"dxo_krylov_cg" in lib.dxo_last_error(h)
        assert lib.dxo_krylov_cg(h, plain, None, None, None, None, 1e-8, 0.0, 10, 8, C.byref(info)) == -1    # as before: NULL arguments
    finally:
        lib.dxo_krylov_destroy(h, ws)
        lib.dxo_krylov_destroy(h, plain)
    out = gmres(identity, b, ctx=ctx, basis="fp32")            # the context still solves
    assert out.converged and out.iterations == 1 and torch.equal(out.x, b)
