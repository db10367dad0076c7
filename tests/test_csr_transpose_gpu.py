"""dxo_csr_transpose / dxo_csr_spmv_t on the device: the transposed matrix on the same pattern is exact data movement, commutes with
the Dirichlet pass, agrees with the assembly of the swapped pair, and the transposed product is the product with the transposed
matrix bit for bit. The accuracy of the transposed product is therefore the existing SpMV's: no tolerance of its own."""
import ctypes as C

import numpy as np
import pytest

from solver_cases import CELLS, _assemble, _cuda, _torch, meshes  # noqa: F401 (meshes: a fixture)
from transpose_cases import form_mesh, random_blocks, some_dirichlet_dofs

pytestmark = pytest.mark.gpu

# bs == gdim, bs == 1: a pair whose swap is in the table (cross-checked against the assembly), and the heat pair, whose swap is not
SQUARE = {True: ("eps", "eps"), False: ("value_grad", "value_grad")}
HEAT = ("grad", "value_grad")


def _sorted_csr(S):
    S = S.tocsr()
    S.sort_indices()
    return S


def _same_csr(a, b):
    return np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data)


def _asym(S):
    return abs(S - S.T).max() / abs(S).max()


def _dirichlet(ctx, A, dofs_d):
    rc = ctx.lib.dxo_csr_dirichlet(ctx._h, A.pattern._h, C.c_void_p(dofs_d.data_ptr()), int(dofs_d.numel()), 1.0, C.c_void_p(A.values.data_ptr()))
    ctx.check(rc, "dxo_csr_dirichlet")


def _check_matrix(ctx, torch, A, rng):
    """The exactness of the transposition and the bit identity of the transposed product, on one assembled matrix."""
    from dolfinx_external_operator_amd.operand_eval import DeviceCSR

    S = A.to_scipy()
    assert _asym(S) >= 1e-3, "a symmetric matrix would hide a missing transpose"
    T = A.transpose()
    assert T.pattern is A.pattern and T.values.data_ptr() != A.values.data_ptr()
    assert _same_csr(_sorted_csr(T.to_scipy()), _sorted_csr(S.T))
    assert np.array_equal(A.to_scipy().data, S.data)                        # out of place leaves A alone
    B = DeviceCSR(A.pattern, A.values.clone())
    assert B.transpose(out=B.values) is B                                   # in place
    assert torch.equal(B.values, T.values)
    B.transpose(out=B.values)                                               # twice: the bits are back
    assert torch.equal(B.values, A.values)
    assert torch.equal(T.transpose().values, A.values)
    other = torch.empty_like(A.values)
    assert A.transpose(out=other).values is other and torch.equal(other, T.values)
    # the transposed product is the product with the transposed matrix, bit for bit
    n = A.pattern.n_rows
    x, y0 = _cuda(rng.normal(size=n)), _cuda(rng.normal(size=n))
    try:
        for lanes in (8, 16, 32, 64):
            ctx.set_option("spmv_lanes", lanes)
            for alpha, beta in ((1.0, 0.0), (-0.5, 2.0)):
                if beta == 0.0:
                    ya = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
                    yb = ya.clone()
                else:
                    ya, yb = y0.clone(), y0.clone()
                A.matvec(x, ya, alpha, beta, transpose=True)
                T.matvec(x, yb, alpha, beta)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(ya).all()), (lanes, alpha, beta)
                assert torch.equal(ya, yb), (lanes, alpha, beta, float((ya - yb).abs().max()))
    finally:
        ctx.set_option("spmv_lanes", 0)
    assert torch.equal(A.matvec(x, transpose=True), T.matvec(x))
    return T


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("degree", [1, 2])
def test_transpose_is_exact_and_spmv_t_is_its_product_bit_for_bit(ctx, meshes, cell, degree):
    from dolfinx_external_operator_amd.operand_eval import DeviceCSR

    torch = _torch(ctx)
    m = form_mesh(cell, degree)
    dm = meshes(m)
    G, nn = m.gdim, m.node_x.shape[0]
    rng = np.random.Generator(np.random.PCG64(17))
    for vector in (False, True):
        bs = G if vector else 1
        dofs = some_dirichlet_dofs(nn * bs)
        dofs_d = torch.from_numpy(dofs).cuda()
        test, trial = SQUARE[vector]
        Cb = random_blocks(m, test, trial, bs, rng)
        A = _assemble(ctx, dm, test, trial, bs, Cb, bcs=dofs)
        T = _check_matrix(ctx, torch, A, rng)
        # against the existing assembly of the swapped pair with C^T
        Ts = _assemble(ctx, dm, trial, test, bs, np.ascontiguousarray(Cb.transpose(0, 2, 1)), bcs=dofs)
        err = float((T.values - Ts.values).abs().max())
        print(f"{cell} P{degree} bs {bs}: transpose against the swapped assembly {err / float(A.values.abs().max()):.2e} of max|A|")
        assert err <= 1e-12 * float(A.values.abs().max())
        # the Dirichlet pass commutes with the transposition, exactly
        A0 = _assemble(ctx, dm, test, trial, bs, Cb)
        assert _asym(A0.to_scipy()) >= 1e-3
        first = DeviceCSR(A0.pattern, A0.values.clone())
        _dirichlet(ctx, first, dofs_d)
        first.transpose(out=first.values)
        then = A0.transpose()
        _dirichlet(ctx, then, dofs_d)
        torch.cuda.synchronize()
        assert torch.equal(first.values, then.values)
        assert torch.equal(first.values, T.values)
    # the heat pair: non-square blocks, the swap is not in the table
    _check_matrix(ctx, torch, _assemble(ctx, dm, *HEAT, 1, random_blocks(m, *HEAT, 1, rng), bcs=some_dirichlet_dofs(nn)), rng)


def test_error_paths(ctx, meshes):
    torch = _torch(ctx)
    m = form_mesh("triangle", 1)
    dm = meshes(m)
    rng = np.random.Generator(np.random.PCG64(1))
    A = _assemble(ctx, dm, "eps", "eps", 2, random_blocks(m, "eps", "eps", 2, rng))
    n, lib, h, P = A.pattern.n_rows, ctx.lib, ctx._h, C.c_void_p
    x = _cuda(rng.normal(size=n))
    with pytest.raises(ValueError):
        A.matvec(x[: n // 2].contiguous(), transpose=True)                  # a vector of the scalar field on the bs 2 pattern
    with pytest.raises(ValueError, match="transpose"):
        A.transpose(out=torch.empty(A.pattern.nnz // 2, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="transpose"):
        A.transpose(out=torch.empty(A.pattern.nnz, dtype=torch.float32, device="cuda"))
    vals, xp = P(A.values.data_ptr()), P(x.data_ptr())
    y = torch.empty_like(x)
    yp = P(y.data_ptr())
    assert lib.dxo_csr_transpose(h, None, vals, vals) == -1
    assert lib.dxo_csr_transpose(h, A.pattern._h, None, vals) == -1
    assert lib.dxo_csr_transpose(h, A.pattern._h, vals, P(A.values.data_ptr() + 4)) == -5
    assert lib.dxo_csr_spmv_t(h, A.pattern._h, vals, 1.0, None, 0.0, yp) == -1
    assert lib.dxo_csr_spmv_t(h, A.pattern._h, vals, 1.0, P(x.data_ptr() + 4), 0.0, yp) == -5
    assert "dxo_csr_spmv_t" in lib.dxo_last_error(h).decode()
    # the pattern of a multigrid level has no mesh: DXO_E_DIM
    m2 = form_mesh("quadrilateral", 2)
    bcs = np.array([0], dtype=np.int32)
    S = _assemble(ctx, meshes(m2), "grad", "grad", 1, np.broadcast_to(np.eye(2), (m2.num_cells * m2.nq, 2, 2)).copy(), bcs=bcs)
    amg = S.amg(bcs, coarse_rows=10)
    assert amg.n_levels >= 2
    lev = amg._info(1)
    assert lib.dxo_csr_transpose(h, lev.csr, lev.values, lev.values) == -2
    assert lib.dxo_csr_spmv_t(h, lev.csr, lev.values, 1.0, xp, 0.0, yp) == -2
    assert "multigrid level" in lib.dxo_last_error(h).decode()
    torch.cuda.synchronize()
