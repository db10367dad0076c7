"""dxo_csr_create / dxo_bilinear_assemble / dxo_csr_dirichlet on the device: the assembled matrix of the bilinear form of a pair of
linear operand kinds, against the pattern and dense oracles of tests/test_assemble_oracle_cpu.py, against the matrix-free operators
and against the heat demo's own comparison of assembled Jacobians (demo_nonlinear_heat_equation_part2.py:313-335)."""
import ctypes as C
import sys

import numpy as np
import pytest

from oracle.form_oracle import apply_bcs, csr_to_dense, dense_by_probes, dense_ref, heat_setting, pattern_ref
from oracle.operand_oracle import DEFGRAD, GRAD, VALUE
from solver_cases import CELLS, PAIRS, _cuda, _value_size, _zeros
from tools.synthetic import structured_mesh

pytestmark = pytest.mark.gpu


def _assemble(ctx, dm, test, trial, bs, Cd, **kw):
    import torch

    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    A = dm.bilinear_assemble(test, trial, bs, Cd.data_ptr(), dm.csr_pattern(bs), **kw)
    torch.cuda.synchronize()
    return A


def _dense(A):
    indptr, indices, values = A.to_numpy()
    return csr_to_dense(indptr, indices, values, A.shape[0])


def _csr_matvec(A, v):
    indptr, indices, values = A.to_numpy()
    rows = np.repeat(np.arange(A.shape[0]), np.diff(indptr))
    return np.bincount(rows, weights=values * v[indices], minlength=A.shape[0])


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("degree", [1, 2])
def test_pattern_is_the_oracle_pattern(ctx, cell, degree):
    from dolfinx_external_operator_amd import DeviceMesh

    m = structured_mesh(cell, CELLS[cell], degree, distort=0.2, seed=7)
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    try:
        for bs in (1, m.gdim):
            pat = dm.csr_pattern(bs)
            indptr, indices = pattern_ref(m, bs)
            assert pat.indptr.dtype.itemsize == 8 and pat.indices.dtype.itemsize == 4
            assert np.array_equal(pat.indptr.cpu().numpy(), indptr)
            assert np.array_equal(pat.indices.cpu().numpy(), indices)
            assert pat.n_rows == m.node_x.shape[0] * bs and pat.nnz == indices.size and pat.build_ms >= 0.0
            assert dm.csr_pattern(bs) is pat                     # once per mesh and block size
    finally:
        dm.close()


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("degree", [1, 2])
def test_every_pair_matches_the_dense_oracle(ctx, cell, degree):
    from dolfinx_external_operator_amd import DeviceMesh

    m = structured_mesh(cell, CELLS[cell], degree, distort=0.2, seed=7)
    G = m.gdim
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    rng = np.random.Generator(np.random.PCG64(13))
    try:
        for test, trial, vector in PAIRS:
            bs = G if vector else 1
            Cb = rng.normal(size=(m.num_cells * m.nq, _value_size(test, G, bs), _value_size(trial, G, bs)))
            got = _dense(_assemble(ctx, dm, test, trial, bs, _cuda(Cb)))
            ref = dense_ref(m, test, trial, bs, Cb)
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (test, trial, bs, np.abs(got - ref).max())
    finally:
        dm.close()


@pytest.mark.parametrize("cell,n,test,trial,vector", [("triangle", (24, 24), "grad", "grad", True),
                                                     ("hexahedron", (5, 4, 4), "grad", "grad", True),
                                                     ("quadrilateral", (24, 24), "grad", "value_grad", False),
                                                     ("tetrahedron", (8, 8, 6), "value_grad", "value_grad", False)])
def test_matrix_agrees_with_the_matrix_free_operators(ctx, cell, n, test, trial, vector):
    """A v (host CSR product and torch's sparse CSR product on the device) = dxo_bilinear_apply v; diag A = dxo_bilinear_diagonal."""
    import torch

    from dolfinx_external_operator_amd import DeviceMesh

    m = structured_mesh(cell, n, 2, distort=0.2, seed=5)
    G, nn = m.gdim, m.node_x.shape[0]
    bs = G if vector else 1
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    rng = np.random.Generator(np.random.PCG64(5))
    try:
        Cd = _cuda(rng.normal(size=(m.num_cells * m.nq, _value_size(test, G, bs), _value_size(trial, G, bs))))
        A = _assemble(ctx, dm, test, trial, bs, Cd)
        assert 2000 <= A.shape[0] <= 20000
        v = rng.normal(size=nn * bs)
        vd, Kv, dg = _cuda(v), _zeros(nn * bs), _zeros(nn * bs)
        dm.bilinear_apply(test, trial, bs, Cd.data_ptr(), vd.data_ptr(), Kv.data_ptr())
        dm.bilinear_diagonal(test, trial, bs, Cd.data_ptr(), dg.data_ptr())
        torch.cuda.synchronize()
        Kv, dg = Kv.cpu().numpy(), dg.cpu().numpy()
        scale = np.abs(Kv).max()
        assert np.abs(_csr_matvec(A, v) - Kv).max() <= 1e-13 * scale
        Av = (A.to_torch() @ vd.reshape(-1, 1)).reshape(-1)
        assert Av.is_cuda
        assert np.abs(Av.cpu().numpy() - Kv).max() <= 1e-13 * scale
        indptr, indices, values = A.to_numpy()
        diag = np.array([values[indptr[r]:indptr[r + 1]][indices[indptr[r]:indptr[r + 1]] == r][0] for r in range(A.shape[0])])
        assert np.abs(diag - dg).max() <= 1e-13 * np.abs(dg).max()
    finally:
        dm.close()


def test_eps_pair_with_the_von_mises_tangent_is_tangent_apply(ctx):
    import torch

    from dolfinx_external_operator_amd import DeviceMesh, VmParams

    m = structured_mesh("triangle", (20, 20), 2, distort=0.2, seed=3)
    G, nn, d = 2, m.node_x.shape[0], 4
    npts = m.num_cells * m.nq
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    rng = np.random.Generator(np.random.PCG64(3))
    try:
        E = 70e3
        prm = VmParams(E, 0.3, 250.0, E * (E / 100) / (E - E / 100))
        u = 4e-3 * rng.normal(size=nn * G)
        C_tang, sigma, dp = np.zeros(npts * d * d), np.zeros(npts * d), np.zeros(npts)
        dm.von_mises(prm, u, np.zeros(npts * d), np.zeros(npts), C_tang, sigma, dp)
        assert (dp > 0).mean() > 0.1
        Cd, v = _cuda(C_tang), rng.normal(size=nn * G)
        A = _assemble(ctx, dm, "eps", "eps", G, Cd)
        Kv = _zeros(nn * G)
        dm.tangent_apply(Cd.data_ptr(), _cuda(v).data_ptr(), Kv.data_ptr())
        torch.cuda.synchronize()
        Kv = Kv.cpu().numpy()
        assert np.abs(_csr_matvec(A, v) - Kv).max() <= 1e-13 * np.abs(Kv).max()
    finally:
        dm.close()


def test_heat_demo_matrices_on_the_device(ctx):
    """C = [dq/dT | dq/dsigma] from dxo_heat_field: one (grad, value_grad) assembly is the explicit-Jacobian matrix; (grad, value_grad)
    with [dq/dT | 0] SET, then (grad, grad) with dq/dsigma accumulated, give the same matrix."""
    import torch

    from dolfinx_external_operator_amd import MEM_DEVICE, DeviceMesh

    m, _, _, explicit = heat_setting()
    nn, npts = m.node_x.shape[0], m.num_cells * m.nq
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        q, dqdT, dqds = _zeros(npts * 2), _zeros(npts * 2), _zeros(npts * 4)
        T = _cuda(m.node_x[:, 0] ** 2 + m.node_x[:, 1])
        dm.heat(1.0, 1.0, T.data_ptr(), q.data_ptr(), dqdT.data_ptr(), dqds.data_ptr(), mem=MEM_DEVICE)
        Cd = torch.cat([dqdT.reshape(npts, 2, 1), dqds.reshape(npts, 2, 2)], dim=2).contiguous().reshape(-1)
        A = _assemble(ctx, dm, "grad", "value_grad", 1, Cd)
        E = dense_by_probes(explicit, m, 1)
        assert np.abs(_dense(A) - E).max() <= 1e-12 * np.abs(E).max()
        C1 = torch.cat([dqdT.reshape(npts, 2, 1), torch.zeros(npts, 2, 2, dtype=torch.float64, device="cuda")], dim=2).contiguous().reshape(-1)
        values = torch.full((A.values.numel(),), 1e30, dtype=torch.float64, device="cuda")
        ctx.set_option("consumer_overwrite", 1)
        try:
            _assemble(ctx, dm, "grad", "value_grad", 1, C1, values=values)
        finally:
            ctx.set_option("consumer_overwrite", 0)
        B = _assemble(ctx, dm, "grad", "grad", 1, dqds.contiguous(), values=values)
        assert B.values is values
        assert float((values - A.values).abs().max()) <= 1e-13 * float(A.values.abs().max())
    finally:
        dm.close()


def test_determinism_chunks_and_atomics(ctx):
    import torch

    from dolfinx_external_operator_amd import DeviceMesh

    m = structured_mesh("quadrilateral", (12, 10), 2, distort=0.2, seed=8)
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    rng = np.random.Generator(np.random.PCG64(8))
    Cd = _cuda(rng.normal(size=m.num_cells * m.nq * 16))
    try:
        a = _assemble(ctx, dm, "grad", "grad", 2, Cd).values
        b = _assemble(ctx, dm, "grad", "grad", 2, Cd).values
        assert torch.equal(a, b)
        for chunk in (1, 7):
            ctx.set_option("assemble_chunk_cells", chunk)
            try:
                c = _assemble(ctx, dm, "grad", "grad", 2, Cd).values
            finally:
                ctx.set_option("assemble_chunk_cells", 0)
            assert torch.equal(a, c), chunk
        ctx.set_option("adjoint_atomics", 1)
        try:
            at = _assemble(ctx, dm, "grad", "grad", 2, Cd).values
        finally:
            ctx.set_option("adjoint_atomics", 0)
        assert float((at - a).abs().max()) <= 1e-13 * float(a.abs().max())
        # default: accumulate. Entries are added into `values` one cell at a time (as MatSetValues ADD_VALUES does), so the
        # second form's entries join the first's chain: equal to a + a to rounding, not bitwise
        acc = a.clone()
        _assemble(ctx, dm, "grad", "grad", 2, Cd, values=acc)
        assert float((acc - 2 * a).abs().max()) <= 1e-14 * float(a.abs().max())
        assert float((acc - a).abs().max()) > 0.5 * float(a.abs().max())
    finally:
        dm.close()


@pytest.mark.parametrize("diagonal", [1.0, 3.25])
def test_dirichlet_rows_and_columns(ctx, diagonal):
    import torch

    from dolfinx_external_operator_amd import DeviceMesh

    m = structured_mesh("triangle", (4, 3), 2, distort=0.2, seed=4)
    nn = m.node_x.shape[0]
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    rng = np.random.Generator(np.random.PCG64(4))
    try:
        Cb = rng.normal(size=(m.num_cells * m.nq, 4, 4))
        left = np.flatnonzero(np.isclose(m.node_x[:, 0], 0.0))
        dofs = np.concatenate([left * 2, left * 2 + 1, [2 * (nn - 1) + 1]]).astype(np.int32)
        A = _assemble(ctx, dm, "grad", "grad", 2, _cuda(Cb), bcs=torch.from_numpy(dofs).cuda(), diagonal=diagonal)
        ref = apply_bcs(dense_ref(m, "grad", "grad", 2, Cb), dofs, diagonal)
        assert np.abs(_dense(A) - ref).max() <= 1e-12 * np.abs(ref).max()
        assert np.all(_dense(A)[dofs, dofs] == diagonal)
    finally:
        dm.close()


def test_graph_capture_replays_bitwise(ctx):
    import torch

    from dolfinx_external_operator_amd import DeviceMesh

    m = structured_mesh("triangle", (10, 10), 2, distort=0.2, seed=12)
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    rng = np.random.Generator(np.random.PCG64(12))
    Cd = _cuda(rng.normal(size=m.num_cells * m.nq * 16))
    bcs = torch.arange(0, 40, 3, dtype=torch.int32, device="cuda")
    pat = dm.csr_pattern(2)
    try:
        eager = _assemble(ctx, dm, "grad", "grad", 2, Cd, bcs=bcs, diagonal=2.0).values.clone()
        values = torch.empty_like(eager)
        ctx.set_option("consumer_overwrite", 1)
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                dm.bilinear_assemble("grad", "grad", 2, Cd.data_ptr(), pat, values=values, bcs=bcs, diagonal=2.0)
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            values.fill_(7.0)
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            free0 = torch.cuda.mem_get_info()[0]
            g.replay()
            torch.cuda.synchronize()
            assert torch.cuda.memory_allocated() == before
            assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20)
        finally:
            ctx.set_option("consumer_overwrite", 0)
        assert torch.equal(values, eager)
    finally:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        dm.close()


def test_error_paths(ctx):
    import torch

    from dolfinx_external_operator_amd import DeviceMesh

    m = structured_mesh("triangle", (2, 2), 2)
    other = structured_mesh("triangle", (2, 2), 2)
    nn, npts = m.node_x.shape[0], m.num_cells * m.nq
    Cd = _zeros(npts * 16)
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    dm2 = DeviceMesh.from_synthetic(other, ctx=ctx)
    lib, P = ctx.lib, C.c_void_p
    try:
        pat2, pat1 = dm.csr_pattern(2), dm.csr_pattern(1)
        vals = _zeros(pat2.nnz)
        with pytest.raises(ValueError, match="unsupported pair"):
            dm.bilinear_assemble("grad", "eps", 2, Cd.data_ptr(), pat2)
        for t, r, bs in ((GRAD, VALUE, 1), (5, 5, 2), (GRAD, 7, 1), (DEFGRAD, DEFGRAD, 1)):
            pat = pat1 if bs == 1 else pat2
            rc = lib.dxo_bilinear_assemble(ctx._h, dm._h, pat._h, t, r, bs, P(Cd.data_ptr()), P(vals.data_ptr()))
            assert rc == -6, (t, r, bs)
            assert "dxo_bilinear_assemble" in lib.dxo_last_error(ctx._h).decode()
        # a pattern of another block size or another mesh
        assert lib.dxo_bilinear_assemble(ctx._h, dm._h, pat1._h, GRAD, GRAD, 2, P(Cd.data_ptr()), P(vals.data_ptr())) == -2
        assert lib.dxo_bilinear_assemble(ctx._h, dm2._h, pat2._h, GRAD, GRAD, 2, P(Cd.data_ptr()), P(vals.data_ptr())) == -2
        with pytest.raises(ValueError, match="DXO_E_DIM"):
            dm2.bilinear_assemble("grad", "grad", 2, Cd.data_ptr(), pat2)
        # NULL arguments
        assert lib.dxo_bilinear_assemble(ctx._h, dm._h, None, GRAD, GRAD, 2, P(Cd.data_ptr()), P(vals.data_ptr())) == -1
        assert lib.dxo_bilinear_assemble(ctx._h, dm._h, pat2._h, GRAD, GRAD, 2, None, P(vals.data_ptr())) == -1
        assert lib.dxo_bilinear_assemble(ctx._h, dm._h, pat2._h, GRAD, GRAD, 2, P(Cd.data_ptr()), None) == -1
        assert lib.dxo_bilinear_assemble(None, dm._h, pat2._h, GRAD, GRAD, 2, P(Cd.data_ptr()), P(vals.data_ptr())) == -1
        assert lib.dxo_csr_create(ctx._h, None, 2, C.byref(P())) == -1
        assert lib.dxo_csr_info(ctx._h, None, None, None, None, None, None) == -1
        assert lib.dxo_csr_dirichlet(ctx._h, pat2._h, None, 3, 1.0, P(vals.data_ptr())) == -1
        assert lib.dxo_csr_destroy(ctx._h, None) == -1
    finally:
        dm.close()
        dm2.close()
    bare = DeviceMesh(gdim=2, phi=m.phi, dphi=m.dphi, dpsi=m.dpsi, dofmap=m.dofmap, geom_dofmap=m.geom_dofmap, x=m.x,
                      num_field_nodes=nn, ctx=ctx)
    try:
        pat = bare.csr_pattern(2)
        assert lib.dxo_bilinear_assemble(ctx._h, bare._h, pat._h, GRAD, GRAD, 2, P(Cd.data_ptr()), P(_zeros(pat.nnz).data_ptr())) == -6
        with pytest.raises(ValueError, match="weights"):
            bare.bilinear_assemble("grad", "grad", 2, Cd.data_ptr(), pat)
    finally:
        bare.close()
    torch.cuda.synchronize()


def test_device_assembled_newton_matches_the_matrix_free_example():
    """examples/device_assembled_newton.py: the tension test with the assembled Jacobian and a direct solve converges quadratically and
    ends where examples/device_hyperelasticity.py (matrix-free CG) ends."""
    import importlib.util
    import pathlib

    def load(name):
        path = pathlib.Path(__file__).resolve().parents[1] / "examples" / f"{name}.py"
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    rep = load("device_assembled_newton").main(12, verbose=False)
    for step in rep["steps"]:
        r = step["newton_residuals"]
        assert r[-1] <= 1e-8 * r[0] and len(r) <= 11, r
        rho = [x / r[0] for x in r]
        assert len(rho) >= 3 and rho[-2] <= 50.0 * rho[-3] ** 2, r
    # the matrix-free example returns no displacement: its final `u` is read from main's frame as main returns
    mf = load("device_hyperelasticity")
    seen = {}

    def grab(frame, event, arg):
        if event == "return" and frame.f_code is mf.main.__code__:
            seen["u"] = frame.f_locals["u"].cpu().numpy()

    sys.setprofile(grab)
    try:
        ref = mf.main(12, verbose=False)
    finally:
        sys.setprofile(None)
    assert [s["max_uy"] for s in ref["steps"]] == pytest.approx([s["max_uy"] for s in rep["steps"]], rel=1e-8)
    u, u_ref = rep["u"], seen["u"]
    assert np.abs(u - u_ref).max() <= 1e-8 * np.abs(u_ref).max()
