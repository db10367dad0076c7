"""dxo_bilinear_apply / dxo_bilinear_diagonal on the device: the action and the diagonal of the bilinear form of a pair of linear
operand kinds with a per-point block C (the hyperelastic Jacobian with C = dP/dF, the heat Jacobian with C = [dq/dT | dq/dsigma]),
against the NumPy composition pinned in tests/test_bilinear_oracle_cpu.py and against the device's own residuals."""
import ctypes as C

import numpy as np
import pytest

from oracle.form_oracle import bilinear_diag_ref, bilinear_ref, diagonal_by_probes, node_colours
from solver_cases import CELLS, PAIRS, _cuda, _value_size, _zeros
from tools.synthetic import structured_mesh

pytestmark = pytest.mark.gpu


def device_apply(ctx, dm, test, trial, bs, Cd, v, n):
    import torch

    vd, out = _cuda(v), _zeros(n)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    dm.bilinear_apply(test, trial, bs, Cd.data_ptr(), vd.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def device_diag(ctx, dm, test, trial, bs, Cd, n):
    import torch

    out = _zeros(n)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    dm.bilinear_diagonal(test, trial, bs, Cd.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("degree", [1, 2])
def test_every_pair_matches_the_composed_oracle(ctx, cell, degree):
    from dolfinx_external_operator_amd import DeviceMesh

    m = structured_mesh(cell, CELLS[cell], degree, distort=0.2, seed=7)
    G, nn = m.gdim, m.node_x.shape[0]
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    rng = np.random.Generator(np.random.PCG64(11))
    colour = node_colours(m)
    try:
        for test, trial, vector in PAIRS:
            bs = G if vector else 1
            n = nn * bs
            Cb = rng.normal(size=(m.num_cells * m.nq, _value_size(test, G, bs), _value_size(trial, G, bs)))
            Cd = _cuda(Cb)
            v = rng.normal(size=n)
            got, ref = device_apply(ctx, dm, test, trial, bs, Cd, v, n), bilinear_ref(m, test, trial, bs, Cb, v)
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (test, trial, bs, np.abs(got - ref).max())
            dg = device_diag(ctx, dm, test, trial, bs, Cd, n)
            dref = bilinear_diag_ref(m, test, trial, bs, Cb)
            assert np.abs(dg - dref).max() <= 1e-12 * np.abs(dref).max(), (test, trial, bs)
            if n <= 200:      # and e_i . K e_i through the device's own action, one colour at a time
                probe = diagonal_by_probes(lambda x: device_apply(ctx, dm, test, trial, bs, Cd, x, n), nn, bs, colour)
                assert np.abs(dg - probe).max() <= 1e-12 * np.abs(probe).max(), (test, trial, bs)
    finally:
        dm.close()


@pytest.mark.parametrize("cell,n", [("triangle", (4, 3)), ("hexahedron", (2, 1, 2)), ("tetrahedron", (2, 2, 1))])
def test_eps_pair_agrees_with_tangent_apply(ctx, cell, n):
    """("eps", "eps", gdim) on the C_tang dxo_von_mises_field writes is dxo_tangent_apply / dxo_tangent_diagonal."""
    import torch

    from dolfinx_external_operator_amd import DeviceMesh, VmParams

    m = structured_mesh(cell, n, 2, distort=0.2, seed=3)
    G, nn = m.gdim, m.node_x.shape[0]
    d = 4 if G == 2 else 6
    npts = m.num_cells * m.nq
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    rng = np.random.Generator(np.random.PCG64(3))
    try:
        E = 70e3
        prm = VmParams(E, 0.3, 250.0, E * (E / 100) / (E - E / 100))
        u = 4e-3 * rng.normal(size=nn * G)
        C_tang, sigma, dp = np.zeros(npts * d * d), np.zeros(npts * d), np.zeros(npts)
        dm.von_mises(prm, u, np.zeros(npts * d), np.zeros(npts), C_tang, sigma, dp)
        assert (dp > 0).mean() > 0.1                        # a tangent with plastic points
        Cd, v = _cuda(C_tang), rng.normal(size=nn * G)
        vd, a, b = _cuda(v), _zeros(nn * G), _zeros(nn * G)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        dm.tangent_apply(Cd.data_ptr(), vd.data_ptr(), a.data_ptr())
        dm.bilinear_apply("eps", "eps", G, Cd.data_ptr(), vd.data_ptr(), b.data_ptr())
        da, db = _zeros(nn * G), _zeros(nn * G)
        dm.tangent_diagonal(Cd.data_ptr(), da.data_ptr())
        dm.bilinear_diagonal("eps", "eps", G, Cd.data_ptr(), db.data_ptr())
        torch.cuda.synchronize()
        assert float((a - b).abs().max()) <= 1e-13 * float(a.abs().max())
        assert float((da - db).abs().max()) <= 1e-13 * float(da.abs().max())
    finally:
        dm.close()


def test_hyperelastic_jacobian_is_the_derivative_of_the_device_residual(ctx):
    """K v with C = dP/dF of dxo_isihara_field is the central difference of R(u) = adjoint("F", 2, P(u)); and w . K v = v . K w."""
    import torch

    from dolfinx_external_operator_amd import MEM_DEVICE, DeviceMesh, IsiharaParams

    m = structured_mesh("triangle", (6, 6), 2, distort=0.2, seed=9)
    nn, npts = m.node_x.shape[0], m.num_cells * m.nq
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    prm = IsiharaParams(0.5, 1.0, 1.0, 1.5)
    rng = np.random.Generator(np.random.PCG64(9))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        dP, P = _zeros(npts * 16), _zeros(npts * 4)

        def residual(u):
            R = _zeros(nn * 2)
            ctx.isihara_field(prm, dm._h, MEM_DEVICE, u.data_ptr(), dP.data_ptr(), P.data_ptr())
            dm.adjoint("F", 2, P.data_ptr(), R.data_ptr())
            return R

        u = _cuda(0.01 * rng.normal(size=nn * 2))
        v, w = _cuda(rng.normal(size=nn * 2)), _cuda(rng.normal(size=nn * 2))
        h = 1e-6
        fd = (residual(u + h * v) - residual(u - h * v)) / (2 * h)
        residual(u)                                          # dP at u
        assert not torch.isnan(dP).any()
        Kv, Kw = _zeros(nn * 2), _zeros(nn * 2)
        dm.bilinear_apply("grad", "grad", 2, dP.data_ptr(), v.data_ptr(), Kv.data_ptr())
        dm.bilinear_apply("grad", "grad", 2, dP.data_ptr(), w.data_ptr(), Kw.data_ptr())
        torch.cuda.synchronize()
        assert float((Kv - fd).abs().max()) <= 1e-7 * float(Kv.abs().max())
        a, b = float(torch.dot(w, Kv)), float(torch.dot(v, Kw))
        assert abs(a - b) <= 1e-12 * abs(a)
    finally:
        dm.close()


def test_heat_jacobian_on_the_demo_setting(ctx):
    """Unit square 10 x 10, P1, degree-2 rule, T = x^2 + y (demo_nonlinear_heat_equation_part2.py): with [dq/dT | dq/dsigma] from
    dxo_heat_field, ("grad", "value_grad", 1) is the explicit Jacobian form and the derivative of the device residual adjoint("grad", 1, q)."""
    import torch

    from dolfinx_external_operator_amd import MEM_DEVICE, DeviceMesh
    from oracle.operand_oracle import GRAD, VALUE, eval_operand, operand_adjoint

    m = structured_mesh("triangle", (10, 10), 1)
    nn, npts = m.node_x.shape[0], m.num_cells * m.nq
    A, B = 1.0, 1.0
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.Generator(np.random.PCG64(10))
    try:
        q, dqdT, dqds = _zeros(npts * 2), _zeros(npts * 2), _zeros(npts * 4)

        def residual(T):
            R = _zeros(nn)
            dm.heat(A, B, T.data_ptr(), q.data_ptr(), dqdT.data_ptr(), dqds.data_ptr(), mem=MEM_DEVICE)
            dm.adjoint("grad", 1, q.data_ptr(), R.data_ptr())
            return R

        Tn = m.node_x[:, 0] ** 2 + m.node_x[:, 1]
        T, That = _cuda(Tn), rng.normal(size=nn)
        h = 1e-6
        fd = (residual(T + h * _cuda(That)) - residual(T - h * _cuda(That))) / (2 * h)
        residual(T)
        Cd = torch.cat([dqdT.reshape(npts, 2, 1), dqds.reshape(npts, 2, 2)], dim=2).contiguous().reshape(-1)   # [g][1 + g]
        act = device_apply(ctx, dm, "grad", "value_grad", 1, Cd, That, nn)
        tab = (m.dofmap, m.geom_dofmap, m.x, m.phi, m.dphi, m.dpsi)
        Tq, s = eval_operand(VALUE, 1, Tn, *tab), eval_operand(GRAD, 1, Tn, *tab)
        k = 1.0 / (A + B * Tq)
        S = B * k ** 2 * s * eval_operand(VALUE, 1, That, *tab) - k * eval_operand(GRAD, 1, That, *tab)     # part2.py:328-329
        manual = operand_adjoint(GRAD, 1, S, m.weights, *tab, nn)
        assert np.abs(act - manual).max() <= 1e-12 * np.abs(manual).max()
        assert np.abs(act - fd.cpu().numpy()).max() <= 1e-7 * np.abs(act).max()
    finally:
        dm.close()


def test_reproducible_overwrite_atomics_and_graph_capture(ctx):
    import torch

    from dolfinx_external_operator_amd import DeviceMesh

    m = structured_mesh("triangle", (8, 8), 2, distort=0.2, seed=12)
    nn, npts = m.node_x.shape[0], m.num_cells * m.nq
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    rng = np.random.Generator(np.random.PCG64(12))
    Cd, vd = _cuda(rng.normal(size=npts * 16)), _cuda(rng.normal(size=nn * 2))
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            ctx.set_stream(stream.cuda_stream)
            a, b = _zeros(nn * 2), _zeros(nn * 2)
            dm.bilinear_apply("grad", "grad", 2, Cd.data_ptr(), vd.data_ptr(), a.data_ptr())
            dm.bilinear_apply("grad", "grad", 2, Cd.data_ptr(), vd.data_ptr(), b.data_ptr())
            stream.synchronize()
            assert torch.equal(a, b)                                       # bit-reproducible
            acc = a.clone()
            dm.bilinear_apply("grad", "grad", 2, Cd.data_ptr(), vd.data_ptr(), acc.data_ptr())
            stream.synchronize()
            assert torch.equal(acc, a + a)                                 # default: accumulate
            ctx.set_option("consumer_overwrite", 1)
            try:
                c = torch.full((nn * 2,), 1e30, dtype=torch.float64, device="cuda")
                dm.bilinear_apply("grad", "grad", 2, Cd.data_ptr(), vd.data_ptr(), c.data_ptr())
                dd = torch.full((nn * 2,), 1e30, dtype=torch.float64, device="cuda")
                dm.bilinear_diagonal("grad", "grad", 2, Cd.data_ptr(), dd.data_ptr())
                d0 = _zeros(nn * 2)
                stream.synchronize()
            finally:
                ctx.set_option("consumer_overwrite", 0)
            assert torch.equal(c, a)                                       # SET semantics
            dm.bilinear_diagonal("grad", "grad", 2, Cd.data_ptr(), d0.data_ptr())
            ctx.set_option("adjoint_atomics", 1)
            try:
                at = _zeros(nn * 2)
                dm.bilinear_apply("grad", "grad", 2, Cd.data_ptr(), vd.data_ptr(), at.data_ptr())
                stream.synchronize()
            finally:
                ctx.set_option("adjoint_atomics", 0)
            assert torch.equal(dd, d0)
            assert float((at - a).abs().max()) <= 1e-13 * float(a.abs().max())
        torch.cuda.current_stream().wait_stream(stream)
        # a matvec captured once (after the warm calls above) replays equal to the eager result
        out = _zeros(nn * 2)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            out.zero_()
            dm.bilinear_apply("grad", "grad", 2, Cd.data_ptr(), vd.data_ptr(), out.data_ptr())
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a)
    finally:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        dm.close()


def test_error_paths(ctx):
    import torch

    from dolfinx_external_operator_amd import DeviceMesh
    from oracle.operand_oracle import DEFGRAD, GRAD, VALUE

    m = structured_mesh("triangle", (2, 2), 2)
    nn, npts = m.node_x.shape[0], m.num_cells * m.nq
    Cd, vd, out = _zeros(npts * 16), _zeros(nn * 2), _zeros(nn * 2)
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    try:
        with pytest.raises(ValueError, match="unsupported pair"):
            dm.bilinear_apply("grad", "eps", 2, Cd.data_ptr(), vd.data_ptr(), out.data_ptr())
        with pytest.raises(ValueError, match="unsupported pair"):
            dm.bilinear_diagonal("detF", "detF", 2, Cd.data_ptr(), out.data_ptr())
        lib = ctx.lib
        P = C.c_void_p
        # the library refuses on its own, with a message: a pair outside the table, a nonlinear kind, F with bs = 1
        for t, r, bs in ((GRAD, VALUE, 1), (5, 5, 2), (GRAD, 7, 1), (DEFGRAD, DEFGRAD, 1)):
            rc = lib.dxo_bilinear_apply(ctx._h, dm._h, t, r, bs, P(Cd.data_ptr()), P(vd.data_ptr()), P(out.data_ptr()))
            assert rc == -6, (t, r, bs)
            assert "dxo_bilinear_apply" in lib.dxo_last_error(ctx._h).decode()
            assert lib.dxo_bilinear_diagonal(ctx._h, dm._h, t, r, bs, P(Cd.data_ptr()), P(out.data_ptr())) == -6
        # C must be 16-byte aligned
        rc = lib.dxo_bilinear_apply(ctx._h, dm._h, GRAD, GRAD, 2, P(Cd.data_ptr() + 8), P(vd.data_ptr()), P(out.data_ptr()))
        assert rc == -5
    finally:
        dm.close()
    bare = DeviceMesh(gdim=2, phi=m.phi, dphi=m.dphi, dpsi=m.dpsi, dofmap=m.dofmap, geom_dofmap=m.geom_dofmap, x=m.x,
                      num_field_nodes=nn, ctx=ctx)
    try:
        with pytest.raises(ValueError, match="weights"):
            bare.bilinear_apply("grad", "grad", 2, Cd.data_ptr(), vd.data_ptr(), out.data_ptr())
        with pytest.raises(ValueError, match="weights"):
            bare.bilinear_diagonal("grad", "grad", 2, Cd.data_ptr(), out.data_ptr())
    finally:
        bare.close()
    torch.cuda.synchronize()


def test_device_hyperelasticity_converges_quadratically():
    """examples/device_hyperelasticity.py: the tension test with (dP, P) from dxo_isihara_field, the residual from dxo_operand_adjoint and
    the Newton step solved with K v = dxo_bilinear_apply. Newton converges quadratically only if the action IS the derivative of the
    residual's stress."""
    import importlib.util
    import pathlib

    path = pathlib.Path(__file__).resolve().parents[1] / "examples" / "device_hyperelasticity.py"
    spec = importlib.util.spec_from_file_location("hyper_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rep = mod.main(16, verbose=False)
    for step in rep["steps"]:
        r = step["newton_residuals"]
        assert r[-1] <= 1e-8 * r[0] and len(r) <= 11, r
        rho = [x / r[0] for x in r]
        assert len(rho) >= 3 and rho[-2] <= 50.0 * rho[-3] ** 2, r
