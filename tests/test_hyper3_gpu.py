"""The 3-D Isihara operator on the GPU: dxo_isihara3 (array of 3x3 F) and dxo_isihara3_field (F formed in the kernel from the dof
vector of a gdim = 3 mesh) against the autograd reference of tests/hyper3_cases.py, the 2-D golden through the plane-strain embedding,
the factory make_isihara(dim=3), and a Taylor test of the internal force against the tangent action on the device."""
import ctypes as C
import types

import numpy as np
import pytest

import hyper3_cases as H3
from conftest import assert_close_scaled
from dolfinx_external_operator_amd import MEM_DEVICE, MEM_HOST, DeviceMesh, IsiharaParams, make_isihara
from tools.synthetic import gauss_tensor_rule, structured_mesh, with_rule

pytestmark = pytest.mark.gpu

PRM = IsiharaParams(*H3.DEFAULTS)
E_DIM = -2


def run_host(ctx, F):
    n = F.shape[0]
    dP, P = np.full(n * 81, -7.0), np.full(n * 9, -7.0)
    ctx.isihara3(PRM, n, MEM_HOST, np.ascontiguousarray(F), dP, P)
    return dP.reshape(n, 9, 9), P.reshape(n, 9)


def run_device(ctx, F):
    import torch

    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n = F.shape[0]
    Ft = torch.from_numpy(np.ascontiguousarray(F)).cuda()
    dP = torch.full((n * 81,), -7.0, dtype=torch.float64, device="cuda")
    P = torch.full((n * 9,), -7.0, dtype=torch.float64, device="cuda")
    ctx.isihara3(PRM, n, MEM_DEVICE, Ft.data_ptr(), dP.data_ptr(), P.data_ptr())
    return dP.cpu().numpy().reshape(n, 9, 9), P.cpu().numpy().reshape(n, 9)


@pytest.fixture(scope="module")
def reference_1000():
    F = H3.samples(1000)
    P, dP = H3.reference(F)
    for a in (F, P, dP):
        a.setflags(write=False)
    return F, P, dP


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 1000])
def test_plain_call_matches_autograd(ctx, reference_1000, n):
    """Host arrays, tile borders (64), tails with an odd number of points: P and dP to 1e-12 of the scale, the figure the 2-D kernel is
    held to against its oracle (tests/test_icnn.py); the arithmetic differs from autograd's in grouping only."""
    F, P, dP = (a[:n] for a in reference_1000)
    dPg, Pg = run_host(ctx, F)
    print(f"n = {n}: P {H3.rel_err(Pg, P):.2e}, dP {H3.rel_err(dPg, dP):.2e}")
    assert_close_scaled(Pg, P, 1e-12, "P")
    assert_close_scaled(dPg, dP, 1e-12, "dP")
    if n:
        assert np.all(Pg[0] == 0.0)      # the first sample is the identity: stress free, exactly


def test_plane_strain_embedding_equals_the_2d_golden(ctx, golden):
    g = golden("isihara_analytic.npz")
    dPg, Pg = run_host(ctx, H3.embed_plane_strain(g["F"]))
    ip = H3.IN_PLANE
    assert_close_scaled(Pg[:, ip], g["P"], 1e-12, "in-plane P")
    assert_close_scaled(dPg[:, ip][:, :, ip], g["dP"], 1e-12, "in-plane dP")
    assert np.all(Pg[:, H3.SHEAR_OUT] == 0.0)


def test_negative_determinant_gives_nan_in_its_own_row_only(ctx):
    n, bad = 4097, 2077
    F = H3.small_strain(n, seed=21)
    F[bad] = np.diag([-1.0, 1.0, 1.0]).reshape(9)
    dPg, Pg = run_host(ctx, F)
    nan_rows = np.isnan(dPg).reshape(n, -1).all(axis=1) & np.isnan(Pg).all(axis=1)
    any_nan = np.isnan(dPg).reshape(n, -1).any(axis=1) | np.isnan(Pg).any(axis=1)
    assert np.array_equal(np.flatnonzero(nan_rows), [bad]) and np.array_equal(np.flatnonzero(any_nan), [bad])
    keep = np.arange(n) != bad
    P, dP = H3.reference(F[keep])
    assert_close_scaled(Pg[keep], P, 1e-12, "P beside the NaN row")
    assert_close_scaled(dPg[keep], dP, 1e-12, "dP beside the NaN row")


def test_paths_are_bit_identical(ctx):
    """device pointers against host arrays, nontemporal stores against plain ones, a call against its repetition"""
    F = H3.samples(1237)
    saved = ctx.get_option("nontemporal")
    try:
        outs = {}
        for nt in (0, 1):
            ctx.set_option("nontemporal", nt)
            outs[("host", nt)] = run_host(ctx, F)
            outs[("device", nt)] = run_device(ctx, F)
        outs["again"] = run_host(ctx, F)
    finally:
        ctx.set_option("nontemporal", saved)
    first = outs[("host", 0)]
    assert np.isfinite(first[0]).all() and np.isfinite(first[1]).all()
    for key, (dPg, Pg) in outs.items():
        assert np.array_equal(dPg, first[0]) and np.array_equal(Pg, first[1]), key


def test_tangent_has_major_symmetry(ctx, reference_1000):
    dPg, _ = run_host(ctx, reference_1000[0])
    assert np.abs(dPg - dPg.transpose(0, 2, 1)).max() <= 1e-13 * np.abs(dPg).max()


def test_tangent_has_major_symmetry_point_by_point(ctx, reference_1000):
    """the same figure with every point's own max |dP_p| for a scale: the large points of the batch no longer set the tolerance of the
    small ones"""
    dPg, _ = run_host(ctx, reference_1000[0])
    asym = np.abs(dPg - dPg.transpose(0, 2, 1)).reshape(dPg.shape[0], -1).max(axis=1)
    scale = np.abs(dPg).reshape(dPg.shape[0], -1).max(axis=1)
    worst = int(np.argmax(asym / scale))
    print(f"worst point {worst}: {asym[worst] / scale[worst]:.2e} of its own max |dP|")
    assert np.all(asym <= 1e-13 * scale), (worst, asym[worst], scale[worst])


# ------------------------------------------------------------------------------------------------------------ the fused form
def _mesh(name):
    cell, n, degree, rule = {
        "Q2 hexahedra (2,1,2), 8 points": ("hexahedron", (2, 1, 2), 2, None),
        "Q2 hexahedra (3,3,2), 8 points": ("hexahedron", (3, 3, 2), 2, None),
        "Q2 hexahedra (2,1,2), 27 points": ("hexahedron", (2, 1, 2), 2, 3),
        "Q2 hexahedra (3,3,2), 27 points": ("hexahedron", (3, 3, 2), 2, 3),
        "Q1 hexahedra (3,2,3)": ("hexahedron", (3, 2, 3), 1, None),
        "P2 tetrahedra (2,2,1)": ("tetrahedron", (2, 2, 1), 2, None),
        "P1 tetrahedra (3,2,2)": ("tetrahedron", (3, 2, 2), 1, None),
    }[name]
    m = structured_mesh(cell, n, degree, distort=0.2, seed=4)
    if rule:
        m = with_rule(m, *gauss_tensor_rule("hexahedron", rule))
    return m


def _field(m, amplitude, seed):
    """a smooth displacement plus a little noise, |grad u| of the order of `amplitude`"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = m.node_x
    u = amplitude * np.stack([np.sin(2.0 * x[:, 1] + x[:, 2]), np.cos(1.5 * x[:, 0]) * x[:, 2], x[:, 0] * x[:, 1] - 0.5 * x[:, 2] ** 2], axis=1)
    return np.ascontiguousarray((u + 0.05 * amplitude * rng.normal(size=u.shape)).reshape(-1))


MESHES = ["Q2 hexahedra (2,1,2), 8 points", "Q2 hexahedra (3,3,2), 8 points", "Q2 hexahedra (2,1,2), 27 points",
          "Q2 hexahedra (3,3,2), 27 points", "Q1 hexahedra (3,2,3)", "P2 tetrahedra (2,2,1)", "P1 tetrahedra (3,2,2)"]


@pytest.mark.parametrize("name", MESHES)
def test_fused_form_equals_operand_then_plain_call(ctx, name):
    """F formed in the registers of the fused kernel against evaluate("F", 3, u) followed by the plain call: 1e-13 of the scale, the
    2-D fused form's figure (tests/test_round3_fields_gpu.py); host and device memory bit for bit."""
    import torch

    m = _mesh(name)
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    try:
        n = m.num_cells * m.nq
        u = _field(m, 0.15, 9)
        F = dm.evaluate("F", 3, u).reshape(n, 9)
        assert H3.det_rows(F).min() > 0.2 and np.abs(F - H3.EYE).max() > 0.05
        dP0, P0 = run_host(ctx, F)
        dP1, P1 = np.full(n * 81, -7.0), np.full(n * 9, -7.0)
        ctx.isihara3_field(PRM, dm._h, MEM_HOST, u, dP1, P1)
        print(f"{name}: n = {n}, P {H3.rel_err(P1, P0.reshape(-1)):.2e}, dP {H3.rel_err(dP1, dP0.reshape(-1)):.2e}")
        assert_close_scaled(dP1, dP0, 1e-13, "fused dP")
        assert_close_scaled(P1, P0, 1e-13, "fused P")
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ut = torch.from_numpy(u).cuda()
        dP2 = torch.full((n * 81,), -7.0, dtype=torch.float64, device="cuda")
        P2 = torch.full((n * 9,), -7.0, dtype=torch.float64, device="cuda")
        ctx.isihara3_field(PRM, dm._h, MEM_DEVICE, ut.data_ptr(), dP2.data_ptr(), P2.data_ptr())
        assert np.array_equal(dP2.cpu().numpy(), dP1) and np.array_equal(P2.cpu().numpy(), P1)
    finally:
        dm.close()


def test_fused_form_in_chunks_of_the_host_pipeline(ctx):
    """the host pipeline's chunked ring (cells in chunks, the last one partial) writes what one launch writes"""
    m = structured_mesh("tetrahedron", (4, 3, 3), 2, distort=0.2, seed=4)      # 216 cells, 864 points
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    try:
        n = m.num_cells * m.nq
        u = _field(m, 0.15, 9)
        dP1, P1 = np.empty(n * 81), np.empty(n * 9)
        ctx.isihara3_field(PRM, dm._h, MEM_HOST, u, dP1, P1)
        saved = ctx.get_option("host_chunk_points")
        ctx.set_option("host_chunk_points", 300)
        try:
            dP2, P2 = np.empty(n * 81), np.empty(n * 9)
            ctx.isihara3_field(PRM, dm._h, MEM_HOST, u, dP2, P2)
            F = dm.evaluate("F", 3, u).reshape(n, 9)
            dP3, P3 = run_host(ctx, F)
        finally:
            ctx.set_option("host_chunk_points", saved)
        assert np.array_equal(dP2, dP1) and np.array_equal(P2, P1)
        assert_close_scaled(dP1, dP3, 1e-13, "chunked plain dP")
        assert_close_scaled(P1, P3, 1e-13, "chunked plain P")
    finally:
        dm.close()


def test_a_2d_mesh_is_refused_with_e_dim(ctx, hip_library):
    m = structured_mesh("triangle", (2, 2), 2, distort=0.0, seed=0)
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    try:
        u, dP, P = np.zeros(m.node_x.shape[0] * 2), np.empty(m.num_cells * m.nq * 81), np.empty(m.num_cells * m.nq * 9)
        rc = hip_library.dxo_isihara3_field(ctx._h, C.byref(PRM), dm._h, MEM_HOST, u.ctypes.data, dP.ctypes.data, P.ctypes.data)
        assert rc == E_DIM
        with pytest.raises(ValueError, match="DXO_E_DIM"):
            ctx.isihara3_field(PRM, dm._h, MEM_HOST, u, dP, P)
    finally:
        dm.close()


def test_bad_arguments_answer_as_the_2d_twins(ctx, hip_library):
    """NULL params, n < 0, bad mem, NULL arrays, misaligned pointers: the code of the 2-D entry point given the same call, and that
    code is the documented one"""
    lib, h = hip_library, ctx._h
    buf = np.zeros(4096)
    base = (buf.ctypes.data + 15) & ~15
    want = {"NULL params": -1, "NULL mesh": -1, "n < 0": -3, "bad mem": -4, "NULL F": -1, "NULL dP": -1, "NULL P": -1, "NULL u": -1}
    b = types.SimpleNamespace(prm=C.byref(PRM), F=base, dP=base + 4096, P=base + 16384, u=base, mesh=None)
    for name, args in H3.plain_bad_calls(b):
        rc2, rc3 = lib.dxo_isihara(h, *args), lib.dxo_isihara3(h, *args)
        assert rc3 == rc2 == want.get(name, -5), (name, rc2, rc3)
    m2 = structured_mesh("triangle", (2, 2), 2, distort=0.0, seed=0)
    m3 = structured_mesh("tetrahedron", (1, 1, 1), 2, distort=0.0, seed=0)
    d2, d3 = DeviceMesh.from_synthetic(m2, ctx=ctx), DeviceMesh.from_synthetic(m3, ctx=ctx)
    try:
        b2, b3 = types.SimpleNamespace(**vars(b)), types.SimpleNamespace(**vars(b))
        b2.mesh, b3.mesh = d2._h, d3._h
        for (name, a2), (_, a3) in zip(H3.field_bad_calls(b2), H3.field_bad_calls(b3)):
            rc2, rc3 = lib.dxo_isihara_field(h, *a2), lib.dxo_isihara3_field(h, *a3)
            assert rc3 == rc2 == want.get(name, -5), (name, rc2, rc3)
    finally:
        d2.close()
        d3.close()


# ------------------------------------------------------------------------------------------------------------ the factory
def test_factory_dim3(ctx, golden):
    import torch

    m = _mesh("P2 tetrahedra (2,2,1)")
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    try:
        n = m.num_cells * m.nq
        u = _field(m, 0.15, 9)
        isi = make_isihara(ctx=ctx, dim=3)
        Fvals = dm.operand("F", u).eval(None)
        assert Fvals.shape == (m.num_cells, m.nq, 3, 3)
        dP0, P0 = isi((1,))(Fvals)
        assert isinstance(dP0, np.ndarray) and dP0.shape == (n * 81,) and P0.shape == (n * 9,)
        dPt, Pt = isi((1,))(torch.from_numpy(np.ascontiguousarray(Fvals)).cuda())
        assert dPt.is_cuda and dPt.shape == (n * 81,) and Pt.shape == (n * 9,)
        assert np.array_equal(dPt.cpu().numpy(), dP0) and np.array_equal(Pt.cpu().numpy(), P0)
        lazy = dm.operand("F", u, lazy=True).eval(None)
        dP1, P1 = isi((1,))(lazy)
        assert lazy._value is None           # the fused path: the operand was never evaluated on its own
        assert dP1.shape == (n * 81,) and P1.shape == (n * 9,)
        assert_close_scaled(dP1, dP0, 1e-13, "lazy dP")
        assert_close_scaled(P1, P0, 1e-13, "lazy P")
        P, dP = H3.reference(np.asarray(Fvals).reshape(n, 9))
        assert_close_scaled(P0, P.reshape(-1), 1e-12, "factory P")
        assert_close_scaled(dP0, dP.reshape(-1), 1e-12, "factory dP")
        with pytest.raises(NotImplementedError):
            isi((0,))
        with pytest.raises(ValueError):
            make_isihara(ctx=ctx, dim=3, device_outputs="arena")
        with pytest.raises(ValueError):
            make_isihara(ctx=ctx, dim=2)((1,))(lazy)        # a 3-D operand for the plane-strain operator
        m2 = structured_mesh("triangle", (2, 2), 2, distort=0.0, seed=0)
        d2 = DeviceMesh.from_synthetic(m2, ctx=ctx)
        try:
            with pytest.raises(ValueError):
                isi((1,))(d2.operand("F", np.zeros(m2.node_x.shape[0] * 2), lazy=True).eval(None))
        finally:
            d2.close()
        # the default is the plane-strain operator of before, bit for bit
        g = golden("isihara_analytic.npz")
        F2 = np.ascontiguousarray(g["F"][:300])
        dPa, Pa = make_isihara(ctx=ctx)((1,))(F2)
        dPb, Pb = np.empty(300 * 16), np.empty(300 * 4)
        ctx.isihara(PRM, 300, MEM_HOST, F2, dPb, Pb)
        assert dPa.shape == (300 * 16,) and np.array_equal(dPa, dPb) and np.array_equal(Pa, Pb)
    finally:
        dm.close()


# ------------------------------------------------------------------------------------------------------------ end to end
def test_taylor_remainder_of_the_internal_force_is_second_order(ctx):
    """R(u) = adjoint("F", 3, P(u)), K v = bilinear_apply("grad", "grad", 3, dP(u), v): |R(u + h v) - R(u) - h K v| = O(h^2). Observed
    order >= 1.9 between h = 1e-2, 5e-3, 2.5e-3 (the limit is 2; rounding is far below the remainder at these steps)."""
    import torch

    m = _mesh("P2 tetrahedra (2,2,1)")
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    saved = ctx.get_option("consumer_overwrite")
    try:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_option("consumer_overwrite", 1)
        nn, n = m.node_x.shape[0], m.num_cells * m.nq
        rng = np.random.Generator(np.random.PCG64(17))
        f64 = dict(dtype=torch.float64, device="cuda")
        u = torch.from_numpy(0.02 * rng.uniform(-1.0, 1.0, nn * 3)).cuda()
        v = torch.from_numpy(rng.uniform(-1.0, 1.0, nn * 3)).cuda()
        dP, P, dPs = torch.zeros(n * 81, **f64), torch.zeros(n * 9, **f64), torch.zeros(n * 81, **f64)

        def force(w, tangent):
            R = torch.zeros(nn * 3, **f64)
            ctx.isihara3_field(PRM, dm._h, MEM_DEVICE, w.data_ptr(), tangent.data_ptr(), P.data_ptr())
            dm.adjoint("F", 3, P.data_ptr(), R.data_ptr())
            return R

        R0 = force(u, dP)
        Kv = torch.zeros(nn * 3, **f64)
        dm.bilinear_apply("grad", "grad", 3, dP.data_ptr(), v.data_ptr(), Kv.data_ptr())
        assert float(torch.linalg.norm(Kv)) > 0
        hs = [1e-2, 5e-3, 2.5e-3]
        rem = [float(torch.linalg.norm(force(u + h * v, dPs) - R0 - h * Kv)) for h in hs]
        orders = [np.log(rem[k] / rem[k + 1]) / np.log(hs[k] / hs[k + 1]) for k in range(2)]
        print("remainders", rem, "orders", orders)
        assert min(orders) >= 1.9, (rem, orders)
    finally:
        ctx.set_option("consumer_overwrite", saved)
        dm.close()
