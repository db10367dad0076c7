"""The 3-D network operator on the GPU: dxo_icnn3_eval (array of 3x3 F), dxo_icnn3_field (F from the dof vector of a gdim = 3 mesh),
dxo_icnn3_correction and make_icnn(dim=3) against the reference of tests/icnn3_cases.py, the reference's own 2-D golden through the
plane-strain embedding, the analytic 3-D kernel with the network's hidden path switched off, and a Taylor test of the internal force."""
import ctypes as C
import types

import numpy as np
import pytest

import hyper3_cases as H3
import icnn3_cases as I3
from conftest import assert_close_scaled
from dolfinx_external_operator_amd import MEM_DEVICE, MEM_HOST, DeviceMesh, IsiharaParams, make_icnn
from oracle.icnn_oracle import softplus
from tools.synthetic import structured_mesh

from test_hyper3_gpu import MESHES, _field, _mesh

pytestmark = pytest.mark.gpu

DEFAULT_VARIANT = 2
RTOL_FP32 = 2e-6        # the project's bound for the same network core against its oracle (tests/test_icnn.py)
RTOL_FP64 = 1e-11       # the bound of test_fp64_network_variant_tolerance_study
E_DIM, E_OPTION = -2, -6


@pytest.fixture(scope="module")
def weights(golden):
    return dict(golden("icnn_isihara_weights.npz"))


@pytest.fixture(scope="module")
def model(ctx, weights):
    m = ctx.icnn_create(I3.state_dict(weights))
    yield m
    ctx.icnn_destroy(m)


@pytest.fixture(scope="module")
def oracle_1000(weights):
    """small_strain(1000) through the oracle with the fp32 and with the fp64 network, computed once"""
    F = I3.small_strain(1000)
    out = {"F": F}
    for prec, dt in ((0, np.float32), (1, np.float64)):
        out[prec] = I3.icnn3_stress_tangent(F, weights, net_dtype=dt)
    for v in out.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
    return out


def run_host(ctx, model, F, precision=0, pad=0):
    n = F.shape[0]
    dP, P = np.full(n * 81 + pad, -7.0), np.full(n * 9 + pad, -7.0)
    ctx.icnn3_eval(model, precision, n, MEM_HOST, np.ascontiguousarray(F), dP, P)
    assert np.all(dP[n * 81:] == -7.0) and np.all(P[n * 9:] == -7.0)
    return dP[: n * 81].reshape(n, 9, 9), P[: n * 9].reshape(n, 9)


def run_device(ctx, model, F, precision=0):
    import torch

    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n = F.shape[0]
    Ft = torch.from_numpy(np.ascontiguousarray(F)).cuda()
    dP = torch.full((n * 81 + 8,), -7.0, dtype=torch.float64, device="cuda")
    P = torch.full((n * 9 + 8,), -7.0, dtype=torch.float64, device="cuda")
    ctx.icnn3_eval(model, precision, n, MEM_DEVICE, Ft.data_ptr(), dP.data_ptr(), P.data_ptr())
    dP, P = dP.cpu().numpy(), P.cpu().numpy()
    assert np.all(dP[n * 81:] == -7.0) and np.all(P[n * 9:] == -7.0)
    return dP[: n * 81].reshape(n, 9, 9), P[: n * 9].reshape(n, 9)


class variant:
    """ctx option icnn_variant (and the default kernel's store form) for a block, restored afterwards"""

    def __init__(self, ctx, v, store=None):
        self.ctx, self.v, self.store = ctx, v, store

    def __enter__(self):
        self.saved = self.ctx.get_option("icnn3_store")
        self.ctx.set_option("icnn_variant", self.v)
        if self.store is not None:
            self.ctx.set_option("icnn3_store", self.store)

    def __exit__(self, *exc):
        self.ctx.set_option("icnn_variant", DEFAULT_VARIANT)
        self.ctx.set_option("icnn3_store", self.saved)


KERNELS = [(0, None), (1, None), (2, 0), (2, 1)]      # (icnn_variant, icnn3_store): the default kernel with both store forms
KERNEL_IDS = ["variant 0", "variant 1", "variant 2 rows", "variant 2 staged"]


# ------------------------------------------------------------------------------------------------ 1. plain host call against the oracle
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 129, 513, 1000])
def test_fp64_network_matches_the_oracle(ctx, model, oracle_1000, n):
    dPo, Po = (a[:n] for a in oracle_1000[1])
    dPg, Pg = run_host(ctx, model, oracle_1000["F"][:n], precision=1, pad=8)
    print(f"n = {n}: P {H3.rel_err(Pg, Po):.2e}, dP {H3.rel_err(dPg, dPo):.2e}")
    assert_close_scaled(Pg, Po, RTOL_FP64, "P")
    assert_close_scaled(dPg, dPo, RTOL_FP64, "dP")


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 129, 513, 1000])
def test_fp32_network_matches_the_oracle(ctx, model, oracle_1000, n, kernel):
    """a lone lane, the half-wave ownership at 32, the wave at 64, the workgroup at 512; canaries behind both outputs"""
    dPo, Po = (a[:n] for a in oracle_1000[0])
    with variant(ctx, *kernel):
        dPg, Pg = run_host(ctx, model, oracle_1000["F"][:n], pad=8)
    print(f"n = {n}, {kernel}: P {H3.rel_err(Pg, Po):.2e}, dP {H3.rel_err(dPg, dPo):.2e}")
    assert_close_scaled(Pg, Po, RTOL_FP32, "P")
    assert_close_scaled(dPg, dPo, RTOL_FP32, "dP")


# ------------------------------------------------------------------------------------------------ 2. beyond one pass of the persistent grid
def test_more_tiles_than_the_persistent_grid_holds(ctx, model, weights):
    n = 512 * ctx.device_info()["compute_units"] + 65
    F = I3.small_strain(n, seed=23)
    out = {}
    for kernel, name in zip(KERNELS, KERNEL_IDS):
        with variant(ctx, *kernel):
            out[name] = run_device(ctx, model, F)
    for name in KERNEL_IDS[1:]:
        print(f"{name} against variant 0: P {H3.rel_err(out[name][1], out['variant 0'][1]):.2e}, dP {H3.rel_err(out[name][0], out['variant 0'][0]):.2e}")
        assert_close_scaled(out[name][1], out["variant 0"][1], RTOL_FP32, name + " P")
        assert_close_scaled(out[name][0], out["variant 0"][0], RTOL_FP32, name + " dP")
    # the two store forms of the default kernel share the network and the fp64 formulas; the compiler contracts them into fused
    # multiply-adds differently in the two epilogues: fp64 rounding of a few terms, 1e-13 of the scale (the symmetry test's figure)
    assert_close_scaled(out["variant 2 staged"][1], out["variant 2 rows"][1], 1e-13, "staged against rows, P")
    assert_close_scaled(out["variant 2 staged"][0], out["variant 2 rows"][0], 1e-13, "staged against rows, dP")
    pick = np.arange(0, n, 131)
    dPo, Po = I3.icnn3_stress_tangent(F[pick], weights)
    scale_P, scale_dP = np.abs(out["variant 0"][1]).max(), np.abs(out["variant 0"][0]).max()
    for name in KERNEL_IDS:
        assert np.abs(out[name][1][pick] - Po).max() <= RTOL_FP32 * scale_P, name
        assert np.abs(out[name][0][pick] - dPo).max() <= RTOL_FP32 * scale_dP, name


# ------------------------------------------------------------------------------------------------ 3. the reference pin
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_plane_strain_embedding_equals_the_reference_golden(ctx, model, golden, kernel):
    """the golden's P and dP were produced by the reference's own code for 2x2 F: the embedded 3x3 F must return them in plane"""
    g = golden("icnn_isihara.npz")
    with variant(ctx, *kernel):
        dPg, Pg = run_host(ctx, model, H3.embed_plane_strain(g["F"]))
    ip = H3.IN_PLANE
    print(f"{kernel}: in-plane P {H3.rel_err(Pg[:, ip], g['P']):.2e}, dP {H3.rel_err(dPg[:, ip][:, :, ip], g['dP']):.2e}")
    assert_close_scaled(Pg[:, ip], g["P"], RTOL_FP32, "in-plane P")
    assert_close_scaled(dPg[:, ip][:, :, ip], g["dP"], RTOL_FP32, "in-plane dP")
    assert np.all(Pg[:, H3.SHEAR_OUT] == 0.0)


# ------------------------------------------------------------------------------------------------ 4. hidden path off, fp64
def test_hidden_path_off_equals_the_analytic_3d_kernel(ctx, weights):
    w = dict(weights)
    w["layers__3__weights"] = np.full_like(weights["layers__3__weights"], -100.0)
    a, b, c = (float(v) for v in softplus(weights["skip_layers__3__weights"].astype(np.float64))[0])
    F = I3.moderate(500)
    m = ctx.icnn_create(I3.state_dict(w))
    try:
        dPg, Pg = run_host(ctx, m, F, precision=1)
    finally:
        ctx.icnn_destroy(m)
    dPa, Pa = np.empty(500 * 81), np.empty(500 * 9)
    ctx.isihara3(IsiharaParams(a, b, 0.0, c), 500, MEM_HOST, F, dPa, Pa)
    print(f"P {H3.rel_err(Pg, Pa.reshape(500, 9)):.2e}, dP {H3.rel_err(dPg, dPa.reshape(500, 9, 9)):.2e}")
    assert_close_scaled(Pg, Pa, RTOL_FP64, "P")
    assert_close_scaled(dPg, dPa, RTOL_FP64, "dP")


# ------------------------------------------------------------------------------------------------ 5. inverted and singular F
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_inverted_points_are_finite_and_match_the_oracle(ctx, model, weights, kernel):
    F = I3.inverted(200)
    dPo, Po = I3.icnn3_stress_tangent(F, weights)
    assert np.isfinite(dPo).all() and np.isfinite(Po).all()
    with variant(ctx, *kernel):
        dPg, Pg = run_host(ctx, model, F)
    assert np.isfinite(dPg).all() and np.isfinite(Pg).all()
    assert_close_scaled(Pg, Po, RTOL_FP32, "P")
    assert_close_scaled(dPg, dPo, RTOL_FP32, "dP")


@pytest.mark.parametrize("kernel", KERNELS + [(0, "fp64")], ids=KERNEL_IDS + ["fp64 network"])
def test_singular_and_nan_rows_stay_in_their_own_rows(ctx, model, kernel):
    """det F = 0 and NaN at lanes 0, 31, 32 and 63 of the second tile: every other row bit for bit as in the batch where those rows are the identity"""
    n = 3 * 64 + 5
    F = I3.small_strain(n, seed=29)
    singular = np.array([1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 0.0, 1.0, 1.0])          # second row twice the first
    bad = {64: singular, 64 + 31: np.full(9, np.nan), 64 + 32: singular, 64 + 63: np.full(9, np.nan)}
    Fb, Fc = F.copy(), F.copy()
    for i, v in bad.items():
        Fb[i], Fc[i] = v, H3.EYE
    precision = 1 if kernel[1] == "fp64" else 0
    with variant(ctx, kernel[0], None if kernel[1] == "fp64" else kernel[1]):
        (dPb, Pb), (dPc, Pc) = run_host(ctx, model, Fb, precision), run_host(ctx, model, Fc, precision)
    good = np.ones(n, dtype=bool)
    good[list(bad)] = False
    assert np.isfinite(dPc).all() and np.isfinite(Pc).all()
    assert np.array_equal(dPb[good], dPc[good]) and np.array_equal(Pb[good], Pc[good])
    for i in bad:
        assert not np.isfinite(dPb[i]).all() or not np.isfinite(Pb[i]).all(), i


# ------------------------------------------------------------------------------------------------ 6. paths
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_paths_are_bit_identical(ctx, model, kernel):
    """host arrays, device pointers, and a host call forced into several chunks of the pipeline"""
    F = I3.small_strain(1237, seed=31)
    saved = ctx.get_option("host_chunk_points")
    with variant(ctx, *kernel):
        first = run_host(ctx, model, F)
        dev = run_device(ctx, model, F)
        try:
            ctx.set_option("host_chunk_points", 300)
            chunked = run_host(ctx, model, F)
        finally:
            ctx.set_option("host_chunk_points", saved)
        again = run_host(ctx, model, F)
    assert np.isfinite(first[0]).all() and np.isfinite(first[1]).all()
    for name, (dPg, Pg) in (("device", dev), ("chunked", chunked), ("again", again)):
        assert np.array_equal(dPg, first[0]) and np.array_equal(Pg, first[1]), name


# ------------------------------------------------------------------------------------------------ 7. symmetry
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_tangent_has_major_symmetry(ctx, model, oracle_1000, kernel):
    with variant(ctx, *kernel):
        dPg, _ = run_host(ctx, model, oracle_1000["F"])
    assert np.abs(dPg - dPg.transpose(0, 2, 1)).max() <= 1e-13 * np.abs(dPg).max()


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_tangent_has_major_symmetry_point_by_point(ctx, model, oracle_1000, kernel):
    """the same figure with every point's own max |dP_p| for a scale: the large points of the batch no longer set the tolerance of the
    small ones"""
    with variant(ctx, *kernel):
        dPg, _ = run_host(ctx, model, oracle_1000["F"])
    asym = np.abs(dPg - dPg.transpose(0, 2, 1)).reshape(dPg.shape[0], -1).max(axis=1)
    scale = np.abs(dPg).reshape(dPg.shape[0], -1).max(axis=1)
    worst = int(np.argmax(asym / scale))
    print(f"worst point {worst}: {asym[worst] / scale[worst]:.2e} of its own max |dP|")
    assert np.all(asym <= 1e-13 * scale), (worst, asym[worst], scale[worst])


# ------------------------------------------------------------------------------------------------ 8. field
@pytest.mark.parametrize("name", MESHES)
def test_field_form_equals_operand_then_plain_call(ctx, model, name):
    import torch

    m = _mesh(name)
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    try:
        n = m.num_cells * m.nq
        u = _field(m, 0.15, 9)
        F = dm.evaluate("F", 3, u).reshape(n, 9)
        dP0, P0 = run_host(ctx, model, F)
        dP1, P1 = np.full(n * 81, -7.0), np.full(n * 9, -7.0)
        ctx.icnn3_field(model, 0, dm._h, MEM_HOST, u, dP1, P1)
        assert np.array_equal(dP1, dP0.reshape(-1)) and np.array_equal(P1, P0.reshape(-1))
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ut = torch.from_numpy(u).cuda()
        dP2 = torch.full((n * 81,), -7.0, dtype=torch.float64, device="cuda")
        P2 = torch.full((n * 9,), -7.0, dtype=torch.float64, device="cuda")
        ctx.icnn3_field(model, 0, dm._h, MEM_DEVICE, ut.data_ptr(), dP2.data_ptr(), P2.data_ptr())
        assert np.array_equal(dP2.cpu().numpy(), dP1) and np.array_equal(P2.cpu().numpy(), P1)
    finally:
        dm.close()


def test_a_2d_mesh_is_refused_with_e_dim(ctx, model, hip_library):
    m = structured_mesh("triangle", (2, 2), 2, distort=0.0, seed=0)
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    try:
        u, dP, P = np.zeros(m.node_x.shape[0] * 2), np.empty(m.num_cells * m.nq * 81), np.empty(m.num_cells * m.nq * 9)
        rc = hip_library.dxo_icnn3_field(ctx._h, C.c_void_p(model), 0, dm._h, MEM_HOST, u.ctypes.data, dP.ctypes.data, P.ctypes.data)
        assert rc == E_DIM
        with pytest.raises(ValueError, match="DXO_E_DIM"):
            ctx.icnn3_field(model, 0, dm._h, MEM_HOST, u, dP, P)
    finally:
        dm.close()


def test_bad_arguments_answer_as_the_analytic_twins(ctx, model, hip_library):
    """the bad-argument tables of hyper3_cases with the model in the place of the parameters: the codes of dxo_isihara3 / dxo_isihara3_field
    given the same call; a precision other than 0 or 1 is DXO_E_OPTION as in dxo_icnn_eval"""
    lib, h = hip_library, ctx._h
    prm = IsiharaParams(*H3.DEFAULTS)
    buf = np.zeros(4096)
    base = (buf.ctypes.data + 15) & ~15
    want = {"NULL params": -1, "NULL mesh": -1, "n < 0": -3, "bad mem": -4, "NULL F": -1, "NULL dP": -1, "NULL P": -1, "NULL u": -1}
    ba = types.SimpleNamespace(prm=C.byref(prm), F=base, dP=base + 4096, P=base + 16384, u=base, mesh=None)
    bn = types.SimpleNamespace(**vars(ba))
    bn.prm = C.c_void_p(model)
    for (name, aa), (_, an) in zip(H3.plain_bad_calls(ba), H3.plain_bad_calls(bn)):
        rca, rcn = lib.dxo_isihara3(h, *aa), lib.dxo_icnn3_eval(h, an[0], 0, *an[1:])
        assert rcn == rca == want.get(name, -5), (name, rca, rcn)
    m3 = structured_mesh("tetrahedron", (1, 1, 1), 2, distort=0.0, seed=0)
    d3 = DeviceMesh.from_synthetic(m3, ctx=ctx)
    try:
        ba.mesh = bn.mesh = d3._h
        for (name, aa), (_, an) in zip(H3.field_bad_calls(ba), H3.field_bad_calls(bn)):
            rca, rcn = lib.dxo_isihara3_field(h, *aa), lib.dxo_icnn3_field(h, an[0], 0, *an[1:])
            assert rcn == rca == want.get(name, -5), (name, rca, rcn)
        assert lib.dxo_icnn3_eval(h, bn.prm, 2, 4, 0, bn.F, bn.dP, bn.P) == lib.dxo_icnn_eval(h, bn.prm, 2, 4, 0, bn.F, bn.dP, bn.P) == E_OPTION
        assert lib.dxo_icnn3_field(h, bn.prm, 2, bn.mesh, 0, bn.u, bn.dP, bn.P) == E_OPTION
    finally:
        d3.close()


# ------------------------------------------------------------------------------------------------ 9. factory
def test_factory_dim3(ctx, weights, golden):
    import torch

    sd = I3.state_dict(weights)
    m = _mesh("P2 tetrahedra (2,2,1)")
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    try:
        n = m.num_cells * m.nq
        u = _field(m, 0.15, 9)
        ext = make_icnn(sd, ctx=ctx, dim=3)
        Fvals = dm.operand("F", u).eval(None)
        assert Fvals.shape == (m.num_cells, m.nq, 3, 3)
        dP0, P0 = ext((1,))(Fvals)
        assert isinstance(dP0, np.ndarray) and dP0.shape == (n * 81,) and P0.shape == (n * 9,)
        dPt, Pt = ext((1,))(torch.from_numpy(np.ascontiguousarray(Fvals)).cuda())
        assert dPt.is_cuda and dPt.shape == (n * 81,) and Pt.shape == (n * 9,)
        assert np.array_equal(dPt.cpu().numpy(), dP0) and np.array_equal(Pt.cpu().numpy(), P0)
        lazy = dm.operand("F", u, lazy=True).eval(None)
        dP1, P1 = ext((1,))(lazy)
        assert lazy._value is None           # the field form: the operand was never evaluated on its own
        assert np.array_equal(dP1, dP0) and np.array_equal(P1, P0)
        dPo, Po = I3.icnn3_stress_tangent(np.asarray(Fvals).reshape(n, 9), weights)
        assert_close_scaled(P0, Po, RTOL_FP32, "factory P")
        assert_close_scaled(dP0, dPo, RTOL_FP32, "factory dP")
        dP64, P64 = make_icnn(sd, ctx=ctx, dim=3, precision="fp64")((1,))(Fvals)
        dPo64, Po64 = I3.icnn3_stress_tangent(np.asarray(Fvals).reshape(n, 9), weights, net_dtype=np.float64)
        assert_close_scaled(P64, Po64, RTOL_FP64, "factory fp64 P")
        assert_close_scaled(dP64, dPo64, RTOL_FP64, "factory fp64 dP")
        H9 = ext.correction()
        assert H9.shape == (9,) and np.all(H9[[1, 2, 3, 5, 6, 7]] == 0.0) and H9[0] == H9[4] == H9[8] and abs(H9[0]) < 1e-6
        # outputs= : the results land in the caller's arrays
        tdP, tP = np.zeros(n * 81), np.zeros(n * 9)
        dPb, Pb = make_icnn(sd, ctx=ctx, dim=3, outputs=(tdP, tP))((1,))(Fvals)
        assert np.array_equal(tdP, dP0) and np.array_equal(tP, P0) and np.shares_memory(dPb, tdP) and np.shares_memory(Pb, tP)
        with pytest.raises(NotImplementedError):
            ext((0,))
        with pytest.raises(ValueError):
            make_icnn(sd, ctx=ctx, dim=4)
        with pytest.raises(ValueError):
            make_icnn(sd, ctx=ctx)((1,))(lazy)          # a 3-D operand for the plane-strain operator
        m2 = structured_mesh("triangle", (2, 2), 2, distort=0.0, seed=0)
        d2 = DeviceMesh.from_synthetic(m2, ctx=ctx)
        try:
            with pytest.raises(ValueError):
                ext((1,))(d2.operand("F", np.zeros(m2.node_x.shape[0] * 2), lazy=True).eval(None))
        finally:
            d2.close()
        # without dim: the plane-strain operator of before, 16 / 4 values per point, bit for bit
        g = golden("icnn_isihara.npz")
        F2 = np.ascontiguousarray(g["F"][:300])
        ext2 = make_icnn(sd, ctx=ctx)
        dPa, Pa = ext2((1,))(F2)
        mdl = ctx.icnn_create(sd)
        try:
            dPb, Pb = np.empty(300 * 16), np.empty(300 * 4)
            ctx.icnn_eval(mdl, 0, 300, MEM_HOST, F2, dPb, Pb)
        finally:
            ctx.icnn_destroy(mdl)
        assert dPa.shape == (300 * 16,) and Pa.shape == (300 * 4,) and np.array_equal(dPa, dPb) and np.array_equal(Pa, Pb)
        assert ext2.correction().shape == (4,)
    finally:
        dm.close()


# ------------------------------------------------------------------------------------------------ 10. Taylor test
def test_taylor_remainder_of_the_internal_force_is_second_order(ctx, model):
    """R(u) = adjoint("F", 3, P(u)), K v = bilinear_apply("grad", "grad", 3, dP(u), v), network in fp64: the remainder
    |R(u + h v) - R(u) - h K v| falls fourfold per halving of h (observed order >= 1.9 between h = 1e-2, 5e-3, 2.5e-3, as the analytic
    model is held to)"""
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
            ctx.icnn3_field(model, 1, dm._h, MEM_DEVICE, w.data_ptr(), tangent.data_ptr(), P.data_ptr())
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
