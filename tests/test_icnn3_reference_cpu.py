"""The reference of the 3-D network operator (tests/icnn3_cases.py) checked on the CPU: its two routes against each other, the feature
derivatives against central differences, the plane-strain embedding against the 2-D oracle, the network with its hidden path switched
off against the analytic 3-D Mooney-Rivlin energy; and the C ABI of the new entry points."""
import ctypes as C
import types

import numpy as np
import pytest

import hyper3_cases as H3
import icnn3_cases as I3
from dolfinx_external_operator_amd._lib import declared_symbols
from oracle.icnn_oracle import icnn_stress_tangent, softplus


@pytest.fixture(scope="module")
def weights(golden):
    return dict(golden("icnn_isihara_weights.npz"))


SAMPLES = {"small_strain": I3.small_strain, "moderate": I3.moderate, "inverted": I3.inverted}


@pytest.mark.parametrize("name", list(SAMPLES))
def test_jets_route_equals_whole_network_autograd(weights, name):
    """200 points of each sample, network in fp64 on both routes: 1e-13 of the batch scale (measured 4e-16)"""
    F = SAMPLES[name](200)
    dP, P = I3.icnn3_stress_tangent(F, weights, net_dtype=np.float64)
    dPa, Pa = I3.autograd_stress_tangent(F, weights)
    print(f"{name}: P {H3.rel_err(P, Pa):.2e}, dP {H3.rel_err(dP, dPa):.2e}, symmetry {np.abs(dP - dP.transpose(0, 2, 1)).max() / np.abs(dP).max():.2e}")
    assert np.isfinite(dP).all() and np.isfinite(P).all()
    assert H3.rel_err(P, Pa) <= 1e-13 and H3.rel_err(dP, dPa) <= 1e-13


def test_feature_derivatives_by_finite_differences():
    F = I3.small_strain(50, seed=3)
    K, dK, d2K = I3.features(F)
    h = 1e-6
    for j in range(9):
        Fp, Fm = F.copy(), F.copy()
        Fp[:, j] += h
        Fm[:, j] -= h
        Kp, dKp, _ = I3.features(Fp)
        Km, dKm, _ = I3.features(Fm)
        assert np.max(np.abs((Kp - Km) / (2 * h) - dK[:, :, j])) < 1e-7
        assert np.max(np.abs((dKp - dKm) / (2 * h) - d2K[:, :, :, j])) < 1e-6


def test_features_are_stationary_at_the_identity():
    """why the 3-D stress correction is analytically zero"""
    K, dK, _ = I3.features(H3.EYE[None])
    assert np.abs(K).max() <= 1e-15 and np.abs(dK).max() <= 1e-15


def test_plane_strain_embedding_equals_the_2d_oracle(weights):
    rng = np.random.Generator(np.random.PCG64(19))
    F2 = np.array([1.0, 0.0, 0.0, 1.0]) + 0.1 * rng.normal(size=(300, 4))
    dP2, P2 = icnn_stress_tangent(F2, weights, net_dtype=np.float64)
    dP3, P3 = I3.icnn3_stress_tangent(H3.embed_plane_strain(F2), weights, net_dtype=np.float64)
    ip = H3.IN_PLANE
    print(f"in-plane P {H3.rel_err(P3[:, ip], P2):.2e}, dP {H3.rel_err(dP3[:, ip][:, :, ip], dP2):.2e}, max |P33| {np.abs(P3[:, 8]).max():.3f}")
    assert H3.rel_err(P3[:, ip], P2) <= 1e-13
    assert H3.rel_err(dP3[:, ip][:, :, ip], dP2) <= 1e-13
    assert np.all(P3[:, H3.SHEAR_OUT] == 0.0)
    assert np.abs(P3[:, 8]).max() > 0.1          # the out-of-plane normal stress is there: the embedding is not the 2-D operator padded with zeros


def test_hidden_path_off_is_the_mooney_rivlin_solid(weights):
    """layers.3.weights = -100: softplus of it is 4e-44, the network is y = softplus(skip_layers.3.weights) . x, i.e. the energy
    a K1 + b K2 + c K3 — hyper3_cases' with (c1, c2, c3, c4) = (a, b, 0, c) where det F > 0"""
    w = dict(weights)
    w["layers__3__weights"] = np.full_like(weights["layers__3__weights"], -100.0)
    a, b, c = (float(v) for v in softplus(weights["skip_layers__3__weights"].astype(np.float64))[0])
    F = I3.moderate(200)
    dP, P = I3.icnn3_stress_tangent(F, w, net_dtype=np.float64)
    Pr, dPr = H3.reference(F, (a, b, 0.0, c))
    print(f"(a, b, c) = ({a:.4f}, {b:.4f}, {c:.4f}): P {H3.rel_err(P, Pr):.2e}, dP {H3.rel_err(dP, dPr):.2e}")
    assert H3.rel_err(P, Pr) <= 1e-13 and H3.rel_err(dP, dPr) <= 1e-13


def test_sample_generators():
    assert H3.det_rows(I3.inverted(200)).max() < 0.0
    d = H3.det_rows(I3.moderate(500))
    assert d.min() > 0.5 and d.max() < 2.0


def test_entry_points_exist_and_answer_without_a_context(hip_library):
    """the header declares the three symbols, the binding knows them, the library exports them, the ABI version has not moved"""
    import pathlib

    lib = hip_library
    header = (pathlib.Path(__file__).resolve().parents[1] / "include" / "dxo.h").read_text()
    for name in ("dxo_icnn3_eval", "dxo_icnn3_field", "dxo_icnn3_correction"):
        assert f"int {name}(" in header, name
        assert name in declared_symbols() and hasattr(lib, name), name
    assert "#define DXO_ABI_VERSION 2" in header and lib.dxo_abi_version() == 2
    from dolfinx_external_operator_amd import Context

    for method in ("icnn3_eval", "icnn3_field", "icnn3_correction"):
        assert callable(getattr(Context, method))
    buf = np.zeros(512)
    base = (buf.ctypes.data + 15) & ~15
    model = C.c_void_p(base)            # never dereferenced: the NULL context answers first
    b = types.SimpleNamespace(prm=model, F=base, dP=base + 1024, P=base + 2048, u=base, mesh=None)
    for name, args in H3.plain_bad_calls(b):
        assert lib.dxo_icnn3_eval(None, args[0], 0, *args[1:]) == -1, name
    for name, args in H3.field_bad_calls(b):
        assert lib.dxo_icnn3_field(None, args[0], 0, *args[1:]) == -1, name
    assert lib.dxo_icnn3_correction(None, model, base) == -1
