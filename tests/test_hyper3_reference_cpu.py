"""The 3-D Isihara operator without a GPU: the autograd reference of tests/hyper3_cases.py pinned to the reference's own data through
the plane-strain embedding F = [[F_2, 0], [0, 1]] (tests/golden/isihara_analytic.npz), its invariances, and the C entry points'
behaviour where no device is needed.

A dxo_ctx exists only on a device (dxo_ctx_create answers DXO_E_NODEVICE otherwise), so what can be asked here of the argument checks
is that every bad call answers what its 2-D twin answers on the NULL context both are given; the same list against a real context,
where each check is reached, is tests/test_hyper3_gpu.py::test_bad_arguments_answer_as_the_2d_twins."""
import ctypes as C
import types

import numpy as np

import hyper3_cases as H3
from dolfinx_external_operator_amd import IsiharaParams
from dolfinx_external_operator_amd._lib import declared_symbols


def _golden_embedded(golden):
    g = golden("isihara_analytic.npz")
    return g, H3.embed_plane_strain(g["F"])


def test_plane_strain_embedding_reproduces_the_reference_data(golden):
    """In-plane P and dP of the 3-D energy at [[F_2, 0], [0, 1]] are the golden's to 1e-13 of the scale (measured 6.4e-16, 4.7e-16);
    the out-of-plane shear stresses are exactly 0."""
    g, F = _golden_embedded(golden)
    P, dP = H3.reference(F)
    ip = H3.IN_PLANE
    eP, eD = H3.rel_err(P[:, ip], g["P"]), H3.rel_err(dP[:, ip][:, :, ip], g["dP"])
    print(f"in-plane P {eP:.2e}, dP {eD:.2e}")
    assert eP <= 1e-13 and eD <= 1e-13
    assert np.all(P[:, H3.SHEAR_OUT] == 0.0)


def test_identity_is_stress_free():
    P, dP = H3.reference(H3.EYE[None, :])
    assert np.all(P == 0.0)
    assert np.isfinite(dP).all()


def test_tangent_is_symmetric_and_forward_equals_reverse():
    F = H3.samples(300)
    _, dP = H3.reference(F)
    scale = np.abs(dP).max()
    sym = np.abs(dP - dP.transpose(0, 2, 1)).max() / scale
    rev = np.abs(dP - H3.reference_reverse(F)).max() / scale
    print(f"symmetry {sym:.2e}, forward against reverse {rev:.2e}")
    assert sym <= 1e-13 and rev <= 1e-13


def test_stress_is_objective():
    """P(Q F) = Q P(F) for a rotation Q"""
    rng = np.random.Generator(np.random.PCG64(3))
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    F = H3.samples(200).reshape(-1, 3, 3)
    P, _ = H3.reference(F)
    PQ, _ = H3.reference(np.einsum("ij,njk->nik", Q, F))
    want = np.einsum("ij,njk->nik", Q, P.reshape(-1, 3, 3)).reshape(-1, 9)
    assert H3.rel_err(PQ, want) <= 1e-13


def test_sample_generators_stay_in_the_model_range():
    assert H3.det_rows(H3.small_strain(1200)).min() > 0.5
    assert H3.det_rows(H3.large_stretch(600)).min() > 0.2
    assert H3.samples(1000).shape == (1000, 9) and H3.samples(1).shape == (1, 9)


def test_entry_points_exist_and_answer_as_their_2d_twins_without_a_context(hip_library):
    lib = hip_library
    for name in ("dxo_isihara3", "dxo_isihara3_field"):
        assert name in declared_symbols() and hasattr(lib, name)
    assert lib.dxo_abi_version() == 2
    prm = IsiharaParams(0.5, 1.0, 1.0, 1.5)
    buf = np.zeros(512)
    base = (buf.ctypes.data + 15) & ~15
    b = types.SimpleNamespace(prm=C.byref(prm), F=base, dP=base + 1024, P=base + 2048, u=base, mesh=None)
    for name, args in H3.plain_bad_calls(b):
        rc2, rc3 = lib.dxo_isihara(None, *args), lib.dxo_isihara3(None, *args)
        assert rc3 == rc2 == -1, name
    for name, args in H3.field_bad_calls(b):
        rc2, rc3 = lib.dxo_isihara_field(None, *args), lib.dxo_isihara3_field(None, *args)
        assert rc3 == rc2 == -1, name
