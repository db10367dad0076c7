"""examples/device_mohr_coulomb_3d.py at its smallest size (6 x 6 x 1 Q2 hexahedra, the first three load steps): every step converges
on the assembled-multigrid path and on the matrix-free path, both reach the same displacement, and the one-layer problem keeps the
plane-strain symmetry."""
import importlib.util
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _load(name):
    spec = importlib.util.spec_from_file_location(name, ROOT / "examples" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def reports():
    mod = _load("device_mohr_coulomb_3d")
    out = {}
    for matrix_free in (False, True):
        out[matrix_free] = mod.main(6, steps=3, matrix_free=matrix_free, verbose=False)      # raises if a step does not converge
        for s in out[matrix_free]["steps"]:
            print("matrix-free" if matrix_free else "assembled + AMG", f"load {s['load']:.3f}: residuals",
                  " ".join(f"{r:.2e}" for r in s["newton_residuals"]), "linear its", s["linear_iterations"], "plastic points", s["plastic_points"])
    return out, mod.MAX_NEWTON


@pytest.mark.parametrize("matrix_free", [False, True])
def test_every_load_step_converges(reports, matrix_free):
    rep, cap = reports[0][matrix_free], reports[1]
    assert len(rep["steps"]) == 3 and np.isfinite(rep["u"]).all() and np.abs(rep["u"]).max() > 0
    for s in rep["steps"]:
        r = s["newton_residuals"]
        assert 2 <= len(r) <= cap + 1 and r[-1] <= max(1e-12, 1e-10 * r[0])
    assert rep["steps"][-1]["plastic_points"] > 0            # the return map is at work, not only the elastic branch


@pytest.mark.parametrize("matrix_free", [False, True])
def test_last_newton_step_contracts_faster_than_the_one_before(reports, matrix_free):
    seen = 0
    for s in reports[0][matrix_free]["steps"]:
        r = s["newton_residuals"]
        assert len(r) >= 3, r
        assert r[-1] / r[-2] < r[-2] / r[-3], r
        seen += 1
    assert seen == 3


def test_both_paths_reach_the_same_displacement(reports):
    """Krylov tolerance 1e-12 in both: the final fields agree to 1e-8 of |u|"""
    ua, um = reports[0][False]["u"], reports[0][True]["u"]
    assert np.linalg.norm(ua - um) <= 1e-8 * np.linalg.norm(ua)


def test_out_of_plane_shears_vanish_by_mirror_symmetry(reports):
    """u_z = 0 on both z faces of a single layer: the discrete solution is the plane-strain one, so sigma_xz and sigma_yz are zero up to
    what the linear solves leave. Measured max|sigma_xz, sigma_yz| / max|sigma|: 8.2e-15 (assembled), 8.3e-15 (matrix-free); the bound
    is ten times the larger, 8.3e-14."""
    for matrix_free in (False, True):
        sg = reports[0][matrix_free]["sigma"]
        ratio = np.max(np.abs(sg[:, 4:])) / np.max(np.abs(sg))
        print("matrix-free" if matrix_free else "assembled", f"out-of-plane shears / max|sigma| = {ratio:.3e}")
        assert ratio <= 8.3e-14
        assert np.max(np.abs(sg[:, 3])) > 1e-3 * np.max(np.abs(sg))       # the in-plane shear is there


def test_load_factor_beside_the_plane_strain_example(reports):
    """printed, not asserted: P2 triangles there, Q2 hexahedra here"""
    rep2 = _load("device_mohr_coulomb_slope").main(6, steps=3, solver="amg-rbm", verbose=False)
    rep3 = reports[0][False]
    print(f"load reached: plane strain {rep2['load_reached']:.3f} (factor {rep2['stability_factor']:.3f}), "
          f"3-D {rep3['load_reached']:.3f} (factor {rep3['stability_factor']:.3f})")
    assert rep2["failed"] is None
