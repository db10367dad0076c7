"""examples/device_hyperelasticity_3d.py at its smallest size (3^3 boxes of P2 tetrahedra): every load step converges on the
assembled-multigrid path and on the matrix-free path, both reach the same displacement, and Newton converges quadratically."""
import importlib.util
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def reports():
    spec = importlib.util.spec_from_file_location("device_hyperelasticity_3d", ROOT / "examples" / "device_hyperelasticity_3d.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for matrix_free in (False, True):
        out[matrix_free] = mod.main(3, steps=3, matrix_free=matrix_free, verbose=False)      # raises if a load step does not converge
        for s in out[matrix_free]["steps"]:
            print("matrix-free" if matrix_free else "assembled + AMG", f"load {s['load']:.3f}: residuals",
                  " ".join(f"{r:.2e}" for r in s["newton_residuals"]), "linear its", s["linear_iterations"])
    return out, mod.MAX_NEWTON


@pytest.mark.parametrize("matrix_free", [False, True])
def test_every_load_step_converges(reports, matrix_free):
    rep, cap = reports[0][matrix_free], reports[1]
    assert len(rep["steps"]) == 3 and np.isfinite(rep["u"]).all() and np.abs(rep["u"]).max() > 0.1
    for s in rep["steps"]:
        r = s["newton_residuals"]
        assert 2 <= len(r) <= cap + 1 and r[-1] <= 1e-10 * r[0]


@pytest.mark.parametrize("matrix_free", [False, True])
def test_newton_converges_quadratically(reports, matrix_free):
    """the last Newton step of a load step reduces the residual by more than the step before it did"""
    for s in reports[0][matrix_free]["steps"]:
        r = s["newton_residuals"]
        assert len(r) >= 3, r
        assert r[-1] / r[-2] < r[-2] / r[-3], r


def test_both_paths_reach_the_same_displacement(reports):
    """Krylov tolerance 1e-12 in both: the final fields agree to 1e-8 of |u|"""
    ua, um = reports[0][False]["u"], reports[0][True]["u"]
    assert np.linalg.norm(ua - um) <= 1e-8 * np.linalg.norm(ua)
