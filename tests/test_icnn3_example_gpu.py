"""examples/device_hyperelasticity_3d.py with the trained network as the constitutive law (--model icnn) at its smallest size: 3^3 boxes
of P2 tetrahedra, one load step. Every Newton solve reaches the example's own tolerance within its own iteration cap. How far the
network — trained on plane-strain data — follows the analytic 3-D energy is printed, not asserted."""
import importlib.util
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
WEIGHTS = ROOT / "tests" / "golden" / "icnn_isihara_weights.npz"


def test_network_run_converges_within_the_examples_cap():
    spec = importlib.util.spec_from_file_location("device_hyperelasticity_3d", ROOT / "examples" / "device_hyperelasticity_3d.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net = mod.main(3, steps=1, verbose=False, model="icnn", weights=WEIGHTS)      # raises if the load step does not converge
    ana = mod.main(3, steps=1, verbose=False)
    assert net["model"] == "icnn" and len(net["steps"]) == 1
    for s in net["steps"]:
        r = s["newton_residuals"]
        print("network: residuals", " ".join(f"{x:.2e}" for x in r), "linear its", s["linear_iterations"])
        assert 2 <= len(r) <= mod.MAX_NEWTON + 1 and r[-1] <= 1e-10 * r[0]
    assert np.isfinite(net["u"]).all() and np.abs(net["u"]).max() > 0.1
    diff = np.linalg.norm(net["u"] - ana["u"]) / np.linalg.norm(ana["u"])
    print(f"|u_network - u_analytic| / |u_analytic| = {diff:.3e}, max |du| = {np.abs(net['u'] - ana['u']).max():.3e}")
