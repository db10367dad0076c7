"""examples/device_hyperelasticity_3d.py --matrix-free with and without --recompute at its smallest size: 3^3 boxes of P2 tetrahedra,
one load step. Both runs reach the example's own tolerance with the same number of Newton iterations, and the recompute run holds no
quadrature data. The displacement difference and the cg counts are printed, not asserted: no bound for them can be derived here."""
import importlib.util
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_recompute_run_follows_the_array_run():
    spec = importlib.util.spec_from_file_location("device_hyperelasticity_3d", ROOT / "examples" / "device_hyperelasticity_3d.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    arr = mod.main(3, steps=1, matrix_free=True, verbose=False)                       # raises if the load step does not converge
    rec = mod.main(3, steps=1, matrix_free=True, recompute=True, verbose=False)
    assert rec["recompute"] and not arr["recompute"]
    assert rec["quadrature_bytes"] == 0 and arr["quadrature_bytes"] == (81 + 9) * 8 * arr["points"]
    for run in (arr, rec):
        assert len(run["steps"]) == 1
        r = run["steps"][0]["newton_residuals"]
        assert 2 <= len(r) <= mod.MAX_NEWTON + 1 and r[-1] <= 1e-10 * r[0]
    assert len(rec["steps"][0]["newton_residuals"]) == len(arr["steps"][0]["newton_residuals"])
    diff = np.linalg.norm(rec["u"] - arr["u"]) / np.linalg.norm(arr["u"])
    print(f"|u_recompute - u_array| / |u_array| = {diff:.3e}")
    print("cg iterations, array route", arr["steps"][0]["linear_iterations"], "recompute", rec["steps"][0]["linear_iterations"])
    for bad in (dict(matrix_free=False), dict(matrix_free=True, model="icnn")):
        with pytest.raises(ValueError, match="recompute"):
            mod.main(3, steps=1, recompute=True, verbose=False, **bad)
