"""examples/device_hyperelasticity_3d.py --matrix-free --recompute at its smallest size (3^3 boxes of P2 tetrahedra, one load step)
under point Jacobi and under the p-multigrid on the operator (--pc pmg): both reach the example's tolerance with the same number of
Newton iterations, neither holds fine quadrature data, and every linear solve under the p-multigrid takes at most half the CG
iterations of the corresponding Jacobi solve. That margin rests on the CPU proxy of tests/test_pmg_reference_cpu.py (a linear
operator: 168 against 14), not on a measurement of this tangent."""
import importlib.util
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _example():
    spec = importlib.util.spec_from_file_location("device_hyperelasticity_3d", ROOT / "examples" / "device_hyperelasticity_3d.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pmg_run_follows_the_jacobi_run():
    mod = _example()
    jac = mod.main(3, steps=1, matrix_free=True, recompute=True, verbose=False, pc="jacobi")      # raises if the load step does not converge
    pmg = mod.main(3, steps=1, matrix_free=True, recompute=True, verbose=False, pc="pmg")
    assert jac["pc"] == "jacobi" and pmg["pc"] == "pmg"
    assert jac["quadrature_bytes"] == 0 and pmg["quadrature_bytes"] == 0
    assert jac["coarse_bytes"] == 0 and pmg["coarse_bytes"] > 0
    # the coarse dP array alone: 81 doubles per cell at the 1-point rule
    assert pmg["coarse_bytes"] >= 81 * 8 * pmg["cells"]
    for run in (jac, pmg):
        assert len(run["steps"]) == 1
        r = run["steps"][0]["newton_residuals"]
        assert 2 <= len(r) <= mod.MAX_NEWTON + 1 and r[-1] <= 1e-10 * r[0]
    assert len(pmg["steps"][0]["newton_residuals"]) == len(jac["steps"][0]["newton_residuals"])
    ij, ip = jac["steps"][0]["linear_iterations"], pmg["steps"][0]["linear_iterations"]
    print("cg iterations per Newton step, Jacobi", ij, "p-multigrid", ip)
    print(f"|u_pmg - u_jacobi| / |u_jacobi| = {np.linalg.norm(pmg['u'] - jac['u']) / np.linalg.norm(jac['u']):.3e}")
    assert len(ij) == len(ip)
    assert all(2 * p <= j for p, j in zip(ip, ij)), (ip, ij)


def test_pmg_needs_the_matrix_free_route():
    mod = _example()
    with pytest.raises(ValueError, match="pmg"):
        mod.main(3, steps=1, pc="pmg", verbose=False)
    with pytest.raises(ValueError, match="pc must be"):
        mod.main(3, steps=1, matrix_free=True, pc="ilu", verbose=False)
