"""NumPy oracle of the single-precision multigrid cycle (dxo_amg_set_precision with DXO_AMG_PRECISION_FP32), cycle_ref of
oracle/amg_oracle.py with precision="fp32", and what it promises (not gpu).

It is the walk of the float64 cycle with A, Dinv, P and every vector of every level but the coarsest in numpy.float32, for the
Jacobi sweeps and for the Chebyshev polynomial; omega and the Chebyshev pairs are made in double and narrowed once; the coarsest level
widens its right-hand side, multiplies by the float64 dense inverse and narrows the result. The hierarchy itself (Dinv, omega, rho, P,
the coarse matrices, the dense inverse) is the float64 one: only the cycle is narrowed, as on the device.

Measured here (one Jacobi sweep, FGMRES(30) to rtol 1e-10, right-hand side seed 1; printed by the tests with -s):

    system                                   rows / levels   |z32 - z64| / |z64|   FGMRES iterations, fp64 / fp32 cycle
    heat 16 x 16                             289 / 3         1.9e-7                19 / 19
    heat 48 x 48                             2401 / 4        2.0e-7                26 / 26
    P2 eps/eps 14 x 14, rigid-body modes     1682 / 3        6.4e-7                74 / 74
    non-symmetric eps 14 x 14                1682 / 3        2.7e-7                171 / 171
    anisotropic 24 x 24, strength 0.25       625 / 4         1.6e-7                23 / 23

This file pins the oracle tests/test_amg_fp32_gpu.py leans on; it passes without the device feature."""
import copy

import numpy as np
import pytest

from oracle.amg_oracle import cycle_ref
from oracle.krylov_oracle import fgmres_ref
from solver_cases import system

SYSTEMS = ["heat", "heat48", "p2_rbm", "nonsym", "aniso"]
# |z32 - z64| / |z64| of one cycle. Below: a float32 walk that silently ran in float64 would differ by rounding of the final cast
# alone or not at all; 1e-9 is two orders under the unit roundoff of float32 (6e-8). Above: a cycle is some tens of float32 sums of
# at most some tens of terms, each a few 6e-8 relative to its terms; 1e-5 is two orders over that roundoff.
F32_LOW, F32_HIGH = 1e-9, 1e-5


def f32_deviation(levels, r):
    """(|z32 - z64| / |z64|, z32, z64) of one cycle on r."""
    z64 = cycle_ref(levels, r)
    z32 = cycle_ref(levels, r, precision="fp32")
    return np.linalg.norm(z32.astype(np.float64) - z64) / np.linalg.norm(z64), z32, z64


@pytest.mark.parametrize("which", SYSTEMS)
def test_the_float32_walk_is_float32_and_close_to_the_float64_walk(which):
    S, _, levels = system(which)
    rng = np.random.Generator(np.random.PCG64(12))
    seen = []
    for _ in range(3):
        r = rng.normal(size=S.shape[0])
        e, z32, z64 = f32_deviation(levels, r)
        assert z32.dtype == np.float32 and z64.dtype == np.float64 and np.isfinite(z32).all()
        assert F32_LOW < e < F32_HIGH, (which, e)
        seen.append(e)
    assert not cycle_ref(levels, np.zeros(S.shape[0]), precision="fp32").any()
    print(f"{which}: rows {S.shape[0]} / {len(levels)} levels, |z32 - z64| / |z64| {max(seen):.2e}")


def test_the_float32_walk_covers_chebyshev():
    """The same three checks with the Chebyshev polynomial of degree 2 on the levels of "heat48" (rho: the one omega was made from)."""
    S, _, shared = system("heat48")
    levels = [copy.copy(L) for L in shared]      # shallow: the cached levels stay as they are
    for L in levels[:-1]:
        L.smoother, L.degree, L.lower, L.rho = "chebyshev", 2, 0.1, (4.0 / 3.0) / L.omega
    r = np.random.Generator(np.random.PCG64(12)).normal(size=S.shape[0])
    e, z32, _ = f32_deviation(levels, r)
    assert z32.dtype == np.float32 and F32_LOW < e < F32_HIGH, e
    print(f"heat48, Chebyshev 2: |z32 - z64| / |z64| {e:.2e}")


@pytest.mark.parametrize("which", SYSTEMS)
def test_fgmres_takes_the_float32_cycle(which):
    """FGMRES(30) to rtol 1e-10 converges on the true residual (fgmres_ref recomputes b - A x in float64 at every restart) with the
    float32 walk as M, in the iterations of the float64 walk +- 2 (equal on all five when this was written)."""
    S, b, levels = system(which)
    out64 = fgmres_ref(S, b, M=lambda r, j: cycle_ref(levels, r), m=30, rtol=1e-10, maxiter=2000)
    out32 = fgmres_ref(S, b, M=lambda r, j: cycle_ref(levels, r, precision="fp32").astype(np.float64), m=30, rtol=1e-10, maxiter=2000)
    (x64, its64, conv64, res64), (x32, its32, conv32, res32) = out64[:4], out32[:4]
    print(f"{which}: FGMRES(30) iterations fp64 / fp32 cycle {its64} / {its32}, true residuals {res64:.5e} / {res32:.5e}")
    assert conv64 and conv32
    assert np.linalg.norm(b - S @ x32) <= 1e-10 * np.linalg.norm(b) * (1 + 1e-6)
    assert abs(its32 - its64) <= 2, (which, its32, its64)
