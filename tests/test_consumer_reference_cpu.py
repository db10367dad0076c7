"""oracle/consumer_reference.py (long double) tied to what the suite already trusts, on the CPU: the float64 NumPy oracle, probing
with unit vectors, and the C port of the reference's von Mises statements. The figures measured here are the constants the
componentwise bound of tests/test_consumer_reference_gpu.py is built from (consumer_cases.C_REF)."""
import numpy as np
import pytest

from consumer_cases import ALL_CASES, C_REF, VM, build_mesh, case_id, make_inputs
from oracle.consumer_reference import (LD, ref_adjoint_eps, ref_tangent_apply, ref_tangent_diagonal, vm_tangent_from_state,
                                       worst_ratio)
from oracle.operand_oracle import EPS_MANDEL, operand_adjoint, tangent_apply
from tools.synthetic import structured_mesh


def float64_ratios(case):
    """Worst componentwise distance of float64 NumPy from the long-double reference on one mesh, per entry point, in units of
    2^-53 * mag[k]."""
    from oracle.consumer_reference import numpy_expand_tangent

    m = build_mesh(case)
    x = make_inputs(case, m)
    nn = m.node_x.shape[0]
    tabs = (m.weights, m.dofmap, m.geom_dofmap, m.x, m.phi, m.dphi, m.dpsi, nn)
    out = {}
    ref, mag = ref_tangent_apply(m, x.C, x.v)
    out["apply"] = worst_ratio(tangent_apply(x.C.reshape(-1), x.v, *tabs), ref, mag)
    ref, mag = ref_adjoint_eps(m, x.S)
    out["force"] = worst_ratio(operand_adjoint(EPS_MANDEL, m.gdim, x.S, *tabs), ref, mag)
    ref, mag = ref_tangent_diagonal(m, x.C)
    out["diag"] = worst_ratio(ref_tangent_diagonal(m, x.C, dtype=np.float64)[0], ref, mag)
    Cvm, Cvm_mag = vm_tangent_from_state(VM, x.sigma, x.dp)
    C64 = numpy_expand_tangent(x.sigma, x.dp.reshape(-1), x.d, E=VM.E, nu=VM.nu)
    ref, mag = ref_tangent_apply(m, Cvm, x.v, C_mag=Cvm_mag)
    out["apply_vm"] = worst_ratio(tangent_apply(C64.reshape(-1), x.v, *tabs), ref, mag)
    ref, mag = ref_tangent_diagonal(m, Cvm, C_mag=Cvm_mag)
    out["diag_vm"] = worst_ratio(ref_tangent_diagonal(m, C64, dtype=np.float64)[0], ref, mag)
    return out


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_float64_oracle_stays_within_c_ref_of_the_long_double_reference(case):
    """ref_tangent_apply / ref_adjoint_eps against oracle.operand_oracle.tangent_apply / operand_adjoint, ref_tangent_diagonal against
    its own float64 twin, and the state-based forms against the same float64 functions fed tests/test_sharding.py's float64
    tangent-from-state, on every mesh of the GPU file: |f64[k] - ref[k]| <= C_REF * 2^-53 * mag[k] in every dof.

    Measured worst ratio per element over its meshes (sizes a-d; `gauss3`: the 3-point-per-direction rule), x86-64 long double:

        element                  apply   force    diag  apply_vm  diag_vm
        triangle P1               3.60    5.48    3.52    3.38     3.56
        triangle P2               4.71    6.26    5.24    4.96     4.64
        quadrilateral Q1          4.90   11.87   13.92    6.38    10.54
        quadrilateral Q2          6.06   14.95   17.10    6.36    19.38
        tetrahedron P1            1.44    1.62    3.98    2.29     3.42
        tetrahedron P2            1.51    3.19    4.64    2.03     4.24
        hexahedron Q1             1.40    3.77    4.29    3.22     4.73
        hexahedron Q2             1.74    5.68    7.77    2.03     7.85
        quadrilateral Q1 gauss3   2.94    1.69    3.66    1.92     3.58
        quadrilateral Q2 gauss3   2.79    4.02    5.41    1.86     4.06
        hexahedron Q1 gauss3      1.38    1.18    5.98    2.37     5.38
        hexahedron Q2 gauss3      2.12    2.91    7.64    2.05     8.24

    The worst of every column is on the 13 x 12 quadrilaterals, where the Jacobian is a difference of coordinates of size 1 at a
    spacing of 1 / 13: an error of the geometry that mag does not contain. consumer_cases.C_REF is the worst of each column rounded
    up to one decimal; the action's also covers the long thin quadrilaterals of the next test (7.64)."""
    got = float64_ratios(case)
    print(case_id(case), " ".join(f"{k}={v:.2f}" for k, v in got.items()))
    for k, v in got.items():
        assert v <= C_REF[k], (k, v)


def test_long_thin_quadrilaterals_are_the_worst_case_of_the_action():
    """The mesh on which the float64 action strays furthest from long double: 17 x 1 distorted quadrilaterals, Q1 and Q2 (measured
    7.64 and 7.27 times 2^-53 * mag[k]). C_REF["apply"] = 7.7 comes from here."""
    worst = 0.0
    for degree in (1, 2):
        m = structured_mesh("quadrilateral", (17, 1), degree, distort=0.2, seed=6)
        d, nn = 4, m.node_x.shape[0]
        rng = np.random.Generator(np.random.PCG64(1))
        A = rng.normal(size=(m.num_cells, m.nq, d, d))
        C = A @ A.transpose(0, 1, 3, 2) + 3 * np.eye(d)
        v = rng.normal(size=nn * 2)
        ref, mag = ref_tangent_apply(m, C, v)
        r = worst_ratio(tangent_apply(C.reshape(-1), v, m.weights, m.dofmap, m.geom_dofmap, m.x, m.phi, m.dphi, m.dpsi, nn), ref, mag)
        print("quadrilateral 17x1 degree", degree, f"{r:.2f}")
        worst = max(worst, r)
    assert worst <= C_REF["apply"]


@pytest.mark.parametrize("cell,n,degree", [("triangle", (2, 1), 2), ("quadrilateral", (2, 1), 2), ("tetrahedron", (1, 1, 1), 2),
                                           ("hexahedron", (2, 1, 1), 1), ("hexahedron", (1, 1, 1), 2)])
def test_direct_diagonal_equals_probing_with_unit_vectors(cell, n, degree):
    """ref_tangent_diagonal forms the diagonal from the columns of B; e_k . K e_k with the float64 oracle's K v is the other way to
    it. With a unit vector the oracle's sum IS the diagonal entry's sum, so the same componentwise bound applies."""
    m = structured_mesh(cell, n, degree, distort=0.2, seed=6)
    G, nn = m.gdim, m.node_x.shape[0]
    d = 4 if G == 2 else 6
    rng = np.random.Generator(np.random.PCG64(2))
    A = rng.normal(size=(m.num_cells, m.nq, d, d))
    C = A @ A.transpose(0, 1, 3, 2) + 3 * np.eye(d)
    ref, mag = ref_tangent_diagonal(m, C)
    probed = np.empty(nn * G)
    for k in range(nn * G):
        e = np.zeros(nn * G)
        e[k] = 1.0
        probed[k] = tangent_apply(C.reshape(-1), e, m.weights, m.dofmap, m.geom_dofmap, m.x, m.phi, m.dphi, m.dpsi, nn)[k]
    assert np.all(ref > 0)
    r = worst_ratio(probed, ref, mag)
    print(cell, degree, f"probing ratio {r:.2f}")
    assert r <= C_REF["diag"]


@pytest.mark.parametrize("d", [4, 6])
def test_tangent_from_state_equals_the_c_port_of_the_reference(oracle, d):
    """vm_tangent_from_state fed the (sigma, dp) the oracle fixture's von Mises returns (the C port of the reference's statements,
    pinned by the goldens) against the C_tang of the same call. The port forms the tangent from the TRIAL state, the closed form from
    the returned one: equal in exact arithmetic. Tolerance, measured here: 8 times the distance of the float64 closed form
    (oracle/consumer_reference.py::numpy_expand_tangent) from the long-double one, max over all entries — measured 3.5e-10 (d = 4) and
    3.0e-10 (d = 6) on entries up to 9.4e4, the port's own distance 4.6e-11 / 3.5e-11. Elastic points: C_elas, bit for bit."""
    from conftest import vm_inputs
    from oracle.consumer_reference import numpy_expand_tangent

    deps, sigma_n, p = vm_inputs(3000, d, seed=11)
    deps[:1000] *= 0.2          # a third of the points stays elastic
    sigma_n[:1000] *= 0.2
    C, s, dp = oracle.von_mises(deps, sigma_n, p, E=VM.E, nu=VM.nu, sigma_0=VM.sigma_0, H=VM.H)
    plastic = dp > 0
    assert 0.2 < plastic.mean() < 0.95
    ref, _ = vm_tangent_from_state(VM, s, dp)
    tol = 8.0 * float(np.abs(numpy_expand_tangent(s, dp, d, E=VM.E, nu=VM.nu) - ref).max())
    dist = float(np.abs(C[plastic] - ref[plastic]).max())
    print(f"d={d}: tolerance {tol:.3e}, port's distance {dist:.3e}, scale {float(np.abs(ref).max()):.3e}")
    assert dist <= tol
    # elastic points: beta = 0, n = 0, so the closed form subtracts exact zeros from C_elas
    E, nu = LD(VM.E), LD(VM.nu)
    one = np.zeros(d, LD)
    one[:3] = 1
    C_el = E * nu / ((1 + nu) * (1 - 2 * nu)) * np.outer(one, one) + 2 * (E / (2 * (1 + nu))) * np.eye(d, dtype=LD)
    assert (~plastic).any() and np.all(ref[~plastic] == C_el[None])
    assert float(np.abs(C[~plastic] - ref[~plastic]).max()) <= tol
    # the mark of the reference's 0/0 point: every entry NaN
    marked, _ = vm_tangent_from_state(VM, s[:1], np.array([-0.0]))
    assert np.isnan(marked).all()
