"""The NumPy yardstick of dxo_bilinear_apply / dxo_bilinear_diagonal, pinned on the CPU.

The reference of the bilinear action is a composition of the existing oracle functions,
    K v = operand_adjoint(test, C : eval_operand(trial, v)),
and of its diagonal the probes e_i . K e_i. These tests pin that composition against what the reference's Jacobian forms mean:
the central finite difference of the hyperelastic residual inner(grad v, P(I + grad u)) dx (demo_hyperelasticity.py:527-529), its
symmetry for the Isihara tangent, and the heat demo's explicit Jacobian form (demo_nonlinear_heat_equation_part2.py:328-329)."""
import numpy as np

from oracle.form_oracle import bilinear_diag_ref, bilinear_ref, tables
from oracle.icnn_oracle import isihara_stress_tangent
from oracle.operand_oracle import DEFGRAD, GRAD, VALUE, eval_operand, operand_adjoint, tangent_apply
from tools.synthetic import structured_mesh


def _hyper_setup(seed=0):
    m = structured_mesh("triangle", (3, 3), degree=2, distort=0.2, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed))
    u = 0.01 * rng.normal(size=m.node_x.shape[0] * 2)         # det F > 0 everywhere

    def tangent(uu):
        F = eval_operand(DEFGRAD, 2, uu, *tables(m)).reshape(-1, 4)
        return isihara_stress_tangent(F)

    def residual(uu):
        _, P = tangent(uu)
        return operand_adjoint(DEFGRAD, 2, P.reshape(m.num_cells, m.nq, 4), m.weights, *tables(m), m.node_x.shape[0])

    return m, rng, u, tangent, residual


def test_hyperelastic_action_is_the_derivative_of_the_residual():
    m, rng, u, tangent, residual = _hyper_setup()
    dP, _ = tangent(u)
    v = rng.normal(size=u.size)
    Kv = bilinear_ref(m, "grad", "grad", 2, dP, v)
    h = 1e-6                                                                   # truncation ~h^2, round-off ~1e-16 / h
    fd = (residual(u + h * v) - residual(u - h * v)) / (2 * h)
    assert np.abs(Kv - fd).max() <= 1e-7 * np.abs(Kv).max()
    # DEFGRAD on either side is the same form (its linearisation is grad)
    assert np.array_equal(bilinear_ref(m, "F", "F", 2, dP, v), Kv)


def test_hyperelastic_action_is_symmetric():
    m, rng, u, tangent, _ = _hyper_setup(seed=1)
    dP, _ = tangent(u)
    v, w = rng.normal(size=u.size), rng.normal(size=u.size)
    a, b = w @ bilinear_ref(m, "grad", "grad", 2, dP, v), v @ bilinear_ref(m, "grad", "grad", 2, dP, w)
    assert abs(a - b) <= 1e-12 * max(abs(a), 1.0)


def test_eps_pair_is_tangent_apply():
    m = structured_mesh("quadrilateral", (3, 2), degree=2, distort=0.2, seed=2)
    rng = np.random.Generator(np.random.PCG64(2))
    C = rng.normal(size=(m.num_cells * m.nq, 4, 4))
    v = rng.normal(size=m.node_x.shape[0] * 2)
    ref = tangent_apply(C, v, m.weights, *tables(m), m.node_x.shape[0])
    assert np.abs(bilinear_ref(m, "eps", "eps", 2, C, v) - ref).max() <= 1e-13 * np.abs(ref).max()


def _heat_setup():
    """The heat demo's setting: unit square 10 x 10, P1, degree-2 rule, T = x^2 + y, k = 1 / (A + B T) (part2.py:209-210)."""
    m = structured_mesh("triangle", (10, 10), degree=1)
    A, B = 1.0, 1.0
    T = m.node_x[:, 0] ** 2 + m.node_x[:, 1]

    def flux(TT):
        Tq = eval_operand(VALUE, 1, TT, *tables(m))[..., 0]
        s = eval_operand(GRAD, 1, TT, *tables(m))
        k = 1.0 / (A + B * Tq)
        return Tq, s, k

    return m, A, B, T, flux


def test_heat_action_is_the_explicit_jacobian_form():
    m, A, B, T, flux = _heat_setup()
    Tq, s, k = flux(T)
    dqdT = B * k[..., None] ** 2 * s                                          # q = -k sigma
    dqds = -k[..., None, None] * np.eye(2)
    Cb = np.concatenate([dqdT[..., None], dqds], axis=-1)                      # [g][1 + g]: [dq/dT | dq/dsigma]
    rng = np.random.Generator(np.random.PCG64(4))
    That = rng.normal(size=T.size)
    act = bilinear_ref(m, "grad", "value_grad", 1, Cb, That)
    # J_manual = inner(B k^2 sigma T_hat, grad T~) dx + inner(-k I grad T_hat, grad T~) dx
    Th = eval_operand(VALUE, 1, That, *tables(m))
    gTh = eval_operand(GRAD, 1, That, *tables(m))
    S = B * k[..., None] ** 2 * s * Th - k[..., None] * gTh
    manual = operand_adjoint(GRAD, 1, S, m.weights, *tables(m), m.node_x.shape[0])
    assert np.abs(act - manual).max() <= 1e-13 * np.abs(manual).max()
    # and the derivative of the flux residual inner(q, grad T~) dx
    def residual(TT):
        _, ss, kk = flux(TT)
        return operand_adjoint(GRAD, 1, -kk[..., None] * ss, m.weights, *tables(m), m.node_x.shape[0])
    h = 1e-6
    fd = (residual(T + h * That) - residual(T - h * That)) / (2 * h)
    assert np.abs(act - fd).max() <= 1e-7 * np.abs(act).max()


def test_diagonal_by_probes_is_the_diagonal():
    """The colouring shortcut of the diagonal agrees with one probe per dof."""
    m = structured_mesh("triangle", (2, 2), degree=2, distort=0.2, seed=5)
    rng = np.random.Generator(np.random.PCG64(5))
    C = rng.normal(size=(m.num_cells * m.nq, 3, 3))
    n = m.node_x.shape[0]
    full = np.array([bilinear_ref(m, "value_grad", "value_grad", 1, C, np.eye(n)[k])[k] for k in range(n)])
    assert np.allclose(bilinear_diag_ref(m, "value_grad", "value_grad", 1, C), full, rtol=0, atol=1e-14 * np.abs(full).max())
