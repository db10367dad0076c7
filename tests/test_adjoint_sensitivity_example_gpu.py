"""examples/device_adjoint_sensitivity.py: the gradient of J = int T^2 dx + int g(T) ds of the Robin heat problem with respect to
(h, c, A, B) from one adjoint solve, with the transposed assembled Jacobian and matrix-free, against central differences.

The yardstick is the finite difference's own error estimate, from forward solves only (no new code): the error of a second-order
central difference at step s/2 is a third of |FD(s) - FD(s/2)|, so |adjoint - FD(s/2)| <= |FD(s) - FD(s/2)| carries a factor 3 of
margin; and the estimate must lie below 1e-4 of the gradient, or the comparison would be vacuous. With s = 5e-3 of the parameter the
estimates measured on an MI355X are 5.5e-7 .. 7.6e-7 of the gradient (1.98e-7, 1.77e-7, 3.68e-8, 4.07e-8 for h, c, A, B) and the
adjoint gradient lies 6.60e-8, 5.89e-8, 1.23e-8, 1.36e-8 from FD(s/2), assembled and matrix-free alike: a third of the estimate, as
the theory says. Truncation dominates; the floor of Newton's tolerance is not reached and nothing is widened."""
import importlib.util
import pathlib

import pytest

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _example():
    spec = importlib.util.spec_from_file_location("device_adjoint_sensitivity", ROOT / "examples" / "device_adjoint_sensitivity.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("matrix_free", [False, True], ids=["assembled", "matrix-free"])
def test_adjoint_gradient_lies_within_the_finite_differences_own_error(matrix_free):
    rep = _example().main(n_side=8, matrix_free=matrix_free)
    assert rep["parameters"] == ["h", "c", "A", "B"]
    for name, grad, fd_h, fd_h2 in zip(rep["parameters"], rep["gradient"], rep["fd_h"], rep["fd_h2"]):
        est = abs(fd_h - fd_h2)
        print(f"dJ/d{name}: adjoint {grad:.12e}, FD(s/2) {fd_h2:.12e}, |adjoint - FD(s/2)| {abs(grad - fd_h2):.3e}, "
              f"estimate {est:.3e} = {est / abs(grad):.2e} of the gradient")
        assert est <= 1e-4 * abs(grad), (name, est, grad)
        assert abs(grad - fd_h2) <= est, (name, grad, fd_h2, est)
