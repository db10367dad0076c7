"""invert_block (csrc/krylov_internal.h) does not depend on the scale of a block: the block-Jacobi inverses of every multigrid level
(block sizes 1, 2, 3 and, on the coarse levels with rigid-body modes, 6) of a matrix scaled by a power of two are the inverses of
the unscaled matrix times the inverse power, bit for bit, and the setup succeeds where the determinant or the squared row norms
of the unscaled block would overflow (2^996, about 1e300) or underflow (2^-900). Every operation of the numeric phase commutes
exactly with a power of two as long as nothing leaves the range of double, so omega and P are equal and the coarse matrices scaled."""
import numpy as np
import pytest

from solver_cases import _case_hierarchy, _cuda, _torch, meshes  # noqa: F401  (meshes is a fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which", ["heat48", "p2_rbm", "hex_bar"])
def test_the_setup_commutes_with_a_power_of_two(ctx, meshes, which):
    from dolfinx_external_operator_amd.operand_eval import DeviceCSR

    torch = _torch(ctx)
    A, amg = _case_hierarchy(ctx, meshes, which)
    r = _cuda(np.random.Generator(np.random.PCG64(4)).normal(size=A.shape[0]))
    z = amg.apply(r).clone()
    dinv = [amg.level_dinv(l) for l in range(amg.n_levels - 1)]
    omega = [d["omega"] for d in amg.levels]
    assert sorted({d["bs"] for d in amg.levels}) == {"heat48": [1], "p2_rbm": [2, 3], "hex_bar": [3, 6]}[which]
    for e in (996, -900):
        s = 2.0 ** e
        amg.setup(DeviceCSR(A.pattern, s * A.values))
        assert [d["omega"] for d in amg.levels] == omega, (which, e)
        for l, d in enumerate(dinv):
            assert np.array_equal(amg.level_dinv(l), d / s), (which, e, l)
        assert torch.equal(amg.apply(r), z / s), (which, e)
