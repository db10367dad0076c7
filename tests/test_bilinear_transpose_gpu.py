"""dxo_bilinear_apply_t on the device: the action of the transposed bilinear form on the forward call's (test, trial) and C, against
the NumPy reference pinned in tests/test_transpose_oracle_cpu.py (the forward reference with the kinds swapped and the blocks
transposed) and against the device's own forward action (duality)."""
import ctypes as C

import numpy as np
import pytest

from oracle.form_oracle import bilinear_ref
from solver_cases import CELLS, PAIRS, _cuda, _zeros
from transpose_cases import form_mesh, random_blocks

pytestmark = pytest.mark.gpu


def _apply(ctx, dm, which, test, trial, bs, Cd, vd, out):
    import torch

    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    getattr(dm, which)(test, trial, bs, Cd.data_ptr(), vd.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("degree", [1, 2])
def test_every_pair_matches_the_reference_and_is_dual_to_the_forward_action(ctx, cell, degree):
    """Blocks of 1, 9 and 81 doubles (8-byte loads), 6 and 12 (non-square), 16 and 36 (held), 81 (streamed). ("F", "grad") and its
    kin are taken as their linearisation."""
    import torch

    from dolfinx_external_operator_amd import DeviceMesh

    m = form_mesh(cell, degree)
    G, nn = m.gdim, m.node_x.shape[0]
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    rng = np.random.Generator(np.random.PCG64(13))
    try:
        for test, trial, vector in PAIRS:
            bs = G if vector else 1
            n = nn * bs
            Cb = random_blocks(m, test, trial, bs, rng)
            Cd = _cuda(Cb)
            v, w = rng.normal(size=n), rng.normal(size=n)
            vd, wd = _cuda(v), _cuda(w)
            ref = bilinear_ref(m, trial, test, bs, np.ascontiguousarray(Cb.transpose(0, 2, 1)), w)
            Ktw = _apply(ctx, dm, "bilinear_apply_t", test, trial, bs, Cd, wd, _zeros(n))
            err = np.abs(Ktw.cpu().numpy() - ref).max()
            print(f"{cell} P{degree} {test}/{trial} bs {bs}: {err / np.abs(ref).max():.2e} of max|ref|")
            assert err <= 1e-12 * np.abs(ref).max(), (test, trial, bs, err)
            # duality on the device, forward and transposed on the same C
            Kv = _apply(ctx, dm, "bilinear_apply", test, trial, bs, Cd, vd, _zeros(n))
            a, b = float(torch.dot(wd, Kv)), float(torch.dot(vd, Ktw))
            assert abs(a - b) <= 1e-12 * float(torch.dot(wd.abs(), Kv.abs())), (test, trial, bs, a, b)
            # accumulated into; two calls give identical bits
            base = rng.normal(size=n)
            acc = _apply(ctx, dm, "bilinear_apply_t", test, trial, bs, Cd, wd, _cuda(base))
            assert np.abs(acc.cpu().numpy() - base - ref).max() <= 1e-12 * np.abs(ref).max() + 4e-16 * np.abs(base).max()
            again = _apply(ctx, dm, "bilinear_apply_t", test, trial, bs, Cd, wd, _zeros(n))
            assert torch.equal(again, Ktw)
            # consumer_overwrite = 1: out prefilled with NaN is SET
            ctx.set_option("consumer_overwrite", 1)
            try:
                nan = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
                got = _apply(ctx, dm, "bilinear_apply_t", test, trial, bs, Cd, wd, nan)
            finally:
                ctx.set_option("consumer_overwrite", 0)
            assert torch.equal(got, Ktw), (test, trial, bs)
    finally:
        dm.close()


def test_error_paths_are_the_forward_calls(ctx):
    import torch

    from dolfinx_external_operator_amd import DeviceMesh
    from oracle.operand_oracle import DEFGRAD, GRAD, VALUE
    from tools.synthetic import structured_mesh

    m = structured_mesh("triangle", (2, 2), 2)
    nn, npts = m.node_x.shape[0], m.num_cells * m.nq
    Cd, vd, out = _zeros(npts * 16), _zeros(nn * 2), _zeros(nn * 2)
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    try:
        with pytest.raises(ValueError, match="unsupported pair"):
            dm.bilinear_apply_t("grad", "eps", 2, Cd.data_ptr(), vd.data_ptr(), out.data_ptr())
        with pytest.raises(ValueError, match="unsupported pair"):
            dm.bilinear_apply_t("value_grad", "grad", 1, Cd.data_ptr(), vd.data_ptr(), out.data_ptr())      # the swap is not in the table
        lib, P = ctx.lib, C.c_void_p
        for t, r, bs in ((GRAD, VALUE, 1), (5, 5, 2), (GRAD, 7, 1), (DEFGRAD, DEFGRAD, 1)):
            rc = lib.dxo_bilinear_apply_t(ctx._h, dm._h, t, r, bs, P(Cd.data_ptr()), P(vd.data_ptr()), P(out.data_ptr()))
            assert rc == -6, (t, r, bs)
            assert "dxo_bilinear_apply_t" in lib.dxo_last_error(ctx._h).decode()
        rc = lib.dxo_bilinear_apply_t(ctx._h, dm._h, GRAD, GRAD, 2, P(Cd.data_ptr() + 8), P(vd.data_ptr()), P(out.data_ptr()))
        assert rc == -5
        assert lib.dxo_bilinear_apply_t(ctx._h, dm._h, GRAD, GRAD, 2, P(Cd.data_ptr()), None, P(out.data_ptr())) == -1
    finally:
        dm.close()
    torch.cuda.synchronize()
