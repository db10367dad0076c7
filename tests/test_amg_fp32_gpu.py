"""dxo_amg_set_precision on the device: the single-precision cycle against the float32 oracle of tests/test_amg_fp32_oracle_cpu.py walked
over the device's own (float64) levels, the three Krylov methods with it, switching back and forth, the refresh of the copies by a
setup, bit identity (two objects, two setups, a captured graph) and the errors.

The cases are those of tests/test_amg_kcycle_gpu.py: the smallest shapes that reach every instantiation of the cycle kernels, through
the 2 -> 3 -> 3 and 3 -> 6 -> 6 rectangular transfers, both smoothers, the masked path and a four-level recursion."""
import ctypes as C

import numpy as np
import pytest

from oracle.amg_oracle import cycle_ref
from solver_cases import (CASES, NOT_DOUBLE, SAME_FORMULAS, _case_hierarchy, _cuda, _device_levels, _heat, _torch,
                          meshes)  # noqa: F401  (meshes is a fixture)

pytestmark = pytest.mark.gpu

SYMMETRIC = ("p2_rbm", "hex_bar", "aniso_soc")      # eps/eps and grad/grad; the heat Jacobian (grad / value_grad) is not counted


def _fp32_bytes(amg):
    """4 x (values + dinv + p_val of every level but the coarsest, + five vectors r, xa, xb, t, d per such level, + r and xa of the
    coarsest); a hierarchy of one level allocates nothing."""
    if amg.n_levels == 1:
        return 0
    dev, entries = amg.levels, 0
    for l, d in enumerate(dev[:-1]):
        bs, bsc = d["bs"], dev[l + 1]["bs"]
        p_blocks = amg.prolongator(l).data.shape[0]
        entries += d["block_nnz"] * bs * bs + d["nodes"] * bs * bs + p_blocks * bs * bsc + 5 * d["rows"]
    return 4 * (entries + 2 * dev[-1]["rows"])


@pytest.mark.parametrize("which", list(CASES))
def test_fp32_cycle_matches_the_float32_oracle_on_the_device_levels(ctx, meshes, which):
    torch = _torch(ctx)
    A, amg = _case_hierarchy(ctx, meshes, which, precision="fp32")
    n_levels, sizes = CASES[which]
    assert amg.n_levels == n_levels and [d["bs"] for d in amg.levels] == sizes, (which, amg.levels)
    assert amg.precision == "fp32" and amg.cycle == "V"
    levels = _device_levels(amg)
    rng = np.random.Generator(np.random.PCG64(12))
    worst = 0.0
    for _ in range(3):
        r = rng.normal(size=A.shape[0])
        zd = amg.apply(_cuda(r))
        assert zd.dtype == torch.float64
        z_dev = zd.cpu().numpy()
        z64 = cycle_ref(levels, r)
        z32 = cycle_ref(levels, r, precision="fp32").astype(np.float64)
        e_ref = np.linalg.norm(z32 - z64) / np.linalg.norm(z64)
        e_dev = np.linalg.norm(z_dev - z64) / np.linalg.norm(z64)
        print(f"{which}: FP32_SEEN e_dev / e_ref {e_dev / e_ref:.3f} (e_dev {e_dev:.3e}, e_ref {e_ref:.3e})")
        worst = max(worst, e_dev / e_ref)
        assert np.isfinite(z_dev).all()
        assert e_dev <= SAME_FORMULAS * e_ref, (which, e_dev, e_ref)
        assert e_dev >= NOT_DOUBLE * e_ref, (which, e_dev, e_ref)
    print(f"{which}: FP32_SEEN largest e_dev / e_ref {worst:.3f}")
    buf = _cuda(r)
    amg.apply(buf, out=buf)                                                        # r may be z
    assert np.array_equal(buf.cpu().numpy(), z_dev)
    z0 = amg.apply(torch.zeros(A.shape[0], dtype=torch.float64, device="cuda"))
    assert not z0.any().item()
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", list(CASES))
def test_solvers_take_the_fp32_hierarchy(ctx, meshes, which):
    from dolfinx_external_operator_amd import cg, fgmres, gmres

    _torch(ctx)
    A, amg = _case_hierarchy(ctx, meshes, which, precision="fp32")
    S = A.to_scipy()
    asym = abs(S - S.T).max() / abs(S).max()
    assert asym <= 1e-12 or which not in SYMMETRIC, (which, asym)
    b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
    bd, bnorm = _cuda(b), np.linalg.norm(b)
    solvers = {"fgmres": lambda: fgmres(A, bd, M=amg, restart=30, rtol=1e-10), "gmres": lambda: gmres(A, bd, M=amg, restart=30, rtol=1e-10)}
    if which in SYMMETRIC:
        solvers["cg"] = lambda: cg(A, bd, M=amg, rtol=1e-10)
    single = {}
    for name, solve in solvers.items():
        out = solve()
        res = np.linalg.norm(b - S @ out.x.cpu().numpy())
        print(f"{which}: {name} with the fp32 cycle: {out.iterations} iterations, |b - A x| / |b| {res / bnorm:.3e}")
        assert out.converged, (which, name)
        assert res <= 2e-10 * bnorm, (which, name, res / bnorm)
        single[name] = out.iterations
    assert amg.set_precision("fp64").setup().precision == "fp64"                    # the same object, the same calls
    for name, solve in solvers.items():
        its = solve().iterations
        print(f"{which}: {name} iterations fp64 / fp32 cycle {its} / {single[name]}")
        assert abs(single[name] - its) <= (30 if name == "gmres" else 2), (which, name, single[name], its)


@pytest.mark.parametrize("which", ["heat48", "hex_bar", "heat48_cheby"])
def test_switching(ctx, meshes, which):
    torch = _torch(ctx)
    A, default = _case_hierarchy(ctx, meshes, which)
    r = _cuda(np.random.Generator(np.random.PCG64(1)).normal(size=A.shape[0]))
    z_default = default.apply(r).clone()
    assert default.precision == "fp64" and default.fp32_bytes == 0
    _, spelled = _case_hierarchy(ctx, meshes, which, precision="fp64")
    assert spelled.fp32_bytes == 0 and torch.equal(spelled.apply(r), z_default)
    assert default.set_precision("fp64") is default                                # the kind it has: nothing happens, no setup needed
    assert torch.equal(default.apply(r), z_default)
    assert default.set_precision("fp32") is default and default.setup() is default and default.precision == "fp32"
    nbytes = default.fp32_bytes
    assert nbytes == _fp32_bytes(default) > 0
    z32 = default.apply(r).clone()
    assert not torch.equal(z32, z_default)
    default.set_precision("fp64").setup()
    assert default.precision == "fp64" and torch.equal(default.apply(r), z_default)  # and back: the default apply bit for bit
    assert default.fp32_bytes == nbytes
    default.set_precision("fp32").setup()                                          # a second switch allocates nothing
    assert default.fp32_bytes == nbytes and torch.equal(default.apply(r), z32)


@pytest.mark.parametrize("which", ["heat48", "p2_rbm"])
def test_a_setup_refreshes_the_copies(ctx, meshes, which):
    from dolfinx_external_operator_amd.operand_eval import DeviceCSR

    torch = _torch(ctx)
    A, amg = _case_hierarchy(ctx, meshes, which, precision="fp32")
    r = _cuda(np.random.Generator(np.random.PCG64(3)).normal(size=A.shape[0]))
    z = amg.apply(r).clone()
    A2 = DeviceCSR(A.pattern, 2.0 * A.values)
    z2 = amg.setup(A2).apply(r)
    half = 0.5 * z
    assert torch.linalg.norm(z2 - half).item() <= 1e-5 * torch.linalg.norm(half).item()      # stale copies would be 100 % off


@pytest.mark.parametrize("which", ["heat48", "hex_bar", "heat48_cheby"])
def test_reproducibility(ctx, meshes, which):
    torch = _torch(ctx)
    A, amg = _case_hierarchy(ctx, meshes, which, precision="fp32")
    r = _cuda(np.random.Generator(np.random.PCG64(1)).normal(size=A.shape[0]))
    z32 = amg.apply(r).clone()
    _, twin = _case_hierarchy(ctx, meshes, which, precision="fp32")
    assert torch.equal(twin.apply(r), z32)                                         # two objects built alike
    amg.setup()
    assert torch.equal(amg.apply(r), z32)                                          # two setups of one object
    z = torch.zeros_like(r)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ctx.set_stream(s.cuda_stream)
            amg.apply(r, out=z)
    torch.cuda.current_stream().wait_stream(s)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        z.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(z, z32)                                                 # a captured graph is the eager call


def test_errors(ctx, meshes, hip_library):
    torch = _torch(ctx)
    lib, h = hip_library, ctx._h
    A, amg = _case_hierarchy(ctx, meshes, "heat48")
    r = _cuda(np.random.Generator(np.random.PCG64(1)).normal(size=A.shape[0]))
    z = amg.apply(r).clone()
    for bad in ("fp16", "FP32", None, 32):
        with pytest.raises(ValueError, match="AMG: precision"):
            amg.set_precision(bad)
        with pytest.raises(ValueError, match="AMG: precision"):
            A.amg(None, coarse_rows=10, precision=bad)
    assert lib.dxo_amg_set_precision(None, amg._h, 1) == -1 and lib.dxo_amg_set_precision(h, None, 1) == -1
    assert lib.dxo_amg_set_precision(h, amg._h, 2) == -6 and lib.dxo_amg_set_precision(h, amg._h, -1) == -6
    kind, nbytes = C.c_int(-1), C.c_int64(-1)
    assert lib.dxo_amg_precision_info(h, None, C.byref(kind), C.byref(nbytes)) == -1
    assert lib.dxo_amg_precision_info(h, amg._h, None, None) == 0
    assert lib.dxo_amg_precision_info(h, amg._h, C.byref(kind), C.byref(nbytes)) == 0 and (kind.value, nbytes.value) == (0, 0)
    assert torch.equal(amg.apply(r), z)                                            # refused calls change nothing
    # between set_precision and setup there is no cycle
    amg.set_precision("fp32")
    with pytest.raises(ValueError, match="DXO_E_OPTION.*dxo_amg_setup"):
        amg.apply(r)
    # K and fp32 exclude each other, in both orders, and the object stays usable
    with pytest.raises(ValueError, match="DXO_E_OPTION.*dxo_amg_set_precision"):
        amg.set_cycle("K")
    assert amg.cycle == "V" and amg.precision == "fp32"
    z32 = amg.setup().apply(r).clone()
    assert not torch.equal(z32, z)
    amg.set_precision("fp64").setup().set_cycle("K")
    with pytest.raises(ValueError, match="DXO_E_OPTION.*dxo_amg_set_cycle"):
        amg.set_precision("fp32")
    assert amg.cycle == "K" and amg.precision == "fp64"
    amg.apply(r)                                                                   # still ready: the refused call changed nothing
    assert torch.equal(amg.set_cycle("V").apply(r), z)
    with pytest.raises(ValueError, match="DXO_E_OPTION.*dxo_amg_set_cycle"):
        _case_hierarchy(ctx, meshes, "heat48", cycle="K", precision="fp32")
    assert torch.equal(amg.set_precision("fp32").setup().apply(r), z32)


def _scaled(ctx, meshes, scale):
    from dolfinx_external_operator_amd.operand_eval import DeviceCSR

    A, bcs = _heat(ctx, meshes, 48)
    return DeviceCSR(A.pattern, scale * A.values), bcs


def test_an_entry_beyond_the_range_of_float_fails_the_fp32_setup(ctx, meshes):
    """Values scaled by 1e60: finite in double, infinite in float. The fp64 setup succeeds, the fp32 setup answers DXO_E_OPTION and
    names level 0; no fault, no abort, and the object can go back to fp64."""
    torch = _torch(ctx)
    A, bcs = _scaled(ctx, meshes, 1e60)
    amg = A.amg(bcs, coarse_rows=10)
    r = _cuda(np.random.Generator(np.random.PCG64(1)).normal(size=A.shape[0]))
    z = amg.apply(r).clone()
    assert torch.isfinite(z).all().item()
    amg.set_precision("fp32")
    with pytest.raises(ValueError, match="DXO_E_OPTION.*level 0.*float"):
        amg.setup()
    with pytest.raises(ValueError, match="DXO_E_OPTION.*dxo_amg_setup"):
        amg.apply(r)
    with pytest.raises(ValueError, match="DXO_E_OPTION.*level 0.*float"):
        A.amg(bcs, coarse_rows=10, precision="fp32")
    assert torch.equal(amg.set_precision("fp64").setup().apply(r), z)
    # underflow to zero is not an error: one off-diagonal entry of 1e-200 in a matrix of ordinary size
    from dolfinx_external_operator_amd.operand_eval import DeviceCSR

    B, _ = _scaled(ctx, meshes, 1.0)
    indptr, indices, values = B.to_numpy()
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    e = int(np.flatnonzero((indices != rows) & (values != 0.0))[0])
    v = B.values.clone()
    v[e] = 1e-200
    small = DeviceCSR(B.pattern, v).amg(bcs, coarse_rows=10, precision="fp32")
    assert np.float32(1e-200) == 0.0 and torch.isfinite(small.apply(r)).all().item()


def test_values_scaled_by_1e300_fail_the_fp32_setup(ctx, meshes):
    """setup on values scaled by 1e300 raises ValueError under fp32: an error return that names the level, no fault and no abort."""
    _torch(ctx)
    A, bcs = _scaled(ctx, meshes, 1e300)
    with pytest.raises(ValueError, match="DXO_E_OPTION.*level 0.*float"):
        A.amg(bcs, coarse_rows=10, precision="fp32")


def test_values_scaled_by_1e300_pass_the_fp64_setup(ctx, meshes):
    """setup on values scaled by 1e300 succeeds under fp64: invert_block works on the block scaled by a power of two, so neither the
    determinant nor the squared row norms of its singularity test overflow (tests/test_block_inverse_scale_gpu.py)."""
    torch = _torch(ctx)
    A, bcs = _scaled(ctx, meshes, 1e300)
    amg = A.amg(bcs, coarse_rows=10)
    r = _cuda(np.random.Generator(np.random.PCG64(1)).normal(size=A.shape[0]))
    assert torch.isfinite(amg.apply(r)).all().item()
