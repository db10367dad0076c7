"""dxo_amg_set_cycle on the device against the K-cycle oracle of tests/test_fgmres_kcycle_oracle_cpu.py, walked over the device's own
level matrices, prolongators, block inverses, omega and rho: the cycle itself, the level visits, bit identity (two applies, a captured
graph, K -> V, two levels), the guards, and the Krylov methods that take it and refuse it."""
import numpy as np
import pytest

from oracle.amg_oracle import cycle_ref, fgmres_with_cycle, k_visits
from solver_cases import (CASES, K_CYCLE_TOL, _assembled_system, _case_hierarchy, _cuda, _device_levels, _torch,
                          meshes)  # noqa: F401  (meshes is a fixture)

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("which", list(CASES))
def test_k_cycle_matches_the_oracle_on_the_device_levels(ctx, meshes, which):
    torch = _torch(ctx)
    A, amg = _case_hierarchy(ctx, meshes, which, cycle="K")
    n_levels, sizes = CASES[which]
    assert amg.n_levels == n_levels and [d["bs"] for d in amg.levels] == sizes, (which, amg.levels)
    assert amg.cycle == "K"
    # level l is visited 2^l times, the coarsest as often as the level above it: sum_{l < L - 1} 2^l + 2^(L - 2)
    assert amg.visits == sum(2 ** l for l in range(n_levels - 1)) + 2 ** (n_levels - 2) == k_visits(n_levels)
    levels = _device_levels(amg)
    rng = np.random.Generator(np.random.PCG64(12))
    worst, visits = 0.0, [0] * n_levels
    for _ in range(3):
        r = rng.normal(size=A.shape[0])
        z = amg.apply(_cuda(r)).cpu().numpy()
        zr = cycle_ref(levels, r, "K", visits=visits)
        assert np.isfinite(z).all()
        worst = max(worst, np.linalg.norm(z - zr) / np.linalg.norm(zr))
    assert sum(visits) == 3 * amg.visits
    zv = cycle_ref(levels, r)
    print(f"{which}: K_CYCLE_SEEN {worst:.3e} |z| (K against V on this right-hand side: {np.linalg.norm(zr - zv) / np.linalg.norm(zv):.3e})")
    assert worst <= K_CYCLE_TOL, (which, worst)
    buf = _cuda(r)
    amg.apply(buf, out=buf)                                                        # r may be z
    assert np.array_equal(buf.cpu().numpy(), z)
    # the guards: r = 0 gives exactly 0
    z0 = amg.apply(torch.zeros(A.shape[0], dtype=torch.float64, device="cuda"))
    assert not z0.any().item() and torch.isfinite(z0).all().item()
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", ["heat48", "hex_bar", "heat48_cheby"])
def test_bit_identity(ctx, meshes, which):
    torch = _torch(ctx)
    A, amg = _case_hierarchy(ctx, meshes, which)
    assert amg.cycle == "V" and amg.visits == amg.n_levels
    r = _cuda(np.random.Generator(np.random.PCG64(1)).normal(size=A.shape[0]))
    z_v = amg.apply(r).clone()
    assert amg.set_cycle("K") is amg and amg.cycle == "K"
    z_k = amg.apply(r).clone()                                                    # at once, without a setup
    assert not torch.equal(z_k, z_v)
    for _ in range(2):
        assert torch.equal(amg.apply(r), z_k)                                     # two applies
    _, fresh = _case_hierarchy(ctx, meshes, which, cycle="K")
    assert torch.equal(fresh.apply(r), z_k)                                       # set at creation or afterwards
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
        assert torch.equal(z, z_k)                                                # a captured graph is the eager call
    amg.setup()
    assert amg.cycle == "K" and torch.equal(amg.apply(r), z_k)                    # a setup keeps the cycle
    amg.set_cycle("V")
    assert amg.cycle == "V" and torch.equal(amg.apply(r), z_v)                    # and back: the default object bit for bit
    _, default = _case_hierarchy(ctx, meshes, which)
    assert torch.equal(default.apply(r), z_v)


def test_k_on_two_levels_and_on_one_is_v(ctx, meshes):
    torch = _torch(ctx)
    A, bs, bcs = _assembled_system(ctx, meshes, "heat")
    r = _cuda(np.random.Generator(np.random.PCG64(2)).normal(size=A.shape[0]))
    for coarse_rows, n_levels in ((60, 2), (400, 1)):
        v, k = A.amg(bcs, coarse_rows=coarse_rows), A.amg(bcs, coarse_rows=coarse_rows, cycle="K")
        assert v.n_levels == k.n_levels == n_levels and k.cycle == "K" and k.visits == v.visits == n_levels
        assert torch.equal(k.apply(r), v.apply(r))


@pytest.mark.parametrize("which", ["heat48", "p2_rbm"])
def test_krylov_methods_take_it_or_refuse_it(ctx, meshes, which):
    from dolfinx_external_operator_amd import cg, fgmres, gmres

    _torch(ctx)
    A, amg = _case_hierarchy(ctx, meshes, which, cycle="K")
    S = A.to_scipy()
    b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
    bd = _cuda(b)
    for solve in (gmres, cg):
        with pytest.raises(ValueError, match="DXO_E_OPTION.*K-cycle"):
            solve(A, bd, M=amg)
    out = fgmres(A, bd, M=amg, restart=30, rtol=1e-8)
    _, its, conv, *_ = fgmres_with_cycle(S, b, _device_levels(amg), "K", m=30, rtol=1e-8)
    v = gmres(A, bd, M=amg.set_cycle("V"), restart=30, rtol=1e-8)                 # the same object, as a V-cycle again
    print(f"{which}: FGMRES(30) + K {out.iterations} iterations (oracle {its}) x {k_visits(amg.n_levels)} visits, "
          f"GMRES(30) + V {v.iterations} x {amg.n_levels}")
    assert out.converged and conv and v.converged
    assert np.linalg.norm(b - S @ out.x.cpu().numpy()) <= 1e-8 * np.linalg.norm(b) * (1 + 1e-6)
    assert abs(out.iterations - its) <= 2, (which, out.iterations, its)


def test_errors(ctx, meshes, hip_library):
    import ctypes as C

    lib, h = hip_library, ctx._h
    A, bs, bcs = _assembled_system(ctx, meshes, "heat")
    amg = A.amg(bcs, coarse_rows=10)
    for bad in ("W", "k", None):
        with pytest.raises(ValueError, match="AMG: cycle"):
            amg.set_cycle(bad)
        with pytest.raises(ValueError, match="AMG: cycle"):
            A.amg(bcs, coarse_rows=10, cycle=bad)
    assert lib.dxo_amg_set_cycle(None, amg._h, 1) == -1 and lib.dxo_amg_set_cycle(h, None, 1) == -1
    assert lib.dxo_amg_set_cycle(h, amg._h, 2) == -6 and lib.dxo_amg_set_cycle(h, amg._h, -1) == -6
    assert amg.cycle == "V"                                                        # a refused call changes nothing
    kind, visits = C.c_int(-1), C.c_int64(-1)
    assert lib.dxo_amg_cycle_info(h, None, C.byref(kind), C.byref(visits)) == -1
    assert lib.dxo_amg_cycle_info(h, amg._h, None, None) == 0
    assert lib.dxo_amg_cycle_info(h, amg._h, C.byref(kind), C.byref(visits)) == 0 and (kind.value, visits.value) == (0, amg.n_levels)
