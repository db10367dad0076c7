"""dxo_amg_* on the device against the NumPy / SciPy oracle of tests/test_amg_oracle_cpu.py: aggregates and patterns exactly, omega,
P and the coarse matrices within the forward bound of a sum in another order (each kernel on the device's own inputs), the cycle and
the preconditioned solves against the oracle cycle."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg

from oracle.amg_oracle import (U, amg_ref, block_diag, cg_with_cycle, coarse_mask_ref, cycle_ref, forward_bound, gmres_with_cycle,
                               operator_complexity, prolongator_ref, rho_ref, same_csr, tentative_ref)
from oracle.form_oracle import heat_setting
from oracle.krylov_oracle import block_jacobi_ref, bottom_dofs, boundary_dofs, elastic_C, gmres_ref
from solver_cases import CYCLE_TOL, _assemble, _assembled_system, _cuda, _torch, meshes  # noqa: F401  (meshes is a fixture)
from tools.synthetic import structured_mesh

pytestmark = pytest.mark.gpu

SYSTEMS = ["heat", "hyperelastic", "hex_eps", "spd_quad"]


COARSE_ROWS = 40        # small enough for three levels at the test sizes


@pytest.mark.parametrize("which", SYSTEMS)
def test_hierarchy_and_cycle_match_the_oracle(ctx, meshes, which):
    torch = _torch(ctx)
    A, bs, bcs = _assembled_system(ctx, meshes, which)
    S = A.to_scipy()
    amg = A.amg(bcs, coarse_rows=COARSE_ROWS)
    ref = amg_ref(S, bs, bcs, coarse_rows=COARSE_ROWS)
    dev = amg.levels
    assert amg.n_levels == len(ref) >= 2, (which, amg.n_levels, len(ref))
    assert [d["rows"] for d in dev] == [L.n_rows for L in ref]
    assert [d["block_nnz"] * bs * bs for d in dev] == [L.indices.size for L in ref]
    assert abs(amg.operator_complexity - operator_complexity(ref)) <= 1e-12
    mask = np.zeros(S.shape[0], dtype=bool)
    mask[bcs] = True
    for l, L in enumerate(ref[:-1]):
        # integers: exactly
        Al = amg.level_matrix(l)
        assert np.array_equal(Al.indptr, L.indptr) and np.array_equal(Al.indices, L.indices)
        assert np.array_equal(amg.aggregates(l), L.agg)
        P = amg.prolongator(l)
        assert np.array_equal(P.indptr, L.Pp.indptr) and np.array_equal(P.indices, L.Pp.indices)
        ap_ptr, ap_idx = amg.ap_pattern(l)
        assert np.array_equal(ap_ptr, L.APp.indptr) and np.array_equal(ap_idx, L.APp.indices)
        Ac = amg.level_matrix(l + 1)
        assert np.array_equal(Ac.indptr, ref[l + 1].indptr) and np.array_equal(Ac.indices, ref[l + 1].indices)
        # numbers: every kernel on the device's own inputs, within the forward bound of its sums
        Dinv, omega = amg.level_dinv(l), dev[l]["omega"]
        Dref = block_jacobi_ref(Al, bs)
        assert np.abs(Dinv - Dref).max() <= 1e-12 * np.abs(Dref).max()          # the figure of test_block_jacobi_matches_numpy
        row_nnz = int(np.diff(Al.indptr).max())
        rho, S_rho = rho_ref(Al, Dinv)
        K = bs * row_nnz + bs
        assert abs(omega * rho - 4.0 / 3.0) <= (4.0 / 3.0) * (forward_bound(K, S_rho) / rho + 4 * U), (which, l, omega, rho)
        assert abs(omega - L.omega) <= 1e-10 * L.omega                           # and the end-to-end oracle value
        T = tentative_ref(L.agg, mask, bs, L.n_agg)
        Pd = P.toarray()
        Pref = prolongator_ref(Al, Dinv, omega, T).toarray()
        S_P = (abs(T) + omega * (abs(block_diag(Dinv)) @ (abs(Al) @ abs(T)))).toarray()
        K = row_nnz + bs + 2
        excess = np.abs(Pd - Pref) - forward_bound(K, S_P)
        print(f"{which} level {l}: P max |dev - ref| {np.abs(Pd - Pref).max():.3e}, bound at that entry "
              f"{forward_bound(K, S_P).reshape(-1)[np.abs(Pd - Pref).argmax()]:.3e}")
        assert excess.max() <= 0.0, (which, l, excess.max())
        Psp = sp.csr_matrix(Pd)
        Cref = (Psp.T @ Al @ Psp).toarray()
        d = np.flatnonzero(np.diag(Cref) == 0.0)
        S_C = (abs(Psp).T @ abs(Al) @ abs(Psp)).toarray()
        K = row_nnz * int(np.diff(Psp.tocsc().indptr).max()) + 2
        Cd = Ac.toarray()
        if d.size:                                                               # an exactly zero diagonal entry becomes 1
            assert (Cd[d, d] == 1.0).all()
            Cref[d, d] = 1.0
        excess = np.abs(Cd - Cref) - forward_bound(K, S_C)
        print(f"{which} level {l}: A_c max |dev - ref| {np.abs(Cd - Cref).max():.3e} of {np.abs(Cref).max():.3e}")
        assert excess.max() <= 0.0, (which, l, excess.max())
        mask = coarse_mask_ref(Ac)
        assert np.array_equal(mask, ref[l + 1].mask)
    # the cycle
    rng = np.random.Generator(np.random.PCG64(12))
    worst = 0.0
    for _ in range(3):
        r = rng.normal(size=S.shape[0])
        z = amg.apply(_cuda(r)).cpu().numpy()
        zr = cycle_ref(ref, r)
        worst = max(worst, np.linalg.norm(z - zr) / np.linalg.norm(zr))
    print(f"{which}: cycle deviation from the oracle {worst:.3e} |z|")
    assert worst <= CYCLE_TOL, (which, worst)
    # r may be z
    buf = _cuda(r)
    amg.apply(buf, out=buf)
    assert np.array_equal(buf.cpu().numpy(), z)
    two = A.amg(bcs, coarse_rows=COARSE_ROWS, sweeps=2)
    ref2 = amg_ref(S, bs, bcs, coarse_rows=COARSE_ROWS, sweeps=2)
    z2, zr2 = two.apply(_cuda(r)).cpu().numpy(), cycle_ref(ref2, r)
    assert np.linalg.norm(z2 - zr2) <= CYCLE_TOL * np.linalg.norm(zr2)
    torch.cuda.synchronize()


def test_setup_and_apply_are_bit_reproducible_and_capture_safe(ctx, meshes):
    torch = _torch(ctx)
    m = structured_mesh("triangle", (14, 14), 2)
    bcs = bottom_dofs(m, 2)
    A = _assemble(ctx, meshes(m), "eps", "eps", 2, elastic_C(m, 1), bcs=bcs)
    amg = A.amg(bcs, coarse_rows=COARSE_ROWS)
    assert amg.n_levels >= 3

    def snapshot():
        return ([amg.level_matrix(l) for l in range(amg.n_levels)], [amg.prolongator(l) for l in range(amg.n_levels - 1)],
                [d["omega"] for d in amg.levels])

    first = snapshot()
    r = _cuda(np.random.Generator(np.random.PCG64(1)).normal(size=A.shape[0]))
    z_first = amg.apply(r).clone()
    amg.setup()
    again = snapshot()
    assert all(same_csr(a, b) for a, b in zip(first[0], again[0]))
    assert all(np.array_equal(a.data, b.data) and np.array_equal(a.indices, b.indices) for a, b in zip(first[1], again[1]))
    assert first[2] == again[2]
    for _ in range(2):
        assert torch.equal(amg.apply(r), z_first)
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
        assert torch.equal(z, z_first)


@pytest.mark.parametrize("which", ["heat", "hyperelastic", "hex_eps"])
def test_gmres_with_the_cycle_on_assembled_systems(ctx, meshes, which):
    from dolfinx_external_operator_amd import gmres

    A, bs, bcs = _assembled_system(ctx, meshes, which)
    S = A.to_scipy()
    b = np.random.Generator(np.random.PCG64(8)).normal(size=S.shape[0])
    ref = scipy.sparse.linalg.spsolve(S.tocsc(), b)
    amg = A.amg(bcs, coarse_rows=COARSE_ROWS)
    out = gmres(A, _cuda(b), M=amg, restart=30, rtol=1e-12, maxiter=5000)
    x = out.x.cpu().numpy()
    assert out.converged and not out.breakdown, which
    assert np.linalg.norm(x - ref) <= 1e-8 * np.linalg.norm(ref), which
    levels = amg_ref(S, bs, bcs, coarse_rows=COARSE_ROWS)
    _, its, conv, _ = gmres_with_cycle(S, b, levels, m=30, rtol=1e-12, maxiter=5000)
    _, its_bj, _, _ = gmres_ref(S, b, inv=block_jacobi_ref(S, bs), m=30, rtol=1e-12, maxiter=5000)
    print(f"{which}: GMRES(30) iterations with the cycle {out.iterations} (oracle {its}), block Jacobi oracle {its_bj}")
    assert conv and abs(out.iterations - its) <= 2, (which, out.iterations, its)
    again = gmres(A, _cuda(b), M=amg, restart=30, rtol=1e-12, maxiter=5000)
    assert again.iterations == out.iterations and np.array_equal(again.x.cpu().numpy(), x)


def test_cg_with_the_cycle_on_the_spd_system(ctx, meshes):
    from dolfinx_external_operator_amd import cg

    A, bs, bcs = _assembled_system(ctx, meshes, "spd_quad")
    S = A.to_scipy()
    b = np.random.Generator(np.random.PCG64(9)).normal(size=S.shape[0])
    ref = scipy.sparse.linalg.spsolve(S.tocsc(), b)
    amg = A.amg(bcs, coarse_rows=COARSE_ROWS)
    out = cg(A, _cuda(b), M=amg, rtol=1e-12, maxiter=5000)
    assert out.converged and np.linalg.norm(out.x.cpu().numpy() - ref) <= 1e-8 * np.linalg.norm(ref)
    _, its, conv = cg_with_cycle(S, b, amg_ref(S, bs, bcs, coarse_rows=COARSE_ROWS), rtol=1e-12, maxiter=5000)
    bj = cg(A, _cuda(b), M=A.block_jacobi(), rtol=1e-12, maxiter=5000)
    print(f"spd_quad: CG iterations with the cycle {out.iterations} (oracle {its}), block Jacobi {bj.iterations}")
    assert conv and abs(out.iterations - its) <= 2, (out.iterations, its)
    assert out.iterations < bj.iterations


def test_heat_256_converges_where_block_jacobi_needs_more(ctx, meshes):
    """The P1 heat Jacobian at 256 x 256 (66 049 dofs): block-Jacobi GMRES(30) does not reach rtol 1e-8 in 3000 iterations."""
    from dolfinx_external_operator_amd import gmres

    m, dqdT, dqds, _ = heat_setting(256)
    Cb = np.concatenate([dqdT[..., None], dqds], axis=-1).reshape(m.num_cells * m.nq, 2, 3)
    bcs = boundary_dofs(m, 1)
    A = _assemble(ctx, meshes(m), "grad", "value_grad", 1, -Cb, bcs=bcs)
    S = A.to_scipy()
    b = np.random.Generator(np.random.PCG64(3)).normal(size=S.shape[0])
    amg = A.amg(bcs)
    out = gmres(A, _cuda(b), M=amg, restart=30, rtol=1e-8, maxiter=3000)
    levels = amg_ref(S, 1, bcs)
    assert [d["rows"] for d in amg.levels] == [L.n_rows for L in levels]
    xr, its, conv, _ = gmres_with_cycle(S, b, levels, m=30, rtol=1e-8, maxiter=3000)
    bj = gmres(A, _cuda(b), M=A.block_jacobi(), restart=30, rtol=1e-8, maxiter=3000)
    print(f"heat 256: rows {[d['rows'] for d in amg.levels]}, complexity {amg.operator_complexity:.3f}, symbolic {amg.build_ms:.1f} ms, "
          f"cycle {out.iterations} its in {out.ms:.1f} ms (oracle {its}), block Jacobi {bj.iterations} its in {bj.ms:.1f} ms, "
          f"converged {bj.converged}, residual {bj.residual:.2e}")
    assert out.converged and conv and abs(out.iterations - its) <= 2, (out.iterations, its)
    x = out.x.cpu().numpy()
    assert np.linalg.norm(b - S @ x) <= 1e-8 * np.linalg.norm(b) * (1 + 1e-6)
    assert np.linalg.norm(x - xr) <= 1e-6 * np.linalg.norm(xr)
    assert bj.iterations > out.iterations


def test_setup_alone_follows_a_change_of_the_values(ctx, meshes):
    torch = _torch(ctx)
    m = structured_mesh("triangle", (9, 8), 2, distort=0.1, seed=4)
    dm = meshes(m)
    bcs = bottom_dofs(m, 2)
    A = _assemble(ctx, dm, "eps", "eps", 2, elastic_C(m, 1), bcs=bcs)
    amg = A.amg(bcs, coarse_rows=COARSE_ROWS)
    r = _cuda(np.random.Generator(np.random.PCG64(2)).normal(size=A.shape[0]))
    before = amg.apply(r).clone()
    B = _assemble(ctx, dm, "eps", "eps", 2, elastic_C(m, 7), bcs=bcs)           # a Newton-like change: another C, the same pattern
    assert B.pattern is A.pattern
    A.values.copy_(B.values)
    amg.setup()                                                                 # no new symbolic phase
    fresh = B.amg(bcs, coarse_rows=COARSE_ROWS)
    assert amg.n_levels == fresh.n_levels
    for l in range(amg.n_levels):
        assert same_csr(amg.level_matrix(l), fresh.level_matrix(l))
    for l in range(amg.n_levels - 1):
        assert np.array_equal(amg.prolongator(l).data, fresh.prolongator(l).data)
    after = amg.apply(r)
    assert torch.equal(after, fresh.apply(r)) and not torch.equal(after, before)
    assert torch.equal(amg.setup(B).apply(r), after)                            # or hand the other matrix over


def test_errors(ctx, meshes, hip_library):
    from dolfinx_external_operator_amd import gmres
    from dolfinx_external_operator_amd._lib import KRYLOV_APPLY_FN, AmgLevelInfo, KrylovInfo, KrylovOp, KrylovPc

    torch = _torch(ctx)
    lib, h = hip_library, ctx._h
    m = structured_mesh("triangle", (6, 6), 2)
    dm = meshes(m)
    bcs = bottom_dofs(m, 2)
    A = _assemble(ctx, dm, "eps", "eps", 2, elastic_C(m), bcs=bcs)
    n = A.shape[0]
    amg = A.amg(bcs, coarse_rows=COARSE_ROWS)
    b, x = _cuda(np.ones(n)), torch.zeros(n, dtype=torch.float64, device="cuda")
    # another size, another block size
    m2 = structured_mesh("triangle", (4, 4), 2)
    dm2 = meshes(m2)
    A2 = _assemble(ctx, dm2, "eps", "eps", 2, elastic_C(m2), bcs=bottom_dofs(m2, 2))
    A1 = _assemble(ctx, dm, "grad", "grad", 1, np.broadcast_to(np.eye(2), (m.num_cells * m.nq, 2, 2)).copy(), bcs=bottom_dofs(m, 1))
    for other in (A2, A1):
        with pytest.raises(ValueError, match="multigrid preconditioner covers"):
            gmres(other, _cuda(np.ones(other.shape[0])), M=amg)
    with pytest.raises(ValueError, match="another pattern"):
        amg.setup(A2)
    with pytest.raises(ValueError, match="AMG.apply: r"):
        amg.apply(_cuda(np.ones(n - 2)))
    for kw in ({"coarse_rows": 0}, {"max_levels": 0}, {"sweeps": 0}):
        with pytest.raises(ValueError, match="at least 1"):
            A.amg(bcs, **kw)
    # the C ABI
    ws, raw = C.c_void_p(), C.c_void_p()
    assert lib.dxo_krylov_create(h, n, 30, C.byref(ws)) == 0
    try:
        assert lib.dxo_amg_create(h, A.pattern._h, None, 0, 10, 0, 1, C.byref(raw)) == -3
        assert lib.dxo_amg_create(h, A.pattern._h, None, 0, 0, 40, 1, C.byref(raw)) == -3
        assert lib.dxo_amg_create(h, A.pattern._h, None, 0, 10, 40, 0, C.byref(raw)) == -3
        assert lib.dxo_amg_create(h, None, None, 0, 10, 40, 1, C.byref(raw)) == -1
        bct = torch.from_numpy(np.asarray(bcs, dtype=np.int32)).cuda()
        assert lib.dxo_amg_create(h, A.pattern._h, C.c_void_p(bct.data_ptr()), -1, 10, 40, 1, C.byref(raw)) == -3
        assert lib.dxo_amg_create(h, A.pattern._h, None, 3, 10, 40, 1, C.byref(raw)) == -1
        assert lib.dxo_amg_create(h, A.pattern._h, C.c_void_p(bct.data_ptr()), bct.numel(), 10, 40, 1, C.byref(raw)) == 0
        bp, xp, vals = C.c_void_p(b.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(A.values.data_ptr())
        assert lib.dxo_amg_apply(h, raw, bp, xp) == -6                                  # before setup
        info = KrylovInfo()
        op = KrylovOp(n, A.pattern._h, vals, KRYLOV_APPLY_FN(), None)
        for fn in (lib.dxo_krylov_gmres, lib.dxo_krylov_cg):
            assert fn(h, ws, C.byref(op), C.byref(KrylovPc(3, 2, n, raw)), bp, xp, 1e-8, 0.0, 100, 8, C.byref(info)) == -6
        assert lib.dxo_amg_setup(h, raw, None) == -1
        assert lib.dxo_amg_setup(h, raw, vals) == 0
        assert lib.dxo_amg_apply(h, raw, bp, None) == -1
        assert lib.dxo_amg_apply(h, raw, C.c_void_p(b.data_ptr() + 4), xp) == -5
        for fn in (lib.dxo_krylov_gmres, lib.dxo_krylov_cg):
            x.zero_()
            assert fn(h, ws, C.byref(op), C.byref(KrylovPc(3, 2, n, raw)), bp, xp, 1e-8, 0.0, 1000, 8, C.byref(info)) == 0
            assert info.converged and info.iterations > 0
            assert fn(h, ws, C.byref(op), C.byref(KrylovPc(3, 3, n, raw)), bp, xp, 1e-8, 0.0, 100, 8, C.byref(info)) == -2      # block size
            assert fn(h, ws, C.byref(op), C.byref(KrylovPc(3, 2, n - 2, raw)), bp, xp, 1e-8, 0.0, 100, 8, C.byref(info)) == -3  # size
            assert fn(h, ws, C.byref(op), C.byref(KrylovPc(3, 2, n, None)), bp, xp, 1e-8, 0.0, 100, 8, C.byref(info)) == -1
        nl = C.c_int()
        lev = AmgLevelInfo()
        assert lib.dxo_amg_info(h, raw, C.byref(nl), None, None, 1, C.byref(lev)) == 0 and nl.value >= 2
        assert lib.dxo_amg_info(h, raw, None, None, None, nl.value, C.byref(lev)) == -3
        # a level's pattern has no mesh: it cannot be assembled into or given Dirichlet rows
        lib.dxo_amg_info(h, raw, None, None, None, 1, C.byref(lev))
        dofs = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert lib.dxo_csr_dirichlet(h, lev.csr, C.c_void_p(dofs.data_ptr()), 1, 1.0, lev.values) == -2
        Cd = _cuda(elastic_C(m))
        assert lib.dxo_bilinear_assemble(h, dm._h, lev.csr, 2, 2, 2, C.c_void_p(Cd.data_ptr()), lev.values) == -2
    finally:
        lib.dxo_krylov_destroy(h, ws)
        if raw.value:
            lib.dxo_amg_destroy(h, raw)
    # singular: a zeroed diagonal block on the fine level, a zero row in a matrix that is its own coarsest level
    indptr, indices = A.pattern.indptr.cpu().numpy(), A.pattern.indices.cpu().numpy()
    node = 7
    keep = A.values.clone()
    for r in (2 * node, 2 * node + 1):
        cols = np.arange(indptr[r], indptr[r + 1])
        A.values[torch.from_numpy(cols[(indices[cols] // 2) == node]).cuda()] = 0.0
    with pytest.raises(ValueError, match="DXO_E_SINGULAR"):
        A.amg(bcs, coarse_rows=COARSE_ROWS)
    with pytest.raises(ValueError, match="DXO_E_SINGULAR"):
        amg.setup()
    with pytest.raises(ValueError, match="DXO_E_OPTION"):
        amg.apply(b)                                                                    # the failed setup left no hierarchy
    A.values.copy_(keep)
    A.values[int(indptr[2 * node]):int(indptr[2 * node + 1])] = 0.0
    with pytest.raises(ValueError, match="DXO_E_SINGULAR"):
        A.amg(bcs, max_levels=1)
    A.values.copy_(keep)
    assert torch.isfinite(amg.setup().apply(b)).all()
