"""dxo_amg_create_soc on the device against the oracle of tests/test_amg_soc_oracle_cpu.py: the masks, the aggregates and the patterns
exactly, dinv_f, omega_F, P and the coarse matrices against the oracle's value from the device's own inputs of that kernel, the cycle
and the iteration counts against the oracle's, and that strength 0 is the object of earlier versions bit for bit."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from dolfinx_external_operator_amd._lib import ERRORS
from oracle.amg_oracle import (U, amg_ref, block_diag, cg_with_cycle, coarse_mask_ref, cycle_ref, filtered_ref, forward_bound,
                               gmres_with_cycle, lumped_inverse_ref, prolongator_ref, rho_ref, same_csr, strength_ref, tentative_ref)
from oracle.krylov_oracle import boundary_dofs
from solver_cases import (CYCLE_TOL, GPU_THETAS, THETA, _aniso, _assemble, _cuda, _soc_snapshot, _soc_system, _torch,
                          meshes)  # noqa: F401  (meshes is a fixture)
from tools.synthetic import structured_mesh

pytestmark = pytest.mark.gpu

SYSTEMS = sorted(GPU_THETAS)
CYCLE_TOL_CHEBY = 1.3e-12    # the figure of tests/test_amg_cheby_gpu.py for Chebyshev smoothing


def _np(B):
    return None if B is None else B.cpu().numpy()


def _same_snapshot(a, b, masks_only=False):
    same = all(np.array_equal(x, y) for x, y in zip(a[2], b[2])) and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
    if masks_only:
        return same
    return (same and all(same_csr(x, y) for x, y in zip(a[0], b[0])) and a[4] == b[4]
            and all(np.array_equal(x.data, y.data) and np.array_equal(x.indices, y.indices) for x, y in zip(a[1], b[1])))


@pytest.mark.parametrize("which", SYSTEMS)
def test_hierarchy_and_cycle_match_the_oracle(ctx, meshes, which):
    torch = _torch(ctx)
    A, bs0, bcs, B, cr = _soc_system(ctx, meshes, which)
    theta = GPU_THETAS[which]
    S = A.to_scipy()
    amg = A.amg(bcs, coarse_rows=cr, near_nullspace=B, strength=theta)
    ref = amg_ref(S, bs0, bcs, near_nullspace=_np(B), strength=theta, coarse_rows=cr)
    dev = amg.levels
    assert amg.strength == theta
    assert amg.n_levels == len(ref) >= 2, (which, amg.n_levels, len(ref))
    assert [d["rows"] for d in dev] == [L.n_rows for L in ref]
    assert [d["bs"] for d in dev] == [L.bs for L in ref]
    assert amg.unlumped_nodes == [int(L.fell.sum()) for L in ref[:-1]]
    mask = np.zeros(S.shape[0], dtype=bool)
    mask[bcs] = True
    for l, L in enumerate(ref[:-1]):
        bs, bsc = L.bs, L.bs_coarse
        Al = amg.level_matrix(l)
        assert np.array_equal(Al.indptr, L.indptr) and np.array_equal(Al.indices, L.indices)
        # the mask: the oracle's from the device's own level matrix, exactly; no test value lies at its threshold
        strong = amg.strong_mask(l)
        sref, closest = strength_ref(Al, Al.indptr, Al.indices, bs, theta)
        assert closest > 4 * bs * bs * U, (which, l, closest)
        assert np.array_equal(strong, sref) and np.array_equal(strong, L.strong), (which, l)
        assert np.array_equal(amg.aggregates(l), L.agg)
        P = amg.prolongator(l)
        assert np.array_equal(P.indptr, L.Pp.indptr) and np.array_equal(P.indices, L.Pp.indices)
        ap_ptr, ap_idx = amg.ap_pattern(l)
        assert np.array_equal(ap_ptr, L.APp.indptr) and np.array_equal(ap_idx, L.APp.indices)
        Ac = amg.level_matrix(l + 1)
        assert np.array_equal(Ac.indptr, ref[l + 1].indptr) and np.array_equal(Ac.indices, ref[l + 1].indices)
        # dinv_f: the inverses of the lumped blocks. The closed-form inverse is no sum: the figure of the block inverses of
        # tests/test_amg_gpu.py (1e-12 of the largest entry) on blocks whose entries are sums of at most row_nnz terms
        AF, lumped, diag, n_strong = filtered_ref(Al, Al.indptr, Al.indices, bs, strong)
        Dref, fell = lumped_inverse_ref(lumped, diag, n_strong)
        Dinv_f, omega_f = amg.level_dinv_f(l), dev[l]["omega_f"]
        print(f"{which} level {l}: dinv_f max |dev - ref| {np.abs(Dinv_f - Dref).max():.3e} of {np.abs(Dref).max():.3e}, "
              f"{int((n_strong == 0).sum())} nodes without a strong neighbour, {int(fell.sum())} fell back")
        assert np.abs(Dinv_f - Dref).max() <= 1e-12 * np.abs(Dref).max()
        assert not Dinv_f[n_strong == 0].any()
        # omega_F from rho_F = |Dinv_F A^F|_inf; an entry of the lumped block is itself a sum of up to row_nnz terms
        absAF = filtered_ref(abs(Al), Al.indptr, Al.indices, bs, strong)[0]
        row_nnz = int(np.diff(Al.indptr).max())
        rho_f, _ = rho_ref(AF, Dinv_f)
        S_rho = np.asarray((abs(block_diag(Dinv_f)) @ absAF).sum(axis=1)).ravel().max()
        K = 2 * bs * row_nnz + bs
        assert abs(omega_f * rho_f - 4.0 / 3.0) <= (4.0 / 3.0) * (forward_bound(K, S_rho) / rho_f + 4 * U), (which, l, omega_f, rho_f)
        assert abs(omega_f - L.omega_f) <= 1e-10 * L.omega_f
        assert abs(dev[l]["omega"] - L.omega) <= 1e-10 * L.omega                 # the sweeps keep the omega of the full matrix
        # P = T - omega_F Dinv_F A^F T on the device's dinv_f and omega_F
        T = amg.tentative(l) if B is not None else tentative_ref(L.agg, mask, bs, L.n_agg)
        Pd = P.toarray()
        Pref = prolongator_ref(AF, Dinv_f, omega_f, T).toarray()
        S_P = (abs(T) + omega_f * (abs(block_diag(Dinv_f)) @ (absAF @ abs(T)))).toarray()
        K = 2 * row_nnz + bs + 2
        excess = np.abs(Pd - Pref) - forward_bound(K, S_P)
        print(f"{which} level {l}: P max |dev - ref| {np.abs(Pd - Pref).max():.3e}")
        assert excess.max() <= 0.0, (which, l, excess.max())
        alone = np.flatnonzero(np.repeat(n_strong == 0, bs))
        assert np.array_equal(Pd[alone], T.toarray()[alone])                      # not smoothed: the row of T
        Psp = sp.csr_matrix(Pd)
        Cref = (Psp.T @ Al @ Psp).toarray()
        d = np.flatnonzero(np.diag(Cref) == 0.0)
        S_C = (abs(Psp).T @ abs(Al) @ abs(Psp)).toarray()
        K = row_nnz * int(np.diff(Psp.tocsc().indptr).max()) + 2
        Cd = Ac.toarray()
        if d.size:
            assert (Cd[d, d] == 1.0).all()
            Cref[d, d] = 1.0
        excess = np.abs(Cd - Cref) - forward_bound(K, S_C)
        print(f"{which} level {l}: A_c max |dev - ref| {np.abs(Cd - Cref).max():.3e} of {np.abs(Cref).max():.3e}")
        assert excess.max() <= 0.0, (which, l, excess.max())
        mask = coarse_mask_ref(Ac)
    rng = np.random.Generator(np.random.PCG64(12))
    worst = 0.0
    for _ in range(3):
        r = rng.normal(size=S.shape[0])
        z = amg.apply(_cuda(r)).cpu().numpy()
        zr = cycle_ref(ref, r)
        worst = max(worst, np.linalg.norm(z - zr) / np.linalg.norm(zr))
    print(f"{which}: cycle deviation from the oracle {worst:.3e} |z|")
    assert worst <= CYCLE_TOL, (which, worst)
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", SYSTEMS)
def test_iteration_counts_match_the_oracle(ctx, meshes, which):
    from dolfinx_external_operator_amd import cg, gmres

    A, bs, bcs, B, cr = _soc_system(ctx, meshes, which)
    theta = GPU_THETAS[which]
    S = A.to_scipy()
    b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
    amg = A.amg(bcs, coarse_rows=cr, near_nullspace=B, strength=theta)
    ref = amg_ref(S, bs, bcs, near_nullspace=_np(B), strength=theta, coarse_rows=cr)
    if bs == 1:
        out = cg(A, _cuda(b), M=amg, rtol=1e-8, maxiter=2000)
        _, its, conv = cg_with_cycle(S, b, ref, rtol=1e-8, maxiter=2000)
        plain = cg(A, _cuda(b), M=A.amg(bcs, coarse_rows=cr, strength=0.0), rtol=1e-8, maxiter=2000)
        print(f"{which}: CG iterations {out.iterations} (oracle {its}), without strength {plain.iterations}, rows "
              f"{[d['rows'] for d in amg.levels]}, complexity {amg.operator_complexity:.2f}")
        assert plain.converged and 2 * out.iterations <= plain.iterations, (which, out.iterations, plain.iterations)
    else:
        out = gmres(A, _cuda(b), M=amg, restart=30, rtol=1e-8, maxiter=2000)
        _, its, conv, _ = gmres_with_cycle(S, b, ref, m=30, rtol=1e-8, maxiter=2000)
        print(f"{which}: GMRES(30) iterations {out.iterations} (oracle {its}), rows {[d['rows'] for d in amg.levels]}")
    assert out.converged and conv and abs(out.iterations - its) <= 2, (which, out.iterations, its)
    x = out.x.cpu().numpy()
    assert np.linalg.norm(b - S @ x) <= 1e-8 * np.linalg.norm(b) * (1 + 1e-6)


@pytest.mark.parametrize("which", ["aniso_tri", "p2_tri_rbm"])
def test_strength_zero_is_the_object_of_earlier_versions(ctx, meshes, which):
    A, bs, bcs, B, cr = _soc_system(ctx, meshes, which)
    r = _cuda(np.random.Generator(np.random.PCG64(3)).normal(size=A.shape[0]))
    today = A.amg(bcs, coarse_rows=cr, near_nullspace=B)
    zero = A.amg(bcs, coarse_rows=cr, near_nullspace=B, strength=0.0)
    bc = _torch(ctx).from_numpy(np.asarray(bcs, dtype=np.int32)).cuda()
    h = C.c_void_p()
    rc = ctx.lib.dxo_amg_create_soc(ctx._h, A.pattern._h, C.c_void_p(A.values.data_ptr()), C.c_void_p(bc.data_ptr()), int(bc.numel()),
                                    C.c_void_p(B.data_ptr()) if B is not None else None, 0 if B is None else B.shape[1], 0.0, 10, cr, 1,
                                    C.byref(h))
    ctx.check(rc, "dxo_amg_create_soc")
    try:
        ctx.check(ctx.lib.dxo_amg_setup(ctx._h, h, C.c_void_p(A.values.data_ptr())), "dxo_amg_setup")
        z = r.clone().zero_()
        ctx.check(ctx.lib.dxo_amg_apply(ctx._h, h, C.c_void_p(r.data_ptr()), C.c_void_p(z.data_ptr())), "dxo_amg_apply")
        th, st, ns, nu = C.c_double(-1.0), C.c_void_p(1), C.c_int64(), C.c_int64(-1)
        ctx.check(ctx.lib.dxo_amg_soc_info(ctx._h, h, 0, C.byref(th), C.byref(st), C.byref(ns), C.byref(nu), None, None), "dxo_amg_soc_info")
        assert th.value == 0.0 and not st.value and ns.value == today.levels[0]["block_nnz"] and nu.value == 0
        z_today = today.apply(r)
        assert np.array_equal(z.cpu().numpy(), z_today.cpu().numpy())
    finally:
        ctx.lib.dxo_amg_destroy(ctx._h, h)
    assert zero.strength == 0.0 and zero.n_levels == today.n_levels >= 2
    assert _same_snapshot(_soc_snapshot(today), _soc_snapshot(zero))
    assert all(d["omega_f"] is None for d in zero.levels) and zero.strong_mask(0).all() and zero.unlumped_nodes == [0] * (zero.n_levels - 1)
    assert np.array_equal(zero.apply(r).cpu().numpy(), today.apply(r).cpu().numpy())


def test_creation_setup_and_replay_are_bit_reproducible(ctx, meshes):
    torch = _torch(ctx)
    A, bs, bcs, B, cr = _soc_system(ctx, meshes, "aniso_tri")
    amg = A.amg(bcs, coarse_rows=cr, strength=THETA)
    other = A.amg(bcs, coarse_rows=cr, strength=THETA)
    assert amg.n_levels >= 3
    first = _soc_snapshot(amg)
    assert _same_snapshot(first, _soc_snapshot(other))                    # two creations
    r = _cuda(np.random.Generator(np.random.PCG64(1)).normal(size=A.shape[0]))
    z_first = amg.apply(r).clone()
    assert torch.equal(other.apply(r), z_first)
    amg.setup()
    assert _same_snapshot(first, _soc_snapshot(amg))                      # two setups
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


def test_setup_with_new_values_keeps_the_masks_and_the_aggregates(ctx, meshes):
    _torch(ctx)
    m = structured_mesh("triangle", (24, 24), 1, distort=0.1, seed=2)
    bcs = boundary_dofs(m, 1)
    dm = meshes(m)
    Cb = np.broadcast_to(np.diag([1.0, 1e-3]), (m.num_cells * m.nq, 2, 2)).copy()
    A = _assemble(ctx, dm, "grad", "grad", 1, Cb, bcs=bcs)
    A2 = _assemble(ctx, dm, "grad", "grad", 1, Cb * np.array([[1.0, 1.0], [1.0, 300.0]]), bcs=bcs)      # a milder anisotropy
    amg = A.amg(bcs, coarse_rows=60, strength=THETA)
    first = _soc_snapshot(amg)
    amg.setup(A2)
    second = _soc_snapshot(amg)
    assert _same_snapshot(first, second, masks_only=True)
    assert all(np.array_equal(x.indices, y.indices) for x, y in zip(first[1], second[1]))
    assert not np.array_equal(first[1][0].data, second[1][0].data)
    ref = amg_ref(A2.to_scipy(), 1, bcs, strength=THETA, coarse_rows=60, frozen=amg_ref(A.to_scipy(), 1, bcs, strength=THETA, coarse_rows=60))
    r = np.random.Generator(np.random.PCG64(2)).normal(size=A.shape[0])
    z, zr = amg.apply(_cuda(r)).cpu().numpy(), cycle_ref(ref, r)
    assert np.linalg.norm(z - zr) <= CYCLE_TOL * np.linalg.norm(zr)


def test_chebyshev_and_power_iteration_on_a_strength_hierarchy(ctx, meshes):
    from dolfinx_external_operator_amd import cg

    A, bs, bcs, B, cr = _soc_system(ctx, meshes, "aniso_tri")
    S = A.to_scipy()
    amg = A.amg(bcs, coarse_rows=cr, strength=THETA)
    masks = [amg.strong_mask(l) for l in range(amg.n_levels)]
    amg.set_smoother("chebyshev", degree=2, rho="power")
    amg.setup()
    assert all(np.array_equal(a, amg.strong_mask(l)) for l, a in enumerate(masks))
    ref = amg_ref(S, 1, bcs, strength=THETA, smoother="chebyshev", rho="power", degree=2, coarse_rows=cr)
    assert [d["rows"] for d in amg.levels] == [L.n_rows for L in ref]
    for d, L in zip(amg.levels[:-1], ref[:-1]):
        assert abs(d["omega_f"] - L.omega_f) <= 1e-10 * L.omega_f and abs(d["omega"] - L.omega) <= 1e-10 * L.omega
    b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
    z, zr = amg.apply(_cuda(b)).cpu().numpy(), cycle_ref(ref, b)
    dev = np.linalg.norm(z - zr) / np.linalg.norm(zr)
    print(f"aniso_tri, Chebyshev 2 with power rho: cycle deviation from the oracle {dev:.3e} |z|")
    assert dev <= CYCLE_TOL_CHEBY
    out = cg(A, _cuda(b), M=amg, rtol=1e-8, maxiter=2000)
    _, its, conv = cg_with_cycle(S, b, ref, rtol=1e-8, maxiter=2000)
    print(f"aniso_tri, Chebyshev 2 with power rho: CG iterations {out.iterations} (oracle {its})")
    assert out.converged and conv and abs(out.iterations - its) <= 2, (out.iterations, its)


def test_isotropic_q1_gives_one_level_and_one_iteration(ctx, meshes):
    from dolfinx_external_operator_amd import cg

    _torch(ctx)
    m = structured_mesh("quadrilateral", (20, 20), 1)
    bcs = boundary_dofs(m, 1)
    A = _assemble(ctx, meshes(m), "grad", "grad", 1, np.broadcast_to(np.eye(2), (m.num_cells * m.nq, 2, 2)).copy(), bcs=bcs)
    amg = A.amg(bcs, coarse_rows=10, strength=THETA)
    assert amg.n_levels == 1 and amg.unlumped_nodes == [] and amg.strong_mask(0).all()
    b = np.random.Generator(np.random.PCG64(1)).normal(size=A.shape[0])
    out = cg(A, _cuda(b), M=amg, rtol=1e-8, check_every=1)          # the host looks at every step: no iterations run past the first
    assert out.converged and out.iterations == 1
    # the same rule on a system that does not fit the dense solve: every node alone leaves more than 4096 rows
    m = structured_mesh("quadrilateral", (80, 80), 1)
    bcs = boundary_dofs(m, 1)
    A = _assemble(ctx, meshes(m), "grad", "grad", 1, np.broadcast_to(np.eye(2), (m.num_cells * m.nq, 2, 2)).copy(), bcs=bcs)
    with pytest.raises(ValueError, match="DXO_E_SIZE"):
        A.amg(bcs, coarse_rows=10, strength=THETA)


@pytest.mark.parametrize("n", [1, 2, 5, 13])
def test_small_and_ragged_node_counts_and_a_lone_node(ctx, meshes, n):
    """(n + 1)^2 nodes: 4 (all on the boundary: fewer blocks in a row than the 8 lanes of its group, no aggregate), 9, 36 (more than
    the 32 nodes of a workgroup, no multiple of them) and 196; from 36 on the diagonal entry of one interior node is 100 times larger,
    so that node has no strong neighbour among nodes that have."""
    from dolfinx_external_operator_amd import cg

    torch = _torch(ctx)
    A, bcs = _aniso(ctx, meshes, "quadrilateral", n=n)
    S = A.to_scipy()
    if n > 2:
        free = np.setdiff1d(np.arange(S.shape[0]), bcs)
        lone = free[free.size // 2]
        d = S.indptr[lone] + np.flatnonzero(S.indices[S.indptr[lone]:S.indptr[lone + 1]] == lone)[0]
        A.values[d] *= 100.0
        torch.cuda.synchronize()
        S = A.to_scipy()
    amg = A.amg(bcs, coarse_rows=3, strength=THETA)
    ref = amg_ref(S, 1, bcs, strength=THETA, coarse_rows=3)
    assert [x["rows"] for x in amg.levels] == [L.n_rows for L in ref]
    for l, L in enumerate(ref[:-1]):
        assert np.array_equal(amg.strong_mask(l), L.strong) and np.array_equal(amg.aggregates(l), L.agg)
    if n > 2:
        assert amg.n_levels >= 2 and ref[0].n_strong_off[lone] == 0 and not amg.level_dinv_f(0)[lone].any()
        P = amg.prolongator(0).tocsr()
        assert P[lone].nnz == 1 and P[lone].sum() == 1.0
    r = np.random.Generator(np.random.PCG64(5)).normal(size=S.shape[0])
    z, zr = amg.apply(_cuda(r)).cpu().numpy(), cycle_ref(ref, r)
    assert np.linalg.norm(z - zr) <= CYCLE_TOL * np.linalg.norm(zr)
    out = cg(A, _cuda(r), M=amg, rtol=1e-8)
    assert out.converged


def test_error_codes(ctx, meshes):
    A, bs, bcs, B, cr = _soc_system(ctx, meshes, "aniso_tri")
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            A.amg(bcs, strength=bad)
        h = C.c_void_p()
        rc = ctx.lib.dxo_amg_create_soc(ctx._h, A.pattern._h, C.c_void_p(A.values.data_ptr()), None, 0, None, 0, bad, 10, 60, 1, C.byref(h))
        assert ERRORS[rc] == "DXO_E_OPTION" and not h.value
    h = C.c_void_p()
    rc = ctx.lib.dxo_amg_create_soc(ctx._h, A.pattern._h, None, None, 0, None, 0, THETA, 10, 60, 1, C.byref(h))
    assert ERRORS[rc] == "DXO_E_NULL" and not h.value
    rc = ctx.lib.dxo_amg_create_soc(ctx._h, A.pattern._h, C.c_void_p(A.values.data_ptr() + 4), None, 0, None, 0, THETA, 10, 60, 1, C.byref(h))
    assert ERRORS[rc] == "DXO_E_ALIGN" and not h.value
