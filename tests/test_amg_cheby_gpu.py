"""dxo_amg_set_smoother on the device against the oracle of tests/test_amg_cheby_oracle_cpu.py, in the manner of test_amg_gpu.py and
test_amg_nns_gpu.py: the power estimate of rho against the oracle's iteration on the device's own Dinv and level matrices; omega, P
and the coarse matrices within the forward bound of a sum in another order (each kernel on the device's own inputs); the Chebyshev
cycle and the preconditioned solves against the oracle cycle; bit-reproducibility, capture, switching the smoother and argument
errors."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg

from oracle.amg_oracle import (U, amg_ref, block_diag, cg_with_cycle, coarse_mask_ref, cycle_ref, forward_bound, gmres_with_cycle,
                               power_rho_ref, prolongator_ref, rho_ref, same_csr, tentative_ref)
from oracle.krylov_oracle import bottom_dofs, elastic_C
from solver_cases import _assemble, _assembled_system, _cuda, _nns_system, _torch, meshes  # noqa: F401  (meshes is a fixture)
from tools.synthetic import structured_mesh

pytestmark = pytest.mark.gpu

COARSE_ROWS = 40
# heat 16 x 16, P2 eps/eps 14 x 14, the hyperelastic tangent, P1 hexahedra 4 x 4 x 4; the block systems with and without rigid-body modes
CASES = [("heat", False), ("p2_eps", False), ("p2_eps", True), ("hyperelastic", False), ("hyperelastic", True), ("hex_eps", False),
         ("hex_eps", True)]
IDS = [w + ("-rbm" if n else "") for w, n in CASES]

# AMG.rho against power_rho_ref on the device's own Dinv and level matrix, relative. Ten products in another summation order and ten
# norms: not derivable. Measured on the seven cases above on an MI355X, in a run in which every other assertion passed; the largest
# over the levels of a case, in the order of CASES: 4.4e-16, 0, 2.6e-16, 1.2e-16, 5.0e-16, 1.5e-16, 1.5e-16. 100 x the largest.
RHO_TOL = 5.1e-14
# the Chebyshev cycle (degree 1, 2 and 3) against vcycle_cheby_ref, relative to |z|; the same run, the largest of a case: 6.2e-16,
# 5.6e-15, 9.4e-15, 2.6e-15, 1.2e-14 (hyperelastic with rigid-body modes), 1.2e-15, 1.8e-15. 100 x the largest (the rule of CYCLE_TOL
# in test_amg_gpu.py).
CHEBY_CYCLE_TOL = 1.3e-12


def _case(ctx, meshes, which, rbm):
    """(DeviceCSR, bs, constrained dofs, near-null space on the device or None, SPD?)"""
    if which == "heat":
        A, bs, bcs = _assembled_system(ctx, meshes, "heat")
        return A, bs, bcs, None, False
    from dolfinx_external_operator_amd import rigid_body_modes

    A, bs, bcs, x, spd = _nns_system(ctx, meshes, which)
    return A, bs, bcs, (rigid_body_modes(x, ctx=ctx) if rbm else None), spd


def _reference(S, bs, bcs, B, **kw):
    return amg_ref(S, bs, bcs, smoother="chebyshev", rho="power", near_nullspace=None if B is None else B.cpu().numpy(), coarse_rows=COARSE_ROWS, **kw)


@pytest.mark.parametrize("which,rbm", CASES, ids=IDS)
def test_rho_hierarchy_and_cycle_match_the_oracle(ctx, meshes, which, rbm):
    torch = _torch(ctx)
    A, bs, bcs, B, _ = _case(ctx, meshes, which, rbm)
    S = A.to_scipy()
    amg = A.amg(bcs, coarse_rows=COARSE_ROWS, near_nullspace=B, smoother="chebyshev", degree=2, rho="power")
    assert amg.smoother == {"smoother": "chebyshev", "degree": 2, "rho": "power", "rho_iters": 10, "lower": 0.1, "safety": 1.1}
    ref = _reference(S, bs, bcs, B, degree=2)
    dev, rhos = amg.levels, amg.rho
    assert amg.n_levels == len(ref) >= (3 if rbm else 2), (which, amg.n_levels, len(ref))
    assert [d["rows"] for d in dev] == [L.n_rows for L in ref]
    assert len(rhos) == amg.n_levels and rhos[-1] is None
    mask = np.zeros(S.shape[0], dtype=bool)
    mask[bcs] = True
    rho_seen = 0.0
    for l, L in enumerate(ref[:-1]):
        bl = dev[l]["bs"]
        Al, Ac, Dinv, omega, P = amg.level_matrix(l), amg.level_matrix(l + 1), amg.level_dinv(l), dev[l]["omega"], amg.prolongator(l)
        assert np.array_equal(Al.indptr, L.indptr) and np.array_equal(Al.indices, L.indices) and bl == L.bs
        # rho: the oracle's iteration on the device's own inputs
        rho = power_rho_ref(Al, Dinv)
        dr = abs(rhos[l] - rho) / rho
        rho_seen = max(rho_seen, dr)
        inf_norm, _ = rho_ref(Al, Dinv)
        print(f"{which} rbm {rbm} level {l}: rho power {rhos[l]:.6f} (oracle {rho:.6f}, deviation {dr:.3e}), inf-norm {inf_norm:.4f}")
        assert dr <= RHO_TOL, (which, l, rhos[l], rho)
        assert abs(rhos[l] - L.rho) <= 1e-10 * L.rho                               # and the end-to-end oracle value
        # omega from the device's rho: one division
        assert abs(omega * rhos[l] - 4.0 / 3.0) <= (4.0 / 3.0) * 4 * U, (which, l, omega, rhos[l])
        # P and A_c from the device's own inputs, within the forward bound of their sums
        T = amg.tentative(l) if rbm else tentative_ref(L.agg, mask, bl, L.n_agg)
        row_nnz = int(np.diff(Al.indptr).max())
        Pd = P.toarray()
        Pref = prolongator_ref(Al, Dinv, omega, T).toarray()
        S_P = (abs(T) + omega * (abs(block_diag(Dinv)) @ (abs(Al) @ abs(T)))).toarray()
        excess = np.abs(Pd - Pref) - forward_bound(row_nnz + bl + 2, S_P)
        assert excess.max() <= 0.0, (which, l, excess.max())
        Psp = sp.csr_matrix(Pd)
        Cref = (Psp.T @ Al @ Psp).toarray()
        d = np.flatnonzero(np.diag(Cref) == 0.0)
        Cref[d, d] = 1.0
        S_C = (abs(Psp).T @ abs(Al) @ abs(Psp)).toarray()
        K = row_nnz * int(np.diff(Psp.tocsc().indptr).max()) + 2
        excess = np.abs(Ac.toarray() - Cref) - forward_bound(K, S_C)
        assert excess.max() <= 0.0, (which, l, excess.max())
        mask = coarse_mask_ref(Ac)
    print(f"{which} rbm {rbm}: RHO_SEEN {rho_seen:.3e}")
    # the cycle, degree 2, 3 and 1
    rng = np.random.Generator(np.random.PCG64(12))
    worst = 0.0
    for degree in (2, 3, 1):
        if degree != 2:
            amg.set_smoother("chebyshev", degree=degree, rho="power").setup()
            ref = _reference(S, bs, bcs, B, degree=degree)
        for _ in range(3):
            r = rng.normal(size=S.shape[0])
            z = amg.apply(_cuda(r)).cpu().numpy()
            zr = cycle_ref(ref, r)
            assert np.isfinite(z).all()
            worst = max(worst, np.linalg.norm(z - zr) / np.linalg.norm(zr))
        buf = _cuda(r)
        amg.apply(buf, out=buf)                                                    # r may be z
        assert np.array_equal(buf.cpu().numpy(), z)
    print(f"{which} rbm {rbm}: CYCLE_SEEN {worst:.3e} |z|")
    assert worst <= CHEBY_CYCLE_TOL, (which, worst)
    torch.cuda.synchronize()


@pytest.mark.parametrize("which,rbm", CASES, ids=IDS)
def test_iteration_counts_match_the_oracle_and_beat_the_default(ctx, meshes, which, rbm):
    from dolfinx_external_operator_amd import cg, gmres

    A, bs, bcs, B, spd = _case(ctx, meshes, which, rbm)
    S = A.to_scipy()
    b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
    xref = scipy.sparse.linalg.spsolve(S.tocsc(), b)
    amg = A.amg(bcs, coarse_rows=COARSE_ROWS, near_nullspace=B, smoother="chebyshev", degree=2, rho="power")
    default = A.amg(bcs, coarse_rows=COARSE_ROWS, near_nullspace=B)
    levels = _reference(S, bs, bcs, B, degree=2)
    if spd:
        out = cg(A, _cuda(b), M=amg, rtol=1e-10, maxiter=5000)
        old = cg(A, _cuda(b), M=default, rtol=1e-10, maxiter=5000)
        _, its, conv = cg_with_cycle(S, b, levels, rtol=1e-10, maxiter=5000)
    else:
        out = gmres(A, _cuda(b), M=amg, restart=30, rtol=1e-10, maxiter=5000)
        old = gmres(A, _cuda(b), M=default, restart=30, rtol=1e-10, maxiter=5000)
        _, its, conv, _ = gmres_with_cycle(S, b, levels, m=30, rtol=1e-10, maxiter=5000)
    print(f"{which} rbm {rbm}: {'CG' if spd else 'GMRES(30)'} iterations with Chebyshev 2 on the power estimate {out.iterations} "
          f"(oracle {its}), default {old.iterations}")
    assert out.converged and old.converged and conv
    assert np.linalg.norm(out.x.cpu().numpy() - xref) <= 1e-7 * np.linalg.norm(xref)
    assert abs(out.iterations - its) <= 2, (which, out.iterations, its)
    if which in ("p2_eps", "hex_eps"):
        assert out.iterations < old.iterations, (which, out.iterations, old.iterations)


def _eps14(ctx, meshes, seed=1):
    m = structured_mesh("triangle", (14, 14), 2)
    bcs = bottom_dofs(m, 2)
    return m, bcs, _assemble(ctx, meshes(m), "eps", "eps", 2, elastic_C(m, seed), bcs=bcs)


def _snapshot(a):
    return ([a.level_matrix(l) for l in range(a.n_levels)], [a.prolongator(l) for l in range(a.n_levels - 1)],
            [d["omega"] for d in a.levels], a.rho)


def _same(p, q):
    return (all(same_csr(a, b) for a, b in zip(p[0], q[0]))
            and all(np.array_equal(a.data, b.data) and np.array_equal(a.indices, b.indices) for a, b in zip(p[1], q[1]))
            and p[2] == q[2] and p[3] == q[3])


@pytest.mark.parametrize("rbm", [False, True])
def test_bit_reproducible_and_capture_safe(ctx, meshes, rbm):
    from dolfinx_external_operator_amd import rigid_body_modes

    torch = _torch(ctx)
    m, bcs, A = _eps14(ctx, meshes)
    kw = {"coarse_rows": COARSE_ROWS, "near_nullspace": rigid_body_modes(m.node_x, ctx=ctx) if rbm else None}
    cheb = {"smoother": "chebyshev", "degree": 3, "rho": "power"}
    amg = A.amg(bcs, **kw, **cheb)
    assert amg.n_levels >= 3
    first = _snapshot(amg)
    r = _cuda(np.random.Generator(np.random.PCG64(1)).normal(size=A.shape[0]))
    z_first = amg.apply(r).clone()
    amg.setup()
    assert _same(first, _snapshot(amg))                                          # two setups
    other = A.amg(bcs, **kw, **cheb)
    assert _same(first, _snapshot(other))                                        # two creations
    assert torch.equal(other.apply(r), z_first)
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
    # the keywords spelled out are the defaults: the same object bit for bit, and rho is then the infinity norm
    plain, spelled = A.amg(bcs, **kw), A.amg(bcs, **kw, smoother="jacobi", rho="inf-norm")
    assert plain.smoother == spelled.smoother and plain.smoother["smoother"] == "jacobi" and plain.smoother["rho"] == "inf-norm"
    assert plain.smoother["degree"] == 1
    assert _same(_snapshot(plain), _snapshot(spelled)) and torch.equal(plain.apply(r), spelled.apply(r))
    assert not torch.equal(plain.apply(r), z_first)
    for l, rho in enumerate(plain.rho[:-1]):
        ref, S_rho = rho_ref(plain.level_matrix(l), plain.level_dinv(l))
        K = plain.levels[l]["bs"] * (int(np.diff(plain.level_matrix(l).indptr).max()) + 1)
        assert abs(rho - ref) <= forward_bound(K, S_rho) and abs(plain.levels[l]["omega"] * rho - 4.0 / 3.0) <= (4.0 / 3.0) * 4 * U
    # the power estimate with Jacobi sweeps: omega of the sweeps and of P follows it
    pj = A.amg(bcs, **kw, rho="power")
    assert pj.rho == first[3] and [d["omega"] for d in pj.levels] == first[2] and _same(_snapshot(pj), first)


def test_switching_the_smoother(ctx, meshes, hip_library):
    from dolfinx_external_operator_amd import cg
    from dolfinx_external_operator_amd._lib import KRYLOV_APPLY_FN, KrylovInfo, KrylovOp, KrylovPc

    torch = _torch(ctx)
    lib, h = hip_library, ctx._h
    m, bcs, A = _eps14(ctx, meshes)
    n = A.shape[0]
    amg = A.amg(bcs, coarse_rows=COARSE_ROWS, sweeps=2)
    r = _cuda(np.random.Generator(np.random.PCG64(1)).normal(size=n))
    z_jacobi, snap_jacobi = amg.apply(r).clone(), _snapshot(amg)
    z, x = torch.zeros_like(r), torch.zeros_like(r)
    rp, zp = C.c_void_p(r.data_ptr()), C.c_void_p(z.data_ptr())
    assert lib.dxo_amg_set_smoother(h, amg._h, 1, 3, 1, 10, 0.1, 1.1) == 0
    assert lib.dxo_amg_apply(h, amg._h, rp, zp) == -6                           # DXO_E_OPTION until the next setup
    ws = C.c_void_p()
    assert lib.dxo_krylov_create(h, n, 30, C.byref(ws)) == 0
    try:
        info = KrylovInfo()
        op = KrylovOp(n, A.pattern._h, C.c_void_p(A.values.data_ptr()), KRYLOV_APPLY_FN(), None)
        for fn in (lib.dxo_krylov_gmres, lib.dxo_krylov_cg):
            assert fn(h, ws, C.byref(op), C.byref(KrylovPc(3, 2, n, amg._h)), rp, C.c_void_p(x.data_ptr()), 1e-8, 0.0, 100, 8, C.byref(info)) == -6
    finally:
        lib.dxo_krylov_destroy(h, ws)
    with pytest.raises(ValueError, match="DXO_E_OPTION"):
        amg.apply(r)
    with pytest.raises(ValueError, match="DXO_E_OPTION"):
        cg(A, r, M=amg)
    kind, degree, rk, it, rho = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_void_p()
    assert lib.dxo_amg_smoother_info(h, amg._h, 0, C.byref(kind), C.byref(degree), C.byref(rk), C.byref(it), C.byref(rho)) == 0
    assert (kind.value, degree.value, rk.value, it.value) == (1, 3, 1, 10) and rho.value
    assert lib.dxo_amg_smoother_info(h, amg._h, amg.n_levels - 1, None, None, None, None, C.byref(rho)) == 0 and rho.value is None
    amg.setup()
    z_cheb = amg.apply(r).clone()
    fresh = A.amg(bcs, coarse_rows=COARSE_ROWS, sweeps=2, smoother="chebyshev", degree=3, rho="power")
    assert torch.equal(z_cheb, fresh.apply(r)) and not torch.equal(z_cheb, z_jacobi)
    assert _same(_snapshot(amg), _snapshot(fresh))
    fresh.close()
    del fresh
    # and back: the original cycle bit for bit, `sweeps` of the creation holds whatever degree says
    assert lib.dxo_amg_set_smoother(h, amg._h, 0, 99, 0, 10, 0.1, 1.1) == 0
    assert lib.dxo_amg_apply(h, amg._h, rp, zp) == -6
    amg.setup()
    assert amg.smoother["smoother"] == "jacobi" and amg.smoother["degree"] == 2 and amg.smoother["rho"] == "inf-norm"
    assert torch.equal(amg.apply(r), z_jacobi) and _same(_snapshot(amg), snap_jacobi)
    # Chebyshev on the infinity norm: allowed, a wide interval
    wide = amg.set_smoother("chebyshev", degree=2).setup()
    assert wide is amg and _same(_snapshot(amg), snap_jacobi)                   # rho, omega, P and the coarse matrices are unchanged
    S = A.to_scipy()
    ref = amg_ref(S, 2, bcs, smoother="chebyshev", rho="inf-norm", degree=2, coarse_rows=COARSE_ROWS, sweeps=2)
    zw, zr = amg.apply(r).cpu().numpy(), cycle_ref(ref, r.cpu().numpy())
    assert np.linalg.norm(zw - zr) <= CHEBY_CYCLE_TOL * np.linalg.norm(zr)


def test_errors(ctx, meshes, hip_library):
    lib, h = hip_library, ctx._h
    m = structured_mesh("triangle", (6, 6), 2)
    bcs = bottom_dofs(m, 2)
    A = _assemble(ctx, meshes(m), "eps", "eps", 2, elastic_C(m), bcs=bcs)
    amg = A.amg(bcs, coarse_rows=COARSE_ROWS)
    r = _cuda(np.ones(A.shape[0]))
    z_before = amg.apply(r).clone()
    for kw in ({"smoother": "gauss-seidel"}, {"rho": "gershgorin"}, {"smoother": "chebyshev", "degree": 0}, {"smoother": "chebyshev", "degree": 9},
               {"rho": "power", "rho_iters": 0}, {"lower": 0.0}, {"lower": 1.0}, {"safety": 0.99},
               {"rho": "power", "safety": float("nan")}):
        with pytest.raises(ValueError, match="AMG:"):
            A.amg(bcs, coarse_rows=COARSE_ROWS, **kw)
        with pytest.raises(ValueError, match="AMG:"):
            amg.set_smoother(**kw)
    with pytest.raises(ValueError, match="AMG:"):
        A.amg(bcs, coarse_rows=COARSE_ROWS, sweeps=9, smoother="chebyshev")          # degree None: the sweeps
    a = amg._h
    assert lib.dxo_amg_set_smoother(None, a, 1, 2, 1, 10, 0.1, 1.1) == -1
    assert lib.dxo_amg_set_smoother(h, None, 1, 2, 1, 10, 0.1, 1.1) == -1
    for args in ((2, 2, 1, 10, 0.1, 1.1), (-1, 2, 1, 10, 0.1, 1.1), (1, 2, 2, 10, 0.1, 1.1), (1, 2, -1, 10, 0.1, 1.1),     # unknown kinds
                 (1, 0, 1, 10, 0.1, 1.1), (1, 9, 1, 10, 0.1, 1.1),                                                         # degree
                 (1, 2, 1, 0, 0.1, 1.1), (0, 1, 0, 0, 0.1, 1.1),                                                           # rho_iters
                 (1, 2, 1, 10, 0.0, 1.1), (1, 2, 1, 10, 1.0, 1.1), (1, 2, 1, 10, float("nan"), 1.1),                       # lower
                 (1, 2, 1, 10, 0.1, 0.999), (1, 2, 1, 10, 0.1, float("nan"))):                                             # safety
        assert lib.dxo_amg_set_smoother(h, a, *args) == -6, args
    # a refused call changes nothing: the object stays ready
    assert amg.smoother == {"smoother": "jacobi", "degree": 1, "rho": "inf-norm", "rho_iters": 10, "lower": 0.1, "safety": 1.1}
    assert np.array_equal(amg.apply(r).cpu().numpy(), z_before.cpu().numpy())
    assert lib.dxo_amg_smoother_info(h, None, 0, None, None, None, None, None) == -1
    assert lib.dxo_amg_smoother_info(h, a, -1, None, None, None, None, None) == -3
    assert lib.dxo_amg_smoother_info(h, a, amg.n_levels, None, None, None, None, None) == -3
    assert lib.dxo_amg_smoother_info(h, a, 0, None, None, None, None, None) == 0
