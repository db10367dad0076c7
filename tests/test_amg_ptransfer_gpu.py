"""dxo_amg_create_transfer on the device against the oracle of tests/test_amg_ptransfer_oracle_cpu.py: the transfer arrays, p_diag, all
patterns and rows per level exactly, A_1 within the forward bound of its sums, the cycle and the solves against the oracle cycle, bit
identity, the defining property (levels 1... are the hierarchy of A_1 itself), a known answer without an oracle, single precision, the
K-cycle, strength of connection and the argument errors."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from oracle.amg_oracle import (amg_ref, cg_with_cycle, cycle_ref, forward_bound, gmres_with_cycle, operator_complexity, p_diag_ref,
                               same_csr, vertex_transfer_ref)
from oracle.form_oracle import apply_bcs, dense_ref
from oracle.krylov_oracle import bottom_dofs, elastic_C, elastic_C3, to_pattern_csr
from solver_cases import (COARSE_ROWS, CYCLE_TOL, K_CYCLE_TOL, NOT_DOUBLE, SAME_FORMULAS, _assemble, _cuda, _device_levels, _torch,
                          meshes)  # noqa: F401  (meshes is a fixture)
from tools.synthetic import coordinate_element_at_nodes, gauss_tensor_rule, structured_mesh, with_rule

pytestmark = pytest.mark.gpu

# cell, boxes, block size, form, 27-point rule, rollers on x = 0
CASES = {
    "tri65": ("triangle", (6, 5), 2, "eps", False, False),
    "tri65_rollers": ("triangle", (6, 5), 2, "eps", False, True),
    "quad54": ("quadrilateral", (5, 4), 2, "eps", False, False),
    "tet222": ("tetrahedron", (2, 2, 2), 3, "eps", False, False),
    "hex333": ("hexahedron", (3, 3, 3), 3, "eps", True, False),
    "tri88_scalar": ("triangle", (8, 8), 1, "grad", False, False),
}
ELASTIC = [k for k, v in CASES.items() if v[3] == "eps"]
VARIANTS = {"default": {}, "cheby": dict(smoother="chebyshev", degree=2, rho="power")}
_HOST = {}


def _point_blocks(m, bs, form):
    if form == "grad":
        return np.broadcast_to(np.eye(m.gdim), (m.num_cells * m.nq, m.gdim, m.gdim)).copy()
    return elastic_C(m) if bs == 2 else elastic_C3(m.num_cells * m.nq)


def _host(which, distort=0.1):
    """(mesh, constrained dofs, oracle W, oracle coarse_to_fine) of a case, made once."""
    key = (which, distort)
    if key not in _HOST:
        cell, n, bs, _, rule27, rollers = CASES[which]
        m = structured_mesh(cell, n, 2, distort=distort, seed=2)
        if rule27:
            m = with_rule(m, *gauss_tensor_rule(cell, 3))
        dofs = bottom_dofs(m, bs)
        if rollers:                                           # the horizontal component on x = 0: partly constrained nodes
            dofs = np.unique(np.concatenate([dofs, np.flatnonzero(np.abs(m.node_x[:, 0]) < 1e-12) * bs]))
        _HOST[key] = (m, dofs) + vertex_transfer_ref(m)
    return _HOST[key]


def _system(ctx, meshes, which, distort=0.1):
    """(mesh, DeviceMesh, DeviceCSR, bs, constrained dofs, NodalTransfer of the library, oracle W, oracle coarse_to_fine). The Q2
    hexahedron is assembled by the device with the 27-point rule if dxo_bilinear_assemble takes it; if it answers DXO_E_SIZE (the
    element does not fit its LDS budget) the oracle's values are written into the device pattern instead."""
    torch = _torch(ctx)
    _, _, bs, form, _, _ = CASES[which]
    m, dofs, W, ctf = _host(which, distort)
    dm = meshes(m)
    try:
        A = _assemble(ctx, dm, form, form, bs, _point_blocks(m, bs, form), bcs=dofs)
    except ValueError as e:
        from dolfinx_external_operator_amd.operand_eval import DeviceCSR

        assert which == "hex333" and "DXO_E_SIZE" in str(e), e
        S = to_pattern_csr(m, apply_bcs(dense_ref(m, form, form, bs, _point_blocks(m, bs, form)), dofs, 1.0), bs)
        pat = dm.csr_pattern(bs)
        assert np.array_equal(pat.indptr.cpu().numpy(), S.indptr) and np.array_equal(pat.indices.cpu().numpy(), S.indices)
        A = DeviceCSR(pat, torch.from_numpy(S.data.copy()).cuda())
        print("hex333: dxo_bilinear_assemble refused nq = 27; the oracle's values were written into the device pattern")
    t = dm.vertex_transfer(coordinate_element_at_nodes(m.cell, 2))
    return m, dm, A, bs, dofs, t, W, ctf


def _kw(ctx, m, variant, rbm):
    from dolfinx_external_operator_amd import rigid_body_modes

    kw = dict(VARIANTS[variant], coarse_rows=COARSE_ROWS)
    okw = dict(kw)
    if rbm:
        kw["near_nullspace"] = rigid_body_modes(m.node_x, ctx=ctx)
        okw["near_nullspace"] = kw["near_nullspace"].cpu().numpy()
    return kw, okw


@pytest.mark.parametrize("which", list(CASES))
def test_hierarchy_matches_the_oracle(ctx, meshes, which):
    m, dm, A, bs, dofs, t, W, ctf = _system(ctx, meshes, which)
    # the transfer of the library is the oracle's
    assert t.n_coarse == W.shape[1] and np.array_equal(t.ptr, W.indptr) and np.array_equal(t.col, W.indices)
    assert np.array_equal(t.w, W.data) and np.array_equal(t.coarse_to_fine, ctf)
    S = A.to_scipy()
    amg = A.amg(dofs, coarse_rows=COARSE_ROWS, first_transfer=t)
    ref = amg_ref(S, bs, dofs, first_transfer=(W, ctf), coarse_rows=COARSE_ROWS)
    info = amg.first_transfer
    mask = np.zeros(S.shape[0], dtype=bool)
    mask[dofs] = True
    # exact: products of binary fractions and 0 / 1
    assert info["n_coarse"] == W.shape[1] and info["p_blocks"] == W.nnz
    assert np.array_equal(info["p_diag"].cpu().numpy(), p_diag_ref(W, ctf, mask, bs))
    dev = amg.levels
    print(f"{which}: rows {[d['rows'] for d in dev]}, complexity {amg.operator_complexity:.3f}")
    assert amg.n_levels == len(ref) >= 2
    assert [d["rows"] for d in dev] == [L.n_rows for L in ref]
    assert [d["bs"] for d in dev] == [bs] * len(ref)
    assert abs(amg.operator_complexity - operator_complexity(ref)) <= 1e-12
    for l, L in enumerate(ref):
        Al = amg.level_matrix(l)
        assert np.array_equal(Al.indptr, L.indptr) and np.array_equal(Al.indices, L.indices)
        if l + 1 == len(ref):
            break
        P = amg.prolongator(l)
        assert np.array_equal(P.indptr, L.Pp.indptr) and np.array_equal(P.indices, L.Pp.indices)
        ap_ptr, ap_idx = amg.ap_pattern(l)
        assert np.array_equal(ap_ptr, L.APp.indptr) and np.array_equal(ap_idx, L.APp.indices)
        if l >= 1:
            assert np.array_equal(amg.aggregates(l), L.agg)
    assert amg.aggregates(0).size == 0 and amg._nns(0)[:2] == (bs, bs)             # level 0 has no aggregates and keeps its block size
    assert np.array_equal(amg.prolongator(0).toarray(), ref[0].P.toarray())
    # A_1 against the SciPy product of the device's own values, within the forward bound of its sums
    P0, A0, A1 = ref[0].P, amg.level_matrix(0), amg.level_matrix(1).toarray()
    Cref = (P0.T @ A0 @ P0).toarray()
    d = np.flatnonzero(np.diag(Cref) == 0.0)
    assert (A1[d, d] == 1.0).all()
    Cref[d, d] = 1.0
    K = int(np.diff(A0.indptr).max()) * int(np.diff(P0.tocsc().indptr).max()) + 2
    excess = np.abs(A1 - Cref) - forward_bound(K, (abs(P0).T @ abs(A0) @ abs(P0)).toarray())
    print(f"{which}: A_1 max |dev - ref| {np.abs(A1 - Cref).max():.3e} of {np.abs(Cref).max():.3e}")
    assert excess.max() <= 0.0, (which, excess.max())
    assert np.array_equal(np.flatnonzero(mask.reshape(-1, bs)[ctf].reshape(-1)), d)      # the unit diagonals are the constrained coarse dofs


# every case under both relaxations; with rigid-body modes where there are any (elasticity)
CYCLES = [(w, v, r) for w in CASES for v in VARIANTS for r in (False, True) if not r or w in ELASTIC]


@pytest.mark.parametrize("which,variant,rbm", CYCLES)
def test_cycle_matches_the_oracle(ctx, meshes, which, variant, rbm):
    m, dm, A, bs, dofs, t, W, ctf = _system(ctx, meshes, which)
    kw, okw = _kw(ctx, m, variant, rbm)
    amg = A.amg(dofs, first_transfer=t, **kw)
    ref = amg_ref(A.to_scipy(), bs, dofs, first_transfer=(W, ctf), **okw)
    assert [d["rows"] for d in amg.levels] == [L.n_rows for L in ref]
    if rbm:
        assert np.array_equal(amg.near_nullspace(1), ref[1].B)                     # the rows of the zeroed B_0 at the coarse nodes
    rng = np.random.Generator(np.random.PCG64(12))
    worst = 0.0
    for _ in range(3):
        r = rng.normal(size=A.shape[0])
        z = amg.apply(_cuda(r)).cpu().numpy()
        zr = cycle_ref(ref, r)
        worst = max(worst, np.linalg.norm(z - zr) / np.linalg.norm(zr))
    print(f"{which} {variant} rbm={rbm}: cycle deviation from the oracle {worst:.3e} |z|")
    assert worst <= CYCLE_TOL, (which, variant, rbm, worst)
    buf = _cuda(r)
    amg.apply(buf, out=buf)                                                        # r may be z
    assert np.array_equal(buf.cpu().numpy(), z)


@pytest.mark.parametrize("which", list(CASES))
def test_iteration_counts_follow_the_oracle(ctx, meshes, which):
    from dolfinx_external_operator_amd import cg, gmres

    m, dm, A, bs, dofs, t, W, ctf = _system(ctx, meshes, which)
    S = A.to_scipy()
    b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
    amg = A.amg(dofs, coarse_rows=COARSE_ROWS, first_transfer=t)
    plain = A.amg(dofs, coarse_rows=COARSE_ROWS)
    ref = amg_ref(S, bs, dofs, first_transfer=(W, ctf), coarse_rows=COARSE_ROWS)
    out = cg(A, _cuda(b), M=amg, rtol=1e-8, maxiter=600)
    _, its, conv = cg_with_cycle(S, b, ref, rtol=1e-8, maxiter=600)
    out_plain = cg(A, _cuda(b), M=plain, rtol=1e-8, maxiter=600)
    print(f"{which}: CG iterations with the p level {out.iterations} (oracle {its}), plain hierarchy {out_plain.iterations}")
    assert out.converged and conv and abs(out.iterations - its) <= 2, (which, out.iterations, its)
    assert np.linalg.norm(b - S @ out.x.cpu().numpy()) <= 1.01e-8 * np.linalg.norm(b)
    if which in ("tri65", "tri88_scalar"):
        g = gmres(A, _cuda(b), M=amg, restart=30, rtol=1e-8, maxiter=600)
        _, gits, gconv, _ = gmres_with_cycle(S, b, ref, m=30, rtol=1e-8, maxiter=600)
        print(f"{which}: GMRES(30) iterations with the p level {g.iterations} (oracle {gits})")
        assert g.converged and gconv and abs(g.iterations - gits) <= 2, (which, g.iterations, gits)


@pytest.mark.parametrize("which", ["tri65_rollers", "hex333"])
def test_bit_identity_and_frozen_weights(ctx, meshes, which):
    torch = _torch(ctx)
    m, dm, A, bs, dofs, t, W, ctf = _system(ctx, meshes, which)
    amg = A.amg(dofs, coarse_rows=COARSE_ROWS, first_transfer=t)
    twin = A.amg(dofs, coarse_rows=COARSE_ROWS, first_transfer=t)

    def snapshot(a):
        return [a.level_matrix(l) for l in range(a.n_levels)], [a.prolongator(l) for l in range(a.n_levels - 1)], [d["omega"] for d in a.levels]

    first, other = snapshot(amg), snapshot(twin)
    assert all(same_csr(a, b) for a, b in zip(first[0], other[0])) and first[2] == other[2]          # two creations
    assert all(np.array_equal(a.data, b.data) for a, b in zip(first[1], other[1]))
    pd = amg.first_transfer["p_diag"].clone()
    r = _cuda(np.random.Generator(np.random.PCG64(1)).normal(size=A.shape[0]))
    z_first = amg.apply(r).clone()
    assert torch.equal(twin.apply(r), z_first)
    keep = A.values.clone()
    A.values.mul_(3.0)
    amg.setup()
    assert torch.equal(amg.first_transfer["p_diag"], pd)                           # setup() leaves the weights alone
    assert not same_csr(amg.level_matrix(1), first[0][1])
    A.values.copy_(keep)
    amg.setup()
    again = snapshot(amg)
    assert all(same_csr(a, b) for a, b in zip(first[0], again[0])) and first[2] == again[2]          # two setups
    assert torch.equal(amg.first_transfer["p_diag"], pd) and torch.equal(amg.apply(r), z_first)
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


def _direct(ctx, meshes, which, amg, dofs, ctf, bs, **kw):
    """The hierarchy the library builds when handed A_1 and the level-1 constrained set: A_1's values on the pattern of the degree-1
    mesh (which is A_1's pattern)."""
    from dolfinx_external_operator_amd.operand_eval import DeviceCSR

    torch = _torch(ctx)
    cell, n = CASES[which][:2]
    dm1 = meshes(structured_mesh(cell, n, 1, distort=0.1, seed=2))
    pat, A1 = dm1.csr_pattern(bs), amg.level_matrix(1)
    assert np.array_equal(pat.indptr.cpu().numpy(), A1.indptr) and np.array_equal(pat.indices.cpu().numpy(), A1.indices)
    mask = np.zeros(amg.n, dtype=bool)
    mask[dofs] = True
    dofs1 = np.flatnonzero(mask.reshape(-1, bs)[ctf].reshape(-1))
    D = DeviceCSR(pat, torch.from_numpy(A1.data.copy()).cuda())
    return D, D.amg(dofs1, coarse_rows=COARSE_ROWS, **kw)


def _assert_levels_below_are(amg, direct):
    assert amg.n_levels == direct.n_levels + 1
    dev, ddev, rho, drho = amg.levels, direct.levels, amg.rho, direct.rho
    for l in range(direct.n_levels):
        assert same_csr(amg.level_matrix(l + 1), direct.level_matrix(l)), l
        assert dev[l + 1]["omega"] == ddev[l]["omega"] and rho[l + 1] == drho[l] and dev[l + 1]["bs"] == ddev[l]["bs"]
        if l + 1 < direct.n_levels:
            assert np.array_equal(amg.aggregates(l + 1), direct.aggregates(l))
            a, b = amg.prolongator(l + 1), direct.prolongator(l)
            assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data), l
            assert np.array_equal(amg.level_dinv(l + 1), direct.level_dinv(l))


@pytest.mark.parametrize("rbm", [False, True])
@pytest.mark.parametrize("which", ["tri65_rollers", "tet222", "hex333"])
def test_levels_below_are_the_hierarchy_of_a1_bit_for_bit(ctx, meshes, which, rbm):
    torch = _torch(ctx)
    m, dm, A, bs, dofs, t, W, ctf = _system(ctx, meshes, which)
    kw, _ = _kw(ctx, m, "default", rbm)
    amg = A.amg(dofs, first_transfer=t, **kw)
    assert amg.n_levels >= 3
    if rbm:
        kw["near_nullspace"] = torch.from_numpy(amg.near_nullspace(1)).cuda()
    _, direct = _direct(ctx, meshes, which, amg, dofs, ctf, bs, **{k: v for k, v in kw.items() if k != "coarse_rows"})
    _assert_levels_below_are(amg, direct)
    if rbm:
        assert np.array_equal(amg.near_nullspace(2), direct.near_nullspace(1)) and amg.dead_columns[1:] == direct.dead_columns


@pytest.mark.parametrize("which", ["tri65", "tet222"])
def test_a1_is_the_degree_one_matrix_on_affine_cells(ctx, meshes, which):
    """Without an oracle: on undistorted affine P2 cells with a constant C the degree-2 quadrature is exact for both spaces and the
    degree-1 space is a subspace, so A_1 = P^T A P is the matrix bilinear_assemble gives on the degree-1 mesh with the same C and
    constraints. The two differ by the rounding of three sums. (a) the Galerkin sum on the device's values: forward_bound with
    S = |P|^T |A| |P|. (b), (c) the two assemblies, (c) carried through P: an entry is a sum over at most `cells` cells, nq points
    and D^2 products B_k C_kl B_l. C is symmetric positive definite with non-negative entries, so per point |B_i|^T C |B_j| <=
    kappa sqrt((B_i^T C B_i)(B_j^T C B_j)) with kappa = lambda_max / lambda_min of C, and by Cauchy-Schwarz over points and cells the
    sum over absolute values is at most kappa sqrt(A_ii A_jj)."""
    cell, n, bs, form, _, _ = CASES[which]
    m, dm, A, _, dofs, t, W, ctf = _system(ctx, meshes, which, distort=0.0)
    amg = A.amg(dofs, coarse_rows=COARSE_ROWS, first_transfer=t)
    m1 = structured_mesh(cell, n, 1)
    dofs1 = bottom_dofs(m1, bs)
    A1 = _assemble(ctx, meshes(m1), form, form, bs, _point_blocks(m1, bs, form), bcs=dofs1).to_scipy()
    G = amg.level_matrix(1)
    assert np.array_equal(G.indptr, A1.indptr) and np.array_equal(G.indices, A1.indices)
    Ce = _point_blocks(m1, bs, form)[0]
    ev = np.linalg.eigvalsh(Ce)
    kappa = ev[-1] / ev[0]
    cells = 6 if m.gdim == 2 else 24                          # Kuhn simplices around an interior vertex (an edge has fewer)
    K_asm = cells * m.nq * Ce.size
    P0, A0 = amg.prolongator(0).tocsr(), amg.level_matrix(0)
    S2 = kappa * np.sqrt(np.outer(A0.diagonal(), A0.diagonal()))
    S1 = kappa * np.sqrt(np.outer(A1.diagonal(), A1.diagonal()))
    K_c = int(np.diff(A0.indptr).max()) * int(np.diff(P0.tocsc().indptr).max()) + 2
    pattern2 = sp.csr_matrix((np.ones_like(A0.data), A0.indices, A0.indptr), shape=A0.shape).toarray()      # the stored entries
    tol = (forward_bound(K_c, (abs(P0).T @ abs(A0) @ abs(P0)).toarray()) + forward_bound(K_asm, S1)
           + abs(P0).T.toarray() @ (forward_bound(K_asm, S2) * pattern2) @ abs(P0).toarray())
    diff = np.abs(G.toarray() - A1.toarray())
    print(f"{which}: max |P^T A P - A(P1)| {diff.max():.3e} of {np.abs(A1).max():.3e}, the bound there {tol.reshape(-1)[diff.argmax()]:.3e}")
    assert (diff <= tol).all(), (which, (diff - tol).max())
    assert tol.max() <= 1e-8 * np.abs(A1).max()               # and the bound is tight enough to mean something


@pytest.mark.parametrize("which", ["tri65", "tet222"])
def test_fp32_cycle_against_the_float32_oracle(ctx, meshes, which):
    torch = _torch(ctx)
    m, dm, A, bs, dofs, t, W, ctf = _system(ctx, meshes, which)
    amg = A.amg(dofs, coarse_rows=COARSE_ROWS, first_transfer=t, precision="fp32")
    assert amg.precision == "fp32" and amg.first_transfer is not None
    levels = _device_levels(amg)
    rng = np.random.Generator(np.random.PCG64(12))
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
        assert e_dev <= SAME_FORMULAS * e_ref and e_dev >= NOT_DOUBLE * e_ref, (which, e_dev, e_ref)
    z32_first = amg.apply(_cuda(r)).clone()
    amg.setup()
    assert torch.equal(amg.apply(_cuda(r)), z32_first)
    z64_dev = amg.set_precision("fp64").setup().apply(_cuda(r))
    assert torch.equal(z64_dev, A.amg(dofs, coarse_rows=COARSE_ROWS, first_transfer=t).apply(_cuda(r)))


def test_k_cycle_on_a_p_hierarchy(ctx, meshes):
    torch = _torch(ctx)
    m, dm, A, bs, dofs, t, W, ctf = _system(ctx, meshes, "hex333")
    amg = A.amg(dofs, coarse_rows=COARSE_ROWS, first_transfer=t, cycle="K")
    assert amg.n_levels == 3 and amg.cycle == "K" and amg.visits == 1 + 2 + 2
    levels = _device_levels(amg)
    r = np.random.Generator(np.random.PCG64(12)).normal(size=A.shape[0])
    z = amg.apply(_cuda(r))
    zr = cycle_ref(levels, r, "K")
    dev = np.linalg.norm(z.cpu().numpy() - zr) / np.linalg.norm(zr)
    print(f"hex333: K_CYCLE_SEEN {dev:.3e} |z|")
    assert dev <= K_CYCLE_TOL
    assert torch.equal(amg.apply(_cuda(r)), z)                                     # a repeat is bit-identical
    for e in (-40, 37):                                                           # homogeneous of degree one, bit for bit
        assert torch.equal(amg.apply(_cuda(r * 2.0 ** e)), z * 2.0 ** e)
    v = A.amg(dofs, coarse_rows=COARSE_ROWS, first_transfer=t)
    assert not torch.equal(v.apply(_cuda(r)), z)
    assert torch.equal(amg.set_cycle("V").apply(_cuda(r)), v.apply(_cuda(r)))


def test_strength_starts_on_level_one(ctx, meshes):
    m, dm, A, bs, dofs, t, W, ctf = _system(ctx, meshes, "hex333")
    amg = A.amg(dofs, coarse_rows=COARSE_ROWS, first_transfer=t, strength=0.1)
    assert amg.n_levels >= 3
    assert not amg._soc(0)[1] and amg._soc(0)[5] is None and amg.strong_mask(0).all()      # no mask, no filtered matrix on level 0
    assert amg._soc(1)[1] and amg.levels[1]["omega_f"] is not None                  # level 1 has both
    _, direct = _direct(ctx, meshes, "hex333", amg, dofs, ctf, bs, strength=0.1)
    _assert_levels_below_are(amg, direct)
    assert np.array_equal(amg.strong_mask(1), direct.strong_mask(0))
    plain = A.amg(dofs, coarse_rows=COARSE_ROWS, first_transfer=t)
    assert not amg.strong_mask(1).all() or np.array_equal(amg.aggregates(1), plain.aggregates(1))
    r = _cuda(np.random.Generator(np.random.PCG64(2)).normal(size=A.shape[0]))
    assert np.isfinite(amg.apply(r).cpu().numpy()).all()


def test_errors_of_create_transfer(ctx, meshes, hip_library):
    from dolfinx_external_operator_amd._lib import AmgTransfer

    torch = _torch(ctx)
    lib, h = hip_library, ctx._h
    m, dm, A, bs, dofs, t, W, ctf = _system(ctx, meshes, "tri65")
    bct = torch.from_numpy(np.asarray(dofs, dtype=np.int32)).cuda()
    vals = C.c_void_p(A.values.data_ptr())

    def create(ptr=t.ptr, col=t.col, w=t.w, c2f=t.coarse_to_fine, n_coarse=t.n_coarse, first=True, theta=0.0, values=vals, null=None):
        arrays = [np.ascontiguousarray(a) for a in (ptr, col, w, c2f)]
        p = [None if null == k else a.ctypes.data for k, a in enumerate(arrays)]
        desc = AmgTransfer(n_coarse, *p)
        raw = C.c_void_p()
        rc = lib.dxo_amg_create_transfer(h, A.pattern._h, values, C.c_void_p(bct.data_ptr()), bct.numel(), None, 0, theta,
                                         C.byref(desc) if first else None, 10, COARSE_ROWS, 1, C.byref(raw))
        if rc == 0:
            nl = C.c_int()
            assert lib.dxo_amg_info(h, raw, C.byref(nl), None, None, 0, None) == 0
            on = C.c_int()
            assert lib.dxo_amg_transfer_info(h, raw, C.byref(on), None, None, None, None) == 0
            lib.dxo_amg_destroy(h, raw)
            return rc, nl.value, on.value
        assert not raw.value
        return rc, 0, 0

    plain = A.amg(dofs, coarse_rows=COARSE_ROWS)
    assert create() == (0, 3, 1)
    assert create(first=False) == (0, plain.n_levels, 0)                           # NULL: dxo_amg_create_soc exactly
    assert plain.first_transfer is None
    for k in range(4):
        assert create(null=k)[0] == -1                                             # DXO_E_NULL
    assert create(values=None)[0] == -1
    assert create(theta=1.0)[0] == -6
    row = int(np.flatnonzero(np.diff(t.ptr) == 2)[0])                              # an edge midpoint: two coarse nodes
    e = int(t.ptr[row])
    col = t.col.copy()
    col[e], col[e + 1] = col[e + 1], col[e]
    assert create(col=col)[0] == -6                                                # not ascending: DXO_E_OPTION
    col = t.col.copy()
    col[e + 1] = t.n_coarse
    assert create(col=col)[0] == -3                                                # out of range: DXO_E_SIZE
    col[e + 1] = -1
    assert create(col=col)[0] == -3
    ptr = t.ptr.copy()
    ptr[row + 1] = ptr[row]                                                        # a fine node without an entry
    assert create(ptr=ptr)[0] == -3
    ptr = t.ptr.copy()
    ptr[0] = 1
    assert create(ptr=ptr)[0] == -3
    c2f = t.coarse_to_fine.copy()
    c2f[1] = c2f[0]
    assert create(c2f=c2f)[0] == -6                                                # not injective
    c2f = t.coarse_to_fine.copy()
    c2f[0] = t.ptr.size - 1
    assert create(c2f=c2f)[0] == -3                                                # out of range
    c2f = t.coarse_to_fine.copy()
    c2f[0] = row
    assert create(c2f=c2f)[0] == -6                                                # its row is not the single entry (v, 1)
    w = t.w.copy()
    w[int(t.ptr[t.coarse_to_fine[0]])] = 0.5
    assert create(w=w)[0] == -6
    w = t.w.copy()
    w[e] = np.nan
    assert create(w=w)[0] == -6
    assert create(n_coarse=0)[0] == -3
    # the stagnation rule: a transfer that keeps more than 0.8 of the nodes (here: every node is its own coarse node)
    n = t.ptr.size - 1
    ident = (np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), np.ones(n), np.arange(n, dtype=np.int32))
    assert create(*ident, n_coarse=n)[0] == -3
    # the Python layer
    with pytest.raises(ValueError, match="first_transfer has"):
        plain.A.amg(dofs, first_transfer=_system(ctx, meshes, "quad54")[5])
    with pytest.raises(ValueError, match="degree 1"):
        meshes(structured_mesh("triangle", (3, 3), 1)).vertex_transfer(coordinate_element_at_nodes("triangle", 1))
    one = A.amg(dofs, coarse_rows=10 ** 6, first_transfer=t)                        # level 0 is the coarsest: checked, not used
    assert one.n_levels == 1 and one.first_transfer is None
