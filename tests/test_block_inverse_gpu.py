"""The pieces krylov.hip and amg.hip share (csrc/krylov_internal.h) on blocks that finite-element assembly never makes, against the
exact yardstick of tests/test_block_inverse_oracle_cpu.py: invert_block and the register Gauss-Jordan gj6 with pivots off the
diagonal, the singularity rule on both sides of its threshold and on NaN / Inf, the dense coarsest inverse with a zero diagonal, and
dxo_csr_spmv / CG on the block-size-6 patterns that dxo_amg_info hands out (row_product<6, 8 ... 64>)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from oracle.block_inverse_oracle import (ACCEPTED, DENSE_CASES, U, adversarial_blocks, cofactor_bound, exact_inverse, gj_exchanges,
                                         node_blocks, refined_solve, values_with_blocks, zero_diagonal_system)
from oracle.form_oracle import pattern_ref
from oracle.krylov_oracle import bottom_dofs, elastic_C3
from solver_cases import _assemble, _cuda, _torch, meshes  # noqa: F401  (meshes is a fixture)
from tools.synthetic import structured_mesh

pytestmark = pytest.mark.gpu

DXO_OK, DXO_E_DIM, DXO_E_SINGULAR = 0, -2, -8

# E = max |B_dev - B_exact| / (u kappa_inf max |B_exact|) of a block, u = 2^-53.
# bs 1, 2, 3: nothing is measured: every entry is held to cofactor_bound, the forward bound of the closed forms.
# bs 6 (gj6, Gauss-Jordan with partial pivoting in registers): the a-priori bound carries the growth factor 2^5 and n^3 and is of no
# use, so the constant is 100 x the largest E of the elimination, the rule of CYCLE_TOL and QR_TOL. The figures are those of a
# float64 transcription of gj6 in NumPy on the blocks of this module (the device differs from it by the fused multiply-adds alone):
# perm 0, dense 6.6e-2, rowscaled 8.8e-15 (kappa_inf carries the scaling), near 1.8e-1. Every run prints the device's own figures.
E6_TOL = 18.0
# the dense coarsest inverse (amg_dense_step, n = 306 and 32) applied to three right-hand sides against the refined solve:
# E = max |z_dev - z_ref| / (u kappa_inf max |z_ref|). The same transcription: 6.2e-3 (n 306, kappa_inf 2.0e4), 1.4e-2 (n 32,
# kappa_inf 1.8e3). 100 x the larger.
DENSE_TOL = 1.4

CASES = {"bs1_16": ("triangle", (3, 3), 1), "bs2_16": ("triangle", (3, 3), 2), "bs3_27": ("tetrahedron", (2, 2, 2), 3),
         "bs2_306": ("triangle", (17, 16), 2), "bs6_22": None}


class _Pattern:
    """A dxo_csr handle with host copies of its arrays."""

    def __init__(self, handle, bs, indptr, indices):
        self.h, self.bs, self.indptr, self.indices = handle, bs, indptr, indices
        self.n_rows, self.n_nodes = indptr.size - 1, (indptr.size - 1) // bs


@pytest.fixture(scope="module")
def hex_bar(ctx):
    """The hex_bar hierarchy of test_amg_nns_gpu.py (hexahedron (32, 3, 3), coarse_rows 40, rigid-body modes) with the patterns and
    matrices of its levels of block size 6."""
    from dolfinx_external_operator_amd import DeviceMesh, rigid_body_modes

    torch = _torch(ctx)
    m = structured_mesh("hexahedron", (32, 3, 3), 1, distort=0.1, seed=2)
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    bcs = bottom_dofs(m, 3)
    A = _assemble(ctx, dm, "eps", "eps", 3, elastic_C3(m.num_cells * m.nq), bcs=bcs)
    amg = A.amg(bcs, near_nullspace=rigid_body_modes(m.node_x, ctx=ctx), coarse_rows=40)
    assert amg.n_levels >= 3
    levels = {}
    for l in (1, 2):
        S = amg.level_matrix(l)
        info = amg._info(l)
        assert amg._nns(l)[0] == 6
        levels[l] = (_Pattern(info.csr, 6, S.indptr.astype(np.int64), S.indices.astype(np.int32)), S, info.values)
    assert levels[1][0].n_nodes == 22 and levels[2][0].n_nodes == 3
    torch.cuda.synchronize()
    yield {"amg": amg, "levels": levels, "A": A}
    amg.close()
    dm.close()


def _pattern(ctx, meshes, hex_bar, case):
    if CASES[case] is None:
        return hex_bar["levels"][1][0]
    cell, n, bs = CASES[case]
    m = structured_mesh(cell, n, 1)
    p = meshes(m).csr_pattern(bs)
    pat = _Pattern(p._h, bs, p.indptr.cpu().numpy(), p.indices.cpu().numpy())
    ref = pattern_ref(m, bs)
    assert np.array_equal(pat.indptr, ref[0]) and np.array_equal(pat.indices, ref[1])
    return pat


def _block_jacobi(ctx, lib, pat, vals):
    """(return code, inv (nodes, bs, bs)) of dxo_csr_block_jacobi; inv starts as NaN, so what is read was written."""
    torch = _torch(ctx)
    v = _cuda(vals)
    inv = torch.full((pat.n_nodes * pat.bs * pat.bs,), float("nan"), dtype=torch.float64, device="cuda")
    rc = lib.dxo_csr_block_jacobi(ctx._h, pat.h, C.c_void_p(v.data_ptr()), C.c_void_p(inv.data_ptr()))
    torch.cuda.synchronize()
    return rc, inv.cpu().numpy().reshape(-1, pat.bs, pat.bs)


_REFS = {}


def _reference(case, bs, n_nodes):
    """(blocks, family per node, exact inverses, kappa_inf per node, entrywise bound or None), made once per case."""
    if case not in _REFS:
        blocks, names = node_blocks(bs, n_nodes, seed=11 + bs)
        ex = [exact_inverse(a) for a in blocks]
        bound = np.stack([cofactor_bound(a)[0] for a in blocks]) if bs <= 3 else None
        _REFS[case] = (blocks, names, np.stack([e[0] for e in ex]), np.array([e[2] for e in ex]), bound)
    return _REFS[case]


def _block_E(got, exact, kappa):
    return np.max(np.abs(got - exact), axis=(1, 2)) / (U * kappa * np.max(np.abs(exact), axis=(1, 2)))


def _check_inverses(case, got, ref, skip=None):
    """Every node but `skip` within the tolerance; returns E per node."""
    blocks, names, exact, kappa, bound = ref
    keep = np.ones(len(blocks), dtype=bool)
    if skip is not None:
        keep[skip] = False
    assert np.isfinite(got[keep]).all(), case
    E = _block_E(got, exact, kappa)
    if bound is not None:
        excess = (np.abs(got - exact) - bound)[keep]
        assert excess.max() <= 0.0, (case, names[int(np.argmax(excess.max(axis=(1, 2))))], float(excess.max()))
    else:
        worst = int(np.argmax(np.where(keep, E, 0.0)))
        assert E[keep].max() <= E6_TOL, (case, names[worst], float(E[worst]))
    return E


@pytest.mark.parametrize("case", list(CASES))
def test_accepted_blocks_invert_within_the_bound(ctx, meshes, hip_library, hex_bar, case):
    pat = _pattern(ctx, meshes, hex_bar, case)
    ref = _reference(case, pat.bs, pat.n_nodes)
    blocks, names = ref[0], ref[1]
    if pat.bs >= 2:                  # the inputs reach the exchange (bs 6: gj6's compare-and-select)
        assert sum(bool(gj_exchanges(a)) for a in blocks) >= pat.n_nodes // 4
    assert pat.n_nodes == {"bs1_16": 16, "bs2_16": 16, "bs3_27": 27, "bs2_306": 306, "bs6_22": 22}[case]
    vals = values_with_blocks(pat.indptr, pat.indices, pat.bs, blocks, seed=5)
    rc, got = _block_jacobi(ctx, hip_library, pat, vals)
    for f in ACCEPTED:
        on = np.array([n == f for n in names])
        if on.any():
            E = _block_E(got, ref[2], ref[3])
            print(f"{case}: family {f}: largest E {E[on].max():.3e} (kappa_inf up to {ref[3][on].max():.2e})")
    assert rc == DXO_OK, (case, rc)
    _check_inverses(case, got, ref)
    # the off-diagonal blocks are not read: other noise, the same bits; and a second call repeats the first
    rc2, again = _block_jacobi(ctx, hip_library, pat, values_with_blocks(pat.indptr, pat.indices, pat.bs, blocks, seed=6))
    assert rc2 == DXO_OK and np.array_equal(again, got)
    assert np.array_equal(_block_jacobi(ctx, hip_library, pat, vals)[1], got)


@pytest.mark.parametrize("case", list(CASES))
def test_a_rejected_block_zeroes_its_inverse_and_raises_the_flag(ctx, meshes, hip_library, hex_bar, case):
    pat = _pattern(ctx, meshes, hex_bar, case)
    ref = _reference(case, pat.bs, pat.n_nodes)
    rejected = adversarial_blocks(pat.bs, seed=31 + pat.bs)["rejected"]
    assert set(rejected) == ({"zero", "nan", "inf"} | ({"tiny", "duplicate"} if pat.bs >= 2 else set()))
    good = values_with_blocks(pat.indptr, pat.indices, pat.bs, ref[0], seed=5)
    for name, bad in rejected.items():
        for node in (0, pat.n_nodes // 2, pat.n_nodes - 1):
            blocks = ref[0].copy()
            blocks[node] = bad
            with np.errstate(invalid="ignore"):
                rc, got = _block_jacobi(ctx, hip_library, pat, values_with_blocks(pat.indptr, pat.indices, pat.bs, blocks, seed=5))
            assert rc == DXO_E_SINGULAR, (case, name, node, rc)
            assert "singular" in ctx.lib.dxo_last_error(ctx._h).decode()
            assert np.array_equal(got[node], np.zeros((pat.bs, pat.bs))), (case, name, node, got[node])   # exactly zero, no NaN
            _check_inverses(case, got, ref, skip=node)
            rc, got = _block_jacobi(ctx, hip_library, pat, good)                 # repaired: the flag is cleared
            assert rc == DXO_OK, (case, name, node, rc)
            _check_inverses(case, got, ref)


@pytest.mark.parametrize("which", list(DENSE_CASES))
def test_dense_coarsest_inverse_under_forced_pivoting(ctx, meshes, which):
    from dolfinx_external_operator_amd.operand_eval import DeviceCSR

    torch = _torch(ctx)
    cell, n, bs = DENSE_CASES[which]
    indptr, indices, vals, seed = zero_diagonal_system(which)
    p = meshes(structured_mesh(cell, n, 1)).csr_pattern(bs)
    assert np.array_equal(p.indptr.cpu().numpy(), indptr) and np.array_equal(p.indices.cpu().numpy(), indices)
    A = DeviceCSR(p, _cuda(vals))
    S = A.to_scipy().toarray()
    N = S.shape[0]
    assert not np.diag(S).any() and N == {"p1_306": 306, "p1_bs2": 32}[which]
    amg = A.amg(None, max_levels=1)                                # setup() inside: no zero pivot reported
    assert amg.n_levels == 1
    R = np.random.Generator(np.random.PCG64(100 + seed)).normal(size=(N, 3))
    X, res = refined_solve(S, R)
    assert res <= 2 * U
    kappa = np.linalg.cond(S, np.inf)
    worst = 0.0
    for k in range(3):
        z = amg.apply(_cuda(R[:, k]))
        zh = z.cpu().numpy()
        assert np.isfinite(zh).all()
        worst = max(worst, float(np.max(np.abs(zh - X[:, k])) / (U * kappa * np.max(np.abs(X[:, k])))))
        assert torch.equal(amg.apply(_cuda(R[:, k])), z)                       # bitwise repeatable
    print(f"{which}: dense inverse, largest E {worst:.3e} (kappa_inf {kappa:.2e}, n {N})")
    assert worst <= DENSE_TOL, (which, worst)
    amg.setup()
    assert np.array_equal(amg.apply(_cuda(R[:, 2])).cpu().numpy(), zh)         # and so is the setup
    amg.close()


# ---- SpMV and CG on the patterns of block size 6
def _spmv(ctx, lib, pat, values_ptr, alpha, x, beta, y):
    rc = lib.dxo_csr_spmv(ctx._h, pat.h, C.c_void_p(values_ptr), float(alpha), C.c_void_p(x.data_ptr()), float(beta), C.c_void_p(y.data_ptr()))
    assert rc == DXO_OK, (rc, ctx.lib.dxo_last_error(ctx._h))
    return y


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("values", ["own", "random"])
def test_spmv_on_a_block_size_6_level_matches_scipy(ctx, hip_library, hex_bar, level, values):
    torch = _torch(ctx)
    pat, S, own_ptr = hex_bar["levels"][level]
    rng = np.random.Generator(np.random.PCG64(3 + level))
    if values == "random":
        vd = _cuda(rng.normal(size=pat.indices.size))
        S = sp.csr_matrix((vd.cpu().numpy(), pat.indices, pat.indptr), shape=S.shape)
        ptr = vd.data_ptr()
    else:
        ptr = own_ptr
    n = pat.n_rows
    assert n == 6 * pat.n_nodes and (level == 1 or np.diff(pat.indptr).max() // 6 < 8)      # level 2: fewer blocks than any lane width
    x, y0 = rng.normal(size=n), rng.normal(size=n)
    xd = _cuda(x)
    scale = np.linalg.norm(abs(S) @ abs(x)) + np.linalg.norm(y0)
    for lanes in (0, 8, 16, 32, 64):
        ctx.set_option("spmv_lanes", lanes)
        try:
            for alpha, beta in ((1.0, 0.0), (2.5, -0.5), (-1.0, 1.0), (0.0, 3.0)):
                y = _spmv(ctx, hip_library, pat, ptr, alpha, xd, beta, _cuda(y0)).cpu().numpy()
                ref = alpha * (S @ x) + beta * y0
                assert np.linalg.norm(y - ref) <= 1e-14 * (abs(alpha) + abs(beta)) * scale, (level, values, lanes, alpha, beta)
            nan = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")             # beta = 0: y is not read, all is written
            first = _spmv(ctx, hip_library, pat, ptr, 1.5, xd, 0.0, nan).cpu().numpy()
            assert np.isfinite(first).all() and np.linalg.norm(first - 1.5 * (S @ x)) <= 1e-14 * 1.5 * scale, (level, values, lanes)
            for _ in range(2):
                again = _spmv(ctx, hip_library, pat, ptr, 1.5, xd, 0.0, torch.empty_like(nan)).cpu().numpy()
                assert np.array_equal(again, first), (level, values, lanes)                      # bitwise repeatable
        finally:
            ctx.set_option("spmv_lanes", 0)


def test_cg_on_the_block_size_6_level(ctx, hip_library, hex_bar):
    from dolfinx_external_operator_amd._lib import KRYLOV_APPLY_FN, KrylovInfo, KrylovOp, KrylovPc

    torch = _torch(ctx)
    lib, h = hip_library, ctx._h
    pat, S, own_ptr = hex_bar["levels"][1]
    Sd = S.toarray()
    n = pat.n_rows
    assert np.abs(Sd - Sd.T).max() <= 1e-12 * np.abs(Sd).max() and np.linalg.eigvalsh(0.5 * (Sd + Sd.T)).min() > 0.0      # SPD
    b = np.random.Generator(np.random.PCG64(9)).normal(size=n)
    xref = np.linalg.solve(Sd, b)
    bd, xd = _cuda(b), torch.zeros(n, dtype=torch.float64, device="cuda")
    ws = C.c_void_p()
    assert lib.dxo_krylov_create(h, n, 1, C.byref(ws)) == DXO_OK
    try:
        op = KrylovOp(n, pat.h, C.c_void_p(own_ptr), KRYLOV_APPLY_FN(), None)
        info = KrylovInfo()
        rtol = 1e-10
        rc = lib.dxo_krylov_cg(h, ws, C.byref(op), None, C.c_void_p(bd.data_ptr()), C.c_void_p(xd.data_ptr()), rtol, 0.0, 2000, 8, C.byref(info))
        assert rc == DXO_OK and info.converged and not info.breakdown, (rc, info.iterations, info.residual)
        x = xd.cpu().numpy()
        assert np.linalg.norm(b - Sd @ x) <= rtol * np.linalg.norm(b) * (1 + 1e-6)
        # |x - x*| <= |A^-1| |r| <= rtol |A^-1| |A| |x*|
        assert np.linalg.norm(x - xref) <= rtol * np.linalg.cond(Sd) * np.linalg.norm(xref) * (1 + 1e-6)
        # block Jacobi has no kernel of block size 6: refused, not applied with another one
        inv = torch.zeros(pat.n_nodes * 36, dtype=torch.float64, device="cuda")
        pc = KrylovPc(2, 6, n, C.c_void_p(inv.data_ptr()))
        before = xd.clone()
        assert lib.dxo_krylov_cg(h, ws, C.byref(op), C.byref(pc), C.c_void_p(bd.data_ptr()), C.c_void_p(xd.data_ptr()), rtol, 0.0, 10, 8,
                                 C.byref(info)) == DXO_E_DIM
        assert lib.dxo_block_jacobi_apply(h, 6, n, C.c_void_p(inv.data_ptr()), C.c_void_p(bd.data_ptr()), C.c_void_p(xd.data_ptr())) == DXO_E_DIM
        torch.cuda.synchronize()
        assert torch.equal(xd, before)
    finally:
        lib.dxo_krylov_destroy(h, ws)


def test_level_one_mean_neighbour_count_is_below_the_lane_switch(hex_bar):
    """Why spmv_lanes is forced above: left alone, every level of the suite's 3-D systems takes 8 lanes per node."""
    pat = hex_bar["levels"][1][0]
    assert pat.indices.size / 36 / pat.n_nodes < 16.0
