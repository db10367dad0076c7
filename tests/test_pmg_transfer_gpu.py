"""dxo_pmg_create, dxo_pmg_restrict and dxo_pmg_prolong on the device against tests/pmg_reference.py: the transfers bit for bit (the
weights of the degree-1 element at the nodes of the degree-2 element are powers of two, so every product is exact and only the order
of a sum matters), the adjoint pair, the constrained dofs, the coarse constrained list and the argument errors of the creation."""
import ctypes as C

import numpy as np
import pytest

from oracle.amg_oracle import vertex_transfer_ref
from pmg_reference import PmgRef
from solver_cases import _cuda, _torch
from tools.synthetic import structured_mesh

pytestmark = pytest.mark.gpu

# rows of 1 and 2 entries (triangles, tetrahedra), and of 1, 2, 4 and 8 (hexahedra)
MESHES = {"tri3": ("triangle", (3, 3)), "tet2": ("tetrahedron", (2, 2, 2)), "hex2": ("hexahedron", (2, 2, 2)), "tri40": ("triangle", (40, 40))}
_HOST = {}


def host(which):
    if which not in _HOST:
        cell, n = MESHES[which]
        m = structured_mesh(cell, n, 2, distort=0.1, seed=2)
        _HOST[which] = (m,) + vertex_transfer_ref(m)
    return _HOST[which]


def face_dofs(m, bs, rollers=False):
    """The face x_last = 0 clamped; with rollers also the first component alone on x_0 = 0: partly constrained nodes."""
    on = np.flatnonzero(np.abs(m.node_x[:, -1]) < 1e-12)
    dofs = (on[:, None] * bs + np.arange(bs)).reshape(-1)
    if rollers:
        dofs = np.unique(np.concatenate([dofs, np.flatnonzero(np.abs(m.node_x[:, 0]) < 1e-12) * bs]))
    return dofs


def transfer_of(W, ctf):
    from dolfinx_external_operator_amd import NodalTransfer

    return NodalTransfer(W.shape[1], W.indptr, W.indices, W.data, ctf)


def check(ctx, which, bs, dofs, seed=0):
    from dolfinx_external_operator_amd import PMG

    _torch(ctx)
    m, W, ctf = host(which)
    assert set(np.log2(W.data)) <= {0.0, -1.0, -2.0, -3.0}                         # powers of two
    ref = PmgRef(W, ctf, bs, dofs)
    pmg = PMG(transfer_of(W, ctf), bs, constrained=None if dofs is None else dofs, ctx=ctx)
    assert pmg.n == ref.n and pmg.n_coarse == ref.nc
    assert np.array_equal(pmg.p_diag.cpu().numpy(), ref.p_diag)
    cc = pmg.coarse_constrained
    assert str(cc.dtype) == "torch.int32" and cc.is_cuda and np.array_equal(cc.cpu().numpy(), ref.coarse_constrained)
    rng = np.random.Generator(np.random.PCG64(seed))
    r, e = rng.normal(size=ref.n), rng.normal(size=ref.nc)
    rc = pmg.restrict(_cuda(r)).cpu().numpy()
    x = pmg.prolong(_cuda(e)).cpu().numpy()
    assert np.array_equal(rc, ref.restrict(r)), which                              # bit for bit the sequential sums
    assert np.array_equal(x, ref.prolong(e)), which
    # the adjoint pair: both sides are sum_iv p_iv e_v r_i; a transfer sum has at most 8 (P e) or 27 (P^T r) terms, a dot product n or
    # n_c, each term rounded once more: |lhs - rhs| <= 1.01 (8 + 27 + n + n_c) u S, S the same sum over absolute values
    lhs, rhs = x @ r, e @ rc
    S = np.abs(e) @ (np.abs(ref.P).T @ np.abs(r))
    assert abs(lhs - rhs) <= 1.01 * (35 + ref.n + ref.nc) * 2.0 ** -53 * S, (lhs, rhs, S)
    # constrained dofs receive and send exactly 0
    mask = ref.mask
    if mask.any():
        assert not x[mask].any() and not rc[ref.coarse_constrained].any()
        only = np.where(mask, r, 0.0)
        assert not pmg.restrict(_cuda(only)).cpu().numpy().any()
        conly = np.zeros(ref.nc)
        conly[ref.coarse_constrained] = e[ref.coarse_constrained]
        assert not pmg.prolong(_cuda(conly)).cpu().numpy().any()
    # out= is SET, not accumulated into
    buf = _cuda(np.full(ref.nc, 7.0))
    pmg.restrict(_cuda(r), out=buf)
    assert np.array_equal(buf.cpu().numpy(), rc)
    buf = _cuda(np.full(ref.n, 7.0))
    pmg.prolong(_cuda(e), out=buf)
    assert np.array_equal(buf.cpu().numpy(), x)
    pmg.close()
    return ref


@pytest.mark.parametrize("clamped", [False, True])
@pytest.mark.parametrize("bs", [1, 2, 3])
@pytest.mark.parametrize("which", ["tri3", "tet2", "hex2"])
def test_transfers_bit_for_bit(ctx, which, bs, clamped):
    m, W, _ = host(which)
    counts = set(np.diff(W.indptr))
    assert counts == ({1, 2, 4, 8} if which == "hex2" else {1, 2})
    ref = check(ctx, which, bs, face_dofs(m, bs, rollers=bs > 1) if clamped else None, seed=bs)
    if clamped and bs > 1:                                                       # a partly constrained node keeps its other components
        part = ref.mask.reshape(-1, bs)
        assert (part.any(axis=1) & ~part.all(axis=1)).any()


def test_transfers_across_workgroups_and_the_grid_stride(ctx):
    """P2 triangles 40^2: 19683 fine and 5043 coarse dofs at bs 3, 77 and 20 workgroups; with the cap of the grid at 3 workgroups
    (option pmg_grid_blocks) every thread strides, 26 times on the fine vector."""
    m, _, _ = host("tri40")
    dofs = face_dofs(m, 3, rollers=True)
    check(ctx, "tri40", 3, dofs, seed=5)
    saved = ctx.get_option("pmg_grid_blocks")
    try:
        ctx.set_option("pmg_grid_blocks", 3)
        check(ctx, "tri40", 3, dofs, seed=6)
        check(ctx, "tri40", 2, None, seed=7)
    finally:
        ctx.set_option("pmg_grid_blocks", saved)
    with pytest.raises(ValueError):
        ctx.set_option("pmg_grid_blocks", -1)


def test_errors_of_create(ctx, hip_library):
    """Every malformed transfer of the list of dxo_amg_create_transfer with its code, NULLs and the block size. The stagnation rule
    of that list is a stopping rule of the multigrid's coarsening, not a property of a transfer: here the identity is a valid one."""
    from dolfinx_external_operator_amd._lib import AmgTransfer

    torch = _torch(ctx)
    lib, h = hip_library, ctx._h
    m, W, ctf = host("tri3")
    t = transfer_of(W, ctf)
    n = t.ptr.size - 1
    bct = torch.from_numpy(face_dofs(m, 2).astype(np.int32)).cuda()

    def create(ptr=t.ptr, col=t.col, w=t.w, c2f=t.coarse_to_fine, n_coarse=t.n_coarse, null=None, bs=2, n_nodes=n, desc=True, bc=bct, n_bc=None,
               out=True):
        arrays = [np.ascontiguousarray(a) for a in (ptr, col, w, c2f)]
        p = [None if null == k else a.ctypes.data for k, a in enumerate(arrays)]
        d = AmgTransfer(n_coarse, *p)
        raw = C.c_void_p()
        rc = lib.dxo_pmg_create(h, n_nodes, bs, C.byref(d) if desc else None, C.c_void_p(bc.data_ptr()) if bc is not None else None,
                                (bct.numel() if bc is not None else 0) if n_bc is None else n_bc, C.byref(raw) if out else None)
        if rc == 0:
            nc = C.c_int64()
            assert lib.dxo_pmg_info(h, raw, C.byref(nc), None, None, None, None, None, None, None, None) == 0
            assert lib.dxo_pmg_destroy(h, raw) == 0
            assert lib.dxo_pmg_destroy(h, raw) == -6                                  # no longer a live object: refused, not freed twice
            return rc, nc.value
        assert not raw.value
        return rc, 0

    assert create() == (0, t.n_coarse * 2)
    assert create(bc=None) == (0, t.n_coarse * 2)
    for k in range(4):
        assert create(null=k)[0] == -1                                             # DXO_E_NULL
    assert create(desc=False)[0] == -1 and create(out=False)[0] == -1
    assert create(bc=None, n_bc=3)[0] == -1                                        # a count without a list
    for bs in (0, 4, 6):
        assert create(bs=bs)[0] == -2                                              # DXO_E_DIM
    assert create(n_bc=-1)[0] == -3 and create(n_nodes=-1)[0] == -3
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
    c2f[0] = n
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
    assert create(n_coarse=n + 1)[0] == -3                                         # more coarse nodes than nodes
    ident = (np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), np.ones(n), np.arange(n, dtype=np.int32))
    assert create(*ident, n_coarse=n) == (0, n * 2)                                # the identity: valid here
