"""The array-free 3-D hyperelastic consumers on the GPU: dxo_isihara3_residual, dxo_isihara3_tangent_apply and
dxo_isihara3_tangent_diagonal form the internal force, K v and diag(K) of the analytic Isihara model from the dof vector alone.
They are held to the CPU oracles (tests/hyper3_cases.py for the model, oracle/form_oracle.py and oracle/operand_oracle.py for the
forms), to the array route on the device (dxo_isihara3_field, then adjoint("F") / bilinear_apply / bilinear_diagonal), to a Taylor
remainder of their own, to the symmetry of the operator, to the invariances of the energy, to the NaN pattern of the array route on an
inverted cell, and to the consumer semantics (out +=, SET with consumer_overwrite, bit-reproducible). The meshes are the 13 of
hyper3_reference_cases.FUSED_MESHES: one and several wave groups, ragged last groups, 55 and 63 points per group, compile-time and
run-time node counts, cells_per_wave = 2."""
import ctypes as C
import functools

import numpy as np
import pytest

import hyper3_cases as H3
from dolfinx_external_operator_amd import MEM_DEVICE, DeviceMesh, IsiharaParams
from hyper3_reference_cases import FUSED_MESHES, fused_mesh
from oracle.form_oracle import bilinear_diag_ref, bilinear_ref, diagonal_by_probes, node_colours, tables
from oracle.operand_oracle import DEFGRAD, eval_operand, operand_adjoint
from solver_cases import _cuda, _zeros
from test_hyper3_gpu import _field
from tools.synthetic import structured_mesh

pytestmark = pytest.mark.gpu

PRM = IsiharaParams(*H3.DEFAULTS)
NAMES = list(FUSED_MESHES)
TOL = 1e-12      # of max |ref|: the figure of these consumers against the same oracle (tests/test_bilinear_gpu.py)
E_NULL, E_DIM, E_OPTION = -1, -2, -6
ENTRIES = ("dxo_isihara3_residual", "dxo_isihara3_tangent_apply", "dxo_isihara3_tangent_diagonal")


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@functools.lru_cache(maxsize=None)
def case(name):
    """What the three entries are held to on the mesh `name`, computed once on the CPU and read-only: the field u, a direction v, the
    smallest det F, and the oracle's residual, action and diagonal with (P, dP) = H3.reference(F), F from the operand oracle."""
    m = fused_mesh(name)
    nn, nc, nq = m.node_x.shape[0], m.num_cells, m.nq
    u = _field(m, 0.15, 9)
    v = np.random.Generator(np.random.PCG64(23)).normal(size=nn * 3)
    F = eval_operand(DEFGRAD, 3, u, *tables(m)).reshape(-1, 9)
    P, dP = H3.reference(F)
    R = operand_adjoint(DEFGRAD, 3, P.reshape(nc, nq, 9), m.weights, *tables(m), nn)
    Kv = bilinear_ref(m, "grad", "grad", 3, dP, v)
    dg = bilinear_diag_ref(m, "grad", "grad", 3, dP)
    out = dict(u=u, v=v, det_min=float(H3.det_rows(F).min()), R=np.asarray(R).reshape(-1), Kv=Kv, diag=dg)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return m, out


class Device:
    """the mesh on the device and the three new entries on torch tensors"""

    def __init__(self, ctx, m):
        import torch

        self.ctx, self.m, self.n = ctx, m, m.node_x.shape[0] * 3
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        self.dm = DeviceMesh.from_synthetic(m, ctx=ctx)

    def residual(self, u, out=None):
        out = _zeros(self.n) if out is None else out
        self.dm.isihara3_residual(PRM, u.data_ptr(), out.data_ptr())
        return out

    def apply(self, u, v, out=None):
        out = _zeros(self.n) if out is None else out
        self.dm.isihara3_tangent_apply(PRM, u.data_ptr(), v.data_ptr(), out.data_ptr())
        return out

    def diagonal(self, u, out=None):
        out = _zeros(self.n) if out is None else out
        self.dm.isihara3_tangent_diagonal(PRM, u.data_ptr(), out.data_ptr())
        return out

    def array_route(self, u, v, refused=False):
        """(R, K v, diag K) through dP[n][9][9] and P[n][9]. refused: the mesh is one of ARRAY_ROUTE_REFUSES, where adjoint("F") and
        bilinear_diagonal must answer DXO_E_SIZE; their places in the result are None"""
        npts = self.m.num_cells * self.m.nq
        dP, P = _zeros(npts * 81), _zeros(npts * 9)
        self.ctx.isihara3_field(PRM, self.dm._h, MEM_DEVICE, u.data_ptr(), dP.data_ptr(), P.data_ptr())
        R, Kv, dg = _zeros(self.n), _zeros(self.n), _zeros(self.n)
        self.dm.bilinear_apply("grad", "grad", 3, dP.data_ptr(), v.data_ptr(), Kv.data_ptr())
        if refused:
            with pytest.raises(ValueError, match="DXO_E_SIZE"):
                self.dm.adjoint("F", 3, P.data_ptr(), R.data_ptr())
            with pytest.raises(ValueError, match="DXO_E_SIZE"):
                self.dm.bilinear_diagonal("grad", "grad", 3, dP.data_ptr(), dg.data_ptr())
            return None, Kv, None
        self.dm.adjoint("F", 3, P.data_ptr(), R.data_ptr())
        self.dm.bilinear_diagonal("grad", "grad", 3, dP.data_ptr(), dg.data_ptr())
        return R, Kv, dg

    def close(self):
        self.dm.close()


@pytest.fixture
def device(ctx):
    made = []

    def make(m):
        made.append(Device(ctx, m))
        return made[-1]

    yield make
    for d in made:
        d.close()


@pytest.mark.parametrize("name", NAMES)
def test_against_the_cpu_oracles(device, name):
    """R, K v and diag(K) against the float64 oracles at u = _field(m, 0.15, 9), where det F > 0.2 on every mesh: 1e-12 of max |ref|."""
    m, ref = case(name)
    assert ref["det_min"] > 0.2, ref["det_min"]
    d = device(m)
    u, v = _cuda(ref["u"]), _cuda(ref["v"])
    got = {"R": d.residual(u), "Kv": d.apply(u, v), "diag": d.diagonal(u)}
    err = {k: _rel(g.cpu().numpy(), ref[k]) for k, g in got.items()}
    print(f"{name}: det F >= {ref['det_min']:.3f}, R {err['R']:.2e}, K v {err['Kv']:.2e}, diag {err['diag']:.2e}")
    for k, e in err.items():
        assert e <= TOL, (k, e)


# Where the array route has no residual and no diagonal to compare with. dxo_operand_adjoint and dxo_bilinear_diagonal ask for more
# than the 64 KiB of LDS on Q2 hexahedra with 27 or 28 points per cell: the tables take 28 736 / 29 792 bytes, and beside them four
# waves' regions of 1216 doubles (the staging space of the tangent rows; the parked matrices of 64 points) and the vertices come to
# 67 648 / 68 704 and 69 248 / 70 304 bytes ("which the 27-point rule's do not fit"). The new entries stage nothing and
# park the matrices of the group's own 54 / 56 points: 62 144 ... 65 440 bytes. On these meshes the test asserts the array route's
# refusal and compares K v alone; R and the diagonal are held to the CPU oracle and to the probes there like everywhere else.
ARRAY_ROUTE_REFUSES = [name for name in NAMES if name.endswith((", 27 points", "7x2x2 points"))]
assert len(ARRAY_ROUTE_REFUSES) == 3


@pytest.mark.parametrize("name", NAMES)
def test_against_the_array_route_on_the_device(device, name):
    """The same three vectors through dxo_isihara3_field and the array consumers: 1e-12 of max |ref| and nothing tighter, the two
    routes contract in a different order. Observed maximum over the 13 meshes on an MI355X: R 3.5e-16, K v 5.6e-16, diag 3.7e-16
    (R and diag over the ten meshes on which the array route has them, see ARRAY_ROUTE_REFUSES)."""
    m, ref = case(name)
    d = device(m)
    u, v = _cuda(ref["u"]), _cuda(ref["v"])
    old = d.array_route(u, v, refused=name in ARRAY_ROUTE_REFUSES)
    new = (d.residual(u), d.apply(u, v), d.diagonal(u))
    err = [None if b is None else _rel(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(new, old)]
    print(f"{name}: new against array route, R {err[0]}, K v {err[1]}, diag {err[2]}")
    for what, e in zip(("R", "Kv", "diag"), err):
        assert e is None or e <= TOL, (what, e)
    assert all(bool(np.isfinite(a.cpu().numpy()).all()) for a in new)


@pytest.mark.parametrize("name", ["P2 tetrahedra (2,2,1)", "Q2 hexahedra (2,1,2), 27 points"])
def test_taylor_remainder_with_the_new_entries_only(device, name):
    """|R(u + h v) - R(u) - h K(u) v| = O(h^2) with R and K v from the new entries: observed order >= 1.9 between h = 1e-2, 5e-3,
    2.5e-3, the steps and the bound of test_hyper3_gpu.test_taylor_remainder_of_the_internal_force_is_second_order."""
    import torch

    m = fused_mesh(name)
    d = device(m)
    rng = np.random.Generator(np.random.PCG64(17))
    u, v = _cuda(0.02 * rng.uniform(-1.0, 1.0, d.n)), _cuda(rng.uniform(-1.0, 1.0, d.n))
    R0, Kv = d.residual(u), d.apply(u, v)
    assert float(torch.linalg.norm(Kv)) > 0
    hs = [1e-2, 5e-3, 2.5e-3]
    rem = [float(torch.linalg.norm(d.residual(u + h * v) - R0 - h * Kv)) for h in hs]
    orders = [np.log(rem[k] / rem[k + 1]) / np.log(hs[k] / hs[k + 1]) for k in range(2)]
    print(name, "remainders", rem, "orders", orders)
    assert min(orders) >= 1.9, (rem, orders)


@pytest.mark.parametrize("name", NAMES)
def test_symmetry_and_the_diagonal_by_probes(device, name):
    """w . K v = v . K w to 1e-12 of it for two random vectors, and diag(K) is e_i . K e_i through the NEW action, one node colour at
    a time, to 1e-12 of the largest entry."""
    import torch

    m, ref = case(name)
    d = device(m)
    rng = np.random.Generator(np.random.PCG64(29))
    u, v, w = _cuda(ref["u"]), _cuda(rng.normal(size=d.n)), _cuda(rng.normal(size=d.n))
    a, b = float(torch.dot(w, d.apply(u, v))), float(torch.dot(v, d.apply(u, w)))
    print(f"{name}: w.Kv = {a!r}, v.Kw = {b!r}, difference {abs(a - b) / abs(a):.2e} of it")
    assert abs(a - b) <= 1e-12 * abs(a)
    probe = diagonal_by_probes(lambda x: d.apply(u, _cuda(x)).cpu().numpy(), m.node_x.shape[0], 3, node_colours(m))
    dg = d.diagonal(u).cpu().numpy()
    print(f"{name}: diagonal against probes {_rel(dg, probe):.2e}")
    assert np.abs(dg - probe).max() <= TOL * np.abs(probe).max()


def _rigid_modes(x):
    """the three translations and the three infinitesimal rotations e_k x (x - centre) at the nodes x, (6, n * 3)"""
    xc = x - x.mean(axis=0)
    modes = [np.tile(e, (x.shape[0], 1)) for e in np.eye(3)] + [np.cross(e, xc) for e in np.eye(3)]
    return np.array([mo.reshape(-1) for mo in modes])


@pytest.mark.parametrize("name", ["Q2 hexahedra (2,1,2), 8 points", "P2 tetrahedra (2,2,1)"])
def test_invariance_known_answers(device, name):
    """The energy depends on C = F^T F alone and is stress free at F = I. At u = 0: K t = 0 for the translations and K rho = 0 for the
    infinitesimal rotations, to 1e-12 s with s = max |K(0) r| of a random unit-scale r. At the finite rotation u = Q x - x (in the
    quadratic field space exactly): R = 0 to 1e-12 s_R, s_R = max |R| of a 10 % uniaxial stretch, and K t = 0 to 1e-12 s."""
    m = fused_mesh(name)
    d = device(m)
    x = m.node_x
    rng = np.random.Generator(np.random.PCG64(31))
    zero, r = _zeros(d.n), _cuda(rng.normal(size=d.n))
    modes = _rigid_modes(x)
    s = float(d.apply(zero, r).abs().max())
    assert s > 0
    for k, mode in enumerate(modes):
        worst = float(d.apply(zero, _cuda(mode)).abs().max())
        print(f"{name}: u = 0, rigid mode {k}: max |K mode| = {worst:.2e} = {worst / s:.2e} s")
        assert worst <= TOL * s, (k, worst, s)
    stretch = np.zeros_like(x)
    stretch[:, 0] = 0.1 * x[:, 0]
    s_R = float(d.residual(_cuda(stretch)).abs().max())
    assert s_R > 0
    axis, angle = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), 0.7
    A = np.cross(np.eye(3), axis)
    Q = np.eye(3) + np.sin(angle) * A + (1.0 - np.cos(angle)) * A @ A      # Rodrigues
    assert np.allclose(Q @ Q.T, np.eye(3)) and np.isclose(np.linalg.det(Q), 1.0)
    uq = _cuda(x @ Q.T - x)
    worst = float(d.residual(uq).abs().max())
    print(f"{name}: finite rotation: max |R| = {worst:.2e} = {worst / s_R:.2e} s_R")
    assert worst <= TOL * s_R, (worst, s_R)
    for k in range(3):
        worst = float(d.apply(uq, _cuda(modes[k])).abs().max())
        print(f"{name}: finite rotation, translation {k}: max |K t| = {worst:.2e} = {worst / s:.2e} s")
        assert worst <= TOL * s, (k, worst, s)


# (mesh, cell, local node, factor): the node moves by -factor (x_node - centroid of the cell's nodes), through the cell
INVERTED = [("P2 tetrahedra (2,2,1)", 5, 3, 4.0), ("P1 tetrahedra (3,2,2)", 7, 2, 2.5)]


@pytest.mark.parametrize("name,cell,local,factor", INVERTED)
def test_nan_containment_on_an_inverted_cell(device, name, cell, local, factor):
    """One dof moved so that det F < 0 at every point of a cell (and |det F| > 0.05 at every point of the mesh, by the operand
    oracle): the NaNs of R, K v and the diagonal sit on exactly the dofs where the array route puts them, the dofs of the inverted
    cells, and the finite entries agree with the array route's."""
    m = fused_mesh(name)
    d = device(m)
    nodes = m.dofmap[cell]
    u = _field(m, 0.05, 3).reshape(-1, 3)
    u[nodes[local]] -= factor * (m.node_x[nodes[local]] - m.node_x[nodes].mean(axis=0))
    det = H3.det_rows(eval_operand(DEFGRAD, 3, u.reshape(-1), *tables(m)).reshape(-1, 9)).reshape(m.num_cells, m.nq)
    assert np.abs(det).min() > 0.05 and (det[cell] < 0).all()
    bad_cells = np.flatnonzero((det < 0).any(axis=1))
    expect = np.zeros((m.node_x.shape[0], 3), dtype=bool)
    expect[np.unique(m.dofmap[bad_cells])] = True
    assert expect.any() and not expect.all()
    ud, vd = _cuda(u), _cuda(np.random.Generator(np.random.PCG64(37)).normal(size=d.n))
    old = d.array_route(ud, vd)
    new = (d.residual(ud), d.apply(ud, vd), d.diagonal(ud))
    for what, a, b in zip(("R", "Kv", "diag"), new, old):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(np.isnan(b), expect.reshape(-1)), what      # the array route: every dof of the inverted cells
        assert np.array_equal(np.isnan(a), np.isnan(b)), what
        keep = ~np.isnan(b)
        assert np.isfinite(a[keep]).all() and np.abs(a[keep] - b[keep]).max() <= TOL * np.abs(b[keep]).max(), what


@pytest.mark.parametrize("name", ["P2 tetrahedra (2,2,1), 7 points", "Q2 hexahedra (3,3,2), 27 points"])
def test_consumer_semantics(ctx, device, name):
    """Two consecutive calls are bit-identical. With consumer_overwrite = 0 a prefilled vector receives prefill + result: node_sum
    adds the node's sum to the prefill in one addition, so the difference to prefill + (zero-filled call) is the rounding of that
    addition, 2^-53 |prefill + result|, beside the 1e-15 max |result| granted to the result itself. With consumer_overwrite = 1 a
    vector prefilled with NaN comes back finite and bit-identical to the zero-filled call."""
    import torch

    m, ref = case(name)
    d = device(m)
    u, v = _cuda(ref["u"]), _cuda(ref["v"])
    calls = {"R": lambda out=None: d.residual(u, out), "Kv": lambda out=None: d.apply(u, v, out), "diag": lambda out=None: d.diagonal(u, out)}
    saved = ctx.get_option("consumer_overwrite")
    try:
        ctx.set_option("consumer_overwrite", 0)
        zero_filled = {k: f() for k, f in calls.items()}
        for k, f in calls.items():
            assert torch.isfinite(zero_filled[k]).all() and float(zero_filled[k].abs().max()) > 0, k
            assert torch.equal(f(), zero_filled[k]), k
            prefill = _cuda(np.random.Generator(np.random.PCG64(41)).normal(size=d.n) * float(zero_filled[k].abs().max()))
            want = prefill + zero_filled[k]
            got = f(prefill.clone())
            bound = 1e-15 * float(zero_filled[k].abs().max()) + 2.0 ** -53 * want.abs()
            assert bool(((got - want).abs() <= bound).all()), (k, float((got - want).abs().max()))
        ctx.set_option("consumer_overwrite", 1)
        for k, f in calls.items():
            got = f(torch.full((d.n,), float("nan"), dtype=torch.float64, device="cuda"))
            assert torch.isfinite(got).all() and torch.equal(got, zero_filled[k]), k
    finally:
        ctx.set_option("consumer_overwrite", saved)


def test_refusals(ctx, hip_library):
    """NULL params / mesh / arrays: DXO_E_NULL; a 2-D mesh: DXO_E_DIM; a mesh without weights: DXO_E_OPTION; and dxo_last_error names
    the entry after every refusal. Through ctypes, as H3.field_bad_calls does for the array route."""
    lib, h = hip_library, ctx._h
    m3 = structured_mesh("tetrahedron", (1, 1, 1), 2, distort=0.0, seed=0)
    m2 = structured_mesh("triangle", (2, 2), 2, distort=0.0, seed=0)
    d3, d2 = DeviceMesh.from_synthetic(m3, ctx=ctx), DeviceMesh.from_synthetic(m2, ctx=ctx)
    bare = DeviceMesh(gdim=3, phi=m3.phi, dphi=m3.dphi, dpsi=m3.dpsi, dofmap=m3.dofmap, geom_dofmap=m3.geom_dofmap, x=m3.x,
                      num_field_nodes=m3.node_x.shape[0], ctx=ctx)
    buf = _zeros(3 * max(m3.node_x.shape[0] * 3, m2.node_x.shape[0] * 3))
    n = buf.numel() // 3
    a, b, c = (buf.data_ptr() + 8 * n * k for k in range(3))
    prm = C.byref(PRM)
    try:
        # (what, code, arguments after ctx) per entry: residual (prm, mesh, u, R), apply (prm, mesh, u, v, out), diagonal (prm, mesh, u, out)
        def calls(arrays):
            return [("NULL params", E_NULL, (None, d3._h) + arrays), ("NULL mesh", E_NULL, (prm, None) + arrays),
                    ("2-D mesh", E_DIM, (prm, d2._h) + arrays), ("no weights", E_OPTION, (prm, bare._h) + arrays)] + \
                   [(f"NULL array {k}", E_NULL, (prm, d3._h) + arrays[:k] + (None,) + arrays[k + 1:]) for k in range(len(arrays))]

        for entry, arrays in zip(ENTRIES, ((a, b), (a, b, c), (a, b))):
            fn = getattr(lib, entry)
            for what, code, args in calls(arrays):
                rc = fn(h, *args)
                assert rc == code, (entry, what, rc)
                msg = lib.dxo_last_error(h).decode()
                assert msg.startswith(entry + ":"), (entry, what, msg)
            assert fn(None, *calls(arrays)[0][2]) == E_NULL      # a NULL context, before anything else
        with pytest.raises(ValueError, match="DXO_E_DIM"):
            d2.isihara3_residual(PRM, a, b)
    finally:
        for dm in (d3, d2, bare):
            dm.close()
