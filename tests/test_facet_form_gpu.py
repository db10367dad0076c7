"""dxo_mesh_set_facet_geometry / dxo_facet_set_* / dxo_eval_facet_geometry / dxo_facet_adjoint / dxo_facet_pressure on the device:
against the NumPy oracle of tests/test_facet_oracle_cpu.py, the divergence theorem against the cell adjoint of DIV, adjointness with
dxo_eval_operand_facets, the resultant of a pressure on the quarter annulus, reproducibility, graph capture, errors, and the
example that solves the von Mises demo's cylinder on the device."""
import ctypes as C

import numpy as np
import pytest

from test_facet_oracle_cpu import CELLS, facet_geometry_ref, mirrored
from tools.synthetic import exterior_facets, facet_geometry, facet_tables, quarter_annulus, structured_mesh

pytestmark = pytest.mark.gpu

# linear kinds of dxo_facet_adjoint and whether they take bs = 1
KINDS = [("value", True), ("grad", True), ("value_grad", True), ("eps", False), ("div", False), ("F", False)]


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).cuda()


def _zeros(n):
    import torch

    return torch.zeros(n, dtype=torch.float64, device="cuda")


def _mesh(ctx, m, geometry=True):
    from dolfinx_external_operator_amd import DeviceMesh

    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    dm.set_facet_tables(*facet_tables(m)[:3])
    if geometry:
        dm.set_facet_geometry(*facet_geometry(m.cell))
    return dm


def _sync(ctx):
    import torch

    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    return torch


def _pressure(ctx, dm, fs, n, p=None, scale=1.0, out=None):
    torch = _sync(ctx)
    out = _zeros(n) if out is None else out
    dm.facet_pressure(fs, out.data_ptr(), None if p is None else p.data_ptr(), scale)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("mirror", [False, True])
def test_geometry_matches_the_oracle(ctx, cell, degree, mirror):
    m = structured_mesh(cell, CELLS[cell], degree, distort=0.2, seed=3)
    if mirror:
        m = mirrored(m)
    nf = len(facet_geometry(cell)[1])
    ents = np.array([(c, f) for c in range(m.num_cells) for f in range(nf)], dtype=np.int32)
    dm = _mesh(ctx, m)
    try:
        fs = dm.facet_set(ents)
        assert dm.facet_set(ents.copy()) is fs                       # kept by the mesh, keyed by the entities' bytes
        nq = facet_tables(m)[0].shape[1]
        nd, dS = _zeros(len(ents) * nq * m.gdim), _zeros(len(ents) * nq)
        torch = _sync(ctx)
        dm.facet_geometry(fs, nd.data_ptr(), dS.data_ptr())
        torch.cuda.synchronize()
        n_ref, dS_ref = facet_geometry_ref(m, ents)
        assert np.abs(nd.cpu().numpy() - n_ref.reshape(-1)).max() <= 1e-13
        assert np.abs(dS.cpu().numpy() - dS_ref.reshape(-1)).max() <= 1e-13 * dS_ref.max()
        only = _zeros(len(ents) * nq)
        dm.facet_geometry(fs, None, only.data_ptr())                 # either output may be absent
        torch.cuda.synchronize()
        assert torch.equal(only, dS)
    finally:
        dm.close()


@pytest.mark.parametrize("cell,n,distort", [("triangle", (6, 5), 0.2), ("tetrahedron", (3, 2, 3), 0.2),
                                            ("quadrilateral", (5, 6), 0.0), ("hexahedron", (3, 2, 3), 0.0)])
@pytest.mark.parametrize("degree", [1, 2])
def test_divergence_identity(ctx, cell, n, distort, degree):
    """int_boundary v . n ds = int div v dx for every v of the space: exact at the degree-2 rules on these meshes."""
    m = structured_mesh(cell, n, degree, distort=distort, seed=8)
    G, nn = m.gdim, m.node_x.shape[0]
    dm = _mesh(ctx, m)
    try:
        got = _pressure(ctx, dm, dm.facet_set(exterior_facets(m)), nn * G).cpu().numpy()
        ones, div = _cuda(np.ones(m.num_cells * m.nq)), _zeros(nn * G)
        torch = _sync(ctx)
        dm.adjoint("div", G, ones.data_ptr(), div.data_ptr())
        torch.cuda.synchronize()
        ref = div.cpu().numpy()
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    finally:
        dm.close()


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("degree", [1, 2])
def test_adjointness_with_the_facet_operand(ctx, cell, degree):
    """<u, facet_adjoint(kind, S)> = sum_eq dS S . operand_facets(kind, u), every linear kind and block size."""
    m = structured_mesh(cell, CELLS[cell], degree, distort=0.2, seed=9)
    G, nn = m.gdim, m.node_x.shape[0]
    rng = np.random.Generator(np.random.PCG64(21))
    ents = exterior_facets(m)
    ents = ents[rng.permutation(len(ents))[: max(3, len(ents) * 2 // 3)]]     # a subset, not in cell order
    dm = _mesh(ctx, m)
    try:
        fs = dm.facet_set(ents)
        _, dS = facet_geometry_ref(m, ents)
        for kind, scalar in KINDS:
            for bs in ((1, G) if scalar else (G,)):
                u = rng.normal(size=nn * bs)
                e = dm.evaluate_facets(kind, bs, u, ents)
                if kind == "F":
                    e = e - np.eye(G).reshape(-1)                      # F = I + grad u: the adjoint is that of its linear part
                S = rng.normal(size=e.shape)
                out = _zeros(nn * bs)
                torch = _sync(ctx)
                dm.facet_adjoint(kind, bs, _cuda(S).data_ptr(), fs, out.data_ptr())
                torch.cuda.synchronize()
                lhs = float(u @ out.cpu().numpy())
                rhs = float(np.einsum("eq,eqk,eqk->", dS, S, e))
                assert abs(lhs - rhs) <= 1e-12 * np.einsum("eq,eqk,eqk->", dS, np.abs(S), np.abs(e)), (kind, bs, lhs, rhs)
    finally:
        dm.close()


def test_resultant_on_the_inner_arc(ctx):
    """sum over nodes of the pressure vector = scale * int n ds = -scale * R_i per component on the polygonal inner arc (the outward
    normal of the solid points towards the axis there); facet_adjoint(VALUE, 2, S = p n) agrees with facet_pressure to rounding."""
    R_i, scale = 1.0, 3.25
    m, tags = quarter_annulus(4, 16, R_i=R_i)
    nn = m.node_x.shape[0]
    dm = _mesh(ctx, m)
    try:
        fs = dm.facet_set(tags["inner"])
        f = _pressure(ctx, dm, fs, nn * 2, scale=scale).cpu().numpy().reshape(nn, 2)
        assert np.allclose(f.sum(axis=0), [-scale * R_i, -scale * R_i], rtol=1e-13)
        rng = np.random.Generator(np.random.PCG64(2))
        n, dS = facet_geometry_ref(m, tags["inner"])
        p = rng.uniform(0.5, 1.5, size=dS.shape)
        fp = _pressure(ctx, dm, fs, nn * 2, p=_cuda(p), scale=scale).cpu().numpy()
        out = _zeros(nn * 2)
        torch = _sync(ctx)
        dm.facet_adjoint("value", 2, _cuda(scale * p[..., None] * n).data_ptr(), fs, out.data_ptr())
        torch.cuda.synchronize()
        assert np.abs(out.cpu().numpy() - fp).max() <= 1e-14 * np.abs(fp).max()
    finally:
        dm.close()


def test_reproducible_capturable_and_always_accumulating(ctx):
    import torch

    m = structured_mesh("hexahedron", (6, 5, 4), 2, distort=0.1, seed=2)
    nn = m.node_x.shape[0]
    dm = _mesh(ctx, m)
    try:
        fs = dm.facet_set(exterior_facets(m))
        p = _cuda(np.random.Generator(np.random.PCG64(4)).normal(size=fs.n * 4))
        a = _pressure(ctx, dm, fs, nn * 3, p=p, scale=2.0)
        b = _pressure(ctx, dm, fs, nn * 3, p=p, scale=2.0)
        assert torch.equal(a, b)
        # consumer_overwrite does not apply: the call adds on top of what out holds
        base = _cuda(np.arange(nn * 3, dtype=np.float64))
        ctx.set_option("consumer_overwrite", 1)
        try:
            c = _pressure(ctx, dm, fs, nn * 3, p=p, scale=2.0, out=base.clone())
        finally:
            ctx.set_option("consumer_overwrite", 0)
        assert torch.equal(c, base + a)
        # graph capture after set creation replays bitwise equal
        out = _zeros(nn * 3)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ctx.set_stream(side.cuda_stream)
            dm.facet_pressure(fs, out.data_ptr(), p.data_ptr(), 2.0)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            out.zero_()
            dm.facet_pressure(fs, out.data_ptr(), p.data_ptr(), 2.0)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a)
    finally:
        dm.close()


def test_errors(ctx):
    from dolfinx_external_operator_amd import DeviceMesh
    from dolfinx_external_operator_amd.operand_eval import KINDS as KIND_ID

    m = structured_mesh("triangle", (3, 3), 2)
    other = structured_mesh("triangle", (3, 3), 2)
    nn = m.node_x.shape[0]
    ents = exterior_facets(m)
    out, S = _zeros(nn * 2), _zeros(len(ents) * 2 * 4)
    dm = _mesh(ctx, m, geometry=False)
    dm2 = _mesh(ctx, other)
    try:
        fs = dm.facet_set(ents)
        with pytest.raises(ValueError, match="DXO_E_OPTION"):            # geometry not set
            dm.facet_pressure(fs, out.data_ptr())
        w, nref, jref = facet_geometry("triangle")
        with pytest.raises(ValueError, match="DXO_E_DIM"):               # nq differs from the tables'
            dm.set_facet_geometry(np.append(w, 0.5), nref, jref)
        with pytest.raises(ValueError, match="DXO_E_DIM"):               # nf differs
            dm.set_facet_geometry(w, nref[:2], jref[:2])
        dm.set_facet_geometry(w, nref, jref)
        with pytest.raises(ValueError, match="DXO_E_DIM"):               # a set of another mesh
            dm2.facet_pressure(fs, out.data_ptr())
        bad = ents.copy()
        bad[0, 1] = 3
        with pytest.raises(ValueError, match="DXO_E_SIZE"):
            dm.facet_set(bad)
        bad = ents.copy()
        bad[-1, 0] = m.num_cells
        with pytest.raises(ValueError, match="DXO_E_SIZE"):
            dm.facet_set(bad)
        lib = ctx.lib
        for kind in ("C", "I1", "detF"):
            with pytest.raises(ValueError, match="facet_adjoint"):       # refused in Python
                dm.facet_adjoint(kind, 2, S.data_ptr(), fs, out.data_ptr())
            rc = lib.dxo_facet_adjoint(ctx._h, dm._h, fs._h, KIND_ID[kind], 2, C.c_void_p(S.data_ptr()), C.c_void_p(out.data_ptr()))
            assert rc == -6                                              # DXO_E_OPTION in the library
        rc = lib.dxo_facet_pressure(ctx._h, dm._h, fs._h, None, 1.0, None)
        assert rc == -1
        rc = lib.dxo_facet_pressure(ctx._h, dm._h, fs._h, None, 1.0, C.c_void_p(out.data_ptr() + 4))
        assert rc == -5
        bare = DeviceMesh.from_synthetic(m, ctx=ctx)
        try:
            with pytest.raises(ValueError, match="DXO_E_OPTION"):        # no facet tables
                bare.facet_set(ents)
        finally:
            bare.close()
    finally:
        dm.close()
        dm2.close()


def test_example_cylinder(ctx):
    """The demo's cylinder on an 8 x 32 P2 mesh: elastic first step against Lame, converged Newton everywhere, monotone response,
    plastic at the end."""
    import pathlib
    import sys

    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1] / "examples"))
    from device_cylinder_plasticity import lame_inner_displacement, main

    rep = main(n_r=8, n_theta=32, verbose=False)
    steps = rep["steps"]
    assert len(steps) == 20 and steps[0]["load"] == 0.0
    first = steps[1]
    assert first["plastic_fraction"] == 0.0 and first["max_dp"] == 0.0
    lame = lame_inner_displacement(first["load"])
    assert abs(first["u_x"] - lame) <= 0.01 * abs(lame), (first["u_x"], lame)
    for s in steps:
        assert s["relative_residual"] < 1e-8, s
    ux = [s["u_x"] for s in steps]
    assert all(b > a for a, b in zip(ux, ux[1:])), ux
    assert steps[-1]["plastic_fraction"] > 0.0
