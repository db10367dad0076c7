"""The dispatch from (gdim, block size, operand kind) to a kernel, walked in full: every (bs, kind) with bs in {1, gdim, 4} and the nine
kinds, on P1 triangles (2 x 2 unit square, 3-point rule) and P1 tetrahedra (the unit cube, 4-point rule). Where
dxo_operand_value_size admits the triple, dxo_eval_operand and dxo_eval_operand_facets agree with the NumPy oracle (tolerance of
tests/test_operand_eval.py), and for the linear kinds at bs in {1, gdim} dxo_operand_adjoint and dxo_facet_adjoint satisfy
<S, B u>_w = <B^T S, u> against the evaluated operand (tolerance of tests/test_adjoint_gpu.py). Where it refuses the triple, the four
entry points answer with their codes. The other parity tests sample this table; a wrong template argument in it would hide between
their samples."""
import ctypes as C

import numpy as np
import pytest

from oracle.operand_oracle import _geometry, eval_operand, eval_operand_facets
from tools.synthetic import exterior_facets, facet_geometry, facet_tables, structured_mesh

E_DIM, E_OPTION, MEM_HOST = -2, -6, 0
KINDS = {"value": 0, "grad": 1, "eps": 2, "F": 3, "value_grad": 4, "C": 5, "I1": 6, "detF": 7, "div": 8}      # include/dxo.h
PER_COMPONENT, NONLINEAR = ("value", "grad", "value_grad"), ("C", "I1", "detF")
MESHES = {2: ("triangle", (2, 2)), 3: ("tetrahedron", (1, 1, 1))}


def value_size(gdim, bs, kind):
    """include/dxo.h: value / grad / value_grad take any block size, the kinds of a displacement gradient bs = gdim alone."""
    if kind in PER_COMPONENT:
        return {"value": bs, "grad": bs * gdim, "value_grad": bs * (1 + gdim)}[kind]
    if bs != gdim:
        return E_DIM
    return {"eps": 2 * gdim if gdim == 2 else 6, "F": gdim * gdim, "C": gdim * gdim, "I1": 1, "detF": 1, "div": 1}[kind]


def adjoint_code(gdim, bs, kind):
    """dxo_operand_adjoint / dxo_facet_adjoint: the nonlinear kinds first (DXO_E_OPTION), then the triple, then bs = 1 or gdim."""
    if kind in NONLINEAR:
        return E_OPTION
    return E_DIM if value_size(gdim, bs, kind) < 0 or bs not in (1, gdim) else 0


def walk(gdim):
    return [(bs, kind) for bs in (1, gdim, 4) for kind in KINDS]


@pytest.fixture(scope="module", params=[2, 3], ids=["triangles", "tetrahedra"])
def setting(request):
    """Mesh, tables, facets, one field per block size and the oracle's operands: computed once, read by both tests."""
    gdim = request.param
    cell, n = MESHES[gdim]
    m = structured_mesh(cell, n, 1)
    tabs = facet_tables(m)[:3]
    ents = np.ascontiguousarray(exterior_facets(m), dtype=np.int32)
    rng = np.random.Generator(np.random.PCG64(40 + gdim))
    u = {bs: rng.normal(size=m.node_x.shape[0] * bs) for bs in (1, gdim, 4)}
    ref, ref_f = {}, {}
    for bs, kind in walk(gdim):
        if value_size(gdim, bs, kind) >= 0:
            ref[bs, kind] = eval_operand(KINDS[kind], bs, u[bs], m.dofmap, m.geom_dofmap, m.x, m.phi, m.dphi, m.dpsi)
            ref_f[bs, kind] = eval_operand_facets(KINDS[kind], bs, u[bs], m.dofmap, m.geom_dofmap, m.x, *tabs, ents)
    for a in list(ref.values()) + list(ref_f.values()) + list(u.values()):
        a.setflags(write=False)
    return gdim, m, tabs, ents, u, ref, ref_f


def test_the_walk_leaves_out_no_triple(setting):
    """The oracle alone: 27 triples per gdim, 15 admitted (3 per-component kinds at three block sizes, the six others at bs = gdim),
    each with an operand of the admitted value size on the cells and on the facets; the oracle refuses the 12 others too."""
    gdim, m, tabs, ents, u, ref, ref_f = setting
    assert m.nq == gdim + 1 and m.dofmap.shape[1] == gdim + 1 and len(ents) > 0
    cases = walk(gdim)
    assert len(cases) == len(set(cases)) == 27
    admitted = [c for c in cases if value_size(gdim, *c) >= 0]
    assert len(admitted) == 15 and set(ref) == set(ref_f) == set(admitted)
    for bs, kind in cases:
        D = value_size(gdim, bs, kind)
        if D >= 0:
            assert ref[bs, kind].shape == (m.num_cells, m.nq, D) and ref_f[bs, kind].shape == (len(ents), tabs[0].shape[1], D)
            assert np.abs(ref[bs, kind]).max() > 0 and np.abs(ref_f[bs, kind]).max() > 0
        else:
            with pytest.raises(ValueError):
                eval_operand(KINDS[kind], bs, u[bs], m.dofmap, m.geom_dofmap, m.x, m.phi, m.dphi, m.dpsi)
    adjoints = [c for c in cases if adjoint_code(gdim, *c) == 0]
    assert len(adjoints) == 9 and all(bs in (1, gdim) and kind not in NONLINEAR for bs, kind in adjoints)


@pytest.mark.gpu
def test_every_block_size_and_kind(ctx, setting):
    import torch

    from dolfinx_external_operator_amd import DeviceMesh

    gdim, m, tabs, ents, u, ref, ref_f = setting
    nn, lib = m.node_x.shape[0], ctx.lib
    rng = np.random.Generator(np.random.PCG64(7))
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    try:
        dm.set_facet_tables(*tabs)
        dm.set_facet_geometry(*facet_geometry(m.cell))
        fs = dm.facet_set(ents)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        dS = torch.zeros(len(ents) * tabs[0].shape[1], dtype=torch.float64, device="cuda")
        dm.facet_geometry(fs, None, dS.data_ptr())
        torch.cuda.synchronize()
        dS = dS.cpu().numpy().reshape(len(ents), -1)
        _, det = _geometry(m.dofmap, m.geom_dofmap, m.x, m.dphi, m.dpsi, np.arange(m.num_cells))
        wdet = m.weights[None, :] * np.abs(det)
        dummy = torch.zeros(64, dtype=torch.float64, device="cuda")
        host = np.zeros(64)

        def eval_codes(bs, kind):
            """dxo_eval_operand and dxo_eval_operand_facets past the Python checks, for a triple they refuse: their return codes"""
            return (lib.dxo_eval_operand(ctx._h, dm._h, KINDS[kind], bs, MEM_HOST, host.ctypes.data, None, m.num_cells, host.ctypes.data),
                    lib.dxo_eval_operand_facets(ctx._h, dm._h, KINDS[kind], bs, MEM_HOST, host.ctypes.data, ents.ctypes.data, len(ents),
                                                host.ctypes.data))

        def adjoint_codes(bs, kind):
            """the same for dxo_operand_adjoint and dxo_facet_adjoint"""
            d = C.c_void_p(dummy.data_ptr())
            return (lib.dxo_operand_adjoint(ctx._h, dm._h, KINDS[kind], bs, d, None, m.num_cells, d),
                    lib.dxo_facet_adjoint(ctx._h, dm._h, fs._h, KINDS[kind], bs, d, d))

        for bs, kind in walk(gdim):
            D, adj = value_size(gdim, bs, kind), adjoint_code(gdim, bs, kind)
            assert lib.dxo_operand_value_size(gdim, bs, KINDS[kind]) == D, (bs, kind)
            if D < 0:
                assert eval_codes(bs, kind) == (D, D) and adjoint_codes(bs, kind) == (adj, adj), (bs, kind)
                continue
            e, ef = dm.evaluate(kind, bs, u[bs]), dm.evaluate_facets(kind, bs, u[bs], ents)
            for name, got, want in (("cells", e, ref[bs, kind]), ("facets", ef, ref_f[bs, kind])):
                err = np.abs(got - want).max() / np.abs(want).max()
                print(f"gdim {gdim} bs {bs} {kind:10s} {name:6s} rel err {err:.2e}")
                assert got.shape == want.shape and err <= 1e-13, (bs, kind, name)
            if adj != 0:
                assert adjoint_codes(bs, kind) == (adj, adj), (bs, kind)
                continue
            if kind == "F":      # F = I + grad u: the adjoint is that of its linear part
                e, ef = e - np.eye(gdim).reshape(-1), ef - np.eye(gdim).reshape(-1)
            for name, Bu, w, call in (("cells", e, wdet, lambda S, out: dm.adjoint(kind, bs, S.data_ptr(), out.data_ptr())),
                                      ("facets", ef, dS, lambda S, out: dm.facet_adjoint(kind, bs, S.data_ptr(), fs, out.data_ptr()))):
                S = rng.normal(size=Bu.shape)
                St = torch.from_numpy(np.ascontiguousarray(S).reshape(-1)).cuda()
                out = torch.zeros(nn * bs, dtype=torch.float64, device="cuda")
                call(St, out)
                torch.cuda.synchronize()
                lhs, rhs = np.sum(w[:, :, None] * Bu * S), u[bs] @ out.cpu().numpy()      # <B u, S>_w  vs  <u, B^T S>
                print(f"gdim {gdim} bs {bs} {kind:10s} {name:6s} adjoint identity {abs(lhs - rhs):.2e} of {max(abs(lhs), np.abs(w).sum()):.2e}")
                assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), np.abs(w).sum()), (bs, kind, name, lhs, rhs)
    finally:
        dm.close()
