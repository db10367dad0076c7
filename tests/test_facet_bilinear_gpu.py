"""dxo_facet_bilinear_apply / _diagonal / _assemble on the device: against the NumPy dense oracle of tests/facet_bilinear_cases.py,
against each other and the three-call composition they replace, over more than one workgroup, accumulation, reproducibility and
chunking, on top of a cell matrix with Dirichlet rows, under graph capture, every refusal, and examples/device_robin_heat.py.

Tolerances are those of tests/test_assemble_gpu.py and tests/test_bilinear_gpu.py: 1e-12 of the largest reference entry against
the NumPy oracle, 1e-13 of the largest entry between two device paths."""
import ctypes as C
import functools
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

from facet_bilinear_cases import (CELLS, DEGREES, cached_dense_ref, entity_list, facet_bilinear_dense_ref, mesh_case, random_block,
                                  trial_cases, value_size)
from oracle.form_oracle import apply_bcs, csr_to_dense, dense_ref
from tools.synthetic import exterior_facets, facet_geometry, facet_tables, structured_mesh

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _cuda(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).cuda()      # a copy: the cached references are read-only


def _zeros(n):
    import torch

    return torch.zeros(n, dtype=torch.float64, device="cuda")


def _mesh(ctx, m):
    from dolfinx_external_operator_amd import DeviceMesh

    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    dm.set_facet_tables(*facet_tables(m)[:3])
    dm.set_facet_geometry(*facet_geometry(m.cell))
    return dm


def _sync(ctx):
    import torch

    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    return torch


def _apply(ctx, dm, fs, trial, bs, Cd, vd, out=None):
    torch = _sync(ctx)
    out = _zeros(vd.numel()) if out is None else out
    dm.facet_bilinear_apply(trial, bs, Cd.data_ptr(), vd.data_ptr(), fs, out.data_ptr())
    torch.cuda.synchronize()
    return out


def _diagonal(ctx, dm, fs, trial, bs, Cd, n, out=None):
    torch = _sync(ctx)
    out = _zeros(n) if out is None else out
    dm.facet_bilinear_diagonal(trial, bs, Cd.data_ptr(), fs, out.data_ptr())
    torch.cuda.synchronize()
    return out


def _assemble(ctx, dm, fs, trial, bs, Cd, **kw):
    torch = _sync(ctx)
    A = dm.facet_bilinear_assemble(trial, bs, Cd.data_ptr(), fs, dm.csr_pattern(bs), **kw)
    torch.cuda.synchronize()
    return A


def _dense(A):
    indptr, indices, values = A.to_numpy()
    return csr_to_dense(indptr, indices, values, A.shape[0])


def _csr_diagonal(A):
    indptr, indices, values = A.to_numpy()
    rows = np.repeat(np.arange(A.shape[0]), np.diff(indptr))
    d = np.zeros(A.shape[0])
    d[rows[indices == rows]] = values[indices == rows]
    return d


# ---- 1. the dense oracle
@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("which", ["subset", "all"])
def test_apply_diagonal_and_matrix_match_the_dense_oracle(ctx, cell, degree, which):
    m = mesh_case(cell, degree)
    rng = np.random.Generator(np.random.PCG64(41))
    dm = _mesh(ctx, m)
    try:
        fs = dm.facet_set(entity_list(m, which))
        for trial, bs in trial_cases(m.gdim):
            _, ents, Cb, K = cached_dense_ref(cell, degree, which, trial, bs)
            assert fs.n == len(ents) and np.abs(K).max() > 0
            Cd, v = _cuda(Cb), rng.normal(size=K.shape[0])
            Kv = _apply(ctx, dm, fs, trial, bs, Cd, _cuda(v)).cpu().numpy()
            dg = _diagonal(ctx, dm, fs, trial, bs, Cd, K.shape[0]).cpu().numpy()
            A = _dense(_assemble(ctx, dm, fs, trial, bs, Cd))
            ref_v, ref_d = K @ v, np.diag(K)
            errs = (np.abs(Kv - ref_v).max() / np.abs(ref_v).max(), np.abs(dg - ref_d).max() / np.abs(ref_d).max(),
                    np.abs(A - K).max() / np.abs(K).max())
            print(f"{cell} P{degree} {which} ({trial}, {bs}): apply {errs[0]:.1e} diagonal {errs[1]:.1e} matrix {errs[2]:.1e}")
            assert errs[0] <= 1e-12 and errs[1] <= 1e-12 and errs[2] <= 1e-12, (trial, bs, errs)
    finally:
        dm.close()


# ---- 2. consistency between the device paths
@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("degree", DEGREES)
def test_paths_agree_on_the_device(ctx, cell, degree):
    """CSR . v (DeviceCSR.matvec) = apply v; the CSR diagonal = diagonal; apply = evaluate_facets -> einsum with C ->
    facet_adjoint("value")."""
    import torch

    m = mesh_case(cell, degree)
    G, nn = m.gdim, m.node_x.shape[0]
    rng = np.random.Generator(np.random.PCG64(43))
    ents = entity_list(m, "all")
    dm = _mesh(ctx, m)
    try:
        fs = dm.facet_set(ents)
        ents_d = torch.from_numpy(fs.entities).cuda()
        nq = dm.nq_facet
        for trial, bs in trial_cases(G):
            D = value_size(trial, G, bs)
            Cd = _cuda(random_block(m, ents, trial, bs, seed=5))
            vd = _cuda(rng.normal(size=nn * bs))
            Kv = _apply(ctx, dm, fs, trial, bs, Cd, vd)
            scale = float(Kv.abs().max())
            A = _assemble(ctx, dm, fs, trial, bs, Cd)
            Av = A.matvec(vd)
            torch.cuda.synchronize()
            assert float((Av - Kv).abs().max()) <= 1e-13 * scale, (trial, bs)
            dg = _diagonal(ctx, dm, fs, trial, bs, Cd, nn * bs).cpu().numpy()
            assert np.abs(_csr_diagonal(A) - dg).max() <= 1e-13 * np.abs(dg).max(), (trial, bs)
            # the composition the call replaces
            _sync(ctx)
            e = dm.evaluate_facets_device(trial, bs, vd, ents_d)
            assert e.shape == (fs.n, nq, D)
            if trial == "F":
                e = e - torch.eye(G, dtype=torch.float64, device="cuda").reshape(-1)
            S = torch.einsum("eqir,eqr->eqi", Cd.reshape(fs.n, nq, bs, D), e).contiguous()
            three = _zeros(nn * bs)
            dm.facet_adjoint("value", bs, S.data_ptr(), fs, three.data_ptr())
            torch.cuda.synchronize()
            assert float((three - Kv).abs().max()) <= 1e-13 * scale, (trial, bs)
    finally:
        dm.close()


# ---- 3. more than one workgroup
@pytest.mark.parametrize("degree", DEGREES)
def test_more_entities_than_one_workgroup_round(ctx, degree):
    """Triangles (40, 30): 140 boundary edges at 2 points each. A round of the vector kernels and of the assembly's element kernel
    takes 128 entities (the parked blocks are 26 doubles per entity at most): two workgroups, the second with 12 entities. Degree 1
    against the dense oracle; degree 2, whose dense matrix would take 0.8 GB, against the oracle's action and between the paths."""
    import torch

    from facet_bilinear_cases import facet_bilinear_apply_ref

    m = mesh_case("triangle", degree, n=(40, 30))
    ents = exterior_facets(m)
    assert len(ents) == 140 and facet_tables(m)[0].shape[1] == 2
    rng = np.random.Generator(np.random.PCG64(47))
    nn = m.node_x.shape[0]
    dm = _mesh(ctx, m)
    try:
        fs = dm.facet_set(ents)
        for trial, bs in (("value_grad", 2), ("grad", 1)):
            Cb = random_block(m, ents, trial, bs, seed=7)
            Cd, v = _cuda(Cb), rng.normal(size=nn * bs)
            vd = _cuda(v)
            Kv = _apply(ctx, dm, fs, trial, bs, Cd, vd)
            ref_v = facet_bilinear_apply_ref(m, ents, trial, bs, Cb, v)
            assert np.abs(Kv.cpu().numpy() - ref_v).max() <= 1e-12 * np.abs(ref_v).max()
            dg = _diagonal(ctx, dm, fs, trial, bs, Cd, nn * bs).cpu().numpy()
            A = _assemble(ctx, dm, fs, trial, bs, Cd)
            Av = A.matvec(vd)
            torch.cuda.synchronize()
            assert float((Av - Kv).abs().max()) <= 1e-13 * float(Kv.abs().max())
            assert np.abs(_csr_diagonal(A) - dg).max() <= 1e-13 * np.abs(dg).max()
            if degree == 1:
                K = facet_bilinear_dense_ref(m, ents, trial, bs, Cb)
                assert np.abs(dg - np.diag(K)).max() <= 1e-12 * np.abs(np.diag(K)).max()
                indptr, indices, values = A.to_numpy()
                rows = np.repeat(np.arange(K.shape[0]), np.diff(indptr))
                inside = np.zeros(K.shape, dtype=bool)
                inside[rows, indices] = True
                assert np.abs(K[~inside]).max() == 0.0
                assert np.abs(values - K[rows, indices]).max() <= 1e-12 * np.abs(K).max()
    finally:
        dm.close()


# ---- 4. accumulation and reproducibility
def test_accumulates_reproduces_and_ignores_the_chunk_size(ctx):
    import torch

    m = mesh_case("hexahedron", 2)
    G, nn = 3, m.node_x.shape[0]
    ents = entity_list(m, "all")
    rng = np.random.Generator(np.random.PCG64(53))
    dm = _mesh(ctx, m)
    try:
        fs = dm.facet_set(ents)
        Cd = _cuda(random_block(m, ents, "value_grad", G, seed=9))
        vd = _cuda(rng.normal(size=nn * G))
        a = _apply(ctx, dm, fs, "value_grad", G, Cd, vd)
        assert torch.equal(a, _apply(ctx, dm, fs, "value_grad", G, Cd, vd))                  # repeated calls are bitwise equal
        twice = _apply(ctx, dm, fs, "value_grad", G, Cd, vd, out=a.clone())                  # x + x is exact: bitwise twice one call
        assert torch.equal(twice, 2 * a) and float(a.abs().max()) > 0
        d = _diagonal(ctx, dm, fs, "value_grad", G, Cd, nn * G)
        assert torch.equal(d, _diagonal(ctx, dm, fs, "value_grad", G, Cd, nn * G))
        assert torch.equal(_diagonal(ctx, dm, fs, "value_grad", G, Cd, nn * G, out=d.clone()), 2 * d)
        # consumer_overwrite does not apply: the call adds on top of what out holds
        A = _assemble(ctx, dm, fs, "value_grad", G, Cd).values
        assert torch.equal(A, _assemble(ctx, dm, fs, "value_grad", G, Cd).values)
        base = _cuda(np.arange(nn * G, dtype=np.float64))
        ctx.set_option("consumer_overwrite", 1)
        try:
            on_top = _apply(ctx, dm, fs, "value_grad", G, Cd, vd, out=base.clone())
            # the entries join the chains already in `values` one entity at a time: twice one call to rounding, not bitwise
            acc = _assemble(ctx, dm, fs, "value_grad", G, Cd, values=A.clone()).values
        finally:
            ctx.set_option("consumer_overwrite", 0)
        assert torch.equal(on_top, base + a)
        assert float((acc - 2 * A).abs().max()) <= 1e-14 * float(A.abs().max())
        assert float((acc - A).abs().max()) > 0.5 * float(A.abs().max())
        for chunk in (1, 3, 0):
            ctx.set_option("assemble_chunk_cells", chunk)
            try:
                c = _assemble(ctx, dm, fs, "value_grad", G, Cd).values
            finally:
                ctx.set_option("assemble_chunk_cells", 0)
            assert torch.equal(A, c), chunk
    finally:
        dm.close()


# ---- 5. a cell matrix plus the facet matrix, then the Dirichlet rows
@pytest.mark.parametrize("cell,cell_pair,trial,bs_is_g", [("triangle", ("grad", "value_grad"), "value", False),
                                                          ("hexahedron", ("eps", "eps"), "value_grad", True)])
@pytest.mark.parametrize("diagonal", [1.0, 3.25])
def test_facet_term_on_top_of_a_cell_matrix_with_bcs(ctx, cell, cell_pair, trial, bs_is_g, diagonal):
    import torch

    m = mesh_case(cell, 2)
    G, nn = m.gdim, m.node_x.shape[0]
    bs = G if bs_is_g else 1
    rng = np.random.Generator(np.random.PCG64(59))
    ents = exterior_facets(m, where=lambda X: np.all(X[..., 0] == 1.0, axis=1))
    assert len(ents) > 0
    cell_sizes = {"grad": bs * G, "value_grad": bs * (1 + G), "eps": 4 if G == 2 else 6}
    Cc = rng.normal(size=(m.num_cells * m.nq, cell_sizes[cell_pair[0]], cell_sizes[cell_pair[1]]))
    Cf = random_block(m, ents, trial, bs, seed=13)
    left = np.flatnonzero(np.isclose(m.node_x[:, 0], 0.0))
    dofs = (left[:, None] * bs + np.arange(bs)).reshape(-1).astype(np.int32)
    dm = _mesh(ctx, m)
    try:
        _sync(ctx)
        pat = dm.csr_pattern(bs)
        Ccd, Cfd = _cuda(Cc), _cuda(Cf)              # kept alive: the calls take raw pointers
        A = dm.bilinear_assemble(*cell_pair, bs, Ccd.data_ptr(), pat)
        B = dm.facet_bilinear_assemble(trial, bs, Cfd.data_ptr(), dm.facet_set(ents), pat, values=A.values,
                                       bcs=torch.from_numpy(dofs).cuda(), diagonal=diagonal)
        torch.cuda.synchronize()
        assert B.values is A.values
        ref = apply_bcs(dense_ref(m, *cell_pair, bs, Cc) + facet_bilinear_dense_ref(m, ents, trial, bs, Cf), dofs, diagonal)
        got = _dense(B)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
        assert np.all(got[dofs, dofs] == diagonal)
    finally:
        dm.close()


# ---- 6. graph capture
def test_graph_capture_replays_bitwise(ctx):
    import torch

    m = mesh_case("quadrilateral", 2, n=(10, 9))
    G, nn = 2, m.node_x.shape[0]
    ents = exterior_facets(m)
    rng = np.random.Generator(np.random.PCG64(61))
    dm = _mesh(ctx, m)
    try:
        fs, pat = dm.facet_set(ents), dm.csr_pattern(G)
        Cd, vd = _cuda(random_block(m, ents, "eps", G, seed=15)), _cuda(rng.normal(size=nn * G))
        # the warm-up call: the assembly's scratch is allocated here
        eager_v = _apply(ctx, dm, fs, "eps", G, Cd, vd).clone()
        eager_d = _diagonal(ctx, dm, fs, "eps", G, Cd, nn * G).clone()
        eager_a = _assemble(ctx, dm, fs, "eps", G, Cd).values.clone()
        out_v, out_d, values = _zeros(nn * G), _zeros(nn * G), _zeros(pat.nnz)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            out_v.zero_()
            out_d.zero_()
            values.zero_()
            dm.facet_bilinear_apply("eps", G, Cd.data_ptr(), vd.data_ptr(), fs, out_v.data_ptr())
            dm.facet_bilinear_diagonal("eps", G, Cd.data_ptr(), fs, out_d.data_ptr())
            dm.facet_bilinear_assemble("eps", G, Cd.data_ptr(), fs, pat, values=values)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        for t in (out_v, out_d, values):
            t.fill_(7.0)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        free0 = torch.cuda.mem_get_info()[0]
        g.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20)
        assert torch.equal(out_v, eager_v) and torch.equal(out_d, eager_d) and torch.equal(values, eager_a)
    finally:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        dm.close()


# ---- 7. error paths (argument checks only)
def test_error_paths(ctx):
    import torch

    from dolfinx_external_operator_amd import DeviceMesh
    from dolfinx_external_operator_amd.operand_eval import KINDS as KIND_ID

    m = structured_mesh("triangle", (3, 3), 2)
    other = structured_mesh("triangle", (3, 3), 2)
    nn = m.node_x.shape[0]
    ents = exterior_facets(m)
    lib, P = ctx.lib, C.c_void_p
    V, GRAD = KIND_ID["value"], KIND_ID["grad"]
    dm, dm2 = _mesh(ctx, m), _mesh(ctx, other)
    bare = DeviceMesh.from_synthetic(m, ctx=ctx)
    bare.set_facet_tables(*facet_tables(m)[:3])
    plain = DeviceMesh.from_synthetic(m, ctx=ctx)          # no facet tables
    try:
        fs, empty = dm.facet_set(ents), dm.facet_set(np.zeros((0, 2), dtype=np.int32))
        pat1, pat2, pat_other = dm.csr_pattern(1), dm.csr_pattern(2), dm2.csr_pattern(2)
        Cd, v, out = _zeros(len(ents) * 2 * 2 * 6), _zeros(nn * 2), _zeros(nn * 2)
        vals = _zeros(pat2.nnz)
        c, vp, op, vl = P(Cd.data_ptr()), P(v.data_ptr()), P(out.data_ptr()), P(vals.data_ptr())

        def calls(mesh, fset, test, trial, bs, c=c, vp=vp, op=op, vl=vl, pat=None):
            pat = (pat1 if bs == 1 else pat2) if pat is None else pat
            return (lib.dxo_facet_bilinear_apply(ctx._h, mesh, fset, test, trial, bs, c, vp, op),
                    lib.dxo_facet_bilinear_diagonal(ctx._h, mesh, fset, test, trial, bs, c, op),
                    lib.dxo_facet_bilinear_assemble(ctx._h, mesh, fset, pat._h, test, trial, bs, c, vl))

        assert calls(dm._h, fs._h, V, GRAD, 2) == (0, 0, 0)
        # from here on every call is refused (or sees the empty set): with C = v = 1 an accepted one would change the sentinels
        Cd.fill_(1.0)
        v.fill_(1.0)
        out.fill_(3.0)
        vals.fill_(5.0)
        # the test kind must be VALUE
        for test in ("grad", "value_grad", "eps"):
            assert calls(dm._h, fs._h, KIND_ID[test], V, 2) == (-6, -6, -6)
            assert "dxo_facet_bilinear_assemble" in lib.dxo_last_error(ctx._h).decode()
            with pytest.raises(ValueError, match="test kind"):
                dm.facet_bilinear_apply("value", 2, Cd.data_ptr(), v.data_ptr(), fs, out.data_ptr(), test=test)
        # nonlinear and unknown trial kinds
        for trial in ("C", "I1", "detF"):
            assert calls(dm._h, fs._h, V, KIND_ID[trial], 2) == (-6, -6, -6)
            with pytest.raises(ValueError, match="facet_bilinear_diagonal"):
                dm.facet_bilinear_diagonal(trial, 2, Cd.data_ptr(), fs, out.data_ptr())
        assert calls(dm._h, fs._h, V, 99, 2) == (-6, -6, -6)
        # block sizes that do not fit
        for trial, bs in (("eps", 1), ("div", 1), ("F", 1), ("value", 3), ("grad", 0)):
            assert calls(dm._h, fs._h, V, KIND_ID[trial], bs) == (-2, -2, -2), (trial, bs)
            with pytest.raises(ValueError, match="facet_bilinear_assemble"):
                dm.facet_bilinear_assemble(trial, bs, Cd.data_ptr(), fs, pat2)
        # a pattern of another block size or mesh
        assert lib.dxo_facet_bilinear_assemble(ctx._h, dm._h, fs._h, pat1._h, V, GRAD, 2, c, vl) == -2
        assert lib.dxo_facet_bilinear_assemble(ctx._h, dm._h, fs._h, pat_other._h, V, GRAD, 2, c, vl) == -2
        # a set of another mesh; geometry not set
        assert calls(dm2._h, fs._h, V, GRAD, 2, pat=pat_other) == (-2, -2, -2)
        assert calls(bare._h, bare.facet_set(ents)._h, V, GRAD, 2, pat=bare.csr_pattern(2)) == (-6, -6, -6)
        # an empty set touches nothing, also with NULL arrays
        assert calls(dm._h, empty._h, V, GRAD, 2, c=None, vp=None, op=None, vl=None) == (0, 0, 0)
        # NULL
        assert calls(None, fs._h, V, GRAD, 2) == (-1, -1, -1) and calls(dm._h, None, V, GRAD, 2) == (-1, -1, -1)
        assert calls(dm._h, fs._h, V, GRAD, 2, c=None) == (-1, -1, -1)
        assert calls(dm._h, fs._h, V, GRAD, 2, op=None, vl=None) == (-1, -1, -1)
        assert lib.dxo_facet_bilinear_apply(ctx._h, dm._h, fs._h, V, GRAD, 2, c, None, op) == -1
        assert lib.dxo_facet_bilinear_assemble(ctx._h, dm._h, fs._h, None, V, GRAD, 2, c, vl) == -1
        assert lib.dxo_facet_bilinear_apply(None, dm._h, fs._h, V, GRAD, 2, c, vp, op) == -1
        assert lib.dxo_facet_bilinear_diagonal(None, dm._h, fs._h, V, GRAD, 2, c, op) == -1
        assert lib.dxo_facet_bilinear_assemble(None, dm._h, fs._h, pat2._h, V, GRAD, 2, c, vl) == -1
        # misaligned
        assert calls(dm._h, fs._h, V, GRAD, 2, c=P(Cd.data_ptr() + 4)) == (-5, -5, -5)
        assert calls(dm._h, fs._h, V, GRAD, 2, op=P(out.data_ptr() + 4), vl=P(vals.data_ptr() + 4)) == (-5, -5, -5)
        assert lib.dxo_facet_bilinear_apply(ctx._h, dm._h, fs._h, V, GRAD, 2, c, P(v.data_ptr() + 4), op) == -5
        with pytest.raises(ValueError, match="values must be"):
            dm.facet_bilinear_assemble("grad", 2, Cd.data_ptr(), fs, pat2, values=_zeros(3))
        # the refusals wrote nothing
        torch.cuda.synchronize()
        assert bool((out == 3.0).all()) and bool((vals == 5.0).all())
        # evaluate_facets_device checks its tensors before the library is called
        ents_d = torch.from_numpy(fs.entities).cuda()
        assert dm.evaluate_facets_device("value", 2, v, ents_d).shape == (fs.n, 2, 2)
        for bad_u in (v[:-1], v.float(), v.cpu(), v.data_ptr()):
            with pytest.raises(ValueError, match="evaluate_facets_device: u"):
                dm.evaluate_facets_device("value", 2, bad_u, ents_d)
        for bad_e in (ents_d.long(), ents_d.reshape(-1), ents_d.t(), fs.entities, ents_d.cpu()):
            with pytest.raises(ValueError, match="evaluate_facets_device: entities"):
                dm.evaluate_facets_device("value", 2, v, bad_e)
        with pytest.raises(ValueError, match="evaluate_facets_device: out"):
            dm.evaluate_facets_device("value", 2, v, ents_d, out=_zeros(fs.n * 2 * 2 + 1))
        with pytest.raises(ValueError, match="not defined"):
            dm.evaluate_facets_device("eps", 1, v, ents_d)
        with pytest.raises(ValueError, match="facet tables"):
            plain.evaluate_facets_device("value", 2, v, ents_d)
    finally:
        plain.close()
        bare.close()
        dm.close()
        dm2.close()


def test_a_facet_rule_too_large_for_the_lds_budget_is_refused(ctx):
    """dxo_facet_bilinear_assemble parks nq_facet blocks of 37 doubles per entity for (value_grad, bs = gdim = 3): with 224 facet
    points one entity exceeds 64 KiB and the call answers DXO_E_SIZE before anything is launched or allocated."""
    from dolfinx_external_operator_amd import DeviceMesh
    from dolfinx_external_operator_amd.operand_eval import KINDS as KIND_ID

    m = structured_mesh("tetrahedron", (1, 1, 1), 1)
    nq, nd, ng = 224, m.dofmap.shape[1], m.geom_dofmap.shape[1]
    rng = np.random.Generator(np.random.PCG64(67))
    w, nref, jref = facet_geometry("tetrahedron")
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    try:
        dm.set_facet_tables(rng.normal(size=(4, nq, nd)), rng.normal(size=(4, nq, nd, 3)), rng.normal(size=(4, nq, ng, 3)))
        dm.set_facet_geometry(np.full(nq, 0.5 / nq), nref, jref)
        fs, pat = dm.facet_set(exterior_facets(m)), dm.csr_pattern(3)
        Cd, vals = _zeros(fs.n * nq * 3 * 12), _zeros(pat.nnz)
        vals.fill_(5.0)
        P = C.c_void_p
        rc = ctx.lib.dxo_facet_bilinear_assemble(ctx._h, dm._h, fs._h, pat._h, KIND_ID["value"], KIND_ID["value_grad"], 3, P(Cd.data_ptr()),
                                                 P(vals.data_ptr()))
        assert rc == -3 and "LDS" in ctx.lib.dxo_last_error(ctx._h).decode()
        with pytest.raises(ValueError, match="DXO_E_SIZE"):
            dm.facet_bilinear_assemble("value_grad", 3, Cd.data_ptr(), fs, pat, values=vals)
        assert bool((vals == 5.0).all())
    finally:
        dm.close()


# ---- 8. the example, as a subprocess
@functools.lru_cache(maxsize=None)
def _example(*flags):
    res = subprocess.run([sys.executable, str(ROOT / "examples" / "device_robin_heat.py"), "8", *flags], capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_example_converges_and_the_matrix_free_path_follows_it():
    """|R| <= 1e-10 |R_0| with the full Jacobian, assembled or matrix-free, in the same number of iterations, and the two histories
    agree to 1e-8 of every entry, above the rounding floor of the residual evaluation. The floor: an entry of R sums at most 6 cells x
    3 points x 2 gradient components + 2 facets x 2 points = 40 products, each formed with about three roundings, so some 128 rounded
    operations on terms no larger than the entries of R_0 (the interior terms balance the boundary flux, which is what R_0 holds). One
    evaluation carries up to 128 u |R_0|, u = 1.1e-16, and the comparison sees two of them: 256 u |R_0| = 2.8e-14 |R_0|. A converged
    history ends below 1e-10 |R_0|, where that floor is 3e-4 of the entry or more: only there does it exceed the relative bound. (The linear
    solves, rtol 1e-12, move R_k+1 by at most 2e-12 |R_k|, which lies under one of the two terms at every entry of a quadratically
    converging history.)"""
    a, mf = _example(), _example("--matrix-free")
    ra, rm = np.array(a["newton_residuals"]), np.array(mf["newton_residuals"])
    assert a["converged"] and mf["converged"] and not a["matrix_free"] and mf["matrix_free"]
    assert ra[-1] <= 1e-10 * ra[0] and rm[-1] <= 1e-10 * rm[0]
    assert len(ra) == len(rm) and len(ra) <= 8
    bound = 1e-8 * ra + 256 * 0.5 * np.finfo(np.float64).eps * ra[0]
    for k, (x, y, b) in enumerate(zip(ra, rm, bound)):
        print(f"iteration {k}: assembled {x:.17e} matrix-free {y:.17e} |difference| {abs(x - y):.3e} bound {b:.3e}")
    assert np.all(np.abs(ra - rm) <= bound)
    assert abs(a["solution_norm"] - mf["solution_norm"]) <= 1e-8 * a["solution_norm"]
    assert a["T_min"] < 0.95 and a["T_max"] == pytest.approx(1.0)      # the boundary flux cooled the far side


def test_example_without_the_facet_jacobian_needs_more_newton_iterations():
    full, without = _example(), _example("--no-facet-jacobian")
    print("full", full["newton_residuals"], "without the facet term", without["newton_residuals"])
    assert full["facet_jacobian"] and not without["facet_jacobian"]
    assert without["newton_iterations"] > full["newton_iterations"]
