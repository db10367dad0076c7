"""The scalar functionals (csrc/functional.hip: dxo_eval_cell_measure, dxo_integrate, dxo_facet_integrate, dxo_operand_moments)
against the long-double reference of tests/functional_cases.py, output entry by output entry, on its meshes, lists and inputs.

Bound, for EVERY entry k: |got[k] - ref[k]| <= c * 2^-53 * mag[k], c = MARGIN * max(C_REF[entry], 1) (functional_cases.allowed);
entries with mag = 0 must be exact. c is not tuned on the kernels. In the same calls: `out` starts as NaN and comes back finite (the
calls SET it), a second call gives identical bits, the empty list gives exactly +0.0, `arange` gives the bits of NULL."""
import ctypes as C
import math

import numpy as np
import pytest

import facet_reference_cases as FC
import functional_cases as F
from functional_cases import allowed, worst_ratio
from test_functional_reference_cpu import divergence_case, quadratic_field

pytestmark = pytest.mark.gpu

EPS53 = F.LD(2.0) ** -53
E_NULL, E_DIM, E_ALIGN, E_OPTION = -1, -2, -5, -6
CROSS_LISTS = ("all", "shuffled", "repeated")       # the lists on which one call is also held against another


class Device:
    """One DeviceMesh (with the facet tables of `facet_case`, if given) and the four calls on host arrays."""

    def __init__(self, ctx, mesh, facet_case=None):
        import torch

        from dolfinx_external_operator_amd import DeviceMesh

        self.torch, self.ctx, self.m = torch, ctx, mesh
        self.dev = torch.device("cuda", ctx.device)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        self.dm = DeviceMesh.from_synthetic(mesh, ctx=ctx)
        if facet_case is not None:
            tabs, geom, _ = FC.rule_tables(facet_case)
            self.dm.set_facet_tables(*tabs)
            self.dm.set_facet_geometry(*geom)

    def close(self):
        self.dm.close()

    def cuda(self, a, dtype=np.float64):
        return None if a is None else self.torch.from_numpy(np.array(a, dtype=dtype)).to(self.dev)       # a copy: the case lists are read-only

    def nan(self, n):
        return self.torch.full((n,), float("nan"), dtype=self.torch.float64, device=self.dev)

    def twice(self, call, n_out):
        """call(out) on an `out` of NaN, twice: identical bits, finite -> the host array."""
        a, b = self.nan(n_out), self.nan(n_out)
        call(a)
        call(b)
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(a, b), "a second call gave other bits"
        assert np.all(np.isfinite(a)), "out was not set"
        return a

    def integrate(self, f, g, cells):
        fd, cd = self.cuda(f), self.cuda(cells, np.int32)
        gd = fd if g is f else self.cuda(g)
        return self.twice(lambda o: self.dm.integrate(fd, gd, cd, out=o), f.shape[-1] if g is None else 1)

    def facet_integrate(self, fs, f, g):
        fd = self.cuda(f)
        gd = fd if g is f else self.cuda(g)
        return self.twice(lambda o: self.dm.facet_integrate(fd, fs, gd, out=o), f.shape[-1] if g is None else 1)

    def moments(self, kind, bs, u, cells):
        ud, cd = self.cuda(u), self.cuda(cells, np.int32)
        return self.twice(lambda o: self.dm.operand_moments(kind, bs, ud, cd, out=o), self.dm.value_size(kind, bs) + 1)


def check(got, ref, mag, entry, where, worst):
    ratio = worst_ratio(got, ref, mag)
    if ratio > worst.get(entry, (-1.0, ""))[0]:
        worst[entry] = (ratio, where)
    assert ratio <= allowed(entry), f"{where}: {ratio:.2f} * 2^-53 * mag, allowed {allowed(entry):.1f}"


def plus_zero(a):
    return np.array_equal(a, np.zeros_like(a)) and not np.any(np.signbit(a))


def report(worst):
    for entry, (ratio, where) in sorted(worst.items()):
        print(f"{entry:18s} {ratio:8.2f}   (c = {allowed(entry):7.1f})   worst at {where}")


@pytest.mark.parametrize("case", F.CELL_CASES, ids=F.cell_case_id)
def test_cell_functionals_match_the_long_double_reference(ctx, case):
    """Every cell list of the case; on each the cell measure, the per-component integrals of every D, the pairing of every D (g drawn,
    g aliased to f), each in every input variant, and the moments of every kind with every block size for u and u + 10^6."""
    m = F.cell_mesh(case)
    d = Device(ctx, m)
    ic, worst, bits = F.CELL_CASES.index(case), {}, {}
    try:
        for il, (name, cells) in enumerate(F.cell_lists(case).items()):
            il = 0 if name == "arange" else il          # arange gets the inputs of NULL (list 0): the two must agree bit for bit
            where = f"{F.cell_case_id(case)}, {name}"
            n = m.num_cells if cells is None else len(cells)
            ld = F.ref_cell_measure(m, cells)
            dx = d.dm.cell_measure(d.cuda(cells, np.int32)).cpu().numpy()
            assert dx.shape == (n, m.nq)
            if n:
                check(dx, *ld, "measure", where, worst)
                total = np.sum(dx.astype(F.LD))          # integrate(ones) against the sum of the device's own measures, in long double
                one = d.integrate(np.ones((n, m.nq, 1)), None, cells)
                assert abs(F.LD(one[0]) - total) <= allowed("integrate") * EPS53 * total, where
            got_all = []
            for item in F.integrate_items(n, m.nq, (1, ic, il)):
                ref, mag = F.ref_integrate(m, item.f, item.g, cells, measure=ld)
                got = d.integrate(item.f, item.g, cells)
                got_all.append(got)
                if n == 0:
                    assert plus_zero(got), f"{where}, {F.item_id(item)}: the empty list gave {got}"
                    continue
                check(got, ref, mag, item.entry, f"{where}, {F.item_id(item)}", worst)
                if item.g is None and not item.variant and name in CROSS_LISTS:        # the components one by one through the pairing with ones
                    paired = d.integrate(item.f, np.ones_like(item.f), cells)
                    by_k = np.array([d.integrate(np.ascontiguousarray(item.f[..., k:k + 1]), np.ones((n, m.nq, 1)), cells)[0] for k in range(item.D)])
                    slack = EPS53 * (allowed("integrate") + allowed("pair")) * mag
                    assert np.all(np.abs(got.astype(F.LD) - by_k) <= slack), f"{where}, {F.item_id(item)}: integrate(f) vs integrate(f_k, ones)"
                    assert abs(np.sum(got.astype(F.LD)) - F.LD(paired[0])) <= np.sum(slack), f"{where}, {F.item_id(item)}: sum_k vs the pairing with ones"
            for item in F.moment_items(m, (2, ic, il)):
                ref, mag = F.ref_operand_moments(m, item.kind, item.bs, item.u, cells, measure=ld)
                got = d.moments(item.kind, item.bs, item.u, cells)
                got_all.append(got)
                if n == 0:
                    assert plus_zero(got), f"{where}, {F.item_id(item)}: the empty list gave {got}"
                    continue
                check(got, ref, mag, item.entry, f"{where}, {F.item_id(item)}", worst)
                if not item.variant and name in CROSS_LISTS:      # the fused form against evaluate -> integrate, at the sum of the two bounds
                    D = d.dm.value_size(item.kind, item.bs)
                    e = d.torch.empty((n, m.nq, D), dtype=d.torch.float64, device=d.dev)
                    cd, ud = d.cuda(cells, np.int32), d.cuda(item.u)
                    d.dm.evaluate_device(item.kind, item.bs, ud.data_ptr(), n, e.data_ptr(), None if cd is None else cd.data_ptr())
                    if D in F.INTEGRATE_SIZES:
                        parts = d.dm.integrate(e, cells=cd).cpu().numpy()
                        slack = EPS53 * (allowed(item.entry) + allowed("integrate")) * mag[:D]
                        assert np.all(np.abs(got[:D].astype(F.LD) - parts) <= slack), f"{where}, {F.item_id(item)}: moments[:D] vs integrate(evaluate)"
                    sq = d.dm.integrate(e, e, cells=cd).cpu().numpy()
                    assert abs(F.LD(got[D]) - F.LD(sq[0])) <= EPS53 * (allowed(item.entry) + allowed("pair")) * mag[D], \
                        f"{where}, {F.item_id(item)}: moments[D] vs integrate(e, e)"
            bits[name] = (dx, got_all)
        assert np.array_equal(bits["all"][0], bits["arange"][0]), "cell_measure: arange and NULL differ"
        for a, b in zip(bits["all"][1], bits["arange"][1]):
            assert np.array_equal(a, b), "arange and NULL gave other bits"
        report(worst)
    finally:
        d.close()


@pytest.mark.parametrize("case", F.FACET_CASES, ids=FC.case_id)
def test_facet_functionals_match_the_long_double_reference(ctx, case):
    """Every entity list of the case (those of facet_reference_cases and the lists around W groups); the per-component integrals and
    the pairing, every D and input variant."""
    m = FC.mesh_of(case)
    tabs, geom, _ = FC.rule_tables(case)
    nq = geom[0].size
    d = Device(ctx, m, case)
    ic, worst = F.FACET_CASES.index(case), {}
    try:
        for il, (name, ents) in enumerate(F.facet_lists(case).items()):
            where = f"{FC.case_id(case)}, {name}"
            fs = d.dm.facet_set(ents)
            ld = F.ref_facet_measure(m, tabs, geom, ents) if len(ents) else None
            for item in F.integrate_items(len(ents), nq, (3, ic, il)):
                got = d.facet_integrate(fs, item.f, item.g)
                if len(ents) == 0:
                    assert plus_zero(got), f"{where}, {F.item_id(item)}: the empty set gave {got}"
                    continue
                ref, mag = F.ref_facet_integrate(m, tabs, geom, ents, item.f, item.g, measure=ld)
                check(got, ref, mag, "facet_" + item.entry, f"{where}, {F.item_id(item)}", worst)
        report(worst)
    finally:
        d.close()


def _compute_units(ctx):
    return int(ctx.device_info()["compute_units"])


@pytest.mark.parametrize("cell", F.GROUP_CELLS)
def test_a_list_past_the_grid_cap(ctx, cell):
    """(4 * 8 * compute_units + 5) groups, D = 1, about half a million points: the persistent group loop of each cell kernel and of
    the facet kernel takes a second trip. cell_measure, integrate, the pairing, the "value" moments; facet_integrate and its pairing."""
    case = next(c for c in F.CELL_CASES if F.is_size(c, cell, 2, "d"))
    m, cu = F.cell_mesh(case), _compute_units(ctx)
    cells = F.big_cells(case, cu)
    n = len(cells)
    assert -(-n // (64 // m.nq)) > F.cap_groups(cu)
    rng = np.random.Generator(np.random.PCG64(77))
    f, g, u = rng.normal(size=(n, m.nq, 1)), rng.normal(size=(n, m.nq, 1)), rng.normal(size=m.node_x.shape[0])
    fcase = next(c for c in F.FACET_CASES if F.carries_facet_group_lists(c) and c[0] == cell)
    d = Device(ctx, m, fcase)
    worst = {}
    try:
        ld = F.ref_cell_measure(m, cells)
        check(d.dm.cell_measure(d.cuda(cells, np.int32)).cpu().numpy(), *ld, "measure", "big", worst)
        check(d.integrate(f, None, cells), *F.ref_integrate(m, f, None, cells, measure=ld), "integrate", "big", worst)
        check(d.integrate(f, g, cells), *F.ref_integrate(m, f, g, cells, measure=ld), "pair", "big", worst)
        check(d.moments("value", 1, u, cells), *F.ref_operand_moments(m, "value", 1, u, cells, measure=ld), "moments:value", "big", worst)
        tabs, geom, _ = FC.rule_tables(fcase)
        ents = F.big_entities(fcase, cu)
        nq = geom[0].size
        _, first, inv = np.unique(ents[:, 0].astype(np.int64) * 16 + ents[:, 1], return_index=True, return_inverse=True)   # the reference once per distinct entity
        meas = tuple(a[inv] for a in F.ref_facet_measure(FC.mesh_of(fcase), tabs, geom, ents[first]))
        ff, gf = rng.normal(size=(len(ents), nq, 1)), rng.normal(size=(len(ents), nq, 1))
        fs = d.dm.facet_set(ents)
        check(d.facet_integrate(fs, ff, None), *F.ref_facet_integrate(m, tabs, geom, ents, ff, None, measure=meas), "facet_integrate", "big", worst)
        check(d.facet_integrate(fs, ff, gf), *F.ref_facet_integrate(m, tabs, geom, ents, ff, gf, measure=meas), "facet_pair", "big", worst)
        report(worst)
    finally:
        d.close()


@pytest.mark.parametrize("cell", ["triangle", "quadrilateral", "tetrahedron", "hexahedron"])
def test_known_answers(ctx, cell):
    """Answers no oracle is needed for (each first asked of the reference in test_functional_reference_cpu.py): int 1 dx = 1 and
    int 1 ds = 2 gdim on the distorted size-b quadratic mesh of the unit square / cube, and the divergence theorem for a quadratic
    field on the undistorted one, int div u dx (operand_moments) = int u . n ds (evaluate_facets_device, facet_geometry,
    facet_integrate with g = n), held to the sum of the two sides' bounds."""
    fcase = next(c for c in FC.ALL_CASES if c[0] == cell and c[1] == 2 and c[2] == "b" and not c[3] and c[4] == "deg2")
    m = FC.mesh_of(fcase)
    G = m.gdim
    tabs, geom, _ = FC.rule_tables(fcase)
    d = Device(ctx, m, fcase)
    try:
        one = np.ones((m.num_cells, m.nq, 1))
        _, mag = F.ref_integrate(m, one)
        vol = d.integrate(one, None, None)
        assert abs(F.LD(vol[0]) - 1) <= allowed("integrate") * EPS53 * mag[0] + 1e-17, vol
        ents = FC.entity_lists(fcase)["exterior"]
        one = np.ones((len(ents), geom[0].size, 1))
        _, mag = F.ref_facet_integrate(m, tabs, geom, ents, one)
        surf = d.facet_integrate(d.dm.facet_set(ents), one, None)
        assert abs(F.LD(surf[0]) - 2 * G) <= allowed("facet_integrate") * EPS53 * mag[0] + 1e-17, surf
    finally:
        d.close()
    m, tabs, geom, ents = divergence_case(cell)
    d = Device(ctx, m, fcase)
    try:
        u = quadratic_field(m.node_x[:, :G])
        _, lmag = F.ref_operand_moments(m, "div", G, u)
        lhs = d.moments("div", G, u, None)[0]
        fs = d.dm.facet_set(ents)
        val = d.dm.evaluate_facets_device("value", G, d.cuda(u), d.cuda(ents, np.int32))
        nrm = d.torch.empty_like(val)
        d.dm.facet_geometry(fs, nrm.data_ptr(), None)
        rhs = d.dm.facet_integrate(val, fs, g=nrm).cpu().numpy()[0]
        from oracle.facet_reference import ref_facet_geometry
        from oracle.operand_reference import ref_operand_facets

        _, vmag = ref_operand_facets(m, "value", G, u, *tabs, ents)
        _, nmag, _, dSm = ref_facet_geometry(m, tabs, geom, ents)
        rmag = np.einsum("eq,eqi,eqi->", dSm, vmag, nmag)
        bound = EPS53 * (allowed("moments:div") * lmag[0] + allowed("facet_pair") * rmag)
        print(f"{cell}: int div u dx = {lhs!r}, int u.n ds = {rhs!r}, bound {float(bound):.3e}")
        assert abs(F.LD(lhs) - F.LD(rhs)) <= bound
    finally:
        d.close()


def test_capture_and_replay(ctx):
    """After one warm-up call each call is captured in a graph on the context's stream (one linear stream) and replayed with changed
    inputs: the bits of a direct call."""
    import torch

    fcase = next(c for c in FC.ALL_CASES if c[0] == "hexahedron" and c[1] == 2 and c[2] == "b" and not c[3] and c[4] == "deg2")
    m = FC.mesh_of(fcase)
    G, nq, nqf = m.gdim, m.nq, FC.nq_of(fcase)
    ents = FC.entity_lists(fcase)["exterior"]
    rng = np.random.Generator(np.random.PCG64(3))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = Device(ctx, m, fcase)        # the context now launches on `stream`
        try:
            dm, fs = d.dm, d.dm.facet_set(ents)
            n = m.num_cells
            f, g, ff, u = (d.cuda(rng.normal(size=s)) for s in ((n, nq, 6), (n, nq, 6), (len(ents), nqf, 3), (m.node_x.shape[0] * G,)))
            outs = {k: d.nan(s) for k, s in (("dx", n * nq), ("int", 6), ("pair", 1), ("facet", 3), ("mom", 7))}

            def calls():
                dm.cell_measure(out=outs["dx"].view(n, nq))
                dm.integrate(f, out=outs["int"])
                dm.integrate(f, g, out=outs["pair"])
                dm.facet_integrate(ff, fs, out=outs["facet"])
                dm.operand_moments("eps", G, u, out=outs["mom"])

            calls()                      # warm-up: the scratch is allocated here
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                calls()
            for t in (f, g, ff, u):
                t.copy_(d.cuda(rng.normal(size=tuple(t.shape))))
            graph.replay()
            stream.synchronize()
            replayed = {k: v.clone() for k, v in outs.items()}
            for v in outs.values():
                v.fill_(float("nan"))
            calls()
            stream.synchronize()
            for k in outs:
                assert torch.equal(replayed[k], outs[k]) and bool(torch.isfinite(outs[k]).all()), k
        finally:
            d.close()
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)


def test_error_codes(ctx):
    """NULL, misalignment, weights / facet geometry not set, a D outside the served set, a foreign facet set, a block size without a
    fused form: the stated code, and a dxo_last_error that names the call."""
    import torch

    from dolfinx_external_operator_amd import DeviceMesh

    fcase = next(c for c in FC.ALL_CASES if c[0] == "triangle" and c[1] == 2 and c[2] == "b" and not c[3] and c[4] == "deg2")
    m = FC.mesh_of(fcase)
    tabs, geom, _ = FC.rule_tables(fcase)
    d, other = Device(ctx, m, fcase), Device(ctx, m, fcase)
    lib, h = ctx.lib, ctx._h
    P = C.c_void_p
    try:
        buf = torch.zeros(m.num_cells * m.nq * 13 + 8, dtype=torch.float64, device=d.dev)
        u = torch.zeros(m.node_x.shape[0] * 5, dtype=torch.float64, device=d.dev)
        out = torch.zeros(16, dtype=torch.float64, device=d.dev)
        p, q, o = buf.data_ptr(), u.data_ptr(), out.data_ptr()
        fs, fs_other = d.dm.facet_set(FC.entity_lists(fcase)["exterior"]), other.dm.facet_set(FC.entity_lists(fcase)["exterior"])
        bare = DeviceMesh(gdim=m.gdim, phi=m.phi, dphi=m.dphi, dpsi=m.dpsi, dofmap=m.dofmap, geom_dofmap=m.geom_dofmap, x=m.x,
                          num_field_nodes=m.node_x.shape[0], ctx=ctx)      # no weights, no facet tables
        no_geom = DeviceMesh.from_synthetic(m, ctx=ctx)
        no_geom.set_facet_tables(*tabs)                                     # tables, no facet geometry
        fs_no_geom = no_geom.facet_set(FC.entity_lists(fcase)["exterior"])
        M, nc = d.dm._h, m.num_cells

        def expect(code, name, rc):
            text = lib.dxo_last_error(h).decode()
            assert rc == code, (name, rc, text)
            assert name in text, (name, text)

        expect(E_NULL, "dxo_eval_cell_measure", lib.dxo_eval_cell_measure(h, None, None, nc, P(p)))
        expect(E_NULL, "dxo_eval_cell_measure", lib.dxo_eval_cell_measure(h, M, None, nc, None))
        expect(E_ALIGN, "dxo_eval_cell_measure", lib.dxo_eval_cell_measure(h, M, None, nc, P(p + 4)))
        expect(E_OPTION, "dxo_eval_cell_measure", lib.dxo_eval_cell_measure(h, bare._h, None, nc, P(p)))
        expect(E_NULL, "dxo_integrate", lib.dxo_integrate(h, M, None, nc, 3, None, None, P(o)))
        expect(E_NULL, "dxo_integrate", lib.dxo_integrate(h, M, None, nc, 3, P(p), None, None))
        expect(E_ALIGN, "dxo_integrate", lib.dxo_integrate(h, M, None, nc, 3, P(p + 4), None, P(o)))
        expect(E_ALIGN, "dxo_integrate", lib.dxo_integrate(h, M, None, nc, 3, P(p), P(p + 4), P(o)))
        expect(E_ALIGN, "dxo_integrate", lib.dxo_integrate(h, M, None, nc, 3, P(p), None, P(o + 4)))
        expect(E_OPTION, "dxo_integrate", lib.dxo_integrate(h, bare._h, None, nc, 3, P(p), None, P(o)))
        for D in (0, 5, 7, 8, 13):
            expect(E_DIM, "dxo_integrate", lib.dxo_integrate(h, M, None, nc, D, P(p), None, P(o)))
        expect(E_DIM, "dxo_integrate", lib.dxo_integrate(h, M, None, nc, 0, P(p), P(p), P(o)))
        assert lib.dxo_integrate(h, M, None, nc, 13, P(p), P(p), P(o)) == 0          # the pairing serves any D
        F_ = fs._h
        expect(E_NULL, "dxo_facet_integrate", lib.dxo_facet_integrate(h, M, None, 1, P(p), None, P(o)))
        expect(E_NULL, "dxo_facet_integrate", lib.dxo_facet_integrate(h, M, F_, 1, None, None, P(o)))
        expect(E_NULL, "dxo_facet_integrate", lib.dxo_facet_integrate(h, M, F_, 1, P(p), None, None))
        expect(E_ALIGN, "dxo_facet_integrate", lib.dxo_facet_integrate(h, M, F_, 1, P(p + 4), None, P(o)))
        expect(E_DIM, "dxo_facet_integrate", lib.dxo_facet_integrate(h, M, F_, 5, P(p), None, P(o)))
        expect(E_DIM, "dxo_facet_integrate", lib.dxo_facet_integrate(h, M, fs_other._h, 1, P(p), None, P(o)))      # a foreign set
        expect(E_OPTION, "dxo_facet_integrate", lib.dxo_facet_integrate(h, no_geom._h, fs_no_geom._h, 1, P(p), None, P(o)))
        K = {"value": 0, "grad": 1, "eps": 2}
        expect(E_NULL, "dxo_operand_moments", lib.dxo_operand_moments(h, M, K["value"], 1, None, None, nc, P(o)))
        expect(E_NULL, "dxo_operand_moments", lib.dxo_operand_moments(h, M, K["value"], 1, P(q), None, nc, None))
        expect(E_ALIGN, "dxo_operand_moments", lib.dxo_operand_moments(h, M, K["value"], 1, P(q + 4), None, nc, P(o)))
        expect(E_OPTION, "dxo_operand_moments", lib.dxo_operand_moments(h, bare._h, K["value"], 1, P(q), None, nc, P(o)))
        expect(E_OPTION, "dxo_operand_moments", lib.dxo_operand_moments(h, M, 99, 1, P(q), None, nc, P(o)))
        expect(E_DIM, "dxo_operand_moments", lib.dxo_operand_moments(h, M, K["value"], 5, P(q), None, nc, P(o)))   # dxo_eval_operand takes bs = 5
        expect(E_DIM, "dxo_operand_moments", lib.dxo_operand_moments(h, M, K["eps"], 1, P(q), None, nc, P(o)))
        torch.cuda.synchronize()
        # the Python layer names the expected shape
        with pytest.raises(ValueError, match=r"shape \(\d+, 3, n\)"):
            d.dm.integrate(torch.zeros(5, device=d.dev, dtype=torch.float64))
        with pytest.raises(ValueError, match="float64"):
            d.dm.integrate(torch.zeros((nc, m.nq, 1), device=d.dev, dtype=torch.float32))
        with pytest.raises(ValueError, match="served"):
            d.dm.integrate(torch.zeros((nc, m.nq, 5), device=d.dev, dtype=torch.float64))
        with pytest.raises(ValueError, match="fused"):
            d.dm.operand_moments("value", 5, u)
        for x in (bare, no_geom):
            x.close()
    finally:
        d.close()
        other.close()


def test_the_example_runs(ctx):
    """examples/device_functionals.py end to end: its own asserts compare every device result with the host quadrature."""
    import importlib.util
    import pathlib

    spec = importlib.util.spec_from_file_location("device_functionals", pathlib.Path(__file__).resolve().parent.parent / "examples" / "device_functionals.py")
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    got = ex.main()
    assert math.isclose(got["l2_error"], math.sqrt(ex.L2_ERROR_SQ_EXACT), rel_tol=1e-12)
