"""The boundary-facet layer (csrc/facet_form.hip: dxo_eval_facet_geometry, dxo_facet_pressure, dxo_facet_adjoint,
dxo_facet_bilinear_apply / _diagonal / _assemble) against the long-double reference of oracle/facet_reference.py, entry by entry, on
the meshes, facet rules, entity lists and inputs of tests/facet_reference_cases.py — and never one HIP result against another, the
bit-identity checks apart.

Bound, for EVERY entry k: |got[k] - (r0[k] + ref[k])| <= c * 2^-53 * mag[k] + t[k] * 2^-53 * |r0[k]|. r0 is what the output held
before the call (all these calls accumulate; the geometry call overwrites: r0 = 0), mag[k] the same sum as ref[k] with the absolute
value of every factor and term, c = MARGIN * C_REF[entry] (facet_reference_cases.py): 8 times what float64 NumPy itself loses against
long double on these cases. t = 1 for the dof vectors, because facet_node_sum forms a node's sum in a register and adds it to `out`
once; for dxo_facet_bilinear_assemble t[k] is the number of entity contributions to entry k, because assemble_rows (csr.h) adds every
entity's row straight into `values` (dst[jj] += src[...] inside its loop over the node's incidences), one rounding against what the
entry holds each time. Entries with mag = 0 — untouched nodes, pattern entries no entity reaches — hold r0 exactly. c is not tuned on
the kernels; the ratios they show on the MI355X are in profiles/facet_reference_ratios.txt."""
import os
import zlib

import numpy as np
import pytest

from facet_reference_cases import (ALL_CASES, C_REF, MARGIN, RESOLVES, case_id, entity_lists, item_id, mesh_of, old_criterion, reference,
                                   rule_tables, work_items)
from oracle.facet_reference import LD, scatter_csr

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, -7.25
EPS53 = LD(2.0) ** -53
CHUNK = 5          # assemble_chunk_cells that splits every workgroup round of facet_assemble_elem (24 entities or more)


def ratio_to_reference(got, ref, mag, r0, t=1, keep=None):
    """max_k (|got - (r0 + ref)| - t 2^-53 |r0|) / (2^-53 mag) over the entries of `keep`; an entry with mag = 0 must hold r0 exactly."""
    got, r0 = np.asarray(got).reshape(-1), np.asarray(r0).reshape(-1)
    ref, mag = np.asarray(ref).reshape(-1), np.asarray(mag).reshape(-1)
    err = np.abs(got.astype(LD) - (r0.astype(LD) + ref)) - t * EPS53 * np.abs(r0.astype(LD))
    keep = np.ones(err.shape, dtype=bool) if keep is None else keep
    zero = keep & (mag == 0)
    assert np.array_equal(got[zero], r0[zero]), "an entry with mag = 0 does not hold what it held before the call"
    nz = keep & (mag != 0)
    return float(np.max(np.maximum(err[nz], 0) / (EPS53 * mag[nz]), initial=0.0))


def record(line):
    print(line)
    path = os.environ.get("DXO_FACET_RATIOS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


class Device:
    """One DeviceMesh with the case's facet tables, and the device calls of the work items. run() starts the output as r0 with a band
    of GUARD sentinels behind it, checks the band, and returns the output as a host array."""

    def __init__(self, ctx, case):
        import torch

        from dolfinx_external_operator_amd import DeviceMesh

        self.torch, self.ctx, self.case = torch, ctx, case
        self.m = mesh_of(case)
        tabs, geom, _ = rule_tables(case)
        self.dev = torch.device("cuda", ctx.device)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        self.dm = DeviceMesh.from_synthetic(self.m, ctx=ctx)
        self.dm.set_facet_tables(*tabs)
        self.dm.set_facet_geometry(*geom)
        self.nq = geom[0].size
        self.patterns = {}

    def close(self):
        self.dm.close()

    def cuda(self, a):
        return self.torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)).to(self.dev)

    def pattern(self, bs):
        """(CsrPattern, indptr, indices) of block size bs, the index arrays on the host."""
        if bs not in self.patterns:
            pat = self.dm.csr_pattern(bs)
            self.patterns[bs] = (pat, pat.indptr.cpu().numpy(), pat.indices.cpu().numpy())
        return self.patterns[bs]

    def run(self, call, r0):
        torch = self.torch
        n = r0.size
        buf = torch.cat([torch.from_numpy(np.ascontiguousarray(r0, dtype=np.float64).reshape(-1)),
                         torch.full((GUARD,), SENTINEL, dtype=torch.float64)]).to(self.dev)
        call(buf[:n])
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[n:], np.full(GUARD, SENTINEL)), "the call wrote behind its output"
        return got[:n]

    def call_of(self, fs, item, **replace):
        """-> (call(out tensor), the device arrays it reads, kept alive by the caller). `replace`: other host arrays for S / C / v / p."""
        dm, a = self.dm, {k: replace.get(k, getattr(item, k, None)) for k in ("S", "C", "v", "p")}
        d = {k: self.cuda(x) for k, x in a.items() if x is not None}
        if item.what == "pressure":
            return (lambda o: dm.facet_pressure(fs, o.data_ptr(), d["p"].data_ptr() if "p" in d else None, item.scale)), d
        if item.what == "adjoint":
            return (lambda o: dm.facet_adjoint(item.kind, item.bs, d["S"].data_ptr(), fs, o.data_ptr())), d
        if item.what == "apply":
            return (lambda o: dm.facet_bilinear_apply(item.kind, item.bs, d["C"].data_ptr(), d["v"].data_ptr(), fs, o.data_ptr())), d
        if item.what == "diag":
            return (lambda o: dm.facet_bilinear_diagonal(item.kind, item.bs, d["C"].data_ptr(), fs, o.data_ptr())), d
        if item.what == "matrix":
            pat = self.pattern(item.bs)[0]
            return (lambda o: dm.facet_bilinear_assemble(item.kind, item.bs, d["C"].data_ptr(), fs, pat, values=o)), d
        raise ValueError(item.what)

    def matrix_reference(self, ents, item, Ke, Ka):
        """-> (ref, mag, t, r0) on the entries of the pattern: the element matrices scattered entry by entry, the number of entity
        contributions to every entry, and seeded N(0, 1) values for the pre-filled `values`."""
        _, indptr, indices = self.pattern(item.bs)
        ref, mag = (scatter_csr(self.m, ents, item.bs, x, indptr, indices) for x in (Ke, Ka))
        t = scatter_csr(self.m, ents, item.bs, np.ones(Ke.shape), indptr, indices)
        rng = np.random.Generator(np.random.PCG64(zlib.crc32(f"{case_id(self.case)} {item_id(item)}".encode())))
        return ref, mag, t, rng.normal(size=indices.size)


def check_geometry(d, fs, ents, worst, where):
    """Both outputs in one call, either one alone (identical bits), the bands behind them; the call overwrites."""
    refs = reference(d.case, ents, work_items(d.case, where[1])[0])
    (n, nm), (dS, dm_) = refs["normal"], refs["dS"]
    G = d.m.gdim
    prefill_n, prefill_s = np.full(n.size, 3.5), np.full(dS.size, 3.5)
    out = {}

    def both(o):
        s = d.torch.full((dS.size + GUARD,), SENTINEL, dtype=d.torch.float64, device=d.dev)
        d.dm.facet_geometry(fs, o.data_ptr(), s.data_ptr())
        d.torch.cuda.synchronize()
        s = s.cpu().numpy()
        assert np.array_equal(s[dS.size:], np.full(GUARD, SENTINEL)), "the call wrote behind dS"
        out["dS"] = s[:dS.size]

    out["normal"] = d.run(both, prefill_n)
    alone_n = d.run(lambda o: d.dm.facet_geometry(fs, o.data_ptr(), None), prefill_n)
    alone_s = d.run(lambda o: d.dm.facet_geometry(fs, None, o.data_ptr()), prefill_s)
    assert np.array_equal(alone_n, out["normal"]) and np.array_equal(alone_s, out["dS"]), "one output alone gave other bits"
    assert n.shape == (len(ents), d.nq, G)
    for entry, ref, mag in (("normal", n, nm), ("dS", dS, dm_)):
        ratio = ratio_to_reference(out[entry], ref, mag, np.zeros(ref.size))
        note(worst, entry, "", ratio, where)
        assert ratio <= MARGIN * C_REF[entry], f"{where} {entry}: {ratio:.2f} * 2^-53 * mag, allowed {MARGIN * C_REF[entry]:.1f}"


def note(worst, entry, variant, ratio, where):
    if ratio >= worst.get((entry, variant), (-1.0,))[0]:
        worst[(entry, variant)] = (ratio, where)


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_facet_kernels_match_the_long_double_reference(ctx, case):
    """One DeviceMesh per (mesh, rule); every entity list of the case, and on each the geometry, the pressure load (with p, with
    p = NULL, with scale = -2.5), the adjoint of all six kinds, and action, diagonal and assembled matrix of every trial kind, each
    with every block size it takes and every input variant of facet_reference_cases.work_items. In the same calls: accumulation into a
    pre-filled output, 64 sentinel doubles behind it untouched, identical bits from a second call (no atomics anywhere in the file),
    the assembly once more with assemble_chunk_cells = 5 (identical bits again), and the empty list touching nothing."""
    d = Device(ctx, case)
    worst = {}
    assert ctx.get_option("assemble_chunk_cells") == 0
    try:
        for name, ents in entity_lists(case).items():
            fs = d.dm.facet_set(ents)
            where = (case_id(case), name)
            for item in work_items(case, name):
                if item.what == "geometry":
                    if len(ents):
                        check_geometry(d, fs, ents, worst, where)
                    else:
                        d.dm.facet_geometry(fs, None, None)
                    continue
                (ref, mag), = reference(case, ents, item).values()
                c = MARGIN * C_REF[item.entry]
                call, keep_alive = d.call_of(fs, item)
                t, r0 = 1, item.r0
                if item.what == "matrix":
                    ref, mag, t, r0 = d.matrix_reference(ents, item, ref, mag)
                got = d.run(call, r0)
                if len(ents) == 0:
                    assert np.array_equal(got, r0), f"{where} {item_id(item)}: the empty list touched the output"
                    continue
                ratio = ratio_to_reference(got, ref, mag, r0, t)
                note(worst, item.entry, item.variant, ratio, where + (item.bs,))
                assert ratio <= c, f"{where} {item_id(item)}: {ratio:.2f} * 2^-53 * mag, allowed {c:.1f}"
                assert np.array_equal(d.run(call, r0), got), f"{where} {item_id(item)}: a second call gave other bits"
                if item.what == "matrix":
                    ctx.set_option("assemble_chunk_cells", CHUNK)
                    try:
                        chunked = d.run(call, r0)
                    finally:
                        ctx.set_option("assemble_chunk_cells", 0)
                    assert np.array_equal(chunked, got), f"{where} {item_id(item)}: chunks of {CHUNK} entities gave other bits"
                del keep_alive
        for (entry, variant), (ratio, at) in sorted(worst.items()):
            record(f"{case_id(case):34s} {entry:18s} {variant:7s} {ratio:8.2f}   (c = {MARGIN * C_REF[entry]:6.1f})   worst at {at[1:]}")
    finally:
        ctx.set_option("assemble_chunk_cells", 0)
        d.close()


SIZE_B = [c for c in ALL_CASES if c[1] == 2 and c[2] == "b" and not c[3] and c[4] == "deg2"]


def _cell_dofs(m, cells, bs):
    inside = np.zeros((m.node_x.shape[0], bs), dtype=bool)
    inside[m.dofmap[np.asarray(cells).reshape(-1)]] = True
    return inside.reshape(-1)


@pytest.mark.parametrize("case", SIZE_B, ids=case_id)
def test_a_nan_stays_in_the_cells_it_belongs_to(ctx, case):
    """Quadratic elements, size b, list `all` (a cell carries several entities, its nodes are shared with other cells' entities).
    A NaN block of S / C at ONE facet point of one entity makes exactly the dofs of that entity's cell NaN — in the matrix exactly the
    entries whose row node and column node both belong to that cell — and every other entry stays within the bound of the reference
    that has a zero block at that point. A NaN in v at one node reaches exactly the dofs of the cells that own an entity and contain
    that node."""
    d = Device(ctx, case)
    m = d.m
    ents = entity_lists(case)["all"]
    e_bad, q_bad = len(ents) // 2 + 1, d.nq - 1
    node_bad = int(m.dofmap[ents[e_bad, 0]][0])
    try:
        fs = d.dm.facet_set(ents)
        for item in work_items(case, "all"):
            if item.what in ("geometry", "pressure") or item.variant:
                continue
            c, key = MARGIN * C_REF[item.entry], "S" if item.what == "adjoint" else "C"
            bad, zeroed = np.array(getattr(item, key)), np.array(getattr(item, key))
            bad[e_bad, q_bad], zeroed[e_bad, q_bad] = np.nan, 0.0
            call, keep_alive = d.call_of(fs, item, **{key: bad})
            (ref, mag), = reference(case, ents, type(item)(**{**vars(item), key: zeroed})).values()
            t, r0 = 1, item.r0
            if item.what == "matrix":
                ref, mag, t, r0 = d.matrix_reference(ents, item, ref, mag)
                _, indptr, indices = d.pattern(item.bs)
                expect = scatter_csr(m, ents[e_bad:e_bad + 1], item.bs, np.ones((1,) + (m.dofmap.shape[1] * item.bs,) * 2), indptr, indices) > 0
            else:
                expect = _cell_dofs(m, ents[e_bad, 0], item.bs)
            got = d.run(call, r0)
            assert np.array_equal(np.isnan(got), expect), f"{item_id(item)}: NaN on {np.flatnonzero(np.isnan(got) != expect)[:8]}"
            ratio = ratio_to_reference(got, ref, mag, r0, t, keep=~expect)
            record(f"{case_id(case):34s} {item.entry:18s} {'NaN ' + key:7s} {ratio:8.2f}   (c = {c:6.1f})   bs {item.bs}")
            assert ratio <= c, f"{item_id(item)} beside a NaN block of {key}: {ratio:.2f}, allowed {c:.1f}"
            if item.what == "apply":
                v_bad, v_zero = item.v.reshape(-1, item.bs).copy(), item.v.reshape(-1, item.bs).copy()
                v_bad[node_bad], v_zero[node_bad] = np.nan, 0.0
                owners = np.unique(ents[:, 0])
                expect = _cell_dofs(m, owners[(m.dofmap[owners] == node_bad).any(axis=1)], item.bs)
                call, keep_alive = d.call_of(fs, item, v=v_bad)
                (ref, mag), = reference(case, ents, type(item)(**{**vars(item), "v": v_zero.reshape(-1)})).values()
                got = d.run(call, item.r0)
                assert np.array_equal(np.isnan(got), expect), f"{item_id(item)}: NaN of v on {np.flatnonzero(np.isnan(got) != expect)[:8]}"
                ratio = ratio_to_reference(got, ref, mag, item.r0, keep=~expect)
                record(f"{case_id(case):34s} {item.entry:18s} {'NaN v':7s} {ratio:8.2f}   (c = {c:6.1f})   bs {item.bs}")
                assert ratio <= c, f"{item_id(item)} beside a NaN node of v: {ratio:.2f}, allowed {c:.1f}"
            del keep_alive
    finally:
        d.close()


@pytest.mark.parametrize("case", SIZE_B, ids=case_id)
def test_the_bound_sees_the_relative_error_resolves_names_in_one_entity(ctx, case):
    """What the componentwise bound resolves: the device is handed S / C / p whose values on entity 0 are scaled by
    1 + 10^-RESOLVES[entry], the reference keeps the unscaled ones. Every call must then MISS the bound of the first test — and still
    meet max|got - ref| <= 1e-12 max|ref|, the criterion of tests/test_facet_form_gpu.py and tests/test_facet_bilinear_gpu.py.
    Quadratic elements, size b, the whole boundary, block size gdim, r0 = 0."""
    d = Device(ctx, case)
    m = d.m
    ents = entity_lists(case)["exterior"]
    try:
        fs = d.dm.facet_set(ents)
        for item in work_items(case, "exterior"):
            if item.what == "geometry" or item.variant not in ("", "p") or item.bs != m.gdim:
                continue
            key = {"pressure": "p", "adjoint": "S"}.get(item.what, "C")
            scaled = np.array(getattr(item, key))
            scaled[0] *= 1.0 + 10.0 ** -RESOLVES[item.entry]
            call, keep_alive = d.call_of(fs, item, **{key: scaled})
            (ref, mag), = reference(case, ents, item).values()
            t = 1
            if item.what == "matrix":
                ref, mag, t, _ = d.matrix_reference(ents, item, ref, mag)
            got = d.run(call, np.zeros(ref.size))
            ratio, c = ratio_to_reference(got, ref, mag, np.zeros(ref.size), t), MARGIN * C_REF[item.entry]
            print(f"{case_id(case)} {item.entry}: ratio with entity 0 scaled by 1 + 1e-{RESOLVES[item.entry]}: {ratio:.0f} (c = {c:.1f})")
            assert ratio > c, (item.entry, ratio)
            assert old_criterion(got, ref), item.entry
            del keep_alive
    finally:
        d.close()
