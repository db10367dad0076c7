"""The producer side (dxo_eval_operand, dxo_eval_operand_facets, dxo_eval_coordinate: csrc/operand.hip, operand_facet.hip,
operand_core.h, operand_cell.h) against the long-double reference of oracle/operand_reference.py: all nine operand kinds on all eight
standard elements and two further quadrature rules, over all cells (the register pipeline), through entity lists (operand_point), on
(cell, facet) pairs, dense (bs = 1, gdim) and one component at a time (out_stride / u_stride), from host arrays and from device
pointers, on meshes of at most 200 cells — and never one HIP result against another.

Bound, for EVERY entry k of an operand array: |got[k] - ref[k]| <= c * 2^-53 * mag[k], where mag[k] is the same expression as ref[k]
with the absolute value of every factor and c = MARGIN * C_REF[kind] (operand_cases.py): 8 times what float64 NumPy itself loses
against long double on these meshes. Entries with mag = 0 (the zz slot of 2-D eps) must be exact. c is not tuned on the kernels; the
ratios they show are in profiles/operand_reference_ratios.txt."""
import os

import numpy as np
import pytest

from operand_cases import (ALL_CASES, C_REF, CELL_KINDS, MARGIN, RESOLVES, SIZES, block_sizes, build_mesh, case_id, entity_lists,
                           facet_lists, facet_tabs, fields, kinds_of, resolution_case, scale_one_cell)
from oracle.operand_reference import ref_coordinate, ref_operand, ref_operand_facets, value_size, worst_ratio

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, -7.25
# elements with a lane = cell strain kernel (operand_cell.h DXO_OPERAND_CELL_CASES): (gdim, ndofs, nq, ngeom)
LANE_CELL = {(2, 6, 3, 3), (2, 9, 4, 4)}


def record(line):
    print(line)
    path = os.environ.get("DXO_OPERAND_RATIOS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


class Device:
    """One DeviceMesh and the two ways into it. Every call writes into a buffer pre-filled with SENTINEL that has GUARD more
    sentinels behind it: all of `out` must have been written, nothing behind it, and a second call must return the same bits."""

    def __init__(self, ctx, mesh):
        import torch

        from dolfinx_external_operator_amd import DeviceMesh

        self.torch, self.ctx, self.m = torch, ctx, mesh
        self.dev = torch.device("cuda", ctx.device)
        self.dm = DeviceMesh.from_synthetic(mesh, ctx=ctx)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        self._up = {}

    def close(self):
        self.dm.close()

    def upload(self, a):
        """Host array -> device tensor, kept for the life of the case (keyed by the array object, which the caller keeps alive)."""
        t = self._up.get(id(a))
        if t is None:
            t = self._up[id(a)] = (a, self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev))
        return t[1]

    def _checked(self, shape, call_host, call_device, entry):
        n = int(np.prod(shape))
        for attempt in range(2):
            if entry == "host":
                buf = np.full(n + GUARD, SENTINEL)
                call_host(buf[:n].reshape(shape))
            else:
                t = self.torch.full((n + GUARD,), SENTINEL, dtype=self.torch.float64, device=self.dev)
                call_device(t.data_ptr())
                self.torch.cuda.synchronize()
                buf = t.cpu().numpy()
            assert np.array_equal(buf[n:], np.full(GUARD, SENTINEL)), "the call wrote behind out"
            assert not np.any(buf[:n] == SENTINEL), f"{int(np.sum(buf[:n] == SENTINEL))} entries of out were not written"
            if attempt == 0:
                got = buf[:n].reshape(shape).copy()
            else:
                assert np.array_equal(buf[:n].reshape(shape), got, equal_nan=True), "a second call gave other bits"
        return got

    def operand(self, entry, kind, bs, u, cells=None):
        n = self.m.num_cells if cells is None else len(cells)
        shape = (n, self.m.nq, value_size(kind, bs, self.m.gdim))
        return self._checked(
            shape, lambda out: self.dm.evaluate(kind, bs, u, cells, out=out),
            lambda ptr: self.dm.evaluate_device(kind, bs, self.upload(u).data_ptr(), n, ptr, None if cells is None else self.upload(cells).data_ptr()),
            entry)

    def facets(self, kind, bs, u, ents, nqf):
        shape = (len(ents), nqf, value_size(kind, bs, self.m.gdim))
        return self._checked(shape, lambda out: self.dm.evaluate_facets(kind, bs, u, ents, out=out), None, "host")

    def coordinate(self, entry, cells=None):
        n = self.m.num_cells if cells is None else len(cells)
        return self._checked((n, self.m.nq, self.m.gdim), lambda out: self.dm.coordinate(cells, out=out),
                             lambda ptr: self.dm.coordinate_device(n, ptr, None if cells is None else self.upload(cells).data_ptr()), entry)


def strain_options(mesh, kind):
    """ctx option operand_cell for one kind: both values for eps on the 2-D elements (1: the lane = cell kernel where the element has
    one, operand.hip dispatch_kind; 0: the wave-group kernel), the default alone elsewhere."""
    return (1, 0) if kind == "eps" and mesh.gdim == 2 else (1,)


def kernel_label(mesh, kind, option, all_cells):
    """Which strain kernel the option asks for on this call: the lane = cell kernel serves eps over all cells of the elements of
    LANE_CELL; entity lists, facets and every other element keep the wave-group kernel whatever the option says."""
    if kind != "eps" or mesh.gdim != 2:
        return ""
    lane = option == 1 and all_cells and (mesh.gdim, mesh.dofmap.shape[1], mesh.nq, mesh.geom_dofmap.shape[1]) in LANE_CELL
    return f"operand_cell={option} ({'lane=cell' if lane else 'wave-group'})"


class option:
    """ctx.set_option(key, value) for a with-block, restored on the way out (as test_operand_eval.py's strain_kernels fixture does)."""

    def __init__(self, ctx, key, value):
        self.ctx, self.key, self.value = ctx, key, value

    def __enter__(self):
        self.old = self.ctx.get_option(self.key)
        self.ctx.set_option(self.key, self.value)
        assert self.ctx.get_option(self.key) == self.value

    def __exit__(self, *exc):
        self.ctx.set_option(self.key, self.old)


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_operand_kernels_match_the_long_double_reference(ctx, case):
    """One DeviceMesh per (element, rule, mesh size). Every kind of every block size of operand_cases.block_sizes on every field
    (rough; rough + 1e6; on size b the field whose det F changes sign), three ways: over all cells, through every entity list
    (reversed, with repeats, one cell, empty), both from host arrays and from device pointers, and on both facet lists. eps on the 2-D
    elements under operand_cell = 1 and 0. The operand x the same ways. The reference of a list is the rows it names of the all-cells
    reference (test_operand_reference_cpu.py shows the two equal)."""
    m = build_mesh(case)
    G = m.gdim
    lists, flists, tabs = entity_lists(m), facet_lists(m), facet_tabs(m)
    nqf = tabs[0].shape[1]
    assert ctx.get_option("operand_cell") == 1
    d = Device(ctx, m)
    worst = {}

    def judge(got, ref, mag, kind, bs, path, label, what):
        key = kind + "@facet" if path == "facets" else kind
        c = MARGIN * C_REF[key]
        ratio = worst_ratio(got, ref, mag)
        k = (kind, bs, path.split("/")[0], label)          # the record folds the two entries: worst of host arrays and device pointers
        worst[k] = (max(worst.get(k, (0.0, c))[0], ratio), c)
        assert ratio <= c, f"{case_id(case)} {kind} bs={bs} {path} {label} [{what}]: {ratio:.2f} * 2^-53 * mag, allowed {c:.1f}"

    try:
        d.dm.set_facet_tables(*tabs)
        for bs in block_sizes(G):
            for fname, u in fields(case, m, bs).items():
                for kind in kinds_of(G, bs):
                    ref, mag = ref_operand(m, kind, bs, u)
                    for opt in strain_options(m, kind):
                        with option(ctx, "operand_cell", opt):
                            for entry in ("host", "device"):
                                judge(d.operand(entry, kind, bs, u), ref, mag, kind, bs, f"cells/{entry}", kernel_label(m, kind, opt, True), fname)
                                for lname, cells in lists.items():
                                    got = d.operand(entry, kind, bs, u, cells)
                                    assert got.shape == (len(cells), m.nq, ref.shape[2])
                                    judge(got, ref[cells], mag[cells], kind, bs, f"lists/{entry}", kernel_label(m, kind, opt, False), f"{fname}, {lname}")
                            for lname, ents in flists.items():
                                ref_f, mag_f = ref_operand_facets(m, kind, bs, u, *tabs, ents)
                                judge(d.facets(kind, bs, u, ents, nqf), ref_f, mag_f, kind, bs, "facets", kernel_label(m, kind, opt, False), f"{fname}, {lname}")
        ref, mag = ref_coordinate(m)
        for entry in ("host", "device"):
            judge(d.coordinate(entry), ref, mag, "x", G, f"cells/{entry}", "", "")
            for lname, cells in lists.items():
                judge(d.coordinate(entry, cells), ref[cells], mag[cells], "x", G, f"lists/{entry}", "", lname)
    finally:
        d.close()
        for (kind, bs, path, label), (ratio, c) in worst.items():
            record(f"{case_id(case):30s} {kind:10s} bs={bs} {path:8s} {label:36s} {ratio:7.2f}  (c = {c:.1f})")


def poisoned_slots(kind, bs, G, i):
    """The slots of a point's operand that component i of the field enters."""
    grad = [i * G + j for j in range(G)]
    if kind == "value":
        return [i]
    if kind in ("grad", "F"):
        return grad
    if kind == "value_grad":
        return [i] + [bs + s for s in grad]
    if kind == "detF":
        return [0]
    pairs = [(0, 1)] if G == 2 else [(0, 1), (0, 2), (1, 2)]
    return [i] + [3 + s for s, p in enumerate(pairs) if i in p]          # eps


@pytest.mark.parametrize("cell", list(SIZES))
@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("poison", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_dof_stays_inside_the_cells_that_own_it(ctx, cell, degree, poison):
    """Size b: one component of one interior node — the most shared node of a cell of the ragged second wave group — is NaN, or +inf.
    The non-finite output points are exactly the points of the cells whose dofmap row contains the node, within them exactly the
    slots that component enters (other components of the same points stay finite and inside the bound), and every other entry stays
    inside the bound: the wave-private LDS staging (pipe_commit, store_points, the lane = cell kernel's E and its idle lanes that
    recompute the last cell) leaks nothing. value, grad, eps (both kernels), F, detF with bs = gdim and value_grad with bs = 5
    (per-component launches), over all cells and through the reversed entity list."""
    case = next(c for c in ALL_CASES if c[0] == cell and c[1] == degree and c[4] == "b")
    m = build_mesh(case)
    G, nc = m.gdim, m.num_cells
    victim = 64 // m.nq + 1
    counts = np.bincount(m.dofmap.reshape(-1), minlength=m.node_x.shape[0])
    node = int(m.dofmap[victim][np.argmax(counts[m.dofmap[victim]])])
    owners = (m.dofmap == node).any(axis=1)
    assert 2 <= owners.sum() < nc
    rev = entity_lists(m)["reversed"]
    d = Device(ctx, m)
    try:
        for kind, bs, i in [(k, G, 1) for k in ("value", "grad", "eps", "F", "detF")] + [("value_grad", 5, 3)]:
            u = fields(case, m, bs)["rough"].copy()
            u.reshape(-1, bs)[node, i] = poison
            ref, mag = ref_operand(m, kind, bs, u)
            bad = np.zeros(ref.shape, dtype=bool)
            bad[np.ix_(owners, np.arange(m.nq), poisoned_slots(kind, bs, G, i))] = True
            assert np.array_equal(~np.isfinite(ref), bad), "the reference itself spreads the non-finite dof otherwise"
            for opt in strain_options(m, kind):
                with option(ctx, "operand_cell", opt):
                    for cells in (None, rev):
                        got = d.operand("device", kind, bs, u, cells)
                        r, g, b = (ref, mag, bad) if cells is None else (ref[cells], mag[cells], bad[cells])
                        where = f"{kind} bs={bs} {kernel_label(m, kind, opt, cells is None)} {'all cells' if cells is None else 'reversed list'}"
                        assert np.array_equal((~np.isfinite(got)).any(axis=2), np.broadcast_to((owners if cells is None else owners[cells])[:, None], got.shape[:2])), where
                        assert np.array_equal(~np.isfinite(got), b), f"{where}: non-finite slots differ at {np.argwhere(~np.isfinite(got) != b)[:6].tolist()}"
                        ratio = worst_ratio(got[~b], r[~b], g[~b])
                        record(f"{case_id(case):30s} {kind:10s} bs={bs} {'cells' if cells is None else 'lists':8s} "
                               f"{(kernel_label(m, kind, opt, cells is None) + (' nan' if np.isnan(poison) else ' inf') + ' dof').strip():36s} {ratio:7.2f}  (c = {MARGIN * C_REF[kind]:.1f})")
                        assert ratio <= MARGIN * C_REF[kind], f"{where}: {ratio:.2f}"
    finally:
        d.close()


@pytest.mark.parametrize("cell", list(SIZES))
def test_the_bound_sees_the_relative_error_it_claims_in_one_cell(ctx, cell):
    """What the componentwise bound resolves: the device is handed a field whose dofs on the nodes of cell 0 are scaled by
    1 + 10^-p, p = operand_cases.RESOLVES[kind] (13, value: 14), the reference keeps the unscaled ones. Every kind must then MISS the
    bound of the tests above — and wherever p >= 13 it still meets max|got - ref| <= 1e-13 max|ref|, the criterion of
    test_operand_eval.py and test_form_dispatch_gpu.py. Quadratic elements, size b, bs = gdim, both strain kernels for eps."""
    case = resolution_case(cell)
    m = build_mesh(case)
    G = m.gdim
    u = fields(case, m, G)["rough"]
    d = Device(ctx, m)
    try:
        for kind in CELL_KINDS:
            p = RESOLVES[kind]
            ref, mag = ref_operand(m, kind, G, u)
            ref64 = ref.astype(np.float64)
            for opt in strain_options(m, kind):
                with option(ctx, "operand_cell", opt):
                    got = d.operand("host", kind, G, scale_one_cell(m, u, G, p))
                ratio = worst_ratio(got, ref, mag)
                print(f"{case_id(case)} {kind} {kernel_label(m, kind, opt, True)}: ratio with cell 0 scaled by 1 + 1e-{p}: {ratio:.0f} (c = {MARGIN * C_REF[kind]:.1f})")
                assert ratio > MARGIN * C_REF[kind], (kind, opt, ratio)
                if p >= 13:
                    assert np.abs(got - ref64).max() <= 1e-13 * np.abs(ref64).max(), (kind, opt)
    finally:
        d.close()
