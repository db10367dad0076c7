"""The persistent element kernels past the first trip of their wave-group loop (trip_cases.py says what a trip is): every kernel family
on meshes of 147 to 5400 cells with the option wave_group_blocks = 8 (every wave takes two to four groups: the steady state of the
register pipelines, the fence that ends a trip, a look-ahead past the end of the slice beside groups still in flight), 16 (two
trips) and 0 (the default grid, one trip), each call against the reference of the family's small-mesh test — and never one HIP result
against another, except for the bits: the three calls must agree bit for bit wherever no atomics are involved, because a cell's
element vector does not depend on which wave forms it and node_sum adds a node's entries in a fixed order.

Bounds: trip_cases.py. Long-double references: |got[k] - ref[k]| <= MARGIN * C_REF_TRIP * 2^-53 * mag[k] (+ extra[k]) for EVERY entry;
float64 oracles: the figure of the kernel's small-mesh test, of max |ref|. Every `out` is prefilled and has 64 sentinels behind it.
The ratios are reported apart for the cells (points, dofs) of first trips and of later trips at wave_group_blocks = 8, so that a
failure says which part of the loop is wrong; what an MI355X shows is in profiles/trip_ratios.txt (written when DXO_TRIP_RATIOS names
a file)."""
import os

import numpy as np
import pytest

import hyper3_cases as H3
import hyper3_reference_cases as RC
import trip_cases as T
from consumer_cases import element_name
from oracle.consumer_reference import LD
from oracle.operand_reference import value_size
from test_consumer_reference_gpu import DEFAULTS, OTHER_RULE_OUTCOMES, option_sets, ratio_to_reference

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, -7.25
EPS53 = LD(2.0) ** -53


def record(line):
    print(line)
    path = os.environ.get("DXO_TRIP_RATIOS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


class Bench:
    """One DeviceMesh on the context's stream; uploads kept for the life of the test; guarded outputs."""

    def __init__(self, ctx, name):
        import torch

        from dolfinx_external_operator_amd import DeviceMesh

        self.torch, self.ctx, self.name, self.m = torch, ctx, name, T.mesh(name)
        self.dev = torch.device("cuda", ctx.device)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        assert ctx.get_option("wave_group_blocks") == 0
        self.dm = DeviceMesh.from_synthetic(self.m, ctx=ctx)

    def close(self):
        self.ctx.set_option("wave_group_blocks", 0)
        self.dm.close()

    def up(self, a, dtype=np.float64):
        t = self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).reshape(-1)).to(self.dev)
        assert t.data_ptr() % 16 == 0
        return t

    def guarded(self, prefill):
        """a device buffer holding `prefill` (an array, or (n, value)) with GUARD sentinels behind it"""
        if isinstance(prefill, tuple):
            prefill = np.full(prefill[0], prefill[1])
        return self.up(np.concatenate([np.asarray(prefill, dtype=np.float64).reshape(-1), np.full(GUARD, SENTINEL)]))

    def fetch(self, buf, n, written=False):
        self.torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[n:], np.full(GUARD, SENTINEL)), "the call wrote behind out"
        if written:
            assert not np.any(got[:n] == SENTINEL), f"{int(np.sum(got[:n] == SENTINEL))} entries of out were not written"
        return got[:n]

    def at_every_option(self, run, bits=True, what=""):
        """{option: run()} for wave_group_blocks = 8, 16, 0; with `bits` the three results must be identical (a refusal — a str — too)"""
        out = {}
        for blocks in T.OPTIONS:
            self.ctx.set_option("wave_group_blocks", blocks)
            assert self.ctx.get_option("wave_group_blocks") == blocks
            out[blocks] = run()
        self.ctx.set_option("wave_group_blocks", 0)
        if bits:
            for blocks in T.OPTIONS[1:]:
                a, b = out[T.OPTIONS[0]], out[blocks]
                same = a == b if isinstance(a, str) or isinstance(b, str) else all(np.array_equal(x, y, equal_nan=True) for x, y in zip(_tuple(a), _tuple(b)))
                assert same, f"{self.name} {what}: wave_group_blocks = {blocks} gave other bits than {T.OPTIONS[0]}"
        return out


def _tuple(a):
    return a if isinstance(a, tuple) else (a,)


# The calls that refuse for the LDS budget, observed on the MI355X and asserted, as OTHER_RULE_OUTCOMES of
# tests/test_consumer_reference_gpu.py does, so that a served shape that turns into a refused one (or back) is noticed. Q2 hexahedra
# under the 27-point rule: the tables take 28 KB and the array forms stage tangent rows beside them (there: 66.1 and 67.6 KB of 64).
# One-point rules: a wave holds the dofs and vertices of 64 cells.
_ARRAY_FORMS = [("consumer", f"{entry} [atomics={a}]") for entry in T.CONSUMER_ENTRIES for a in (0, 1)] + \
               [("force through a list", f"atomics={a}") for a in (0, 1)] + [("von_mises_field", "von_mises_residual")] + \
               [("bilinear", f"{entry} {pair} bs=3") for entry, pair in (("apply", "(eps, eps)"), ("diagonal", "(eps, eps)"), ("diagonal", "(grad, grad)"))]
LDS_REFUSED = {"Q2 hexahedra (7,7,3), gauss 3": _ARRAY_FORMS,
               "P1 tetrahedra (10,10,9), 1 point": _ARRAY_FORMS + [("bilinear", "apply (grad, grad) bs=3")]}


class Refusals:
    """what a test saw refuse, compared with LDS_REFUSED[name] at its end"""

    def __init__(self, name, family):
        self.name, self.family, self.seen, self.served = name, family, set(), set()

    def refused(self, label, got):
        """got: {blocks: result or "lds"}; all three calls must answer alike"""
        outcomes = {"lds" if isinstance(g, str) else "ok" for g in got.values()}
        assert len(outcomes) == 1, f"{self.name} {label}: {outcomes} under the three grids"
        (self.seen if outcomes == {"lds"} else self.served).add(label)
        return outcomes == {"lds"}

    def check(self):
        expected = {label for family, label in LDS_REFUSED.get(self.name, ()) if family == self.family}
        assert self.seen == expected, f"{self.name} {self.family}: refused {sorted(self.seen)}, expected {sorted(expected)}; served {sorted(self.served)}"


@pytest.fixture
def bench(ctx):
    made = []

    def make(name):
        made.append(Bench(ctx, name))
        return made[-1]

    yield make
    for b in made:
        b.close()


def split(per_cell_ratio, later):
    """(worst over the first-trip cells, worst over the later-trip cells)"""
    r = np.asarray(per_cell_ratio, dtype=np.float64)
    return float(r[~later].max(initial=0.0)), float(r[later].max(initial=0.0))


def componentwise(got, ref, mag, cells):
    """per cell: max_k |got - ref| / (2^-53 mag) over the cell's entries; an entry with mag = 0 must be exact"""
    err = np.abs(np.asarray(got, dtype=LD).reshape(ref.shape) - ref)
    assert np.all(err[mag == 0] == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(mag > 0, err / (EPS53 * mag), 0)
    return ratio.reshape(cells, -1).max(axis=1).astype(np.float64)


def dof_split(m, bs, later):
    """(nn * bs,) bool: the dofs a later-trip cell touches"""
    nn = m.node_x.shape[0]
    hit = np.zeros(nn, dtype=bool)
    hit[np.unique(m.dofmap[later])] = True
    return np.repeat(hit, bs)


def judge(name, entry, label, first, later, c, unit):
    same = len(set(first)) == 1 and len(set(later)) == 1          # one line per (mesh, entry, option set); the three grids side by side
    fmt = lambda r: f"{r[0]:.3g}" if same else "/".join(f"{x:.3g}" for x in r)          # noqa: E731
    record(f"{name:36s} {entry:22s} {label:30s} first trips {fmt(first):>20s}  later trips {fmt(later):>20s}   "
           f"({'8 = 16 = 0' if same else '8 / 16 / 0'}; allowed {c:.4g} {unit})")
    for blocks, a, b in zip(T.OPTIONS, first, later):
        assert a <= c, f"{name} {entry} [{label}] wave_group_blocks = {blocks}: FIRST-trip cells at {a:.3g}, allowed {c:.4g} {unit}"
        assert b <= c, f"{name} {entry} [{label}] wave_group_blocks = {blocks}: LATER-trip cells at {b:.3g}, allowed {c:.4g} {unit}"


def test_the_option_takes_0_to_65535_and_is_0_by_default(ctx):
    assert ctx.get_option("wave_group_blocks") == 0
    try:
        for value in (1, 8, 65535):
            ctx.set_option("wave_group_blocks", value)
            assert ctx.get_option("wave_group_blocks") == value
        for value in (-1, 65536):
            with pytest.raises(ValueError):
                ctx.set_option("wave_group_blocks", value)
            assert ctx.get_option("wave_group_blocks") == 65535
    finally:
        ctx.set_option("wave_group_blocks", 0)


# ------------------------------------------------------------------------------------------------ operand.hip, operand_cell.h
def _operand_family(bench, name, entries, operand_cell, cells, cpw, label):
    b = bench(name)
    m, ctx = b.m, b.ctx
    G, nc = m.gdim, m.num_cells
    later = T.later_trip_mask(m, 8, cpw)
    cells_t = None if cells is None else b.up(cells, np.int32)
    saved = ctx.get_option("operand_cell")
    try:
        ctx.set_option("operand_cell", operand_cell)
        for kind, bs in entries:
            ref, mag = T.operand_reference(name, kind, bs)
            if cells is not None:
                ref, mag = ref[cells], mag[cells]
            n = nc * m.nq * value_size(kind, bs, G)
            u = b.up(T.operand_field(name, bs))

            def run():
                out = b.guarded((n, SENTINEL))
                b.dm.evaluate_device(kind, bs, u.data_ptr(), nc, out.data_ptr(), None if cells_t is None else cells_t.data_ptr())
                return b.fetch(out, n, written=True)

            got = b.at_every_option(run, what=f"{kind} bs={bs}")
            ratios = [split(componentwise(got[blocks], ref, mag, nc), later) for blocks in T.OPTIONS]
            judge(name, f"{kind} bs={bs}", label, [r[0] for r in ratios], [r[1] for r in ratios], T.MARGIN * T.C_REF_TRIP[kind][0], "* 2^-53 mag")
    finally:
        ctx.set_option("operand_cell", saved)


@pytest.mark.parametrize("name", T.WAVE_GROUP)
def test_operand_eval_on_later_trips(bench, name):
    """csrc/operand.hip operand_eval over all cells: value, grad, eps, F, value_grad, C, I1, det F at bs = gdim and value, grad,
    value_grad at bs = 1, with operand_cell = 0 so that eps takes this kernel on the 2-D meshes too. The register pipeline
    (pipe_load_values / pipe_load_indices inside the loop) on ten meshes; on the one-point tetrahedra operand_can_pipe is false and
    the loop gathers for itself. Reference: oracle.operand_reference.ref_operand (long double)."""
    _operand_family(bench, name, T.operand_entries(name), 0, None, None, "all cells")


@pytest.mark.parametrize("name", T.WAVE_GROUP)
def test_operand_eval_through_a_permuted_cell_list(bench, name):
    """The same entries through a cell list, all cells in a seeded permutation: a list turns the pipeline off (operand_point gathers
    through cells[]), and a wave's group is a run of LIST positions."""
    m = T.mesh(name)
    perm = np.random.Generator(np.random.PCG64(T.seed_of(name) + 3)).permutation(m.num_cells).astype(np.int32)
    assert not np.array_equal(perm, np.arange(m.num_cells))
    _operand_family(bench, name, T.operand_entries(name), 0, perm, None, "permuted list")


@pytest.mark.parametrize("name", T.LANE_CELL)
def test_operand_cell_eps_on_later_trips(bench, name):
    """csrc/operand_cell.h operand_cell_eps (option operand_cell = 1, the default): a wave group is 64 cells, the strains of a group
    are staged in the wave's LDS slice and the fence at the end of a trip lets the next group overwrite it. P2 triangles (50,47) and —
    the Q2 quadrilaterals of the other tests have 19 such groups, one trip — Q2 quadrilaterals (69,68), 74 groups each."""
    m = T.mesh(name)
    assert (m.gdim, m.dofmap.shape[1], m.nq, m.geom_dofmap.shape[1]) in {(2, 6, 3, 3), (2, 9, 4, 4)}      # DXO_OPERAND_CELL_CASES
    _operand_family(bench, name, [("eps", 2)], 1, None, 64, "lane = cell")


# ------------------------------------------------------------------------------------------------ adjoint.hip
def _consumer_calls(b, x):
    from dolfinx_external_operator_amd import VmParams

    G = b.m.gdim
    prm = VmParams(T.VM.E, T.VM.nu, T.VM.sigma_0, T.VM.H)
    C, v, S, sig, dp = b.up(x.C), b.up(x.v), b.up(x.S), b.up(x.sigma), b.up(x.dp)
    keep = (C, v, S, sig, dp, prm)
    return keep, {"apply": lambda o: b.dm.tangent_apply(C.data_ptr(), v.data_ptr(), o),
                  "diag": lambda o: b.dm.tangent_diagonal(C.data_ptr(), o),
                  "apply_vm": lambda o: b.dm.tangent_apply_vm(prm, sig.data_ptr(), dp.data_ptr(), v.data_ptr(), o),
                  "diag_vm": lambda o: b.dm.tangent_diagonal_vm(prm, sig.data_ptr(), dp.data_ptr(), o),
                  "force": lambda o: b.dm.adjoint("eps", G, S.data_ptr(), o)}


def _run_consumer(b, call, r0, n):
    """-> out after the call (it accumulates onto r0), or "lds" if the library refused for the LDS budget and left out alone"""
    buf = b.guarded(r0)
    try:
        call(buf.data_ptr())
    except ValueError as e:
        if "LDS budget" not in str(e):
            raise
        assert np.array_equal(b.fetch(buf, n), r0), "a refused call touched out"
        return "lds"
    return b.fetch(buf, n)


def _prefill(r0, ref):
    """what `out` holds before an accumulating call: consumer_cases' r0 ~ N(0, 1) times max |ref|. On these meshes a cell's
    contribution is of size h^3, and against a prefill of size 1 the bound's allowance 2^-53 |r0| — one rounding of the last addition —
    would dwarf c * 2^-53 * mag and the roundings of the atomics form, one per entry on r0's scale, would be all the test measures"""
    return np.asarray(r0) * float(np.abs(ref).max())


def _judge_consumer(b, name, entry, label, got, ref, mag, r0, later_dofs):
    c = T.MARGIN * T.C_REF_TRIP[entry][0]
    first = [ratio_to_reference(got[blocks], ref, mag, r0, keep=~later_dofs) for blocks in T.OPTIONS]
    later = [ratio_to_reference(got[blocks], ref, mag, r0, keep=later_dofs) for blocks in T.OPTIONS]
    judge(name, entry, label, first, later, c, "* 2^-53 mag")


@pytest.mark.parametrize("name", T.WAVE_GROUP)
def test_consumer_forms_on_later_trips(bench, name):
    """csrc/adjoint.hip: tangent_apply, tangent_diagonal, their state-based forms and the internal force adjoint("eps") under every
    option set of tests/test_consumer_reference_gpu.py that changes the kernel, inputs from consumer_cases.make_inputs, out
    accumulating onto r0 max |ref| (_prefill). Reference: oracle.consumer_reference (long double). With adjoint_atomics = 1 the reference alone applies.
    Q2 hexahedra under the 27-point rule: the array forms refuse for the LDS budget, asserted as OTHER_RULE_OUTCOMES does."""
    b = bench(name)
    m, ctx, case = b.m, b.ctx, T.CASES[name]
    x = T.consumer_inputs(name)
    n = m.node_x.shape[0] * m.gdim
    later_dofs = dof_split(m, m.gdim, T.later_trip_mask(m, 8))
    keep, calls = _consumer_calls(b, x)
    saved = {k: ctx.get_option(k) for k in DEFAULTS}
    assert saved == DEFAULTS and ctx.get_option("consumer_overwrite") == 0
    seen = Refusals(name, "consumer")
    try:
        for entry in T.CONSUMER_ENTRIES:
            ref, mag = T.consumer_reference(name, entry)
            r0 = _prefill(x.r0, ref)
            for opts, label in option_sets(case, entry):
                for k, val in opts.items():
                    ctx.set_option(k, val)
                got = b.at_every_option(lambda: _run_consumer(b, calls[entry], r0, n), bits=not opts["adjoint_atomics"], what=f"{entry} [{label}]")
                if not seen.refused(f"{entry} [{label}]", got):
                    _judge_consumer(b, name, entry, label, got, ref, mag, r0, later_dofs)
        seen.check()
        if case[3] == 3:          # the same answer as on the small meshes of that element
            small = OTHER_RULE_OUTCOMES[element_name(case)]
            assert {label.split(" [")[0] for label in seen.seen} == {e for e, o in small.items() if o == "lds"}
    finally:
        for k, val in saved.items():
            ctx.set_option(k, val)


@pytest.mark.parametrize("name", T.WAVE_GROUP)
def test_internal_force_through_a_permuted_cell_list(bench, name):
    """adjoint("eps") with cells_ptr: all cells in a seeded permutation, S in list order. The sum is the full mesh's, so the reference
    is ref_adjoint_eps of the unpermuted S; a wave's groups are runs of list positions. No bit test here: with a cell list
    two_pass_buffer (csrc/adjoint.hip) returns no element-vector buffer — "nullptr when the call has to use atomics" — so the entries
    of a node meet in fp64 atomics in the order the waves arrive, under either value of adjoint_atomics; the reference alone applies."""
    b = bench(name)
    m, ctx, case = b.m, b.ctx, T.CASES[name]
    x = T.consumer_inputs(name)
    G, nc = m.gdim, m.num_cells
    n = m.node_x.shape[0] * G
    perm = np.random.Generator(np.random.PCG64(T.seed_of(name) + 5)).permutation(nc).astype(np.int32)
    later_dofs = dof_split(m, G, np.isin(np.arange(nc), perm[T.later_trip_mask(m, 8)]))
    S, cells = b.up(x.S[perm]), b.up(perm, np.int32)
    ref, mag = T.consumer_reference(name, "force")
    r0 = _prefill(x.r0, ref)
    seen = Refusals(name, "force through a list")
    saved = ctx.get_option("adjoint_atomics")
    try:
        for atomics in (0, 1):
            ctx.set_option("adjoint_atomics", atomics)
            call = lambda o: b.dm.adjoint("eps", G, S.data_ptr(), o, n_cells=nc, cells_ptr=cells.data_ptr())          # noqa: E731
            got = b.at_every_option(lambda: _run_consumer(b, call, r0, n), bits=False)
            if not seen.refused(f"atomics={atomics}", got):
                _judge_consumer(b, name, "force", f"permuted list, atomics={atomics}", got, ref, mag, r0, later_dofs)
        seen.check()
    finally:
        ctx.set_option("adjoint_atomics", saved)


# ------------------------------------------------------------------------------------------------ hyper3.hip
@pytest.mark.parametrize("name", T.HYPER3_FIELD)
def test_isihara3_field_on_later_trips(bench, name):
    """csrc/hyper3.hip isihara3_field (P and dP from the dof vector, staged per group in the wave's LDS region) on the three quadratic
    3-D meshes and the P1 tetrahedra. Reference: hyper3_reference_cases.fused_reference (long double) with its allowance `extra`
    for the float64 rounding of F."""
    from dolfinx_external_operator_amd import MEM_DEVICE, IsiharaParams

    b = bench(name)
    m, ctx = b.m, b.ctx
    u, P, dP, mP, mdP, eP, edP = RC.fused_reference("isihara3", name)
    assert np.array_equal(u, T.hyper3_field_u(name))
    npts = m.num_cells * m.nq
    later = T.later_trip_mask(m, 8)
    ud, prm = b.up(u), IsiharaParams(*H3.DEFAULTS)

    def run():
        tP, tdP = b.guarded((npts * 9, SENTINEL)), b.guarded((npts * 81, SENTINEL))
        ctx.isihara3_field(prm, b.dm._h, MEM_DEVICE, ud.data_ptr(), tdP.data_ptr(), tP.data_ptr())
        return b.fetch(tP, npts * 9, written=True), b.fetch(tdP, npts * 81, written=True)

    got = b.at_every_option(run, what="isihara3_field")
    for k, (key, ref, mag, extra) in enumerate((("P", P, mP, eP), ("dP", dP, mdP, edP))):
        ref, mag, extra = (np.asarray(a).reshape(npts, -1) for a in (ref, mag, extra))
        bound = LD(T.hyper3_c(key)) * EPS53 * mag + extra
        assert np.all(bound > 0)
        ratios = []
        for blocks in T.OPTIONS:
            err = np.abs(np.asarray(got[blocks][k], dtype=LD).reshape(ref.shape) - ref)
            ratios.append(split((err / bound).reshape(m.num_cells, -1).max(axis=1), later))
        judge(name, f"isihara3_field {key}", f"c = {T.hyper3_c(key):.1f}", [r[0] for r in ratios], [r[1] for r in ratios], 1.0, "of the bound")


# ------------------------------------------------------------------------------------------------ bilinear.h
def _max_rel(got, ref, keep):
    return float(np.abs(got - ref)[keep].max(initial=0.0) / np.abs(ref).max())


@pytest.mark.parametrize("name", T.WAVE_GROUP)
def test_bilinear_forms_on_later_trips(bench, name):
    """csrc/bilinear.h bilinear_apply / bilinear_diagonal for (grad, grad) at bs = gdim and bs = 1, (eps, eps) and (value, value), a
    random block C per point. Reference: oracle.form_oracle (float64), 1e-12 of max |ref| as tests/test_bilinear_gpu.py."""
    b = bench(name)
    m = b.m
    nn = m.node_x.shape[0]
    later = T.later_trip_mask(m, 8)
    pairs = range(len(T.BILINEAR_PAIRS))
    diags = T.in_threads(lambda pair: T.bilinear_diagonal(name, pair), list(pairs))
    seen = Refusals(name, "bilinear")
    for pair in pairs:
        test, trial, _ = T.BILINEAR_PAIRS[pair]
        bs, Cb, v, Kv = T.bilinear_case(name, pair)
        n = nn * bs
        later_dofs = dof_split(m, bs, later)
        Cd, vd = b.up(Cb), b.up(v)
        r0 = np.random.Generator(np.random.PCG64(T.seed_of(name) + 17 + pair)).normal(size=n) * np.abs(Kv).max()
        calls = {"apply": (lambda o: b.dm.bilinear_apply(test, trial, bs, Cd.data_ptr(), vd.data_ptr(), o), Kv),
                 "diagonal": (lambda o: b.dm.bilinear_diagonal(test, trial, bs, Cd.data_ptr(), o), diags[pair])}
        for entry, (call, ref) in calls.items():
            prefill = r0 * (np.abs(ref).max() / np.abs(Kv).max())
            got = b.at_every_option(lambda: _run_consumer(b, call, prefill, n), what=f"bilinear_{entry} ({test}, {trial}) bs={bs}")
            if not seen.refused(f"{entry} ({test}, {trial}) bs={bs}", got):
                # out = prefill + K v in one addition per dof: the rounding of that addition, 2^-53 |prefill + ref|, beside the bound
                first, lat = [], []
                for blocks in T.OPTIONS:
                    d = np.maximum(np.abs(got[blocks] - (prefill + ref)) - 2.0 ** -53 * np.abs(prefill + ref), 0.0)
                    first.append(float(d[~later_dofs].max(initial=0.0) / np.abs(ref).max()))
                    lat.append(float(d[later_dofs].max(initial=0.0) / np.abs(ref).max()))
                judge(name, f"bilinear_{entry}", f"({test}, {trial}) bs={bs}", first, lat, T.TOL_BILINEAR, "max |ref|")
    seen.check()


# ------------------------------------------------------------------------------------------------ hyper3_form.h
@pytest.mark.parametrize("name", T.HYPER3)
def test_array_free_hyperelastic_forms_on_later_trips(bench, name):
    """csrc/hyper3_form.h: residual, tangent action and diagonal of the analytic model from the dof vector alone (isihara3_form<true>
    hands its pipeline over between trips: pf.un = nx.un, the reload of pv, the second look-ahead through nx; isihara3_form_diag parks
    matrices that the next group's gather overwrites). Reference as tests/test_hyper3_mf_gpu.case (float64), 1e-12 of max |ref|."""
    from dolfinx_external_operator_amd import IsiharaParams

    b = bench(name)
    m = b.m
    ref = T.hyper3_mf_case(name)
    assert ref["det_min"] > 0.2, ref["det_min"]
    n = m.node_x.shape[0] * 3
    later_dofs = dof_split(m, 3, T.later_trip_mask(m, 8))
    u, v, prm = b.up(ref["u"]), b.up(ref["v"]), IsiharaParams(*H3.DEFAULTS)
    calls = {"R": lambda o: b.dm.isihara3_residual(prm, u.data_ptr(), o), "Kv": lambda o: b.dm.isihara3_tangent_apply(prm, u.data_ptr(), v.data_ptr(), o),
             "diag": lambda o: b.dm.isihara3_tangent_diagonal(prm, u.data_ptr(), o)}
    seen = Refusals(name, "hyper3_form")
    for key, call in calls.items():
        got = b.at_every_option(lambda: _run_consumer(b, call, np.zeros(n), n), what=key)
        if seen.refused(key, got):
            continue
        first = [_max_rel(got[blocks], ref[key], ~later_dofs) for blocks in T.OPTIONS]
        lat = [_max_rel(got[blocks], ref[key], later_dofs) for blocks in T.OPTIONS]
        judge(name, f"isihara3 {key}", f"det F >= {ref['det_min']:.2f}", first, lat, T.TOL_HYPER3_MF, "max |ref|")
    seen.check()


# ------------------------------------------------------------------------------------------------ vm_field.hip, heat_field.hip, field_ops.hip
def _judge_points(b, name, entry, label, got, refs, later, tol):
    """got: {blocks: tuple of arrays}, refs: the oracle's arrays in the same order; per array max |got - ref| / max |ref|"""
    nc = b.m.num_cells
    for k, (what, ref) in enumerate(refs.items()):
        ref = np.asarray(ref, dtype=np.float64).reshape(nc, -1)
        scale = max(float(np.abs(ref).max()), 1e-300)
        ratios = [split(np.abs(np.asarray(got[blocks][k]).reshape(nc, -1) - ref).max(axis=1) / scale, later) for blocks in T.OPTIONS]
        judge(name, f"{entry} {what}", label, [r[0] for r in ratios], [r[1] for r in ratios], tol, "max |ref|")


@pytest.mark.parametrize("name", T.WAVE_GROUP)
def test_von_mises_field_on_later_trips(bench, oracle, name):
    """csrc/vm_field.hip: the strain formed in the registers of the return-map kernel, device pointers — with the tangent, without it
    (the state-only launch has a grid of its own), and as dxo_von_mises_residual with vm_residual_fused = 1 (on Q2 hexahedra under the
    8-point rule one kernel also scatters the stress; elsewhere the field kernel and the internal force). Inputs of
    tests/test_operand_eval.py::test_fused_operand_plus_von_mises scaled to the mesh; oracle: operand oracle -> von Mises oracle
    (float64), 1e-12 of max |ref|; R: operand_adjoint of the oracle's stress."""
    from dolfinx_external_operator_amd import MEM_DEVICE, VmParams
    from oracle.form_oracle import tables
    from oracle.operand_oracle import EPS_MANDEL, operand_adjoint

    b = bench(name)
    m, ctx = b.m, b.ctx
    x = T.vm_field_case(name)
    d, G, nc = x.d, m.gdim, m.num_cells
    npts, n = nc * m.nq, m.node_x.shape[0] * m.gdim
    prm = VmParams(T.E_VM, 0.3, 250.0, T.E_VM * (T.E_VM / 100) / (T.E_VM - T.E_VM / 100))
    C_o, s_o, dp_o = oracle.von_mises(x.eps.reshape(-1, d), x.sigma_n, x.p)
    assert 0.05 < (dp_o > 0).mean() < 0.98
    R_o = np.asarray(operand_adjoint(EPS_MANDEL, G, s_o.reshape(nc, m.nq, d), m.weights, *tables(m), m.node_x.shape[0])).reshape(-1)
    later = T.later_trip_mask(m, 8)
    u, sn, p = b.up(x.u), b.up(x.sigma_n), b.up(x.p)

    def run(tangent):
        C_t = b.guarded((npts * d * d, SENTINEL)) if tangent else None
        s_t, dp_t = b.guarded((npts * d, SENTINEL)), b.guarded((npts, SENTINEL))
        b.dm.von_mises(prm, u.data_ptr(), sn.data_ptr(), p.data_ptr(), C_t.data_ptr() if tangent else None, s_t.data_ptr(), dp_t.data_ptr(), mem=MEM_DEVICE)
        out = (b.fetch(s_t, npts * d, written=True), b.fetch(dp_t, npts, written=True))
        return out + ((b.fetch(C_t, npts * d * d, written=True),) if tangent else ())

    _judge_points(b, name, "von_mises_field", "with C_tang", b.at_every_option(lambda: run(True), what="von_mises_field"),
                  {"sigma": s_o, "dp": dp_o, "C_tang": C_o}, later, T.TOL_VM_FIELD)
    _judge_points(b, name, "von_mises_field", "state only", b.at_every_option(lambda: run(False), what="von_mises_field, state only"),
                  {"sigma": s_o, "dp": dp_o}, later, T.TOL_VM_FIELD)

    def residual():
        s_t, dp_t, R_t = b.guarded((npts * d, SENTINEL)), b.guarded((npts, SENTINEL)), b.guarded(np.zeros(n))
        try:
            b.dm.von_mises_residual(prm, u.data_ptr(), sn.data_ptr(), p.data_ptr(), s_t.data_ptr(), dp_t.data_ptr(), R_t.data_ptr())
        except ValueError as e:          # the internal force behind the field kernel refuses where adjoint("eps") does
            if "LDS budget" not in str(e):
                raise
            assert not np.any(b.fetch(R_t, n)), "a refused call touched R"
            return "lds"
        return b.fetch(s_t, npts * d, written=True), b.fetch(dp_t, npts, written=True), b.fetch(R_t, n)

    saved = ctx.get_option("vm_residual_fused")
    try:
        ctx.set_option("vm_residual_fused", 1)
        got = b.at_every_option(residual, what="von_mises_residual")
    finally:
        ctx.set_option("vm_residual_fused", saved)
    seen = Refusals(name, "von_mises_field")
    refused = seen.refused("von_mises_residual", got)
    seen.check()
    if refused:
        return
    _judge_points(b, name, "von_mises_residual", "fused = 1", {k: g[:2] for k, g in got.items()}, {"sigma": s_o, "dp": dp_o}, later, T.TOL_VM_FIELD)
    later_dofs = dof_split(m, G, later)
    judge(name, "von_mises_residual R", "fused = 1", [_max_rel(got[k][2], R_o, ~later_dofs) for k in T.OPTIONS],
          [_max_rel(got[k][2], R_o, later_dofs) for k in T.OPTIONS], T.TOL_VM_FIELD, "max |ref|")


@pytest.mark.parametrize("name", T.WAVE_GROUP)
def test_heat_field_on_later_trips(bench, name):
    """csrc/heat_field.hip: T, grad T and the three heat-flux outputs in one launch, device pointers, T = 1 + x^2 + y (+ 0.3 x z) of
    tests/test_operand_eval.py::test_value_and_gradient_in_one_pass_and_fused_heat plus nodal noise so that no two cells agree;
    oracle: operand oracle -> the three formulas (float64), 1e-13 of max |ref| as there."""
    from dolfinx_external_operator_amd import MEM_DEVICE

    b = bench(name)
    m = b.m
    G, npts = m.gdim, m.num_cells * m.nq
    x = T.heat_field_case(name)
    q_o, dT_o, ds_o = T.heat_of(x.vg.reshape(-1, 1 + G), G)
    Td = b.up(x.T)

    def run():
        q, dT, ds = b.guarded((npts * G, SENTINEL)), b.guarded((npts * G, SENTINEL)), b.guarded((npts * G * G, SENTINEL))
        b.dm.heat(1.0, 1.0, Td.data_ptr(), q.data_ptr(), dT.data_ptr(), ds.data_ptr(), mem=MEM_DEVICE)
        return b.fetch(q, npts * G, written=True), b.fetch(dT, npts * G, written=True), b.fetch(ds, npts * G * G, written=True)

    _judge_points(b, name, "heat_field", "", b.at_every_option(run, what="heat_field"), {"q": q_o, "dq/dT": dT_o, "dq/dsigma": ds_o},
                  T.later_trip_mask(m, 8), T.TOL_HEAT_FIELD)


@pytest.mark.parametrize("name", [n for n in T.WAVE_GROUP if T.CASES[n][0] in ("triangle", "quadrilateral")])
def test_isihara_field_on_later_trips(bench, name):
    """csrc/field_ops.hip isihara_field (2-D): F = I + grad u in the registers of the kernel that evaluates the analytic model, P and
    dP staged in the wave's LDS region. Oracle: operand oracle -> oracle.icnn_oracle.isihara_stress_tangent (float64), 1e-12 of max
    |ref| as tests/test_icnn.py holds the point kernel to it."""
    from dolfinx_external_operator_amd import MEM_DEVICE, IsiharaParams
    from oracle.icnn_oracle import isihara_stress_tangent

    b = bench(name)
    m, ctx = b.m, b.ctx
    npts = m.num_cells * m.nq
    x = T.isihara_field_case(name)
    dP_o, P_o = isihara_stress_tangent(np.array(x.F).reshape(-1, 4), T.ISI2)
    assert np.isfinite(dP_o).all() and 0.05 < np.abs(P_o).max() < 1e3
    ud, prm = b.up(x.u), IsiharaParams(*T.ISI2)

    def run():
        tP, tdP = b.guarded((npts * 4, SENTINEL)), b.guarded((npts * 16, SENTINEL))
        ctx.isihara_field(prm, b.dm._h, MEM_DEVICE, ud.data_ptr(), tdP.data_ptr(), tP.data_ptr())
        return b.fetch(tP, npts * 4, written=True), b.fetch(tdP, npts * 16, written=True)

    _judge_points(b, name, "isihara_field", "", b.at_every_option(run, what="isihara_field"), {"P": P_o, "dP": dP_o},
                  T.later_trip_mask(m, 8), T.TOL_ISIHARA_FIELD)
