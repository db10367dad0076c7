"""What tests/test_trips_gpu.py stands on, checked without a GPU: the meshes of trip_cases.py send every wave of a launch with
wave_group_blocks = 8 round its loop two or three times (check_trips), the constants of its componentwise bound are what float64
itself loses against long double on these meshes (C_REF_TRIP), and the bound sees the failure the GPU tests are for — a later-trip
group computed from the data of the group its wave visited one trip earlier."""
import functools

import numpy as np
import pytest

import hyper3_cases as H3
import hyper3_reference_cases as RC
import trip_cases as T
from oracle.consumer_reference import LD, numpy_expand_tangent, ref_tangent_diagonal
from oracle.consumer_reference import worst_ratio as consumer_ratio
from oracle.operand_oracle import EPS_MANDEL, eval_operand, operand_adjoint, tangent_apply
from oracle.operand_reference import KIND_ID, ref_operand
from oracle.operand_reference import worst_ratio as operand_ratio

EPS53 = LD(2.0) ** -53


def test_every_mesh_sends_its_waves_on_three_trips():
    """check_trips(): at wave_group_blocks = 8 the replay visits each group exactly once, some wave makes three trips, two waves of one
    workgroup make different numbers of trips, the number of groups is no multiple of 8 and the last group is ragged; at 16 some wave
    makes two trips; at 0 (the grid of an MI355X) none makes more than one. And the replay itself on a walk small enough to write
    down: 21 groups, 8 workgroups — slice 3 is [7, 10) and its workgroup's waves take [7], [8], [9], []; slice 0 is [0, 2)."""
    for line in T.check_trips():
        print(line)
    w = T.walk(21, 8)
    assert [w[(3, k)] for k in range(4)] == [[7], [8], [9], []] and [w[(0, k)] for k in range(4)] == [[0], [1], [], []]
    w = T.walk(75, 8)
    assert w[(0, 0)] == [0, 4, 8] and w[(0, 1)] == [1, 5] and w[(7, 0)] == [65, 69, 73] and w[(7, 3)] == [68, 72]
    assert T.grid_blocks(75, 8) == 8 and T.grid_blocks(75, 16) == 16 and T.grid_blocks(75, 0) == 24 and T.grid_blocks(75, 3) == 8
    w = T.walk(75, 16)          # two workgroups per XCD, stride 8
    assert w[(0, 0)] == [0, 8] and w[(8, 0)] == [4] and w[(8, 3)] == [7]
    m = T.mesh("Q2 hexahedra (11,9,6)")
    later = T.later_trip_mask(m, 8)
    assert not later[:4 * 8].any() and later[4 * 8:9 * 8].all()          # slice 0 = groups 0 .. 8: the first four are first trips
    stale = T.stale_cells(m, 8)
    assert np.array_equal(stale[:32], np.arange(32)) and np.array_equal(stale[32:40], np.arange(8)) and stale[-1] == (74 - 4) * 8 + 1


@functools.lru_cache(maxsize=None)
def float64_ratios(name):
    """{key of C_REF_TRIP: worst componentwise distance of the float64 twin from the long-double reference on the mesh `name`}, in
    units of 2^-53 * mag[k]"""
    m = T.mesh(name)
    nn = m.node_x.shape[0]
    out = {}
    geo = (m.dofmap, m.geom_dofmap, m.x, m.phi, m.dphi, m.dpsi)
    for kind, bs in (T.operand_entries(name) if name in T.WAVE_GROUP else [("eps", m.gdim)]):
        ref, mag = T.operand_reference(name, kind, bs)
        out[kind] = max(out.get(kind, 0.0), operand_ratio(eval_operand(KIND_ID[kind], bs, T.operand_field(name, bs), *geo), ref, mag))
    if name in T.WAVE_GROUP:
        x = T.consumer_inputs(name)
        tabs = (m.weights,) + geo + (nn,)
        C64 = numpy_expand_tangent(x.sigma, x.dp.reshape(-1), x.d, E=T.VM.E, nu=T.VM.nu)
        twins = {"apply": lambda: tangent_apply(x.C.reshape(-1), x.v, *tabs), "force": lambda: operand_adjoint(EPS_MANDEL, m.gdim, x.S, *tabs),
                 "diag": lambda: ref_tangent_diagonal(m, x.C, dtype=np.float64)[0], "apply_vm": lambda: tangent_apply(C64.reshape(-1), x.v, *tabs),
                 "diag_vm": lambda: ref_tangent_diagonal(m, C64, dtype=np.float64)[0]}
        for entry, twin in twins.items():
            out[entry] = consumer_ratio(twin(), *T.consumer_reference(name, entry))
    if name in T.HYPER3_FIELD:
        from oracle.hyper3_reference import isihara3_ref

        F = np.asarray(T.hyper3_F64(name)).reshape(-1, 9)                 # a float64 F, as the kernels hold it
        P, dP, mP, mdP = isihara3_ref(F, H3.DEFAULTS)
        Pt, dPt, _, _ = isihara3_ref(F, H3.DEFAULTS, dtype=np.float64)
        out["isihara3 P"] = RC.worst_entry(Pt, P, mP, RC.EPS64)[0]
        out["isihara3 dP"] = RC.worst_entry(dPt, dP, mdP, RC.EPS64)[0]
    return out


def test_c_ref_trip_holds_and_is_not_loose():
    """Every figure of trip_cases.C_REF_TRIP holds on every trip mesh, is reached to within a factor four on the mesh it names, and
    that mesh is the worst. Per mesh (printed): the quadrilaterals lose the most, through J."""
    worst = {}
    for name in T.CASES:
        got = float64_ratios(name)
        print(f"{name:36s} " + " ".join(f"{k}={v:.2f}" for k, v in got.items()))
        for k, v in got.items():
            assert v <= T.C_REF_TRIP[k][0], (name, k, v)
            if v > worst.get(k, (0.0, None))[0]:
                worst[k] = (v, name)
    assert set(worst) == set(T.C_REF_TRIP)
    for k, (c, where) in T.C_REF_TRIP.items():
        print(f"{k:12s} measured {worst[k][0]:7.2f} on {worst[k][1]:36s} C_REF_TRIP {c:6.1f}")
        assert worst[k][1] == where and c <= 4.0 * worst[k][0], (k, worst[k], c)


# ------------------------------------------------------------------------------------------------ the failure the GPU tests are for
def _every_later_group_exceeds(ratio_per_cell, m, cpw, blocks, what):
    """ratio_per_cell: (num_cells,) the worst ratio error / bound over what the cell touches. Every later-trip group must hold a cell
    above 1, every first-trip cell of a per-cell output must be exact (checked by the caller)"""
    trip, _ = T.trip_of_group(-(-m.num_cells // cpw), blocks)
    group = np.arange(m.num_cells) // cpw
    for g in np.flatnonzero(trip > 0):
        assert ratio_per_cell[group == g].max() > 1.0, f"{what}: a stale group {g} stays inside the bound"
    return float(min(ratio_per_cell[group == g].max() for g in np.flatnonzero(trip > 0)))


@pytest.mark.parametrize("name", list(T.CASES))
def test_a_stale_pipeline_slot_misses_every_bound(oracle, name):
    """For every reference of the GPU file: the inputs of every later-trip group (wave_group_blocks = 8) are replaced by those of the
    group its wave visited one trip earlier — what a register pipeline that did not advance, or an LDS region read before the next
    gather landed, would deliver — the reference is evaluated on that, rounded to float64, and judged like a kernel's result. It must
    miss the bound on at least one entry of every such group, and sit exactly on the reference in the first-trip cells.
      operand kinds   the cell list of ref_operand names the stale cells (dofs and vertices of the other group);
      consumer forms  the point data (C, S, sigma, dp) of the stale cells, scattered to the true cells' dofs: judged on the dofs each
                      group touches; the same for the float64 bilinear oracle with its block C;
      isihara3_field  the pointwise model of the stale cells' F: the rows of the cached reference;
      array-free hyperelastic forms  the stale cells' F in the float64 oracle of tests/test_hyper3_mf_gpu.py;
      fused field entries  the stale cells' strain, (T, grad T) and 2-D F in the float64 oracles of the von Mises, heat and Isihara
                      kernels, the history variables (sigma_n, p) of the true cells."""
    m, cpw = T.mesh(name), T.case_cpw(name)
    src = T.stale_cells(m, 8, cpw)
    later = T.later_trip_mask(m, 8, cpw)
    assert np.array_equal(src != np.arange(m.num_cells), later) and later.sum() > m.num_cells // 3
    least = {}
    for kind, bs in (T.operand_entries(name) if name in T.WAVE_GROUP else [("eps", m.gdim)]):
        ref, mag = T.operand_reference(name, kind, bs)
        stale = np.asarray(ref_operand(m, kind, bs, T.operand_field(name, bs), cells=src)[0], dtype=np.float64)
        err = np.abs(stale.astype(LD) - ref)
        assert np.all(err[~later] <= EPS53 * mag[~later])                          # only the rounding to float64
        bound = LD(T.MARGIN * T.C_REF_TRIP[kind][0]) * EPS53 * mag
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).reshape(m.num_cells, -1).max(axis=1)
        least[f"{kind} bs={bs}"] = _every_later_group_exceeds(ratio.astype(np.float64), m, cpw, 8, f"{name} {kind} bs={bs}")
    if name in T.WAVE_GROUP:
        nn, G = m.node_x.shape[0], m.gdim
        xs = T.stale_consumer_inputs(name, 8)

        def per_cell(ratio_per_dof, bs):
            return ratio_per_dof.reshape(nn, bs)[m.dofmap].reshape(m.num_cells, -1).max(axis=1)

        for entry in T.CONSUMER_ENTRIES:
            ref, mag = T.consumer_reference(name, entry)
            stale = np.asarray(T.consumer_reference_of(m, xs, entry)[0], dtype=np.float64)
            ratio = (np.abs(stale.astype(LD) - ref) / (LD(T.MARGIN * T.C_REF_TRIP[entry][0]) * EPS53 * mag)).astype(np.float64)
            least[entry] = _every_later_group_exceeds(per_cell(ratio, G), m, cpw, 8, f"{name} {entry}")
        from oracle.form_oracle import bilinear_ref

        for pair, (test, trial, vector) in enumerate(T.BILINEAR_PAIRS):
            bs, Cb, v, Kv = T.bilinear_case(name, pair)
            stale = bilinear_ref(m, test, trial, bs, Cb.reshape(m.num_cells, m.nq, *Cb.shape[1:])[src].reshape(Cb.shape), v)
            ratio = np.abs(stale - Kv) / (T.TOL_BILINEAR * np.abs(Kv).max())
            least[f"bilinear {test},{trial} bs={bs}"] = _every_later_group_exceeds(per_cell(ratio, bs), m, cpw, 8, f"{name} bilinear {pair}")
    if name in T.HYPER3_FIELD:
        _, P, dP, mP, mdP, eP, edP = RC.fused_reference("isihara3", name)
        pts = (src[:, None] * m.nq + np.arange(m.nq)[None, :]).reshape(-1)
        for key, ref, mag, extra in (("P", P, mP, eP), ("dP", dP, mdP, edP)):
            ref, mag, extra = (np.asarray(a).reshape(len(pts), -1) for a in (ref, mag, extra))
            stale = ref[pts].astype(np.float64)
            bound = LD(T.hyper3_c(key)) * EPS53 * mag + extra
            ratio = (np.abs(stale.astype(LD) - ref) / bound).reshape(m.num_cells, -1).max(axis=1).astype(np.float64)
            assert ratio[~later].max() <= 1.0
            least[f"isihara3_field {key}"] = _every_later_group_exceeds(ratio, m, cpw, 8, f"{name} isihara3_field {key}")
    if name in T.HYPER3:
        nn = m.node_x.shape[0]
        true = T.hyper3_mf_case(name, with_diag=False)          # the diagonal is the action probed: its 81 probes add nothing here
        stale = T.hyper3_mf_of(m, np.asarray(T.hyper3_F64(name))[src].reshape(-1, 9), with_diag=False)
        for key in ("R", "Kv"):
            ratio = np.abs(stale[key] - true[key]) / (T.TOL_HYPER3_MF * np.abs(true[key]).max())
            ratio = ratio.reshape(nn, 3)[m.dofmap].reshape(m.num_cells, -1).max(axis=1)
            least[f"hyper3_form {key}"] = _every_later_group_exceeds(ratio, m, cpw, 8, f"{name} hyper3_form {key}")
    if name in T.WAVE_GROUP:
        from oracle.icnn_oracle import isihara_stress_tangent

        def pointwise(what, true, stale, tol):
            for key, a, b in zip(what, true, stale):
                a, b = (np.asarray(z, dtype=np.float64).reshape(m.num_cells, -1) for z in (a, b))
                ratio = np.abs(b - a).max(axis=1) / (tol * np.abs(a).max())
                assert ratio[~later].max() == 0.0
                least[key] = _every_later_group_exceeds(ratio, m, cpw, 8, f"{name} {key}")

        x = T.vm_field_case(name)
        vm = lambda e: oracle.von_mises(np.array(e).reshape(-1, x.d), x.sigma_n, x.p)          # noqa: E731
        pointwise(("vm C_tang", "vm sigma"), vm(x.eps)[:2], vm(x.eps[src])[:2], T.TOL_VM_FIELD)
        h = T.heat_field_case(name)
        heat = lambda vg: T.heat_of(np.array(vg).reshape(-1, 1 + m.gdim), m.gdim)                # noqa: E731
        pointwise(("heat q", "heat dq/dT"), heat(h.vg)[:2], heat(h.vg[src])[:2], T.TOL_HEAT_FIELD)
        if m.gdim == 2:
            i = T.isihara_field_case(name)
            isi = lambda F: isihara_stress_tangent(np.array(F).reshape(-1, 4), T.ISI2)          # noqa: E731
            pointwise(("isihara dP", "isihara P"), isi(i.F), isi(i.F[src]), T.TOL_ISIHARA_FIELD)
    print(name, "least miss over the later-trip groups, as a multiple of the bound:", " ".join(f"{k}: {v:.1e}" for k, v in least.items()))
