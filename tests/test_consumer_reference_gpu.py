"""The consumer side (csrc/adjoint.hip: dxo_tangent_apply[_vm], dxo_tangent_diagonal[_vm], dxo_operand_adjoint for eps) against the
long-double reference of oracle/consumer_reference.py: every instantiation tangent_apply_impl / tangent_diagonal_impl /
dxo_operand_adjoint choose between — all eight standard elements, the options that change the choice, two further quadrature rules —
on meshes of at most 252 cells, and never one HIP result against another.

Bound, for EVERY dof k: |got[k] - (r0[k] + ref[k])| <= c * 2^-53 * mag[k] + 2^-53 |r0[k]|, where r0 is what `out` held before the
call (the calls accumulate), mag[k] the same sum as ref[k] with the absolute value of every factor, and c = MARGIN * C_REF[entry]
(consumer_cases.py): 8 times what float64 NumPy itself loses against long double on these meshes. c is not tuned on the kernels; the
ratios they show are in profiles/consumer_reference_ratios.txt."""
import itertools
import os

import numpy as np
import pytest

from consumer_cases import ALL_CASES, C_REF, MARGIN, VM, build_mesh, case_id, element_name, make_inputs
from oracle.consumer_reference import LD, ref_adjoint_eps, ref_tangent_apply, ref_tangent_diagonal, vm_tangent_from_state

pytestmark = pytest.mark.gpu

ENTRIES = ("apply", "diag", "apply_vm", "diag_vm", "force")
DEFAULTS = {"adjoint_mfma": 1, "adjoint_atomics": 0, "adjoint_cell": 1}
GUARD, SENTINEL = 64, -7.25
EPS53 = LD(2.0) ** -53

# The 3-point-per-direction rules (9 points on quadrilaterals: 7 cells per wave, one idle lane; 27 on hexahedra: 2 cells per wave, ten
# idle lanes). A call either matches the reference ("ok") or refuses with the library's ValueError that names the LDS budget ("lds");
# observed on the MI355X, asserted so that a served shape that turns into a refused one (or back) is noticed. Q2 hexahedra: the tables of
# 27 nodes at 27 points take 28 KB, and with four waves' regions of 9.5 KB (the staging space of the tangent rows) the three wave-group
# kernels ask for 66.1 KB (action, internal force) and 67.6 KB (diagonal) of the 64 KB a workgroup gets.
OTHER_RULE_OUTCOMES = {
    "quadrilateral Q1 gauss3": {"apply": "ok", "diag": "ok", "apply_vm": "ok", "diag_vm": "ok", "force": "ok"},
    "quadrilateral Q2 gauss3": {"apply": "ok", "diag": "ok", "apply_vm": "ok", "diag_vm": "ok", "force": "ok"},
    "hexahedron Q1 gauss3": {"apply": "ok", "diag": "ok", "apply_vm": "ok", "diag_vm": "ok", "force": "ok"},
    "hexahedron Q2 gauss3": {"apply": "lds", "diag": "lds", "apply_vm": "lds", "diag_vm": "lds", "force": "lds"},
}


def option_axes(case, entry):
    """The options that change which kernel serves `entry` on this element (tangent_apply_impl, tangent_diagonal_impl,
    dxo_operand_adjoint). adjoint_atomics always does (one pass with fp64 atomics instead of element vectors + node sums); adjoint_mfma
    only on the elements with a matrix-pipe scatter — Q2 hexahedra in the array forms; Q1 / Q2 hexahedra, P2 triangles and P2 tetrahedra
    in the state-based forms; the hexahedra's internal force — and only with the degree-2 rules these forms are compiled for;
    adjoint_cell only in the internal force: the cross-lane form on hexahedra, the lane = cell form on the quadratic elements."""
    cell, degree, _, rule, _ = case
    axes = ["adjoint_atomics"]
    if rule is not None:
        return axes
    hexa = cell == "hexahedron"
    if entry in ("apply", "diag"):
        if hexa and degree == 2:
            axes.append("adjoint_mfma")
    elif entry in ("apply_vm", "diag_vm"):
        if hexa or (degree == 2 and cell in ("triangle", "tetrahedron")):
            axes.append("adjoint_mfma")
    elif hexa:
        axes += ["adjoint_cell", "adjoint_mfma"]
    elif degree == 2:
        axes.append("adjoint_cell")
    return axes


def option_sets(case, entry):
    axes = option_axes(case, entry)
    for values in itertools.product((0, 1), repeat=len(axes)):
        yield {**DEFAULTS, **dict(zip(axes, values))}, ",".join(f"{a[8:]}={v}" for a, v in zip(axes, values))


def ratio_to_reference(got, ref, mag, r0, keep=None):
    """max_k (|got - (r0 + ref)| - 2^-53 |r0|) / (2^-53 mag) over the dofs of `keep`; a dof with mag = 0 must hold r0 exactly."""
    err = np.abs(np.asarray(got, dtype=LD) - (np.asarray(r0, dtype=LD) + ref)) - EPS53 * np.abs(np.asarray(r0, dtype=LD))
    keep = np.ones(err.shape, dtype=bool) if keep is None else keep
    zero = keep & (mag == 0)
    assert np.array_equal(np.asarray(got)[zero], np.asarray(r0)[zero])
    nz = keep & (mag != 0)
    return float(np.max(np.maximum(err[nz], 0) / (EPS53 * mag[nz]), initial=0.0))


def record(line):
    print(line)
    path = os.environ.get("DXO_CONSUMER_RATIOS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_consumer_kernels_match_the_long_double_reference(ctx, case):
    """One DeviceMesh per (element, rule, mesh size); every entry point under every option set that changes its dispatch.
    Pinned in the same calls: accumulation into a pre-filled `out`, 64 sentinel doubles behind it untouched, identical bits from a second
    call without atomics, the internal force with S at an address that is 8 mod 16 (the hexahedra's cross-lane form then leaves the call
    to the fallback), a C_tang / sigma at such an address refused, and on size b a NaN tangent (sigma = 0 with dp > 0; the dp = -0.0
    mark) confined to the dofs of the cell that owns the point. The degree-2 rules must be served: a refusal there fails the test."""
    import torch

    from dolfinx_external_operator_amd import DeviceMesh, VmParams

    m = build_mesh(case)
    x = make_inputs(case, m)
    G, nn, d = m.gdim, m.node_x.shape[0], x.d
    n = nn * G
    must_serve = case[3] is None
    prm = VmParams(VM.E, VM.nu, VM.sigma_0, VM.H)
    Cvm, Cvm_mag = vm_tangent_from_state(VM, x.sigma, x.dp)
    refs = {"apply": ref_tangent_apply(m, x.C, x.v), "diag": ref_tangent_diagonal(m, x.C),
            "apply_vm": ref_tangent_apply(m, Cvm, x.v, C_mag=Cvm_mag), "diag_vm": ref_tangent_diagonal(m, Cvm, C_mag=Cvm_mag),
            "force": ref_adjoint_eps(m, x.S)}
    dev = torch.device("cuda", ctx.device)

    def aligned(a):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).to(dev)
        assert t.data_ptr() % 16 == 0
        return t

    def misaligned(a):          # the same values at an address that is 8 mod 16: a tensor sliced from element 1
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        t = torch.empty(a.size + 1, dtype=torch.float64, device=dev)[1:]
        t.copy_(torch.from_numpy(a))
        assert t.data_ptr() % 16 == 8
        return t

    C, v, S, sig, dp = aligned(x.C), aligned(x.v), aligned(x.S), aligned(x.sigma), aligned(x.dp)
    S8, C8, sig8 = misaligned(x.S), misaligned(x.C), misaligned(x.sigma)
    prefill = torch.cat([torch.from_numpy(x.r0), torch.full((GUARD,), SENTINEL, dtype=torch.float64)]).to(dev)
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    calls = {"apply": lambda o, C=C: dm.tangent_apply(C.data_ptr(), v.data_ptr(), o),
             "diag": lambda o, C=C: dm.tangent_diagonal(C.data_ptr(), o),
             "apply_vm": lambda o, s=sig, p=dp: dm.tangent_apply_vm(prm, s.data_ptr(), p.data_ptr(), v.data_ptr(), o),
             "diag_vm": lambda o, s=sig, p=dp: dm.tangent_diagonal_vm(prm, s.data_ptr(), p.data_ptr(), o),
             "force": lambda o, S=S: dm.adjoint("eps", G, S.data_ptr(), o)}

    def run(call):
        """-> the dof vector after the call, or "lds" if the library refused for the LDS budget; `out` starts as r0, the guard band
        behind it has to survive, and a refused call has to leave `out` alone."""
        buf = prefill.clone()
        try:
            call(buf.data_ptr())
            outcome = "ok"
        except ValueError as e:
            if "LDS budget" not in str(e):
                raise
            outcome = "lds"
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[n:], np.full(GUARD, SENTINEL)), "the call wrote behind out"
        if outcome == "lds":
            assert np.array_equal(got[:n], x.r0), "a refused call touched out"
            return outcome
        return got[:n]

    saved = {k: ctx.get_option(k) for k in DEFAULTS}
    assert saved == DEFAULTS and ctx.get_option("consumer_overwrite") == 0
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    outcomes = {}
    try:
        for entry in ENTRIES:
            c = MARGIN * C_REF[entry]
            ref, mag = refs[entry]
            variants = [("", calls[entry])]
            if entry == "force":
                variants.append(("S at 8 mod 16", lambda o: calls["force"](o, S=S8)))
            for (opts, label), (vname, call) in itertools.product(option_sets(case, entry), variants):
                for k, val in opts.items():
                    ctx.set_option(k, val)
                got = run(call)
                outcomes.setdefault(entry, set()).add("lds" if isinstance(got, str) else "ok")
                if isinstance(got, str):
                    assert not must_serve, f"{case_id(case)} {entry} [{label}]: refused for the LDS budget"
                    continue
                ratio = ratio_to_reference(got, ref, mag, x.r0)
                record(f"{case_id(case):36s} {entry:9s} {label:28s} {vname:14s} {ratio:8.2f}   (c = {c:.1f})")
                assert ratio <= c, f"{case_id(case)} {entry} [{label}] {vname}: {ratio:.2f} * 2^-53 * mag, allowed {c:.1f}"
                if not opts["adjoint_atomics"]:
                    assert np.array_equal(run(call), got), f"{entry} [{label}] {vname}: a second call gave other bits"
        for k, val in DEFAULTS.items():
            ctx.set_option(k, val)
        # a C_tang / sigma at 8 mod 16 is refused, not computed
        for entry, call in (("apply", lambda o: calls["apply"](o, C=C8)), ("diag", lambda o: calls["diag"](o, C=C8)),
                            ("apply_vm", lambda o: calls["apply_vm"](o, s=sig8)), ("diag_vm", lambda o: calls["diag_vm"](o, s=sig8))):
            if outcomes[entry] == {"ok"}:
                buf = prefill.clone()
                with pytest.raises(ValueError, match="16-byte aligned"):
                    call(buf.data_ptr())
                torch.cuda.synchronize()
                assert np.array_equal(buf.cpu().numpy()[:n], x.r0)
        if not must_serve:
            assert {e: "|".join(sorted(o)) for e, o in outcomes.items()} == OTHER_RULE_OUTCOMES[element_name(case)]
        if case[4] == "b":
            # NaN confinement: one point of a cell of the all-plastic (and ragged) second wave group gets a NaN tangent, by sigma = 0 with
            # dp > 0 (n = 0 / 0) and by the producer's mark dp = -0.0 (a = NaN). The cell's dofs are NaN, every other dof is within the bound
            cell, q = 64 // m.nq + 1, 1
            in_cell = np.zeros((nn, G), dtype=bool)
            in_cell[m.dofmap[cell]] = True
            in_cell = in_cell.reshape(-1)
            for what in ("sigma = 0, dp > 0", "dp = -0.0"):
                s_n, dp_n = x.sigma.copy(), x.dp.copy()
                if what == "dp = -0.0":
                    dp_n[cell, q] = -0.0
                else:
                    s_n[cell, q] = 0.0
                    assert dp_n[cell, q] > 0
                Cn, Cn_mag = vm_tangent_from_state(VM, s_n, dp_n)
                Cn, Cn_mag = Cn.reshape(m.num_cells, m.nq, d, d), Cn_mag.reshape(m.num_cells, m.nq, d, d)
                assert np.isnan(Cn[cell, q]).all() and np.isfinite(np.delete(Cn.reshape(-1, d, d), cell * m.nq + q, axis=0)).all()
                Cn[cell, q] = 0
                Cn_mag[cell, q] = 0
                s_t, dp_t = aligned(s_n), aligned(dp_n)
                for entry in ("apply_vm", "diag_vm"):
                    ref, mag = (ref_tangent_apply(m, Cn, x.v, C_mag=Cn_mag) if entry == "apply_vm" else ref_tangent_diagonal(m, Cn, C_mag=Cn_mag))
                    for mfma in (0, 1):
                        ctx.set_option("adjoint_mfma", mfma)
                        got = run(lambda o: calls[entry](o, s=s_t, p=dp_t))
                        assert np.array_equal(np.isnan(got), in_cell), f"{entry} mfma={mfma} ({what}): NaN on {np.flatnonzero(np.isnan(got) != in_cell)[:8]}"
                        ratio = ratio_to_reference(got, ref, mag, x.r0, keep=~in_cell)
                        record(f"{case_id(case):36s} {entry:9s} {'mfma=%d' % mfma:28s} {'NaN: ' + what:14s} {ratio:8.2f}   (c = {MARGIN * C_REF[entry]:.1f})")
                        assert ratio <= MARGIN * C_REF[entry], f"{entry} mfma={mfma} ({what}): {ratio:.2f}"
    finally:
        for k, val in saved.items():
            ctx.set_option(k, val)
        dm.close()


@pytest.mark.parametrize("cell", ["triangle", "quadrilateral", "tetrahedron", "hexahedron"])
def test_the_bound_sees_a_relative_error_of_1e_12_in_one_cell(ctx, cell):
    """What the componentwise bound resolves: the device is handed tangents (stresses) whose values in cell 0 are scaled by 1 + 1e-12,
    the reference keeps the unscaled ones. The array-form action, the diagonal and the internal force must then MISS the bound of
    the test above — and they still meet max|got - ref| <= 1e-12 max|ref|, the criterion of the older consumer tests. Quadratic
    elements, size b."""
    import torch

    from dolfinx_external_operator_amd import DeviceMesh

    case = next(c for c in ALL_CASES if c[0] == cell and c[1] == 2 and c[4] == "b")
    m = build_mesh(case)
    x = make_inputs(case, m)
    G, n = m.gdim, m.node_x.shape[0] * m.gdim
    refs = {"apply": ref_tangent_apply(m, x.C, x.v), "diag": ref_tangent_diagonal(m, x.C), "force": ref_adjoint_eps(m, x.S)}
    Cp, Sp = x.C.copy(), x.S.copy()
    Cp[0] *= 1.0 + 1e-12
    Sp[0] *= 1.0 + 1e-12
    dev = torch.device("cuda", ctx.device)
    C, S, v = (torch.from_numpy(a.reshape(-1)).to(dev) for a in (Cp, Sp, x.v))
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    calls = {"apply": lambda o: dm.tangent_apply(C.data_ptr(), v.data_ptr(), o), "diag": lambda o: dm.tangent_diagonal(C.data_ptr(), o),
             "force": lambda o: dm.adjoint("eps", G, S.data_ptr(), o)}
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for entry, call in calls.items():
            out = torch.zeros(n, dtype=torch.float64, device=dev)
            call(out.data_ptr())
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            ref, mag = refs[entry]
            ratio = ratio_to_reference(got, ref, mag, np.zeros(n))
            print(f"{case_id(case)} {entry}: ratio with cell 0 scaled by 1 + 1e-12: {ratio:.0f} (c = {MARGIN * C_REF[entry]:.1f})")
            assert ratio > MARGIN * C_REF[entry], (entry, ratio)
            assert np.abs(got - ref.astype(np.float64)).max() <= 1e-12 * np.abs(ref.astype(np.float64)).max()
    finally:
        dm.close()
