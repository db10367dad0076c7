"""The 3-D hyperelastic kernels (dxo_isihara3, dxo_icnn3_eval, dxo_isihara3_field, dxo_icnn3_field: csrc/hyper3.hip, hyper3_core.h,
icnn.hip, field_ops.hip) against the long-double closed form of oracle/hyper3_reference.py, point by point and entry by entry — and
never one HIP result against another.

Bound, for EVERY one of the 9 + 81 outputs k of EVERY point: |got[k] - ref[k]| <= MARGIN * C_REF * eps * mag[k], where mag[k] is the
reference's own sum with the absolute value of every additive term, eps = 2^-53 (2^-24 for the kernels whose network runs in float32)
and C_REF (hyper3_reference_cases.py) is what float64 NumPy loses against long double on the same points. Entries with mag = 0 must be
exact zeros; where the reference is NaN (det F <= 0 in the analytic model) the kernel must be NaN, and nowhere else. The fused calls
are held to ref = model(F_LD), F_LD from oracle/operand_reference.py, and are granted in addition the rounding of F that the operand
tests grant the operand kernels (hyper3_reference_cases.fused_reference). The ratios an MI355X shows are in
profiles/hyper3_reference_ratios.txt (written when DXO_HYPER3_RATIOS names a file)."""
import os

import numpy as np
import pytest

import hyper3_cases as H3
import hyper3_reference_cases as RC
import icnn3_cases as I3
from dolfinx_external_operator_amd import MEM_DEVICE, MEM_HOST, DeviceMesh, IsiharaParams
from test_icnn3_gpu import KERNEL_IDS, KERNELS, variant

pytestmark = pytest.mark.gpu

PRM = IsiharaParams(*H3.DEFAULTS)
PAD, SENTINEL = 8, -7.0
# name -> (model of the reference, key of C_REF, eps, precision, (icnn_variant, icnn3_store) or None)
PLAIN = {"isihara3": ("isihara3", "isihara3", RC.EPS64, None, None),
         "icnn3 fp64 network": ("icnn3", "icnn3 fp64", RC.EPS64, 1, None)}
PLAIN.update({"icnn3 " + name: ("icnn3", "icnn3 fp32", RC.EPS32, 0, kernel) for name, kernel in zip(KERNEL_IDS, KERNELS)})
FUSED = {"isihara3_field": PLAIN["isihara3"], "icnn3_field fp64 network": PLAIN["icnn3 fp64 network"],
         "icnn3_field default": ("icnn3", "icnn3 fp32", RC.EPS32, 0, None)}


def record(line):
    print(line)
    path = os.environ.get("DXO_HYPER3_RATIOS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def model(ctx):
    m = ctx.icnn_create(I3.state_dict(RC.weights()))
    yield m
    ctx.icnn_destroy(m)


class kernel_options:
    """the ctx options that select one network kernel, for a with-block; nothing to set for the analytic model and the fp64 network"""

    def __init__(self, ctx, kernel):
        self.inner = variant(ctx, *kernel) if kernel else None

    def __enter__(self):
        if self.inner:
            self.inner.__enter__()

    def __exit__(self, *exc):
        if self.inner:
            self.inner.__exit__(*exc)


def _launch(ctx, model, precision, plain_args, field_mesh, mem, inp, dP, P):
    if field_mesh is None:
        if precision is None:
            ctx.isihara3(PRM, plain_args, mem, inp, dP, P)
        else:
            ctx.icnn3_eval(model, precision, plain_args, mem, inp, dP, P)
    elif precision is None:
        ctx.isihara3_field(PRM, field_mesh, mem, inp, dP, P)
    else:
        ctx.icnn3_field(model, precision, field_mesh, mem, inp, dP, P)


def call(ctx, model, precision, mem, n, inp, field_mesh=None):
    """One call with PAD sentinels behind both outputs (and the outputs pre-filled with them): -> dP (n, 9, 9), P (n, 9). `inp` is
    F (n, 9) for a plain call and the dof vector for a fused one (field_mesh: the mesh handle)."""
    import torch

    if mem == MEM_HOST:
        dP, P = np.full(n * 81 + PAD, SENTINEL), np.full(n * 9 + PAD, SENTINEL)
        _launch(ctx, model, precision, n, field_mesh, mem, np.ascontiguousarray(inp), dP, P)
    else:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        t_in = torch.from_numpy(np.ascontiguousarray(inp)).cuda()
        t_dP = torch.full((n * 81 + PAD,), SENTINEL, dtype=torch.float64, device="cuda")
        t_P = torch.full((n * 9 + PAD,), SENTINEL, dtype=torch.float64, device="cuda")
        _launch(ctx, model, precision, n, field_mesh, mem, t_in.data_ptr(), t_dP.data_ptr(), t_P.data_ptr())
        torch.cuda.synchronize()
        dP, P = t_dP.cpu().numpy(), t_P.cpu().numpy()
    assert np.all(dP[n * 81:] == SENTINEL) and np.all(P[n * 9:] == SENTINEL), "the call wrote behind an output"
    return dP[: n * 81].reshape(n, 9, 9), P[: n * 9].reshape(n, 9)


# ------------------------------------------------------------------------------------------------------------------ plain calls
@pytest.mark.parametrize("name", list(RC.sample_sets()))
@pytest.mark.parametrize("kernel", list(PLAIN))
def test_plain_call_matches_the_long_double_reference(ctx, model, kernel, name):
    """Every sample set at n = 1, 63, 64, 65, 129 points and whole, from host arrays and from device pointers: a lone lane, a wave
    tile and its borders, two tiles and a point."""
    ref_model, key, eps, precision, options = PLAIN[kernel]
    F = RC.sample_sets()[name]
    P, dP, mP, mdP = RC.reference(ref_model, name)
    cP, cdP = RC.MARGIN * RC.C_REF[key + " P"], RC.MARGIN * RC.C_REF[key + " dP"]
    sizes = sorted({min(n or F.shape[0], F.shape[0]) for n in RC.SIZES})
    with kernel_options(ctx, options):
        for mem, mname in ((MEM_HOST, "host"), (MEM_DEVICE, "device")):
            worst = {"P": (0.0, -1, -1), "dP": (0.0, -1, -1)}
            for n in sizes:
                dPg, Pg = call(ctx, model, precision, mem, n, F[:n])
                worst["P"] = max(worst["P"], RC.worst_entry(Pg, P[:n], mP[:n], eps))
                worst["dP"] = max(worst["dP"], RC.worst_entry(dPg, dP[:n], mdP[:n], eps))
            record(f"plain  {kernel:24s} {name:36s} {mname:6s} P {worst['P'][0]:8.2f} at point {worst['P'][1]:4d} entry {worst['P'][2]:2d} (c = {cP:5.1f})"
                   f"   dP {worst['dP'][0]:8.2f} at point {worst['dP'][1]:4d} entry {worst['dP'][2]:2d} (c = {cdP:5.1f})")
            assert worst["P"][0] <= cP, (kernel, name, mname, worst["P"])
            assert worst["dP"][0] <= cdP, (kernel, name, mname, worst["dP"])


# ------------------------------------------------------------------------------------------------------------------ fused calls
def _judge_fused(got, ref, mag, extra, c, eps):
    """(fraction of the bound c * eps * mag + extra used at the worst entry, point, entry), and the same error in units of eps * mag
    alone (no allowance): what the plain calls are judged in, for the record"""
    frac = RC.worst_entry(got, ref, c * np.asarray(mag), eps, extra)
    return frac, RC.worst_entry(got, ref, mag, eps)[0]


def _share(mag, extra, c, eps):
    """the allowance's share of the bound: (median, largest) over the entries with a bound"""
    first = np.longdouble(c * eps) * mag
    keep = (first + extra) > 0
    share = (extra[keep] / (first + extra)[keep]).astype(np.float64)
    return float(np.median(share)), float(share.max())


def _fused_case(ctx, model, entry, name, chunk_cells=None):
    ref_model, key, eps, precision, _ = FUSED[entry]
    m = RC.fused_mesh(name)
    u, P, dP, mP, mdP, eP, edP = RC.fused_reference(ref_model, name)
    cP, cdP = RC.MARGIN * RC.C_REF[key + " P"], RC.MARGIN * RC.C_REF[key + " dP"]
    n = m.num_cells * m.nq
    pp, table = RC.pass_points(m)
    starts, lengths = RC.group_starts(m)
    odd = int(np.sum(starts % 2))
    sP, sdP = _share(mP, eP, cP, eps), _share(mdP, edP, cdP, eps)
    print(f"{name}: {m.num_cells} cells x {m.nq} points, {len(starts)} wave groups of {lengths[0]} points (last {lengths[-1]}), {odd} of them "
          f"start at an odd point (stress run 9 p0 and tangent run 81 p0 odd); LDS tables {table} doubles, tangent passes of pp = {pp} points; "
          f"the allowance for F is {sP[0]:.2f} (median) / {sP[1]:.2f} (largest) of the bound on P, {sdP[0]:.2f} / {sdP[1]:.2f} on dP")
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    saved = ctx.get_option("host_chunk_points")
    try:
        runs = [("host", MEM_HOST), ("device", MEM_DEVICE)]
        if chunk_cells:
            assert m.num_cells > 2 * chunk_cells
            ctx.set_option("host_chunk_points", chunk_cells * m.nq)
            runs = [(f"host, {-(-m.num_cells // chunk_cells)} chunks", MEM_HOST)]
        for mname, mem in runs:
            dPg, Pg = call(ctx, model, precision, mem, n, u, field_mesh=dm._h)
            (fP, aP), (fdP, adP) = _judge_fused(Pg, P, mP, eP, cP, eps), _judge_fused(dPg, dP, mdP, edP, cdP, eps)
            record(f"fused  {entry:24s} {name:36s} {mname:15s} pp {pp:2d} odd groups {odd:2d}/{len(starts):2d}  P {fP[0]:6.3f} of the bound at point "
                   f"{fP[1]:4d} entry {fP[2]:2d} ({aP:7.2f} eps mag, c = {cP:5.1f})   dP {fdP[0]:6.3f} at point {fdP[1]:4d} entry {fdP[2]:2d} "
                   f"({adP:7.2f} eps mag, c = {cdP:5.1f})")
            assert fP[0] <= 1.0, (entry, name, mname, fP)
            assert fdP[0] <= 1.0, (entry, name, mname, fdP)
    finally:
        ctx.set_option("host_chunk_points", saved)
        dm.close()
    return starts, lengths, pp


@pytest.mark.parametrize("name", list(RC.FUSED_MESHES))
@pytest.mark.parametrize("entry", list(FUSED))
def test_fused_call_matches_the_long_double_reference(ctx, model, entry, name):
    """dxo_isihara3_field, and dxo_icnn3_field with the default kernel and with the fp64 network, on the seven meshes of
    test_hyper3_gpu.MESHES, on five whose wave groups hold an odd number of points (55 or 63: every second group starts its stress run
    and its tangent run at an odd double, the path of hyper3_store_run with an unaligned first double) and on one whose tangent leaves
    in passes of 13 points; host arrays and device pointers."""
    m = RC.fused_mesh(name)
    starts, lengths, _ = _fused_case(ctx, model, entry, name)
    if name in RC.ODD_GROUP_MESHES:
        groups = -(-m.num_cells // (64 // m.nq))
        assert groups >= 3 and len(starts) == groups and ((64 // m.nq) * m.nq) % 2 == 1
        assert set((starts % 2).tolist()) == {0, 1}


# the network's reference of the 1584 points of the 11-point mesh takes 10 s: the analytic model alone runs it
CHUNKED = [(entry, name) for entry in FUSED for name in RC.CHUNK_MESHES if entry == "isihara3_field" or "7 points" in name]


@pytest.mark.parametrize("entry,name", CHUNKED)
def test_fused_host_call_in_three_chunks_matches_the_long_double_reference(ctx, model, entry, name):
    """144 cells with 7 (and, for the analytic model, 11) points each through the host pipeline in chunks of 64 cells (its smallest:
    64, 64 and 16 cells), every chunk a launch of its own whose wave groups alternate in parity; the same per-entry bound."""
    _fused_case(ctx, model, entry, name, chunk_cells=RC.CHUNK_CELLS)
