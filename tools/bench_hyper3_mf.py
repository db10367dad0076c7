#!/usr/bin/env python3
"""The array-free 3-D hyperelastic consumers against the array route, on device memory, about 10^7 quadrature points per mesh:

  Q2 hexahedra, 108 boxes per side, 8-point rule (10.08e6 points) and P2 tetrahedra, 75 boxes per side, 4-point rule (10.13e6 points)

  new route (no quadrature array)                      array route (dP [n][9][9] and P [n][9] in HBM, 720 B per point)
    residual   dxo_isihara3_residual                     field      dxo_isihara3_field
    apply      dxo_isihara3_tangent_apply                adjoint    dxo_operand_adjoint("F", 3)          residual = field + adjoint
    diagonal   dxo_isihara3_tangent_diagonal             apply      dxo_bilinear_apply("grad", "grad", 3)
                                                         diagonal   dxo_bilinear_diagonal("grad", "grad", 3)

`apply_ratio` = new apply ms / array apply ms. `newton_ratio_k50` = one Newton iteration with k = 50 Krylov steps, new over array:
(residual + diagonal + 50 apply) of each route, the array route's residual being field + adjoint. `quadrature_bytes` = what each
route keeps in HBM between the calls; `device_bytes_in_use` = the device's used memory (hipMemGetInfo) while the route's buffers
exist, the mesh, the dof vectors and the element-vector buffer of the two-pass scatter included.
Timing: consumer_overwrite = 1 (a solver's setting), warm-up, then 5 batches of 20 back-to-back launches timed with events on the
launch stream, the median batch reported (tools/bench_timing.py). Prints one JSON line.
Needs an MI355X.    python3 tools/bench_hyper3_mf.py [hex boxes per side] [tet boxes per side]
"""
from __future__ import annotations

import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main(n_hex: int = 108, n_tet: int = 75) -> dict:
    import torch

    from dolfinx_external_operator_amd import MEM_DEVICE, Context, DeviceMesh, IsiharaParams
    from tools.bench_krylov import _batches
    from tools.synthetic import structured_mesh

    ctx = Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_option("consumer_overwrite", 1)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    prm = IsiharaParams(0.5, 1.0, 1.0, 1.5)
    f64 = dict(device=dev, dtype=torch.float64)
    res = {"device": ctx.device_info()["name"], "consumer_overwrite": 1, "meshes": {}}

    def in_use():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free

    for name, cell, side in (("Q2 hexahedra, 8 points", "hexahedron", n_hex), ("P2 tetrahedra, 4 points", "tetrahedron", n_tet)):
        m = structured_mesh(cell, (side,) * 3, 2, distort=0.2, seed=0)
        dm = DeviceMesh.from_synthetic(m, ctx=ctx)
        npts, nn = m.num_cells * m.nq, m.node_x.shape[0]
        r = {"boxes_per_side": side, "cells": m.num_cells, "points": npts, "dofs": nn * 3, "legs": {}}

        def leg(route, what, fn):
            with torch.cuda.stream(stream):
                ms, per = _batches(torch, stream, fn)
            rec = {"ms": round(ms, 4), "batches_ms": [round(t, 4) for t in per], "ns_per_point": round(ms * 1e6 / npts, 4)}
            r["legs"][f"{route}.{what}"] = rec
            print(name, route, what, json.dumps(rec), file=sys.stderr, flush=True)
            return ms

        try:
            with torch.cuda.stream(stream):
                u = 1e-4 * torch.randn(nn * 3, generator=gen, **f64)      # nodes are 1 / (2 side) apart: |grad u| of a few per cent, det F > 0
                v = torch.randn(nn * 3, generator=gen, **f64)
                out = torch.zeros(nn * 3, **f64)
                up, vp, op = u.data_ptr(), v.data_ptr(), out.data_ptr()
                t = {"new.residual": leg("new", "residual", lambda: dm.isihara3_residual(prm, up, op)),
                     "new.apply": leg("new", "apply", lambda: dm.isihara3_tangent_apply(prm, up, vp, op)),
                     "new.diagonal": leg("new", "diagonal", lambda: dm.isihara3_tangent_diagonal(prm, up, op))}
                assert bool(torch.isfinite(out).all())
                used_new = in_use()
                dP, P = torch.empty(npts * 81, **f64), torch.empty(npts * 9, **f64)
                t["array.field"] = leg("array", "field", lambda: ctx.isihara3_field(prm, dm._h, MEM_DEVICE, up, dP.data_ptr(), P.data_ptr()))
                t["array.adjoint"] = leg("array", "adjoint", lambda: dm.adjoint("F", 3, P.data_ptr(), op))
                t["array.apply"] = leg("array", "apply", lambda: dm.bilinear_apply("grad", "grad", 3, dP.data_ptr(), vp, op))
                t["array.diagonal"] = leg("array", "diagonal", lambda: dm.bilinear_diagonal("grad", "grad", 3, dP.data_ptr(), op))
                assert bool(torch.isfinite(out).all())
                used_array = in_use()
            newton_new = t["new.residual"] + t["new.diagonal"] + 50 * t["new.apply"]
            newton_array = t["array.field"] + t["array.adjoint"] + t["array.diagonal"] + 50 * t["array.apply"]
            r.update(apply_ratio=round(t["new.apply"] / t["array.apply"], 3),
                     residual_ratio=round(t["new.residual"] / (t["array.field"] + t["array.adjoint"]), 3),
                     diagonal_ratio=round(t["new.diagonal"] / t["array.diagonal"], 3),
                     newton_k50_ms={"new": round(newton_new, 3), "array": round(newton_array, 3)},
                     newton_ratio_k50=round(newton_new / newton_array, 3),
                     quadrature_bytes={"new": 0, "array": (dP.numel() + P.numel()) * 8},
                     device_bytes_in_use={"new": used_new, "array": used_array})
            del dP, P
        finally:
            dm.close()
        res["meshes"][name] = r
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
