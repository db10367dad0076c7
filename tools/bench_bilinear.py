#!/usr/bin/env python3
"""Standalone timing of dxo_bilinear_apply / dxo_bilinear_diagonal (not a bench.py leg).

    python3 tools/bench_bilinear.py [cells_per_side] [--out FILE]

Legs, all in one process on the same meshes (distorted unit square, ~10^7 points at the default 1291 cells per side, 3-point rule):
  tangent_apply          dxo_tangent_apply on P2 triangles, C_tang [n][4][4]             (the yardstick: same bytes per point)
  bilinear_grad_grad     dxo_bilinear_apply("grad", "grad", 2) on the same mesh and the same 16 doubles per point
  bilinear_grad_grad_diag  its diagonal
  bilinear_heat_p1       dxo_bilinear_apply("grad", "value_grad", 1) on P1 triangles, C [n][2][3]
Every call is timed with HIP events on the launch stream (median of back-to-back launches after a warm-up, tools/bench_secondary._time);
option consumer_overwrite = 1, as a Krylov matvec would run. Prints one JSON line.
"""
from __future__ import annotations

import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def _hbm_gbs(nbytes, ms):
    return nbytes / (ms * 1e-3) / 1e9


def main(n_side: int = 1291, launches: int = 50) -> dict:
    import torch

    from dolfinx_external_operator_amd import Context, DeviceMesh
    from tools.bench_secondary import _time
    from tools.synthetic import structured_mesh

    ctx = Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_option("consumer_overwrite", 1)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    res = {"cells_per_side": n_side, "legs": {}}

    def leg(name, fn, nbytes):
        with torch.cuda.stream(stream):
            med, mean = _time(torch, stream, fn, launches)
        res["legs"][name] = {"ms": round(med, 4), "mean_ms": round(mean, 4), "hbm_GBs": round(_hbm_gbs(nbytes, med), 1)}

    for degree in (2, 1):
        m = structured_mesh("triangle", (n_side, n_side), degree, distort=0.2, seed=0)
        dm = DeviceMesh.from_synthetic(m, ctx=ctx)
        npts, nn = m.num_cells * m.nq, m.node_x.shape[0]
        geo = m.x.nbytes + m.geom_dofmap.nbytes + m.dofmap.nbytes
        res[f"p{degree}_points"] = npts
        try:
            with torch.cuda.stream(stream):
                if degree == 2:
                    Cd = torch.randn(npts * 16, generator=gen, device=dev, dtype=torch.float64)
                    v = torch.randn(nn * 2, generator=gen, device=dev, dtype=torch.float64)
                    out = torch.zeros(nn * 2, device=dev, dtype=torch.float64)
                    nbytes = Cd.numel() * 8 + geo + 2 * v.numel() * 8
                    leg("tangent_apply", lambda: dm.tangent_apply(Cd.data_ptr(), v.data_ptr(), out.data_ptr()), nbytes)
                    leg("bilinear_grad_grad", lambda: dm.bilinear_apply("grad", "grad", 2, Cd.data_ptr(), v.data_ptr(), out.data_ptr()), nbytes)
                    leg("bilinear_grad_grad_diag", lambda: dm.bilinear_diagonal("grad", "grad", 2, Cd.data_ptr(), out.data_ptr()),
                        nbytes - v.numel() * 8)
                    res["grad_grad_over_tangent_apply"] = round(res["legs"]["bilinear_grad_grad"]["ms"] / res["legs"]["tangent_apply"]["ms"], 3)
                else:
                    Cd = torch.randn(npts * 6, generator=gen, device=dev, dtype=torch.float64)
                    v = torch.randn(nn, generator=gen, device=dev, dtype=torch.float64)
                    out = torch.zeros(nn, device=dev, dtype=torch.float64)
                    leg("bilinear_heat_p1", lambda: dm.bilinear_apply("grad", "value_grad", 1, Cd.data_ptr(), v.data_ptr(), out.data_ptr()),
                        Cd.numel() * 8 + geo + 2 * v.numel() * 8)
            stream.synchronize()
        finally:
            dm.close()
    ctx.close()
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    out_file = None
    if "--out" in args:
        i = args.index("--out")
        out_file = args[i + 1]
        del args[i:i + 2]
    r = main(int(args[0]) if args else 1291)
    line = json.dumps(r)
    print(line)
    if out_file:
        pathlib.Path(out_file).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(out_file).write_text(line + "\n")
