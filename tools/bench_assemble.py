#!/usr/bin/env python3
"""Standalone timing of dxo_bilinear_assemble and dxo_csr_create (not a bench.py leg).

    python3 tools/bench_assemble.py [tri_cells_per_side] [hex_boxes_per_side] [--out FILE]

Legs, all in one process (distorted meshes):
  p2_apply                dxo_bilinear_apply("grad", "grad", 2) on P2 triangles, ~10^7 points at 1291 cells per side (the yardstick)
  p2_assemble             dxo_bilinear_assemble of the same form on the same mesh and C
  p2_assemble_atomics     the same with option adjoint_atomics = 1
  p1_heat_assemble        ("grad", "value_grad", 1) on P1 triangles of the same size, C [n][2][3]
  q2hex_assemble          ("grad", "grad", 3) on Q2 hexahedra (default 40^3 boxes: ~2.4 GB of values)
and the pattern build of each mesh (`pattern_ms`, host C++, timed by the library). Every call is timed with HIP events on the launch
stream (median of back-to-back launches after a warm-up, tools/bench_secondary._time); option consumer_overwrite = 1. `model_GB` is the
traffic model of DESIGN.md §9.2 (C read, element matrices written and read, values read and written, pattern arrays read).
Prints one JSON line.
"""
from __future__ import annotations

import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def traffic_model(m, bs, DT, DR, nnz) -> float:
    """bytes of one default assembly: C once, element matrices written + read, values read + written once (chains in cache),
    pos table and incidences read, column indices not touched."""
    nc, nd, nq = m.num_cells, m.dofmap.shape[1], m.nq
    C = nc * nq * DT * DR * 8
    ae = nc * (nd * bs) ** 2 * 8
    return (C + 2 * ae + 2 * nnz * 8 + nc * nd * nd * 2 + nc * nd * 4 + m.x.nbytes + m.geom_dofmap.nbytes) / 1e9


def main(n_side: int = 1291, n_hex: int = 40, launches: int = 10) -> dict:
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
    res = {"tri_cells_per_side": n_side, "hex_boxes_per_side": n_hex, "legs": {}}

    def leg(name, fn, model_GB=None):
        with torch.cuda.stream(stream):
            med, mean = _time(torch, stream, fn, launches)
        r = {"ms": round(med, 4), "mean_ms": round(mean, 4)}
        if model_GB is not None:
            r["model_GB"] = round(model_GB, 3)
            r["model_GBs"] = round(model_GB / (med * 1e-3), 1)
        res["legs"][name] = r

    cases = [("triangle", (n_side, n_side), 2, "grad", "grad", 2), ("triangle", (n_side, n_side), 1, "grad", "value_grad", 1),
             ("hexahedron", (n_hex, n_hex, n_hex), 2, "grad", "grad", 3)]
    for cell, n, degree, test, trial, bs in cases:
        m = structured_mesh(cell, n, degree, distort=0.2, seed=0)
        dm = DeviceMesh.from_synthetic(m, ctx=ctx)
        G = m.gdim
        DT = bs * G
        DR = bs * (1 + G) if trial == "value_grad" else bs * G
        npts, nn = m.num_cells * m.nq, m.node_x.shape[0]
        tag = {("triangle", 2): "p2", ("triangle", 1): "p1_heat", ("hexahedron", 2): "q2hex"}[(cell, degree)]
        try:
            pat = dm.csr_pattern(bs)
            res[f"{tag}_points"], res[f"{tag}_nnz"], res[f"{tag}_pattern_ms"] = npts, pat.nnz, round(pat.build_ms, 1)
            with torch.cuda.stream(stream):
                Cd = torch.randn(npts * DT * DR, generator=gen, device=dev, dtype=torch.float64)
                values = torch.zeros(pat.nnz, device=dev, dtype=torch.float64)
                model = traffic_model(m, bs, DT, DR, pat.nnz)
                leg(f"{tag}_assemble", lambda: dm.bilinear_assemble(test, trial, bs, Cd.data_ptr(), pat, values=values), model)
                if tag == "p2":
                    v = torch.randn(nn * bs, generator=gen, device=dev, dtype=torch.float64)
                    out = torch.zeros(nn * bs, device=dev, dtype=torch.float64)
                    leg("p2_apply", lambda: dm.bilinear_apply(test, trial, bs, Cd.data_ptr(), v.data_ptr(), out.data_ptr()))
                    ctx.set_option("adjoint_atomics", 1)
                    try:
                        leg("p2_assemble_atomics", lambda: dm.bilinear_assemble(test, trial, bs, Cd.data_ptr(), pat, values=values))
                    finally:
                        ctx.set_option("adjoint_atomics", 0)
                    res["p2_assemble_over_apply"] = round(res["legs"]["p2_assemble"]["ms"] / res["legs"]["p2_apply"]["ms"], 2)
                del Cd, values
            stream.synchronize()
        finally:
            dm.close()
            torch.cuda.empty_cache()
    ctx.close()
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    out_file = None
    if "--out" in args:
        i = args.index("--out")
        out_file = args[i + 1]
        del args[i:i + 2]
    r = main(*(int(a) for a in args[:2]))
    line = json.dumps(r)
    print(line)
    if out_file:
        pathlib.Path(out_file).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(out_file).write_text(line + "\n")
