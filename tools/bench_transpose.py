#!/usr/bin/env python3
"""Standalone timing of the transposed operators (csrc/transpose.hip, dxo_bilinear_apply_t; not a bench.py leg).
    python3 tools/bench_transpose.py [tri_cells_per_side] [heat_cells_per_side] [hex_boxes_per_side] [--out FILE]
Systems (distorted meshes, random C), those of tools/bench_krylov.py:
  p2     the assembled ("grad", "grad", 2) matrix on P2 triangles (1291 per side: 10^7 points, 3.07e8 nonzeros)
  heat   the P1 heat matrix ("grad", "value_grad", 1) with Dirichlet boundary (256 per side)
  q2hex  ("eps", "eps", 3) on Q2 hexahedra (40^3 boxes): the action only
Legs per matrix: spmv (dxo_csr_spmv, the baseline), spmv_t (dxo_csr_spmv_t), transpose and transpose_inplace (dxo_csr_transpose), and
`spmv_t_over_spmv`, `transpose_plus_spmv_over_spmv_t`: above 1, a one-off transposed product is cheaper than transposing first. Per
form: apply (dxo_bilinear_apply, the baseline), apply_t (dxo_bilinear_apply_t) and `apply_t_over_apply`.
Timing: warm-up (which also builds the mirror map), then 5 batches of 20 back-to-back launches timed with HIP events on the launch
stream, the MEDIAN batch reported (tools/bench_timing.median_batch). Prints one JSON line; --out FILE writes it with a table.
"""
from __future__ import annotations

import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main(n_side: int = 1291, n_heat: int = 256, n_hex: int = 40) -> dict:
    import numpy as np
    import torch

    from dolfinx_external_operator_amd import Context, DeviceMesh
    from tools.bench_krylov import _batches
    from tools.synthetic import structured_mesh

    ctx = Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_option("consumer_overwrite", 1)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    res = {"tri_cells_per_side": n_side, "heat_cells_per_side": n_heat, "hex_boxes_per_side": n_hex, "legs": {}, "ratios": {}}

    def leg(name, fn):
        with torch.cuda.stream(stream):
            ms, per = _batches(torch, stream, fn)
        res["legs"][name] = {"ms": round(ms, 4), "batches_ms": [round(t, 4) for t in per]}
        print(name, json.dumps(res["legs"][name]), file=sys.stderr, flush=True)
        return ms

    def matrix_legs(tag, A, x, y):
        other = torch.empty_like(A.values)
        t = leg(f"{tag}_spmv", lambda: A.matvec(x, y))
        tt = leg(f"{tag}_spmv_t", lambda: A.matvec(x, y, transpose=True))
        tr = leg(f"{tag}_transpose", lambda: A.transpose(out=other))
        ti = leg(f"{tag}_transpose_inplace", lambda: A.transpose(out=A.values))
        res["ratios"][f"{tag}_spmv_t_over_spmv"] = round(tt / t, 3)
        res["ratios"][f"{tag}_transpose_over_spmv"] = round(tr / t, 3)
        res["ratios"][f"{tag}_transpose_inplace_over_spmv"] = round(ti / t, 3)
        res["ratios"][f"{tag}_transpose_plus_spmv_over_spmv_t"] = round((tr + t) / tt, 3)

    def apply_legs(tag, dm, test, trial, bs, Cd, x, y):
        t = leg(f"{tag}_apply", lambda: dm.bilinear_apply(test, trial, bs, Cd.data_ptr(), x.data_ptr(), y.data_ptr()))
        tt = leg(f"{tag}_apply_t", lambda: dm.bilinear_apply_t(test, trial, bs, Cd.data_ptr(), x.data_ptr(), y.data_ptr()))
        res["ratios"][f"{tag}_apply_t_over_apply"] = round(tt / t, 3)

    for tag, cell, n, degree, test, trial, bs, assembled in (("p2", "triangle", (n_side, n_side), 2, "grad", "grad", 2, True),
                                                             ("heat", "triangle", (n_heat, n_heat), 1, "grad", "value_grad", 1, True),
                                                             ("q2hex", "hexahedron", (n_hex, n_hex, n_hex), 2, "eps", "eps", 3, False)):
        m = structured_mesh(cell, n, degree, distort=0.2, seed=0)
        dm = DeviceMesh.from_synthetic(m, ctx=ctx)
        G = m.gdim
        size = {"grad": bs * G, "eps": 4 if G == 2 else 6, "value_grad": bs * (1 + G)}
        DT, DR = size[test], size[trial]
        npts, nn = m.num_cells * m.nq, m.node_x.shape[0]
        try:
            with torch.cuda.stream(stream):
                Cd = 0.3 * torch.randn(npts * DT * DR, generator=gen, device=dev, dtype=torch.float64)
                Cd.view(npts, DT, DR)[:, :, DR - DT:].add_(torch.eye(DT, device=dev, dtype=torch.float64))
                x = torch.randn(nn * bs, generator=gen, device=dev, dtype=torch.float64)
                y = torch.empty_like(x)
                res[f"{tag}_points"], res[f"{tag}_dofs"] = npts, nn * bs
                if assembled:
                    bcs = None
                    if tag == "heat":
                        X = m.node_x
                        bcs = torch.from_numpy(np.flatnonzero((X.min(axis=1) < 1e-12) | (X.max(axis=1) > 1 - 1e-12)).astype(np.int32)).to(dev)
                    A = dm.bilinear_assemble(test, trial, bs, Cd.data_ptr(), dm.csr_pattern(bs), bcs=bcs)
                    res[f"{tag}_nnz"] = A.pattern.nnz
                    matrix_legs(tag, A, x, y)
                    del A
                apply_legs(tag, dm, test, trial, bs, Cd, x, y)
                del Cd, x, y
            stream.synchronize()
        finally:
            dm.close()
            torch.cuda.empty_cache()
    ctx.close()
    return res


def table(r: dict) -> str:
    lines = ["leg                              ms (median of 5 batches of 20)"]
    lines += [f"{k:<32} {v['ms']:>10.4f}" for k, v in r["legs"].items()]
    lines += ["", "ratio"]
    lines += [f"{k:<48} {v:>8.3f}" for k, v in r["ratios"].items()]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    args = sys.argv[1:]
    out_file = None
    if "--out" in args:
        i = args.index("--out")
        out_file = args[i + 1]
        del args[i:i + 2]
    r = main(*(int(a) for a in args))
    line = json.dumps(r)
    print(line)
    if out_file:
        pathlib.Path(out_file).write_text("# tools/bench_transpose.py on one MI355X\n" + table(r) + "\n" + line + "\n")
