#!/usr/bin/env python3
"""Standalone timing of the boundary-facet loads dxo_facet_pressure and dxo_facet_adjoint (not a bench.py leg).

    python3 tools/bench_facet.py [tri_cells_per_side] [hex_boxes_per_side] [--out FILE]

Meshes (distorted): P2 triangles, default 1291 cells per side (~10^7 cell points), and Q2 hexahedra, default 108^3 boxes
(~10^7 cell points). On each, over the WHOLE exterior (exterior_facets):
  <mesh>_pressure        dxo_facet_pressure with a per-point p
  <mesh>_adjoint_value   dxo_facet_adjoint("value", gdim) with a per-point traction
  <mesh>_internal_force  dxo_operand_adjoint("eps", gdim) over all cells, the term the load is added to
and, for (trial, bs) = ("value", 1) and ("grad", gdim), the facet bilinear forms with a per-point block C:
  <mesh>_bilinear_<trial><bs>_apply / _diagonal / _assemble   dxo_facet_bilinear_apply / _diagonal / _assemble
  <mesh>_bilinear_<trial><bs>_cell_assemble                   dxo_bilinear_assemble on the same pattern, (value, value) for bs = 1 and
                                                              (grad, grad) for bs = gdim: the matrix the facet term is added to
The _assemble and _cell_assemble legs need the cell pattern and are skipped (listed under "skipped") where it is estimated above
MAX_PATTERN_BYTES: Q2 hexahedra 108^3 with bs = 3, about 70 GB. Pass a smaller hex size (40, as tools/bench_assemble.py) to time them.
Every call is timed with HIP events on the launch stream (median of back-to-back launches after a warm-up,
tools/bench_secondary._time). Prints one JSON line.
"""
from __future__ import annotations

import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


MAX_PATTERN_BYTES = 16 << 30     # the assembled legs are skipped on a mesh and block size whose cell pattern is estimated above this


def main(n_side: int = 1291, n_hex: int = 108, launches: int = 20) -> dict:
    import torch

    from dolfinx_external_operator_amd import Context, DeviceMesh
    from tools.bench_secondary import _time
    from tools.synthetic import exterior_facets, facet_geometry, facet_tables, structured_mesh_cached

    ctx = Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    res = {"tri_cells_per_side": n_side, "hex_boxes_per_side": n_hex, "legs": {}}

    def leg(name, fn):
        with torch.cuda.stream(stream):
            med, mean = _time(torch, stream, fn, launches)
        res["legs"][name] = {"ms": round(med, 4), "mean_ms": round(mean, 4)}

    for tag, cell, n in (("p2tri", "triangle", (n_side, n_side)), ("q2hex", "hexahedron", (n_hex, n_hex, n_hex))):
        m = structured_mesh_cached(cell, n, 2, distort=0.2, seed=0)
        dm = DeviceMesh.from_synthetic(m, ctx=ctx)
        try:
            dm.set_facet_tables(*facet_tables(m)[:3])
            dm.set_facet_geometry(*facet_geometry(cell))
            fs = dm.facet_set(exterior_facets(m))
            G, nn, npts = m.gdim, m.node_x.shape[0], m.num_cells * m.nq
            nqf = facet_tables(m)[0].shape[1]
            res[f"{tag}_facets"], res[f"{tag}_facet_points"], res[f"{tag}_cell_points"] = fs.n, fs.n * nqf, npts
            with torch.cuda.stream(stream):
                p = torch.rand(fs.n * nqf, generator=gen, device=dev, dtype=torch.float64)
                t = torch.randn(fs.n * nqf * G, generator=gen, device=dev, dtype=torch.float64)
                sigma = torch.randn(npts * (4 if G == 2 else 6), generator=gen, device=dev, dtype=torch.float64)
                out = torch.zeros(nn * G, device=dev, dtype=torch.float64)
                leg(f"{tag}_pressure", lambda: dm.facet_pressure(fs, out.data_ptr(), p.data_ptr(), 1.0))
                leg(f"{tag}_adjoint_value", lambda: dm.facet_adjoint("value", G, t.data_ptr(), fs, out.data_ptr()))
                leg(f"{tag}_internal_force", lambda: dm.adjoint("eps", G, sigma.data_ptr(), out.data_ptr()))
                # the facet bilinear forms, beside the cell assembly of the same mesh (the matrix the facet term is added to)
                for trial, bs in (("value", 1), ("grad", G)):
                    D = dm.value_size(trial, bs)
                    name = f"{tag}_bilinear_{trial}{bs}"
                    Cf = torch.randn(fs.n * nqf * bs * D, generator=gen, device=dev, dtype=torch.float64)
                    v = torch.randn(nn * bs, generator=gen, device=dev, dtype=torch.float64)
                    outb = torch.zeros(nn * bs, device=dev, dtype=torch.float64)
                    leg(f"{name}_apply", lambda: dm.facet_bilinear_apply(trial, bs, Cf.data_ptr(), v.data_ptr(), fs, outb.data_ptr()))
                    leg(f"{name}_diagonal", lambda: dm.facet_bilinear_diagonal(trial, bs, Cf.data_ptr(), fs, outb.data_ptr()))
                    res[f"{name}_apply_over_adjoint_value"] = round(res["legs"][f"{name}_apply"]["ms"] / res["legs"][f"{tag}_adjoint_value"]["ms"], 3)
                    # the assembled legs need the cell pattern: an upper estimate of its size (values, columns, pos table) decides
                    nd = m.dofmap.shape[1]
                    est = m.num_cells * nd * nd * (bs * bs * 12 + 2)
                    if est > MAX_PATTERN_BYTES:
                        res.setdefault("skipped", {})[f"{name}_assemble"] = f"cell pattern of about {est / 2**30:.0f} GiB"
                        del Cf
                        continue
                    pat = dm.csr_pattern(bs)
                    values = torch.zeros(pat.nnz, device=dev, dtype=torch.float64)
                    leg(f"{name}_assemble", lambda: dm.facet_bilinear_assemble(trial, bs, Cf.data_ptr(), fs, pat, values=values))
                    cell_pair = ("value", "value") if bs == 1 else ("grad", "grad")
                    Dc = dm.value_size(cell_pair[0], bs)
                    Cc = torch.randn(npts * Dc * Dc, generator=gen, device=dev, dtype=torch.float64)
                    leg(f"{name}_cell_assemble", lambda: dm.bilinear_assemble(*cell_pair, bs, Cc.data_ptr(), pat, values=values))
                    stream.synchronize()
                    legs = res["legs"]
                    res[f"{name}_assemble_over_cell_assemble"] = round(legs[f"{name}_assemble"]["ms"] / legs[f"{name}_cell_assemble"]["ms"], 4)
                    del Cf, Cc, values
            stream.synchronize()
            res[f"{tag}_pressure_over_internal_force"] = round(res["legs"][f"{tag}_pressure"]["ms"] / res["legs"][f"{tag}_internal_force"]["ms"], 3)
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
