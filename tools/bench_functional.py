#!/usr/bin/env python3
"""Standalone timing of the scalar functionals (csrc/functional.hip; not a bench.py leg).
    python3 tools/bench_functional.py [tri_cells_per_side] [hex_boxes_per_side] [--out FILE]
Legs, all on the same board in the same run (distorted meshes, random data):
  (a) integrate on P2 triangles (1291 per side: 10^7 points) for D = 1 and 6, without g (`integrate_D*`) and with g (`pair_D*`). The
      integrals read every byte of f (and g) once and write almost nothing, so a read-only stream over the same bytes is their roof.
      dxo_stream_probe has no read-only mix: `probe_copy_*` is its (4, 4) copy READING the same number of bytes (and writing as many, so
      it moves twice the bytes), and `torch_sum_*` is torch's own sum over the same bytes, a read-only pass. `ratio_to_probe` =
      integrate ms / probe ms, `ratio_to_torch_sum` = integrate ms / torch.sum ms, `read_TBs` = bytes of f (and g) / integrate ms.
  (b) operand_moments beside dxo_eval_operand of the same kind ("eps" and "grad", bs = gdim) on P2 triangles and on Q2 hexahedra (108
      boxes per side: 10^7 points): the fused form does the same gathers and arithmetic and omits the output stream. `ratio` =
      moments ms / eval ms.
  cell_measure on both meshes.
Timing: warm-up, then 5 batches of 20 back-to-back launches timed with HIP events on the launch stream, the MEDIAN batch reported
(tools/bench_timing.median_batch). Prints one JSON line.
"""
from __future__ import annotations

import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main(n_side: int = 1291, n_hex: int = 108) -> dict:
    import torch

    from dolfinx_external_operator_amd import Context, DeviceMesh
    from tools.bench_krylov import _batches
    from tools.synthetic import structured_mesh_cached

    ctx = Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    res = {"tri_cells_per_side": n_side, "hex_boxes_per_side": n_hex, "device": ctx.device_info()["name"], "legs": {}}

    def leg(name, fn, read_bytes=None):
        with torch.cuda.stream(stream):
            ms, per = _batches(torch, stream, fn)
        r = {"ms": round(ms, 4), "batches_ms": [round(t, 4) for t in per]}
        if read_bytes is not None:
            r["read_GB"] = round(read_bytes / 1e9, 3)
            r["read_TBs"] = round(read_bytes / 1e9 / ms, 3)
        res["legs"][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        return ms

    for tag, cell, n in (("p2tri", "triangle", (n_side, n_side)), ("q2hex", "hexahedron", (n_hex, n_hex, n_hex))):
        m = structured_mesh_cached(cell, n, 2, distort=0.2, seed=0)
        dm = DeviceMesh.from_synthetic(m, ctx=ctx)
        G, npts, nn = m.gdim, m.num_cells * m.nq, m.node_x.shape[0]
        res[f"{tag}_points"] = npts
        try:
            with torch.cuda.stream(stream):
                dx = torch.empty((m.num_cells, m.nq), device=dev, dtype=torch.float64)
                leg(f"{tag}_cell_measure", lambda: dm.cell_measure(out=dx))
                if tag == "p2tri":       # (a)
                    for D in (1, 6):
                        f = torch.randn((m.num_cells, m.nq, D), generator=gen, device=dev, dtype=torch.float64)
                        g = torch.randn((m.num_cells, m.nq, D), generator=gen, device=dev, dtype=torch.float64)
                        out = torch.empty(D, device=dev, dtype=torch.float64)
                        one = torch.empty(1, device=dev, dtype=torch.float64)
                        dst = torch.empty(2 * f.numel(), device=dev, dtype=torch.float64)
                        both = torch.cat([f.reshape(-1), g.reshape(-1)])
                        for what, nbytes, src, call in (("integrate", 8 * f.numel(), f, lambda: dm.integrate(f, out=out)),
                                                        ("pair", 16 * f.numel(), both, lambda: dm.integrate(f, g, out=one))):
                            t = leg(f"{what}_D{D}", call, nbytes)
                            tiles = nbytes // 4096                   # a (4, 4) tile reads 64 lanes x 4 x 16 bytes
                            tp = leg(f"probe_copy_{what}_D{D}", lambda: ctx.stream_probe(4, 4, tiles, src.data_ptr(), dst.data_ptr()), tiles * 4096)
                            ts = leg(f"torch_sum_{what}_D{D}", lambda: torch.sum(src), nbytes)
                            res["legs"][f"{what}_D{D}"].update(ratio_to_probe=round(t / tp, 3), ratio_to_torch_sum=round(t / ts, 3))
                        del f, g, dst, both
                for kind in ("eps", "grad"):     # (b)
                    D = dm.value_size(kind, G)
                    u = torch.randn(nn * G, generator=gen, device=dev, dtype=torch.float64)
                    e = torch.empty((m.num_cells, m.nq, D), device=dev, dtype=torch.float64)
                    mom = torch.empty(D + 1, device=dev, dtype=torch.float64)
                    te = leg(f"{tag}_eval_{kind}", lambda: dm.evaluate_device(kind, G, u.data_ptr(), m.num_cells, e.data_ptr()))
                    tm = leg(f"{tag}_moments_{kind}", lambda: dm.operand_moments(kind, G, u, out=mom))
                    res["legs"][f"{tag}_moments_{kind}"]["ratio"] = round(tm / te, 3)
                    del u, e
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
    r = main(*(int(a) for a in args))
    line = json.dumps(r)
    print(line)
    if out_file:
        pathlib.Path(out_file).write_text(line + "\n")
