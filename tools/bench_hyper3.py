#!/usr/bin/env python3
"""Rates of the 3-D Isihara operator on device memory, about 10^7 points:

  plain3   dxo_isihara3        72 B read + 720 B written per point
  fused3   dxo_isihara3_field  Q2 hexahedra, 108 boxes per side, 8-point rule: the dof gather read + 720 B written per point
  plain2   dxo_isihara         the plane-strain kernel in the same run: 32 B + 160 B per point
  probe    dxo_stream_probe moving the bytes of plain3 with no arithmetic. The probe has no 1 : 10 mix; reported are its most
           write-heavy mix (13, 43) and the (4, 4) copy, each sized to plain3's total bytes

`TBs` = the leg's model bytes / its time; `plain3_over_probe_*` = plain3 ms / probe ms. Timing: warm-up, then 5 batches of 20
back-to-back launches timed with events on the launch stream, the median batch reported. Prints one JSON line.
Needs an MI355X.    python3 tools/bench_hyper3.py [points] [hex boxes per side]

`--model icnn`: the 3-D network operator instead (dxo_icnn3_eval, fp32 network, shipped weights unless --weights FILE.npz), in one run
  icnn3_v0 / _v1 / _v2_staged / _v2_rows   the three kernels of "icnn_variant"; the default one with both store forms ("icnn3_store")
  icnn2_v2   the plane-strain default kernel: the same GEMMs, 32 B + 160 B per point
  plain3     dxo_isihara3: the same 72 B + 720 B per point with next to no arithmetic
The larger of icnn2_v2 and plain3 is the floor of icnn3_v2, their sum what a kernel that overlaps nothing would cost;
`icnn3_between` = (icnn3_v2 - floor) / (sum - floor) for the store form the library ships.
                    python3 tools/bench_hyper3.py --model icnn [points]
"""
from __future__ import annotations

import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main(n: int = 10_000_000, n_hex: int = 108) -> dict:
    import torch

    from dolfinx_external_operator_amd import MEM_DEVICE, Context, DeviceMesh, IsiharaParams
    from tools.bench_krylov import _batches
    from tools.synthetic import structured_mesh_cached

    ctx = Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    prm = IsiharaParams(0.5, 1.0, 1.0, 1.5)
    n = n // 64 * 64
    res = {"points": n, "hex_boxes_per_side": n_hex, "device": ctx.device_info()["name"], "nontemporal": ctx.get_option("nontemporal"), "legs": {}}

    def leg(name, fn, nbytes):
        with torch.cuda.stream(stream):
            ms, per = _batches(torch, stream, fn)
        r = {"ms": round(ms, 4), "batches_ms": [round(t, 4) for t in per], "GB": round(nbytes / 1e9, 3), "TBs": round(nbytes / 1e9 / ms, 3)}
        res["legs"][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        return ms

    f64 = dict(device=dev, dtype=torch.float64)
    with torch.cuda.stream(stream):
        eye3 = torch.eye(3, **f64).reshape(9)
        F3 = eye3 + 0.1 * torch.randn((n, 9), generator=gen, **f64)
        dP3, P3 = torch.empty(n * 81, **f64), torch.empty(n * 9, **f64)
        t3 = leg("plain3", lambda: ctx.isihara3(prm, n, MEM_DEVICE, F3.data_ptr(), dP3.data_ptr(), P3.data_ptr()), 792 * n)
        assert bool(torch.isfinite(P3).all())

        F2 = torch.eye(2, **f64).reshape(4) + 0.1 * torch.randn((n, 4), generator=gen, **f64)
        dP2, P2 = torch.empty(n * 16, **f64), torch.empty(n * 4, **f64)
        t2 = leg("plain2", lambda: ctx.isihara(prm, n, MEM_DEVICE, F2.data_ptr(), dP2.data_ptr(), P2.data_ptr()), 192 * n)
        del F2, dP2, P2

        for rd, wr in ((13, 43), (4, 4)):
            tiles = 792 * n // ((rd + wr) * 1024)
            src, dst = F3.reshape(-1), dP3      # contents do not matter; sizes do
            if src.numel() * 8 < tiles * rd * 1024:
                src = torch.empty(tiles * rd * 128, **f64)
            if dst.numel() * 8 < tiles * wr * 1024:
                dst = torch.empty(tiles * wr * 128, **f64)
            tp = leg(f"probe_{rd}_{wr}", lambda: ctx.stream_probe(rd, wr, tiles, src.data_ptr(), dst.data_ptr()), tiles * (rd + wr) * 1024)
            res[f"plain3_over_probe_{rd}_{wr}"] = round(t3 / tp, 3)
            del src, dst
        del F3

        m = structured_mesh_cached("hexahedron", (n_hex, n_hex, n_hex), 2, distort=0.2, seed=0)
        dm = DeviceMesh.from_synthetic(m, ctx=ctx)
        try:
            npts, nn = m.num_cells * m.nq, m.node_x.shape[0]
            u = 0.01 * torch.randn(nn * 3, generator=gen, **f64)
            if npts > n:
                dP3, P3 = torch.empty(npts * 81, **f64), torch.empty(npts * 9, **f64)
            # model bytes: the outputs, the dof vector and the coordinates once, the two dofmaps
            nbytes = 720 * npts + 8 * 3 * nn + 8 * 3 * m.x.shape[0] + 4 * (m.dofmap.size + m.geom_dofmap.size)
            tf = leg("fused3", lambda: ctx.isihara3_field(prm, dm._h, MEM_DEVICE, u.data_ptr(), dP3.data_ptr(), P3.data_ptr()), nbytes)
            res["fused3_points"] = npts
            res["fused3_ns_per_point"] = round(tf * 1e6 / npts, 4)
        finally:
            dm.close()
    res["plain3_ns_per_point"] = round(t3 * 1e6 / n, 4)
    res["plain3_TBs_over_plain2_TBs"] = round(res["legs"]["plain3"]["TBs"] / res["legs"]["plain2"]["TBs"], 3)
    res["plain2_ns_per_point"] = round(t2 * 1e6 / n, 4)
    ctx.close()
    print(json.dumps(res))
    return res


def main_icnn(n: int = 10_000_000, weights: str | None = None) -> dict:
    import numpy as np
    import torch

    from dolfinx_external_operator_amd import MEM_DEVICE, Context, IsiharaParams
    from tools.bench_krylov import _batches

    ctx = Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    n = n // 64 * 64
    w = dict(np.load(weights or ROOT / "tests" / "golden" / "icnn_isihara_weights.npz"))
    model = ctx.icnn_create({k.replace("__", "."): v for k, v in w.items()})
    default_store = ctx.get_option("icnn3_store")
    res = {"points": n, "device": ctx.device_info()["name"], "default_icnn3_store": default_store, "legs": {}}

    def leg(name, fn, nbytes):
        with torch.cuda.stream(stream):
            ms, per = _batches(torch, stream, fn)
        r = {"ms": round(ms, 4), "batches_ms": [round(t, 4) for t in per], "ns_per_point": round(ms * 1e6 / n, 4), "TBs": round(nbytes / 1e9 / ms, 3)}
        res["legs"][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        return ms

    f64 = dict(device=dev, dtype=torch.float64)
    try:
        with torch.cuda.stream(stream):
            F3 = torch.eye(3, **f64).reshape(9) + 0.1 * torch.randn((n, 9), generator=gen, **f64)
            dP3, P3 = torch.empty(n * 81, **f64), torch.empty(n * 9, **f64)
            call3 = lambda: ctx.icnn3_eval(model, 0, n, MEM_DEVICE, F3.data_ptr(), dP3.data_ptr(), P3.data_ptr())   # noqa: E731
            t = {}
            for name, variant, store in (("icnn3_v2_rows", 2, 0), ("icnn3_v2_staged", 2, 1), ("icnn3_v1", 1, default_store), ("icnn3_v0", 0, default_store)):
                ctx.set_option("icnn_variant", variant)
                ctx.set_option("icnn3_store", store)
                t[name] = leg(name, call3, 792 * n)
                assert bool(torch.isfinite(P3).all())
            ctx.set_option("icnn_variant", 2)
            ctx.set_option("icnn3_store", default_store)
            prm = IsiharaParams(0.5, 1.0, 1.0, 1.5)
            t["plain3"] = leg("plain3", lambda: ctx.isihara3(prm, n, MEM_DEVICE, F3.data_ptr(), dP3.data_ptr(), P3.data_ptr()), 792 * n)
            F2 = torch.eye(2, **f64).reshape(4) + 0.1 * torch.randn((n, 4), generator=gen, **f64)
            dP2, P2 = torch.empty(n * 16, **f64), torch.empty(n * 4, **f64)
            t["icnn2_v2"] = leg("icnn2_v2", lambda: ctx.icnn_eval(model, 0, n, MEM_DEVICE, F2.data_ptr(), dP2.data_ptr(), P2.data_ptr()), 192 * n)
        floor, total = max(t["icnn2_v2"], t["plain3"]), t["icnn2_v2"] + t["plain3"]
        shipped = t["icnn3_v2_staged" if default_store else "icnn3_v2_rows"]
        res.update(floor_ms=round(floor, 4), sum_ms=round(total, 4), icnn3_between=round((shipped - floor) / (total - floor), 3))
    finally:
        ctx.icnn_destroy(model)
        ctx.close()
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--model" in args:
        k = args.index("--model")
        model_name = args[k + 1]
        del args[k:k + 2]
        wfile = None
        if "--weights" in args:
            k = args.index("--weights")
            wfile = args[k + 1]
            del args[k:k + 2]
        if model_name == "icnn":
            main_icnn(*(int(a) for a in args[:1]), weights=wfile)
        elif model_name == "isihara":
            main(*(int(a) for a in args[:2]))
        else:
            raise SystemExit("--model isihara | icnn")
    else:
        main(*(int(a) for a in args[:2]))
