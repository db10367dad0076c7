#!/usr/bin/env python3
"""Times the 3-D Mohr-Coulomb operator (dxo_mohr_coulomb3) on 10^7 points beside its yardsticks, in one run on one board.

Points: a seeded draw from the frozen tracing pool (tests/golden/mc_tracing_pool.npz, plane strain), each point's increment and state
turned by the SAME seeded random rotation (a unit quaternion per point), so that all six components are in play and every 3-D point is
physically the plane-strain point it was drawn from: the iteration histograms of the two operators should be the same, and both are
printed.
Legs (device memory, diagnostics written):
  mc3          production form (classification + compacted Newton with lane refill) on the pool's mix
  mc3_point    the lane-per-point form (ctx option mc_variant = 0) on the same points
  mc3_elastic  production form, 0 % plastic;   mc3_plastic  production form, 100 % plastic (the pool's plastic points, increments unscaled)
  mc2          dxo_mohr_coulomb on the unrotated points (224 + 28 B per point)
  probe        dxo_stream_probe moving the 432 B per point of mc3 (6 x 16 B in, 21 x 16 B out) with no arithmetic
`mc3_over_mc2` and `mc3_over_probe` are ratios of times. `fp64_ops_per_pass` is a static count: the scalar fp64 arithmetic instructions
(add, sub, mul, div, sqrt) in the host build of ONE Newton pass with its loops fully unrolled, SAME-angle specialisation, compiled
without FMA contraction, both Lode-angle branches included — the same count for mc_core.h's pass beside it. Instructions in the
listing, not instructions executed, and not a hardware counter: it is the ratio of the two that says something.
Timing: warm-up, then 5 batches of 10 back-to-back launches timed with events on the launch stream; the median batch is reported.
Prints one JSON line.    python3 tools/bench_mc3.py [n_points] [--out FILE]
"""
import json
import pathlib
import re
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from tools.mc_inputs import mc_default_params, mc_pool  # noqa: E402

_COUNT_SRC = r"""
#include "mc3_core.h"
extern "C" __attribute__((noinline, flatten)) bool pass2(const mc::Const* k, mc::Lane* L) { return mc::lane_pass<true>(*k, *L); }
extern "C" __attribute__((noinline, flatten)) bool pass3(const mc::Const* k, mc3::Lane* L) { return mc3::lane_pass<true>(*k, *L); }
"""


def fp64_ops_per_pass():
    """scalar fp64 arithmetic instructions of one Newton pass in the host build (static count), or None without a host compiler"""
    csrc = ROOT / "dolfinx_external_operator_amd" / "csrc"
    try:
        with tempfile.TemporaryDirectory() as tmp:
            src = pathlib.Path(tmp) / "count.cpp"
            src.write_text(_COUNT_SRC)
            asm = subprocess.run(["g++", "-O3", "--param", "max-completely-peeled-insns=20000", "--param", "max-completely-peel-times=64", "--param",
                                  "max-unroll-times=64", "-std=c++17", "-ffp-contract=off", "-mno-fma", "-fno-tree-vectorize", "-fno-tree-slp-vectorize",
                                  f"-I{csrc}", "-S", str(src), "-o", "-"],
                                 check=True, capture_output=True, text=True).stdout
    except (OSError, subprocess.CalledProcessError):
        return None
    out = {}
    for name in ("pass2", "pass3"):
        body = asm.split(f"\n{name}:")[1].split(".cfi_endproc")[0]
        out[name] = len(re.findall(r"^\s+v?(?:add|sub|mul|div|sqrt)sd\s", body, flags=re.M))
    return out


def main(n=10_000_000, out=None):
    import torch

    from dolfinx_external_operator_amd import MEM_DEVICE, Context

    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    prm = mc_default_params()
    f64 = dict(dtype=torch.float64, device=dev)
    pool_d, pool_s = (torch.from_numpy(a).to(dev) for a in mc_pool())
    npool = pool_d.shape[0]

    def diag(m):
        return torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, **f64), torch.empty(m, **f64), torch.empty(m, **f64)

    def call2(d, s, Ct, sg, aux):
        ctx.mohr_coulomb(prm, d.shape[0], MEM_DEVICE, d.data_ptr(), s.data_ptr(), Ct.data_ptr(), sg.data_ptr(), *(a.data_ptr() for a in aux))

    def call3(d, s, Ct, sg, aux):
        ctx.mohr_coulomb3(prm, d.shape[0], MEM_DEVICE, d.data_ptr(), s.data_ptr(), Ct.data_ptr(), sg.data_ptr(), *(a.data_ptr() for a in aux))

    # the pool's own classification (by the plane-strain operator): which of its points are plastic
    aux_p = diag(npool)
    call2(pool_d, pool_s, torch.empty(npool * 16, **f64), torch.empty(npool * 4, **f64), aux_p)
    plastic_pool = torch.nonzero(aux_p[1] > 0).reshape(-1)
    elastic_pool = torch.nonzero(aux_p[1] <= 0).reshape(-1)

    g = torch.Generator(device=dev)
    g.manual_seed(2)
    pick = torch.randint(0, npool, (n,), generator=g, device=dev)
    scale = torch.rand(n, 1, generator=g, device=dev, dtype=torch.float64) * 0.5 + 0.5
    quat = torch.randn(n, 4, generator=g, **f64)
    quat /= torch.linalg.norm(quat, dim=1, keepdim=True)

    def rotated(v4):
        """Mandel (n,4) plane strain -> Mandel (n,6) of Q T Q^T, Q from the seeded quaternions; in slabs to bound the temporaries"""
        r2 = np.sqrt(2.0)
        res = torch.empty(v4.shape[0], 6, **f64)
        for a in range(0, v4.shape[0], 2_000_000):
            v, q = v4[a:a + 2_000_000], quat[a:a + 2_000_000]
            w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
            Q = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                             2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                             2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
            T = torch.zeros(v.shape[0], 3, 3, **f64)
            T[:, 0, 0], T[:, 1, 1], T[:, 2, 2] = v[:, 0], v[:, 1], v[:, 2]
            T[:, 0, 1] = T[:, 1, 0] = v[:, 3] / r2
            T = Q @ T @ Q.transpose(1, 2)
            res[a:a + 2_000_000] = torch.stack([T[:, 0, 0], T[:, 1, 1], T[:, 2, 2], r2 * T[:, 0, 1], r2 * T[:, 0, 2], r2 * T[:, 1, 2]], dim=1)
        return res

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / 10)
        return float(np.median(ms))

    res = {"points": n, "bytes_per_point_mc3": 432 + 28, "legs": {}}
    Ct3, sg3, aux3 = torch.empty(n * 36, **f64), torch.empty(n * 6, **f64), diag(n)

    def leg3(name, idx, variant=2, scaled=True):
        d4, s4 = (pool_d[idx] * scale if scaled else pool_d[idx]).contiguous(), pool_s[idx].contiguous()
        d6, s6 = rotated(d4), rotated(s4)
        ctx.set_option("mc_variant", variant)
        try:
            ms = timed(lambda: call3(d6, s6, Ct3, sg3, aux3))
        finally:
            ctx.set_option("mc_variant", 2)
        summ = ctx.mc_summary(n, *aux3[:3], nbins=201)
        res["legs"][name] = {"ms": round(ms, 4), "Gpoints_per_s": round(n / ms * 1e-6, 3), "TBs": round(n * 460 / ms * 1e-9, 3),
                             "plastic_fraction": round(float((aux3[1] > 0).double().mean()), 4),
                             "iterations": {int(k): int(c) for k, c in zip(summ["unique_iters"], summ["counts"])}}
        return d4, s4

    d4, s4 = leg3("mc3", pick)
    leg3("mc3_point", pick, variant=0)
    leg3("mc3_elastic", elastic_pool[torch.randint(0, elastic_pool.numel(), (n,), generator=g, device=dev)])
    # the pool was classified with its full increments: unscaled, every plastic point of it stays plastic
    leg3("mc3_plastic", plastic_pool[torch.randint(0, plastic_pool.numel(), (n,), generator=g, device=dev)], scaled=False)
    del Ct3, sg3
    # yardstick 1: the plane-strain operator on the unrotated points of the first leg
    d4, s4 = (pool_d[pick] * scale).contiguous(), pool_s[pick].contiguous()
    Ct2, sg2, aux2 = torch.empty(n * 16, **f64), torch.empty(n * 4, **f64), diag(n)
    ms2 = timed(lambda: call2(d4, s4, Ct2, sg2, aux2))
    summ = ctx.mc_summary(n, *aux2[:3], nbins=201)
    res["legs"]["mc2"] = {"ms": round(ms2, 4), "Gpoints_per_s": round(n / ms2 * 1e-6, 3),
                          "iterations": {int(k): int(c) for k, c in zip(summ["unique_iters"], summ["counts"])}}
    del Ct2, sg2
    # yardstick 2: the same 432 B per point with no arithmetic
    tiles = (n + 63) // 64
    src, dst = torch.empty(tiles * 6 * 128, **f64), torch.empty(tiles * 21 * 128, **f64)
    msp = timed(lambda: ctx.stream_probe(6, 21, tiles, src.data_ptr(), dst.data_ptr()))
    res["legs"]["probe_6_21"] = {"ms": round(msp, 4), "TBs": round(tiles * 27 * 1024 / msp * 1e-9, 3)}
    ms3 = res["legs"]["mc3"]["ms"]
    res["mc3_over_mc2"] = round(ms3 / ms2, 3)
    res["mc3_over_probe"] = round(ms3 / msp, 3)
    res["mc3_elastic_over_probe"] = round(res["legs"]["mc3_elastic"]["ms"] / msp, 3)
    res["mc3_point_over_mc3"] = round(res["legs"]["mc3_point"]["ms"] / ms3, 3)
    res["same_iteration_histogram_as_mc2"] = res["legs"]["mc3"]["iterations"] == res["legs"]["mc2"]["iterations"]
    ops = fp64_ops_per_pass()
    if ops:
        res["fp64_ops_per_pass"] = {"mc2": ops["pass2"], "mc3": ops["pass3"], "ratio": round(ops["pass3"] / ops["pass2"], 2)}
    ctx.close()
    line = json.dumps(res)
    print(line)
    if out:
        pathlib.Path(out).write_text(line + "\n")
    return res


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out in args:
        args.remove(out)
    main(int(args[0]) if args else 10_000_000, out)
