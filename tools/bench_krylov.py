#!/usr/bin/env python3
"""Standalone timing of the device linear solves (csrc/krylov.hip; not a bench.py leg).
    python3 tools/bench_krylov.py [tri_cells_per_side] [hex_boxes_per_side] [heat_cells_per_side] [amg_cells_per_side] [--out FILE] [--basis fp32]
Legs (distorted meshes, random C):
  p2_spmv / p2_apply        dxo_csr_spmv of the assembled ("grad", "grad", 2) matrix on P2 triangles (1291 per side: 10^7 points,
                            3.07e8 nonzeros) next to the matrix-free dxo_bilinear_apply of the same form
  q2hex_spmv / q2hex_apply  ("eps", "eps", 3) on Q2 hexahedra (40^3 boxes)
  p2_block_jacobi           dxo_csr_block_jacobi (one stream synchronisation included)
  p2_gmres30_iteration      one GMRES(30) cycle (30 iterations, check_every 30) divided by 30; `..._orth_ms` = that minus one SpMV and
                            one block-Jacobi apply: the Gram-Schmidt part (two passes, norm, scaling, Givens)
  heat_solve                one full block-Jacobi GMRES(30) solve of a heat-type Jacobian (P1, ("grad", "value_grad"), Dirichlet
                            boundary) to rtol 1e-8, at most 3000 iterations
--basis fp32 adds, in the same run and on the same systems, the GMRES(30) legs with both kinds of Krylov basis (key "basis"): for the
P2 and the Q2 system and per basis ("fp64", and "fp32_w1" / "fp32_w2" / "fp32_w4": the compressed basis with 1, 2 or 4 rows per
thread, option krylov_basis_width) the ms per iteration of one cycle, the orthogonalisation part and its share, basis_bytes, and one
solve of at most 300 iterations (iterations, true relative residual reached); `orth_ratio` = the orthogonalisation of each fp32
width over the fp64 basis's. Then one multigrid-preconditioned ("eps", "eps", 2) solve on P2 triangles (amg_cells_per_side, default
400; rigid-body modes, lower side clamped, as tools/bench_amg.py --rbm) to rtol 1e-8 by gmres and fgmres with both bases.
Timing: warm-up, then 5 batches of 20 back-to-back launches timed with HIP events on the launch stream, the MEDIAN batch reported
(tools/bench_timing.median_batch). `model_GB` of an SpMV = values + column indices (one per bs^2 block) + row pointers + x once + y;
`frac_6p3` its rate against 6.3 TB/s achievable. Prints one JSON line.
"""
from __future__ import annotations

import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

ACHIEVABLE_TBs = 6.3


def _batches(torch, stream, fn, per_batch=20, batches=5, warm=5):
    from tools.bench_timing import median_batch

    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(per_batch):
            fn()
        b.record(stream)
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) / per_batch)
    return per[median_batch(per)], per


def spmv_model_GB(nnz: int, n: int, bs: int) -> float:
    return (8 * nnz + 4 * nnz / bs ** 2 + 8 * (n // bs + 1) + 8 * n + 8 * n) / 1e9


def main(n_side: int = 1291, n_hex: int = 40, n_heat: int = 256, n_amg: int = 400, basis: str = "fp64") -> dict:
    import torch

    from dolfinx_external_operator_amd import Context, DeviceMesh, fgmres, gmres, rigid_body_modes
    from tools.synthetic import structured_mesh

    ctx = Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_option("consumer_overwrite", 1)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    res = {"tri_cells_per_side": n_side, "hex_boxes_per_side": n_hex, "heat_cells_per_side": n_heat, "legs": {}}

    def leg(name, fn, model_GB=None, per_batch=20):
        with torch.cuda.stream(stream):
            ms, per = _batches(torch, stream, fn, per_batch)
        r = {"ms": round(ms, 4), "batches_ms": [round(t, 4) for t in per]}
        if model_GB is not None:
            r["model_GB"] = round(model_GB, 3)
            r["TBs"] = round(model_GB / ms, 3)
            r["frac_6p3"] = round(model_GB / ms / ACHIEVABLE_TBs, 3)
        res["legs"][name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
        return ms

    def solve_figures(out):
        return {"iterations": out.iterations, "restarts": out.restarts, "converged": out.converged, "residual": out.residual,
                "ms": round(out.ms, 2), "basis_bytes": out.basis_bytes}

    def basis_legs(tag, A, M, b, t_spmv, t_pc):
        """GMRES(30) with the fp64 basis and with the compressed one at every width, same matrix, preconditioner and right-hand side."""
        default_width = ctx.get_option("krylov_basis_width")
        r = {}
        for label, kind, width in (("fp64", "fp64", default_width), ("fp32_w1", "fp32", 1), ("fp32_w2", "fp32", 2), ("fp32_w4", "fp32", 4)):
            ctx.set_option("krylov_basis_width", width)
            t_it = leg(f"{tag}_gmres30_cycle_{label}", lambda: gmres(A, b, x=torch.zeros_like(b), M=M, restart=30, rtol=1e-30, maxiter=30,
                                                                     check_every=30, basis=kind), per_batch=2) / 30
            orth = t_it - t_spmv - t_pc
            out = gmres(A, b, M=M, restart=30, rtol=1e-8, maxiter=300, basis=kind)
            r[label] = {"iteration_ms": round(t_it, 4), "orth_ms": round(orth, 4), "orth_share": round(orth / t_it, 3),
                        "solve_300": solve_figures(out)}
        ctx.set_option("krylov_basis_width", default_width)
        r["orth_ratio"] = {k: round(r[k]["orth_ms"] / r["fp64"]["orth_ms"], 3) for k in r if k != "fp64"}
        r["default_width"] = default_width
        res.setdefault("basis", {})[tag] = r

    for tag, cell, n, test, trial, bs in (("p2", "triangle", (n_side, n_side), "grad", "grad", 2),
                                          ("q2hex", "hexahedron", (n_hex, n_hex, n_hex), "eps", "eps", 3)):
        m = structured_mesh(cell, n, 2, distort=0.2, seed=0)
        dm = DeviceMesh.from_synthetic(m, ctx=ctx)
        G = m.gdim
        D = {"grad": bs * G, "eps": 4 if G == 2 else 6}[test]
        npts, nn = m.num_cells * m.nq, m.node_x.shape[0]
        try:
            with torch.cuda.stream(stream):
                pat = dm.csr_pattern(bs)
                Cd = 0.3 * torch.randn(npts * D * D, generator=gen, device=dev, dtype=torch.float64)
                Cd.view(npts, D, D).add_(torch.eye(D, device=dev, dtype=torch.float64))      # diagonal blocks stay invertible
                A = dm.bilinear_assemble(test, trial, bs, Cd.data_ptr(), pat)
                x = torch.randn(nn * bs, generator=gen, device=dev, dtype=torch.float64)
                y = torch.empty_like(x)
                res[f"{tag}_points"], res[f"{tag}_nnz"], res[f"{tag}_dofs"] = npts, pat.nnz, nn * bs
                t_spmv = leg(f"{tag}_spmv", lambda: A.matvec(x, y), spmv_model_GB(pat.nnz, nn * bs, bs))
                leg(f"{tag}_apply", lambda: dm.bilinear_apply(test, trial, bs, Cd.data_ptr(), x.data_ptr(), y.data_ptr()))
                if tag == "p2":
                    leg("p2_block_jacobi", lambda: A.block_jacobi(), per_batch=5)
                    M = A.block_jacobi()
                    t_pc = leg("p2_block_jacobi_apply", lambda: M.apply(x, y))
                    b = torch.randn(nn * bs, generator=gen, device=dev, dtype=torch.float64)
                    t_it = leg("p2_gmres30_cycle", lambda: gmres(A, b, x=torch.zeros_like(b), M=M, restart=30, rtol=1e-30, maxiter=30,
                                                                 check_every=30), per_batch=2) / 30
                    res["p2_gmres30_iteration_ms"] = round(t_it, 4)
                    res["p2_gmres30_spmv_ms"] = round(t_spmv, 4)
                    res["p2_gmres30_pc_ms"] = round(t_pc, 4)
                    res["p2_gmres30_orth_ms"] = round(t_it - t_spmv - t_pc, 4)
                    if basis == "fp32":
                        basis_legs(tag, A, M, b, t_spmv, t_pc)
                    del M, b
                elif basis == "fp32":
                    M = A.block_jacobi()
                    t_pc = leg(f"{tag}_block_jacobi_apply", lambda: M.apply(x, y))
                    b = torch.randn(nn * bs, generator=gen, device=dev, dtype=torch.float64)
                    basis_legs(tag, A, M, b, t_spmv, t_pc)
                    del M, b
                del A, Cd, x, y
            stream.synchronize()
        finally:
            dm.close()
            torch.cuda.empty_cache()

    # one full solve of a heat-type Jacobian: J = inner(k grad T^ + beta T^, grad T~), Dirichlet boundary
    import numpy as np

    m = structured_mesh("triangle", (n_heat, n_heat), 1, distort=0.2, seed=0)
    dm = DeviceMesh.from_synthetic(m, ctx=ctx)
    try:
        npts = m.num_cells * m.nq
        Cb = np.zeros((npts, 2, 3))
        Cb[:, :, 0] = 0.5                                            # dq/dT part: makes it non-symmetric
        Cb[:, 0, 1] = Cb[:, 1, 2] = 1.0 + 0.5 * np.random.Generator(np.random.PCG64(0)).random(npts)
        x = m.node_x
        bnd = np.flatnonzero((x.min(axis=1) < 1e-12) | (x.max(axis=1) > 1 - 1e-12)).astype(np.int32)
        with torch.cuda.stream(stream):
            Cd = torch.from_numpy(Cb.reshape(-1)).to(dev)
            A = dm.bilinear_assemble("grad", "value_grad", 1, Cd.data_ptr(), dm.csr_pattern(1), bcs=torch.from_numpy(bnd).to(dev))
            b = torch.ones(A.shape[0], device=dev, dtype=torch.float64)
            M = A.block_jacobi()
            gmres(A, b, M=M, rtol=1e-8, maxiter=60)                   # warm-up
            out = gmres(A, b, M=M, rtol=1e-8, maxiter=3000)
        res["heat_solve"] = {"dofs": A.shape[0], "iterations": out.iterations, "converged": out.converged, "residual": out.residual,
                             "ms": round(out.ms, 2), "ms_per_iteration": round(out.ms / max(out.iterations, 1), 4)}
    finally:
        dm.close()

    if basis == "fp32" and n_amg > 0:      # one multigrid-preconditioned elasticity solve with both bases
        m = structured_mesh("triangle", (n_amg, n_amg), 2, distort=0.2, seed=0)
        dm = DeviceMesh.from_synthetic(m, ctx=ctx)
        try:
            npts = m.num_cells * m.nq
            on = np.flatnonzero(np.abs(m.node_x[:, 1] - m.node_x[:, 1].min()) < 1e-12)
            with torch.cuda.stream(stream):
                bcs = torch.from_numpy((on[:, None] * 2 + np.arange(2)).reshape(-1).astype(np.int32)).to(dev)
                Cd = 0.3 * torch.randn(npts * 16, generator=gen, device=dev, dtype=torch.float64)
                Cd.view(npts, 4, 4).add_(torch.eye(4, device=dev, dtype=torch.float64))
                A = dm.bilinear_assemble("eps", "eps", 2, Cd.data_ptr(), dm.csr_pattern(2), bcs=bcs)
                amg = A.amg(bcs, near_nullspace=rigid_body_modes(m.node_x, ctx=ctx))
                b = torch.randn(A.shape[0], generator=gen, device=dev, dtype=torch.float64)
                r = {"dofs": A.shape[0], "levels": [lv["rows"] for lv in amg.levels]}
                for solve in (gmres, fgmres):
                    for kind in ("fp64", "fp32"):
                        solve(A, b, M=amg, restart=30, rtol=1e-8, maxiter=30, basis=kind)       # warm-up
                        out = solve(A, b, M=amg, restart=30, rtol=1e-8, maxiter=3000, basis=kind)
                        true = float((b - A.matvec(out.x)).norm() / b.norm())
                        r[f"{solve.__name__}30_{kind}"] = {**solve_figures(out), "true_residual": true,
                                                           "ms_per_iteration": round(out.ms / max(out.iterations, 1), 4)}
                amg.close()
            res["basis"]["p2eps_amg_rbm"] = r
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
    basis = "fp64"
    if "--basis" in args:
        i = args.index("--basis")
        basis = args[i + 1]
        del args[i:i + 2]
    if basis not in ("fp64", "fp32"):
        raise SystemExit("--basis: fp64 or fp32")
    r = main(*(int(a) for a in args), basis=basis)
    line = json.dumps(r)
    print(line)
    if out_file:
        pathlib.Path(out_file).write_text(line + "\n")
