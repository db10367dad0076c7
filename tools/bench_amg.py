#!/usr/bin/env python3
"""Standalone timing of the multigrid preconditioner (csrc/amg.hip; not a bench.py leg).
    python3 tools/bench_amg.py [tri_cells_per_side] [hex_boxes_per_side] [heat_small] [heat_large] [--out FILE] [--rbm] [--cheby DEG] [--strength THETA[,THETA...]] [--cycle K] [--precision fp32] [--ptransfer] [--hex-rule 27]
Systems (distorted meshes, the lower side clamped so that the matrices are regular):
  p2       ("grad", "grad", 2) on P2 triangles with C = I + 0.3 N(0, 1) per point (1291 per side: 10^7 points), as tools/bench_krylov.py
  q2hex    ("eps", "eps", 3) on Q2 hexahedra (40^3 boxes), the same kind of C
  aniso_*  ("grad", "grad", 1) with C = diag(1, 1e-3) on the heat meshes (P1, Dirichlet boundary), only with --strength
  heat_*   the heat-type Jacobian of tools/bench_krylov.py (P1, ("grad", "value_grad"), Dirichlet boundary) at two sizes (256, 1024)
Per system: dxo_csr_spmv ms, dxo_bilinear_assemble ms, the symbolic phase (host, once), dxo_amg_setup ms, dxo_amg_apply ms and its ratio
to one SpMV beside the model 2 + 3 (c - 1) (c the operator complexity), rows per level, and one GMRES(30) solve to rtol 1e-8 (at most
`maxiter` iterations) with block Jacobi and with the cycle (iterations, ms; the cycle's total adds one setup).
--rbm adds, for the two elasticity-type systems and an ("eps", "eps", 2) system p2eps on the p2 mesh, the same figures for the hierarchy
with the rigid-body modes as near-null space (keys ending in _rbm; symbolic_ms_rbm includes the tentative prolongators).
--cheby DEG adds, for every hierarchy measured (those of --rbm included), the figures of two more relaxations on the same object in the
same run, beside the default's (|Dinv A|_inf, damped Jacobi): power_jacobi (rho from the power iteration, Jacobi) and power_cheby<DEG>
(that rho, Chebyshev of degree DEG): setup ms, apply ms, rho per level, and the GMRES(30) solve (iterations, ms, ms_with_setup).
--strength adds, for every hierarchy measured (those of --rbm included) and every THETA, the hierarchy with strength-of-connection
coarsening and filtered prolongator smoothing (keys ending in _soc<THETA>): creation ms (it includes the numeric phase of every level),
rows per level, operator complexity, setup ms, apply ms, the nodes that fell back to A_ii, and the GMRES(30) solve; with --cheby DEG the
solve is repeated with power_cheby<DEG> on that hierarchy.
--cycle K adds, for every hierarchy and relaxation measured without --strength (the default's, those of --rbm and of --cheby), the
K-cycle on the same object in the same run (key "kcycle" inside the figures of the V-cycle / GMRES(30) line): apply ms, the level visits
of one apply, and one FGMRES(30) solve to rtol 1e-8 (iterations, ms; the setup is the V-cycle's).
--precision fp32 adds, for the same hierarchies and relaxations as --cycle K, the single-precision cycle on the same object in the same
run (key "fp32" beside "kcycle"): setup ms (the double setup plus the casts), apply ms, and one FGMRES(30) solve to rtol 1e-8
(iterations, ms, ms with setup); the object is back in double, set up, afterwards.
--ptransfer adds, for every hierarchy of a quadratic system measured without --strength (the default's and that of --rbm), the hierarchy
with the p-coarsening first level (DeviceMesh.vertex_transfer, first_transfer=; keys amg_p and amg_rbm_p): symbolic ms, rows per level,
operator complexity, setup ms, apply ms and the GMRES(30) solve; with --cheby DEG the solve is repeated with power_cheby<DEG>.
--hex-rule 27 adds the system q2hex27 beside q2hex: the same mesh tabulated at the 27-point Gauss rule, with the constant isotropic
elasticity tensor (lambda 1, mu 0.7). q2hex itself is assembled with the 8-point rule, which under-integrates the 27-node element
(spurious zero-energy modes): no preconditioner makes it converge, see DESIGN 9.5.
Timing: warm-up, then 5 batches timed with HIP events on the launch stream, the MEDIAN batch reported (tools/bench_krylov._batches).
Prints one JSON line."""
from __future__ import annotations

import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main(n_side: int = 1291, n_hex: int = 40, n_heat: int = 256, n_heat_large: int = 1024, maxiter: int = 3000, rbm: bool = False,
         cheby: int = 0, strengths: tuple = (), cycle: str = "V", precision: str = "fp64", ptransfer: bool = False,
         hex_rule: int = 8) -> dict:
    import numpy as np
    import torch

    from dolfinx_external_operator_amd import Context, DeviceMesh, fgmres, gmres, rigid_body_modes
    from tools.bench_krylov import _batches
    from tools.synthetic import coordinate_element_at_nodes, gauss_tensor_rule, structured_mesh, with_rule

    ctx = Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_option("consumer_overwrite", 1)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    res = {"maxiter": maxiter, "systems": {}}

    def timed(fn, per_batch):
        ms, _ = _batches(torch, stream, fn, per_batch=per_batch, warm=2)
        return round(ms, 4)

    def kcycle(amg, A, b, x, y, setup_ms):
        """The K-cycle of the hierarchy as it stands, under FGMRES(30); the object is a V-cycle again afterwards."""
        amg.set_cycle("K")
        f = {"apply_ms": timed(lambda: amg.apply(x, y), 20), "visits": amg.visits}
        fgmres(A, b, M=amg, rtol=1e-8, maxiter=30)                           # warm-up (and the second basis)
        out = fgmres(A, b, M=amg, restart=30, rtol=1e-8, maxiter=maxiter)
        f.update({"iterations": out.iterations, "converged": out.converged, "residual": out.residual, "ms": round(out.ms, 2),
                  "ms_with_setup": round(out.ms + setup_ms, 2)})
        amg.set_cycle("V")
        return f

    def fp32(amg, A, b, x, y):
        """The single-precision cycle of the hierarchy as it stands, under FGMRES(30); the object is in double again afterwards."""
        amg.set_precision("fp32").setup()
        f = {"setup_ms": timed(lambda: amg.setup(), 3), "apply_ms": timed(lambda: amg.apply(x, y), 20), "fp32_bytes": amg.fp32_bytes}
        fgmres(A, b, M=amg, rtol=1e-8, maxiter=30)                           # warm-up (and the second basis)
        out = fgmres(A, b, M=amg, restart=30, rtol=1e-8, maxiter=maxiter)
        f.update({"iterations": out.iterations, "converged": out.converged, "residual": out.residual, "ms": round(out.ms, 2),
                  "ms_with_setup": round(out.ms + f["setup_ms"], 2)})
        amg.set_precision("fp64").setup()
        return f

    def relaxations(amg, A, b, x, y, r, suffix):
        for key, kw in (("power_jacobi", {"rho": "power"}), (f"power_cheby{cheby}", {"smoother": "chebyshev", "degree": cheby, "rho": "power"})):
            amg.set_smoother(**kw).setup()
            f = {"setup_ms": timed(lambda: amg.setup(), 3), "apply_ms": timed(lambda: amg.apply(x, y), 20), "rho": amg.rho}
            gmres(A, b, M=amg, rtol=1e-8, maxiter=30)                        # warm-up
            out = gmres(A, b, M=amg, restart=30, rtol=1e-8, maxiter=maxiter)
            f.update({"iterations": out.iterations, "converged": out.converged, "residual": out.residual, "ms": round(out.ms, 2),
                      "ms_with_setup": round(out.ms + f["setup_ms"], 2)})
            if cycle == "K":
                f["kcycle"] = kcycle(amg, A, b, x, y, f["setup_ms"])
            if precision == "fp32":
                f["fp32"] = fp32(amg, A, b, x, y)
            r[key + suffix] = f

    def with_strength(A, bcs, nns, b, x, y, r, suffix):
        for theta in strengths:
            amg = A.amg(bcs, near_nullspace=nns, strength=theta)
            f = {"creation_ms": round(amg.build_ms, 1), "setup_ms": timed(lambda: amg.setup(), 3), "apply_ms": timed(lambda: amg.apply(x, y), 20),
                 "rows": [d["rows"] for d in amg.levels], "operator_complexity": round(amg.operator_complexity, 4),
                 "unlumped_nodes": amg.unlumped_nodes}
            relax = [("gmres30", {})] + ([(f"gmres30_power_cheby{cheby}", {"smoother": "chebyshev", "degree": cheby, "rho": "power"})] if cheby else [])
            for key, kw in relax:
                if kw:
                    amg.set_smoother(**kw).setup()
                gmres(A, b, M=amg, rtol=1e-8, maxiter=30)                    # warm-up
                out = gmres(A, b, M=amg, restart=30, rtol=1e-8, maxiter=maxiter)
                f[key] = {"iterations": out.iterations, "converged": out.converged, "residual": out.residual, "ms": round(out.ms, 2)}
            r[f"amg{suffix}_soc{theta:g}"] = f
            amg.close()

    def with_ptransfer(dm, m, A, bcs, nns, b, x, y, r, suffix):
        if not ptransfer or m.degree != 2:
            return
        try:
            amg = A.amg(bcs, near_nullspace=nns, first_transfer=dm.vertex_transfer(coordinate_element_at_nodes(m.cell, 2)))
        except ValueError as e:              # a singular level: reported, the other figures of the run stand
            r[f"amg{suffix}_p"] = {"error": str(e)}
            return
        f = {"symbolic_ms": round(amg.build_ms, 1), "setup_ms": timed(lambda: amg.setup(), 3), "apply_ms": timed(lambda: amg.apply(x, y), 20),
             "rows": [d["rows"] for d in amg.levels], "operator_complexity": round(amg.operator_complexity, 4)}
        relax = [("gmres30", {})] + ([(f"gmres30_power_cheby{cheby}", {"smoother": "chebyshev", "degree": cheby, "rho": "power"})] if cheby else [])
        for key, kw in relax:
            g = {}
            if kw:
                amg.set_smoother(**kw).setup()
                g = {"setup_ms": timed(lambda: amg.setup(), 3), "apply_ms": timed(lambda: amg.apply(x, y), 20)}
            gmres(A, b, M=amg, rtol=1e-8, maxiter=30)                        # warm-up
            out = gmres(A, b, M=amg, restart=30, rtol=1e-8, maxiter=maxiter)
            g.update({"iterations": out.iterations, "converged": out.converged, "residual": out.residual, "ms": round(out.ms, 2),
                      "ms_with_setup": round(out.ms + g.get("setup_ms", f["setup_ms"]), 2)})
            f[key] = g
        r[f"amg{suffix}_p"] = f
        amg.close()

    def system(tag, m, test, trial, bs, Cd, bnd):
        dm = DeviceMesh.from_synthetic(m, ctx=ctx)
        try:
            with torch.cuda.stream(stream):
                pat = dm.csr_pattern(bs)
                bcs = torch.from_numpy(bnd.astype(np.int32)).to(dev)
                A = dm.bilinear_assemble(test, trial, bs, Cd.data_ptr(), pat, bcs=bcs)
                n = A.shape[0]
                x = torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
                y = torch.empty_like(x)
                r = {"dofs": n, "nnz": pat.nnz, "points": m.num_cells * m.nq}
                r["spmv_ms"] = timed(lambda: A.matvec(x, y), 20)
                r["assemble_ms"] = timed(lambda: dm.bilinear_assemble(test, trial, bs, Cd.data_ptr(), pat, values=A.values, bcs=bcs), 3)
                amg = A.amg(bcs)
                r["symbolic_ms"] = round(amg.build_ms, 1)
                r["setup_ms"] = timed(lambda: amg.setup(), 3)
                r["apply_ms"] = timed(lambda: amg.apply(x, y), 20)
                c = amg.operator_complexity
                r["levels"] = amg.levels
                r["operator_complexity"] = round(c, 4)
                r["apply_over_spmv"] = round(r["apply_ms"] / r["spmv_ms"], 2)
                r["apply_over_spmv_model"] = round(2 + 3 * (c - 1), 2)
                b = torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
                for name, M in (("block_jacobi", A.block_jacobi()), ("amg", amg)):
                    gmres(A, b, M=M, rtol=1e-8, maxiter=30)                  # warm-up
                    out = gmres(A, b, M=M, restart=30, rtol=1e-8, maxiter=maxiter)
                    r[f"gmres30_{name}"] = {"iterations": out.iterations, "converged": out.converged, "residual": out.residual,
                                            "ms": round(out.ms, 2)}
                r["gmres30_amg"]["ms_with_setup"] = round(r["gmres30_amg"]["ms"] + r["setup_ms"], 2)
                if cycle == "K":
                    r["gmres30_amg"]["kcycle"] = kcycle(amg, A, b, x, y, r["setup_ms"])
                if precision == "fp32":
                    r["gmres30_amg"]["fp32"] = fp32(amg, A, b, x, y)
                if cheby:
                    relaxations(amg, A, b, x, y, r, "")
                amg.close()
                with_ptransfer(dm, m, A, bcs, None, b, x, y, r, "")
                with_strength(A, bcs, None, b, x, y, r, "")
                if rbm and bs == m.gdim:
                    amg = A.amg(bcs, near_nullspace=rigid_body_modes(m.node_x, ctx=ctx))
                    r["symbolic_ms_rbm"] = round(amg.build_ms, 1)
                    r["setup_ms_rbm"] = timed(lambda: amg.setup(), 3)
                    r["apply_ms_rbm"] = timed(lambda: amg.apply(x, y), 20)
                    r["levels_rbm"] = amg.levels
                    r["dead_columns_rbm"] = amg.dead_columns
                    r["operator_complexity_rbm"] = round(amg.operator_complexity, 4)
                    gmres(A, b, M=amg, rtol=1e-8, maxiter=30)
                    out = gmres(A, b, M=amg, restart=30, rtol=1e-8, maxiter=maxiter)
                    r["gmres30_amg_rbm"] = {"iterations": out.iterations, "converged": out.converged, "residual": out.residual,
                                            "ms": round(out.ms, 2), "ms_with_setup": round(out.ms + r["setup_ms_rbm"], 2)}
                    if cycle == "K":
                        r["gmres30_amg_rbm"]["kcycle"] = kcycle(amg, A, b, x, y, r["setup_ms_rbm"])
                    if precision == "fp32":
                        r["gmres30_amg_rbm"]["fp32"] = fp32(amg, A, b, x, y)
                    if cheby:
                        relaxations(amg, A, b, x, y, r, "_rbm")
                    amg.close()
                    with_ptransfer(dm, m, A, bcs, rigid_body_modes(m.node_x, ctx=ctx), b, x, y, r, "_rbm")
                    with_strength(A, bcs, rigid_body_modes(m.node_x, ctx=ctx), b, x, y, r, "_rbm")
            stream.synchronize()
            res["systems"][tag] = r
            print(tag, json.dumps(r), file=sys.stderr, flush=True)
        finally:
            dm.close()
            torch.cuda.empty_cache()

    def lower_side(m, bs):
        on = np.flatnonzero(np.abs(m.node_x[:, 1] - m.node_x[:, 1].min()) < 1e-12)
        return (on[:, None] * bs + np.arange(bs)).reshape(-1)

    for n in (n_heat, n_heat_large):
        if n <= 0:
            continue
        m = structured_mesh("triangle", (n, n), 1, distort=0.2, seed=0)
        npts = m.num_cells * m.nq
        Cb = np.zeros((npts, 2, 3))
        Cb[:, :, 0] = 0.5                                            # dq/dT part: makes it non-symmetric
        Cb[:, 0, 1] = Cb[:, 1, 2] = 1.0 + 0.5 * np.random.Generator(np.random.PCG64(0)).random(npts)
        bnd = np.flatnonzero((m.node_x.min(axis=1) < 1e-12) | (m.node_x.max(axis=1) > 1 - 1e-12))
        system(f"heat_{n}", m, "grad", "value_grad", 1, torch.from_numpy(Cb.reshape(-1)).to(dev), bnd)
        if strengths:
            Ca = np.broadcast_to(np.diag([1.0, 1e-3]), (npts, 2, 2)).copy()
            system(f"aniso_{n}", m, "grad", "grad", 1, torch.from_numpy(Ca.reshape(-1)).to(dev), bnd)
    cases = [("p2", "triangle", (n_side, n_side), "grad", "grad", 2), ("q2hex", "hexahedron", (n_hex, n_hex, n_hex), "eps", "eps", 3)]
    if rbm:
        cases.append(("p2eps", "triangle", (n_side, n_side), "eps", "eps", 2))
    for tag, cell, n, test, trial, bs in cases:
        if n[0] <= 0:
            continue
        m = structured_mesh(cell, n, 2, distort=0.2, seed=0)
        G = m.gdim
        D = {"grad": bs * G, "eps": 4 if G == 2 else 6}[test]
        npts = m.num_cells * m.nq
        Cd = 0.3 * torch.randn(npts * D * D, generator=gen, device=dev, dtype=torch.float64)
        Cd.view(npts, D, D).add_(torch.eye(D, device=dev, dtype=torch.float64))
        system(tag, m, test, trial, bs, Cd, lower_side(m, bs))
        if tag == "q2hex" and hex_rule == 27:
            m27 = with_rule(m, *gauss_tensor_rule(cell, 3))
            Ce = torch.zeros(6, 6, device=dev, dtype=torch.float64)
            Ce[:3, :3] = 1.0
            Ce += 1.4 * torch.eye(6, device=dev, dtype=torch.float64)
            system("q2hex27", m27, test, trial, bs, Ce.expand(m27.num_cells * m27.nq, 6, 6).contiguous().view(-1), lower_side(m27, bs))
    ctx.close()
    return res


if __name__ == "__main__":
    args = sys.argv[1:]
    out_file = None
    if "--out" in args:
        i = args.index("--out")
        out_file = args[i + 1]
        del args[i:i + 2]
    rbm = "--rbm" in args
    if rbm:
        args.remove("--rbm")
    cheby = 0
    if "--cheby" in args:
        i = args.index("--cheby")
        cheby = int(args[i + 1])
        del args[i:i + 2]
    strengths = ()
    if "--strength" in args:
        i = args.index("--strength")
        strengths = tuple(float(t) for t in args[i + 1].split(","))
        del args[i:i + 2]
    cycle = "V"
    if "--cycle" in args:
        i = args.index("--cycle")
        cycle = args[i + 1]
        del args[i:i + 2]
    precision = "fp64"
    if "--precision" in args:
        i = args.index("--precision")
        precision = args[i + 1]
        del args[i:i + 2]
    ptransfer = "--ptransfer" in args
    if ptransfer:
        args.remove("--ptransfer")
    hex_rule = 8
    if "--hex-rule" in args:
        i = args.index("--hex-rule")
        hex_rule = int(args[i + 1])
        del args[i:i + 2]
        if hex_rule not in (8, 27):
            raise SystemExit("--hex-rule takes 8 or 27")
    r = main(*(int(a) for a in args), rbm=rbm, cheby=cheby, strengths=strengths, cycle=cycle, precision=precision, ptransfer=ptransfer,
             hex_rule=hex_rule)
    line = json.dumps(r)
    print(line)
    if out_file:
        pathlib.Path(out_file).write_text(line + "\n")
