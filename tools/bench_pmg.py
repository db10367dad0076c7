#!/usr/bin/env python3
"""One Newton linear solve of the array-free 3-D hyperelastic route under point Jacobi and under the p-multigrid on the operator
(krylov.PMG, dxo_pmg_*), on device memory:

  Q2 hexahedra with the 27-point rule, Q2 hexahedra with the 8-point rule, P2 tetrahedra with the 4-point rule; boxes per side as in
  tools/bench_hyper3_mf.py (108 and 75: about 10^7 points at the 8- and 4-point rules) unless given.

The operator is K(u) v of dxo_isihara3_tangent_apply with identity rows on the clamped face z = 0, u a small random field, the
right-hand side a random vector on the free dofs, CG to 1e-8. The p-multigrid: Chebyshev degree 2, the coarse matrix rediscretised on
DeviceMesh.vertex_mesh (1-point rule on tetrahedra, 8-point rule on hexahedra) from the injected u, a smoothed-aggregation multigrid
with the rigid-body modes of the vertices below it.

Per mesh: iterations and solve ms under both; one apply of the p-multigrid in ms, split into the operator calls (2 degree, timed
alone), the coarse cycle (timed alone), the two transfers (timed alone through dxo_pmg_restrict / dxo_pmg_prolong) and the rest, which
is the Chebyshev kernel's 2 degree launches (by difference); `symbolic_ms` (dxo_pmg_create, the coarse pattern and the multigrid's
symbolic phase, once per mesh), `setup_ms` (per Newton iteration: coarse field, assembly, multigrid setup, dxo_pmg_setup) and the
device memory in use with the p-multigrid's objects alive. Timing: warm-up, then 5 batches of 20, the median batch
(tools/bench_timing.py); solves are timed once, by their own clock. Prints one JSON line.
Needs an MI355X.    python3 tools/bench_pmg.py [hex boxes per side] [tet boxes per side]
"""
from __future__ import annotations

import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main(n_hex: int = 108, n_tet: int = 75) -> dict:
    import numpy as np
    import torch

    from dolfinx_external_operator_amd import MEM_DEVICE, PMG, Context, DeviceMesh, IsiharaParams, cg, rigid_body_modes
    from tools.bench_krylov import _batches
    from tools.synthetic import coordinate_element_at_nodes, gauss_tensor_rule, structured_mesh, vertex_companion, with_rule

    ctx = Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_option("consumer_overwrite", 1)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    prm = IsiharaParams(0.5, 1.0, 1.0, 1.5)
    f64 = dict(device=dev, dtype=torch.float64)
    res = {"device": ctx.device_info()["name"], "rtol": 1e-8, "degree": 2, "meshes": {}}

    def in_use():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free

    cases = (("Q2 hexahedra, 27 points", "hexahedron", n_hex, 3), ("Q2 hexahedra, 8 points", "hexahedron", n_hex, 2),
             ("P2 tetrahedra, 4 points", "tetrahedron", n_tet, 0))
    for name, cell, side, npd in cases:
        m = structured_mesh(cell, (side,) * 3, 2, distort=0.2, seed=0)
        if npd:
            m = with_rule(m, *gauss_tensor_rule(cell, npd))
        crule = gauss_tensor_rule(cell, 2) if cell == "hexahedron" else (np.array([[0.25, 0.25, 0.25]]), np.array([1.0 / 6.0]))
        mc = vertex_companion(m, *crule)
        dm = DeviceMesh.from_synthetic(m, ctx=ctx)
        nn, G = m.node_x.shape[0], 3
        r = {"boxes_per_side": side, "cells": m.num_cells, "points": m.num_cells * m.nq, "dofs": nn * G, "coarse_dofs": m.x.shape[0] * G}
        dmc = pmg = None
        try:
            with torch.cuda.stream(stream):
                fixed = np.zeros((nn, G), dtype=bool)
                fixed[m.node_x[:, 2] < 1e-12] = True
                free = torch.from_numpy(~fixed.reshape(-1)).to(dev)
                bcs = torch.from_numpy(np.flatnonzero(fixed.reshape(-1)).astype(np.int32)).to(dev)
                u = torch.where(free, 1e-4 * torch.randn(nn * G, generator=gen, **f64), torch.zeros(nn * G, **f64))
                b = torch.where(free, torch.randn(nn * G, generator=gen, **f64), torch.zeros(nn * G, **f64))
                Kv, diag = torch.zeros(nn * G, **f64), torch.zeros(nn * G, **f64)

                def K(v, out):
                    vm = torch.where(free, v, torch.zeros_like(v))
                    dm.isihara3_tangent_apply(prm, u.data_ptr(), vm.data_ptr(), Kv.data_ptr())
                    out.copy_(torch.where(free, Kv, v))

                dm.isihara3_tangent_diagonal(prm, u.data_ptr(), diag.data_ptr())
                minv = torch.where(free, 1.0 / diag, torch.ones_like(diag))
                used_jacobi = in_use()
                jac = cg(K, b, M=minv, rtol=1e-8, maxiter=20000, ctx=ctx)
                r["jacobi"] = {"iterations": jac.iterations, "converged": jac.converged, "solve_ms": round(jac.ms, 2), "device_bytes_in_use": used_jacobi}
                print(name, "jacobi", json.dumps(r["jacobi"]), file=sys.stderr, flush=True)

                # the symbolic part, once per mesh
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                transfer = dm.vertex_transfer(coordinate_element_at_nodes(cell, 2))
                pmg = PMG(transfer, G, constrained=bcs, ctx=ctx)
                dmc = dm.vertex_mesh(mc.psi, mc.dpsi, mc.weights)
                ctf = torch.from_numpy(transfer.coarse_to_fine.astype(np.int64)).to(dev)
                nptc = m.num_cells * mc.nq
                dPc, Pc = torch.zeros(nptc * 81, **f64), torch.zeros(nptc * 9, **f64)
                pattern_c = dmc.csr_pattern(G)
                values_c = torch.zeros(pattern_c.nnz, **f64)
                uc = u.view(nn, G)[ctf].reshape(-1).contiguous()
                ctx.isihara3_field(prm, dmc._h, MEM_DEVICE, uc.data_ptr(), dPc.data_ptr(), Pc.data_ptr())
                Ac = dmc.bilinear_assemble("grad", "grad", G, dPc.data_ptr(), pattern_c, values=values_c, bcs=pmg.coarse_constrained, diagonal=1.0)
                amg = Ac.amg(pmg.coarse_constrained, near_nullspace=rigid_body_modes(m.x, ctx=ctx))
                torch.cuda.synchronize()
                symbolic_ms = (time.perf_counter() - t0) * 1e3

                def setup():
                    ctx.isihara3_field(prm, dmc._h, MEM_DEVICE, uc.data_ptr(), dPc.data_ptr(), Pc.data_ptr())
                    A = dmc.bilinear_assemble("grad", "grad", G, dPc.data_ptr(), pattern_c, values=values_c, bcs=pmg.coarse_constrained, diagonal=1.0)
                    amg.setup(A)
                    pmg.setup(K, minv, amg)

                setup()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                setup()
                torch.cuda.synchronize()
                setup_ms = (time.perf_counter() - t0) * 1e3
                used_pmg = in_use()
                sol = cg(K, b, M=pmg, rtol=1e-8, maxiter=2000, ctx=ctx)
                # one apply, and its parts alone
                z, t = torch.zeros(nn * G, **f64), torch.zeros(nn * G, **f64)
                rc, ec = torch.randn(pmg.n_coarse, generator=gen, **f64), torch.zeros(pmg.n_coarse, **f64)
                apply_ms, _ = _batches(torch, stream, lambda: pmg.apply(b, out=z))
                op_ms, _ = _batches(torch, stream, lambda: K(b, t))
                coarse_ms, _ = _batches(torch, stream, lambda: amg.apply(rc, out=ec))
                restrict_ms, _ = _batches(torch, stream, lambda: pmg.restrict(b, out=ec))
                prolong_ms, _ = _batches(torch, stream, lambda: pmg.prolong(rc, out=t))
                calls = pmg.matvecs_per_apply
                r["pmg"] = {"iterations": sol.iterations, "converged": sol.converged, "solve_ms": round(sol.ms, 2),
                            "symbolic_ms": round(symbolic_ms, 1), "setup_ms": round(setup_ms, 2), "rho": pmg.rho,
                            "apply_ms": round(apply_ms, 4), "operator_calls": calls, "operator_ms_per_call": round(op_ms, 4),
                            "coarse_cycle_ms": round(coarse_ms, 4), "restrict_ms": round(restrict_ms, 4), "prolong_ms": round(prolong_ms, 4),
                            "chebyshev_ms_by_difference": round(apply_ms - calls * op_ms - coarse_ms - restrict_ms - prolong_ms, 4),
                            "amg_levels": amg.n_levels, "coarse_quadrature_bytes": (dPc.numel() + Pc.numel()) * 8,
                            "coarse_matrix_bytes": values_c.numel() * 8, "device_bytes_in_use": used_pmg}
                r["solve_ratio_pmg_over_jacobi"] = round(sol.ms / jac.ms, 3) if jac.ms > 0 else None
                print(name, "pmg", json.dumps(r["pmg"]), file=sys.stderr, flush=True)
        finally:
            if pmg is not None:
                pmg.close()
            if dmc is not None:
                dmc.close()
            dm.close()
        res["meshes"][name] = r
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
