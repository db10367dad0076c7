#!/usr/bin/env python3
"""A nonlinear heat problem with a state-dependent boundary flux, solved by Newton's method with the boundary term IN the Jacobian.

Unit square, P2 triangles. Conductivity k(T) = 1 / (A + B T), flux q = -k(T) grad T (doc/demo/demo_nonlinear_heat_equation_part2.py:
209-261), no source. T = T_D on x = 0; on x = 1 the body loses heat by convection and radiation,

    q . n = g(T) = h (T - T_inf) + c (T^4 - T_inf^4),

the other two sides are insulated. Find T with  -int q . grad v dx + int_{x=1} g(T) v ds = 0  for all v. Per Newton iteration:

    q, dq/dT, dq/dsigma = heat flux at (T, grad T)             dxo_heat_field (operand and flux in one launch)
    R  = -sum w|J| grad(v) . q                                  dxo_operand_adjoint, kind "grad"              (SET)
    T at the facet points of x = 1, then g and dg/dT            dxo_eval_operand_facets + torch
    R += sum dS g v                                             dxo_facet_adjoint, kind "value"
    J  = (grad, value_grad) form with -[dq/dT | dq/dsigma]      dxo_bilinear_assemble                         (SET)
    J += sum dS dg/dT T_hat v  on the facets of x = 1           dxo_facet_bilinear_assemble, trial "value", then the Dirichlet rows
    solve J d = -R                                              krylov.gmres with the multigrid of J (J.amg)
    T += d
--matrix-free        J is never formed: a callable operator of dxo_bilinear_apply + dxo_facet_bilinear_apply, GMRES preconditioned by
                     the inverse of dxo_bilinear_diagonal + dxo_facet_bilinear_diagonal.
--no-facet-jacobian  the boundary term is left out of the Jacobian (not of the residual): the iteration still converges for a mild
                     boundary term, but linearly, at about the rate (dg/dT) / k.
Prints one JSON line: the Newton residual history and the norm of the solution.
Needs an MI355X.    python3 examples/device_robin_heat.py [cells_per_side] [--matrix-free] [--no-facet-jacobian] [--h H] [--c C]
"""
import argparse
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dolfinx_external_operator_amd import MEM_DEVICE, Context, DeviceMesh  # noqa: E402
from dolfinx_external_operator_amd.krylov import gmres  # noqa: E402
from dolfinx_external_operator_amd.operand_eval import DeviceCSR  # noqa: E402
from tools.synthetic import exterior_facets, facet_geometry, facet_tables, structured_mesh  # noqa: E402

A_COND, B_COND = 1.0, 1.0           # k = 1 / (A + B T)
T_D, T_INF = 1.0, 0.2


def main(n_side: int = 32, h: float = 0.1, c: float = 0.05, matrix_free: bool = False, facet_jacobian: bool = True,
         max_newton: int = 100, verbose: bool = False) -> dict:
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_option("consumer_overwrite", 1)      # the cell calls SET their output; the facet calls always add on top
    mesh = structured_mesh("triangle", (n_side, n_side), degree=2)
    dm = DeviceMesh.from_synthetic(mesh, ctx=ctx)
    dm.set_facet_tables(*facet_tables(mesh)[:3])
    dm.set_facet_geometry(*facet_geometry(mesh.cell))
    G = 2
    nn, npts = mesh.node_x.shape[0], mesh.num_cells * mesh.nq
    robin = exterior_facets(mesh, where=lambda X: np.all(X[..., 0] == 1.0, axis=1))
    fs = dm.facet_set(robin)
    nfp = fs.n * dm.nq_facet
    ents_d = torch.from_numpy(fs.entities).to(dev)
    fixed = mesh.node_x[:, 0] < 1e-12
    free = torch.from_numpy(~fixed).to(dev)
    bcs = torch.from_numpy(np.flatnonzero(fixed).astype(np.int32)).to(dev)

    f64 = dict(dtype=torch.float64, device=dev)
    T = torch.full((nn,), T_D, **f64)
    q, dqdT, dqds = torch.zeros(npts * G, **f64), torch.zeros(npts * G, **f64), torch.zeros(npts * G * G, **f64)
    mq, Cj = torch.zeros(npts * G, **f64), torch.zeros(npts, G, 1 + G, **f64)
    Tf, g, dg = torch.zeros(nfp, **f64), torch.zeros(nfp, **f64), torch.zeros(nfp, **f64)
    R, Kv, diag = torch.zeros(nn, **f64), torch.zeros(nn, **f64), torch.zeros(nn, **f64)
    pattern = dm.csr_pattern(1)
    values = torch.zeros(pattern.nnz, **f64)
    state = {}

    def residual():
        """R on the free dofs, and the blocks of the Jacobian at the current T: Cj (cells) and dg (facet points)"""
        dm.heat(A_COND, B_COND, T.data_ptr(), q.data_ptr(), dqdT.data_ptr(), dqds.data_ptr(), mem=MEM_DEVICE)
        torch.neg(q, out=mq)
        Cj[:, :, 0] = -dqdT.reshape(npts, G)
        Cj[:, :, 1:] = -dqds.reshape(npts, G, G)
        dm.adjoint("grad", 1, mq.data_ptr(), R.data_ptr())
        dm.evaluate_facets_device("value", 1, T, ents_d, out=Tf)
        g.copy_(h * (Tf - T_INF) + c * (Tf ** 4 - T_INF ** 4))
        dg.copy_(h + 4.0 * c * Tf ** 3)
        dm.facet_adjoint("value", 1, g.data_ptr(), fs, R.data_ptr())
        return torch.where(free, R, torch.zeros_like(R))

    def solve_assembled(b):
        if facet_jacobian:
            dm.bilinear_assemble("grad", "value_grad", 1, Cj.data_ptr(), pattern, values=values)
            dm.facet_bilinear_assemble("value", 1, dg.data_ptr(), fs, pattern, values=values, bcs=bcs, diagonal=1.0)
        else:
            dm.bilinear_assemble("grad", "value_grad", 1, Cj.data_ptr(), pattern, values=values, bcs=bcs, diagonal=1.0)
        if "amg" not in state:
            state["A"] = DeviceCSR(pattern, values)
            state["amg"] = state["A"].amg(constrained=bcs)
        else:
            state["amg"].setup()
        return gmres(state["A"], b, M=state["amg"], restart=30, rtol=1e-12, maxiter=600)

    def jacobian_times(v, out):
        """out = J v with the Dirichlet rows and columns of the assembled form: identity on the fixed dofs"""
        vm = torch.where(free, v, torch.zeros_like(v))
        dm.bilinear_apply("grad", "value_grad", 1, Cj.data_ptr(), vm.data_ptr(), Kv.data_ptr())
        if facet_jacobian:
            dm.facet_bilinear_apply("value", 1, dg.data_ptr(), vm.data_ptr(), fs, Kv.data_ptr())
        out.copy_(torch.where(free, Kv, v))

    def solve_matrix_free(b):
        dm.bilinear_diagonal("grad", "value_grad", 1, Cj.data_ptr(), diag.data_ptr())
        if facet_jacobian:
            dm.facet_bilinear_diagonal("value", 1, dg.data_ptr(), fs, diag.data_ptr())
        minv = torch.where(free, 1.0 / diag, torch.ones_like(diag))
        return gmres(jacobian_times, b, M=minv, restart=60, rtol=1e-12, maxiter=6000, ctx=ctx)

    history, linear_its = [], 0
    for _ in range(max_newton + 1):
        res = residual()
        rn = float(torch.linalg.norm(res))
        history.append(rn)
        if not np.isfinite(rn) or rn <= 1e-10 * history[0] or len(history) > max_newton:
            break
        sol = (solve_matrix_free if matrix_free else solve_assembled)(-res)
        if not sol.converged:
            raise RuntimeError(f"the linear solve of Newton iteration {len(history)} did not converge: {sol}")
        linear_its += sol.iterations
        T += sol.x
        if verbose:
            print(f"Newton {len(history)}: |R| = {rn:.3e}, {sol.iterations} GMRES iterations", file=sys.stderr)
    torch.cuda.synchronize()
    report = {"cells_per_side": n_side, "dofs": nn, "robin_facets": fs.n, "h": h, "c": c, "matrix_free": matrix_free,
              "facet_jacobian": facet_jacobian, "newton_residuals": history, "newton_iterations": len(history) - 1,
              "converged": bool(history[-1] <= 1e-10 * history[0]), "linear_iterations": linear_its,
              "solution_norm": float(torch.linalg.norm(T)), "T_min": float(T.min()), "T_max": float(T.max())}
    dm.close()
    ctx.close()
    return report


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("cells_per_side", nargs="?", type=int, default=32)
    ap.add_argument("--matrix-free", action="store_true")
    ap.add_argument("--no-facet-jacobian", action="store_true")
    ap.add_argument("--h", type=float, default=0.1)
    ap.add_argument("--c", type=float, default=0.05)
    ap.add_argument("--verbose", action="store_true")
    a = ap.parse_args()
    print(json.dumps(main(a.cells_per_side, a.h, a.c, a.matrix_free, not a.no_facet_jacobian, verbose=a.verbose)))
