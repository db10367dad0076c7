#!/usr/bin/env python3
"""A finite-strain Newton solve in three dimensions in which quadrature data never leaves the GPU: a unit cube of the Isihara solid,
clamped at the bottom, compressed and twisted at the top. The 3-D counterpart of examples/device_hyperelasticity.py.

Per Newton iteration:

    dP, P = Isihara(I + grad u)                  dxo_isihara3_field (operand and model in one launch, fp64; F is 3x3, dP [n][9][9])
    R = sum w|J| grad(v) : P  on the free dofs   dxo_operand_adjoint, kind "F", bs = 3
    assembled (the default):
      J = (grad, grad) form with dP              dxo_bilinear_assemble on the CSR pattern of the mesh, Dirichlet rows and columns
      M = smoothed-aggregation multigrid         DeviceCSR.amg(near_nullspace = the six rigid-body modes); symbolic phase once
      solve J d = -R                             cg (or gmres)
    --matrix-free:
      K v: dxo_bilinear_apply("grad", "grad", 3, dP), diag(K): dxo_bilinear_diagonal, Jacobi-preconditioned cg
    --matrix-free --recompute (--model isihara only): no quadrature array at all. R, K v and diag(K) are formed from u alone,
      F = I + grad u and the model evaluated again in the registers of every call (dxo_isihara3_residual,
      dxo_isihara3_tangent_apply, dxo_isihara3_tangent_diagonal): dP [n][9][9] and P [n][9], 720 bytes per point, are never allocated
    --matrix-free --pc pmg: the Krylov solve is preconditioned by a two-level p-multigrid on the operator (krylov.PMG, dxo_pmg_*) in
      place of point Jacobi: Chebyshev smoothing with K v and diag(K) alone, and a coarse correction on the degree-1 space of the same
      cells. Per Newton iteration the coarse u_c = u[coarse_to_fine] is an injection, dxo_isihara3_field (the model's field call) runs on the degree-1
      companion mesh (DeviceMesh.vertex_mesh; the 1-point rule on tetrahedra, the 8-point rule on hexahedra), dxo_bilinear_assemble
      gives the degree-1 matrix with the coarse Dirichlet set of the PMG, and a smoothed-aggregation multigrid with the six
      rigid-body modes of the vertices (symbolic phase once) is the coarse preconditioner. With --recompute the coarse dP array is
      the one quadrature array this route still holds: 81 doubles per coarse point, against 4 (tetrahedra) or 27 (hexahedra) fine
      points per cell, a quarter or 8/27 of the fine dP array, before the per-point data of P (`coarse_bytes` in the report also
      counts the coarse P, the coarse matrix and the values of the hierarchy below it)
    u += d
Only dof vectors are touched outside the kernels; they are torch CUDA tensors.

Mesh: P2 tetrahedra with the 4-point rule (the default), or --hex: Q2 hexahedra with the 27-point Gauss rule (the 8-point rule
under-integrates the Q2 stiffness matrix: it is singular). Load: the top face moves down by `compress` and turns about
the cube's axis by `twist` radians, both reached over `steps` equal load steps; a step's predictor moves every node by the
homogeneous field that meets both faces. The model is fp64 and the tangent exact, so Newton converges quadratically.
--model icnn --weights FILE: the constitutive law is the input-convex network of the reference's demo instead (dxo_icnn3_field: the
operand kernel, then the network kernel on the invariants of the 3x3 F). FILE is the model's state_dict, a torch file
(`Isihara_noise=high.pth`) or an .npz with '__' for '.' in the keys. --precision fp64 (the default here) evaluates the network in
fp64, so that stress and tangent are consistent to fp64 rounding and the residual can fall by the ten decades the Newton loop asks
for; with fp32, the reference's network precision, the stress carries fp32 rounding (about 1e-7) and the loop's tolerance may be out of reach.
Needs an MI355X.    python3 examples/device_hyperelasticity_3d.py [--n 6] [--hex] [--matrix-free [--recompute]] [--solver cg|gmres]
                                                                   [--pc jacobi|pmg] [--model isihara|icnn] [--weights FILE] [--precision fp32|fp64]
"""
import argparse
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dolfinx_external_operator_amd import MEM_DEVICE, PMG, Context, DeviceMesh, IsiharaParams, cg, gmres, rigid_body_modes  # noqa: E402
from tools.synthetic import coordinate_element_at_nodes, gauss_tensor_rule, structured_mesh, vertex_companion, with_rule  # noqa: E402

MAX_NEWTON = 20      # a load step that needs more has failed


def predictor(x: np.ndarray, compress: float, twist: float) -> np.ndarray:
    """u(x) of the homogeneous compression and twist: the section at height z moves down by compress * z and turns by twist * z"""
    ang = twist * x[:, 2]
    dx, dy = x[:, 0] - 0.5, x[:, 1] - 0.5
    u = np.zeros_like(x)
    u[:, 0] = np.cos(ang) * dx - np.sin(ang) * dy - dx
    u[:, 1] = np.sin(ang) * dx + np.cos(ang) * dy - dy
    u[:, 2] = -compress * x[:, 2]
    return u


def load_state_dict(path):
    """the network's state_dict from a torch file or an .npz (keys with '__' for '.')"""
    if path is None:
        raise ValueError("--model icnn needs --weights FILE (the state_dict of the trained network)")
    if str(path).endswith(".npz"):
        return dict(np.load(path))
    return torch.load(path, map_location="cpu")


def main(n_side: int = 6, steps: int = 3, compress: float = 0.15, twist: float = 0.4, hexahedra: bool = False, matrix_free: bool = False,
         solver: str = "cg", verbose: bool = True, c=(0.5, 1.0, 1.0, 1.5), model: str = "isihara", weights=None,
         precision: str = "fp64", recompute: bool = False, pc: str = "jacobi") -> dict:
    """Returns the per-step Newton residual histories, the linear iteration counts, the bytes of quadrature data held
    (`quadrature_bytes`: dP and P, 720 per point; 0 with `recompute`), the preconditioner of the matrix-free solve (`pc`), what its
    coarse level holds (`coarse_bytes`: the coarse dP and P arrays, the coarse matrix and the values of the hierarchy below it; 0
    with "jacobi") and the final displacement (`u`, host array).
    Raises RuntimeError if a load step does not converge within MAX_NEWTON iterations or a linear solve fails."""
    if recompute and not (matrix_free and model == "isihara"):
        raise ValueError("recompute needs matrix_free and the analytic model (--matrix-free --model isihara)")
    if pc not in ("jacobi", "pmg"):
        raise ValueError('pc must be "jacobi" or "pmg"')
    if pc == "pmg" and not matrix_free:
        raise ValueError("pc pmg needs matrix_free (--matrix-free): the assembled route has the multigrid of its matrix")
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_option("consumer_overwrite", 1)      # residual / matvec / diagonal / assembly calls SET their output
    if hexahedra:
        mesh = structured_mesh("hexahedron", (n_side,) * 3, degree=2)
        mesh = with_rule(mesh, *gauss_tensor_rule("hexahedron", 3))
    else:
        mesh = structured_mesh("tetrahedron", (n_side,) * 3, degree=2)
    dm = DeviceMesh.from_synthetic(mesh, ctx=ctx)
    prm = IsiharaParams(*c)
    if model not in ("isihara", "icnn"):
        raise ValueError('model must be "isihara" or "icnn"')
    net = ctx.icnn_create(load_state_dict(weights)) if model == "icnn" else None
    net_precision = {"fp32": 0, "fp64": 1}[precision]
    G = 3
    x = mesh.node_x
    nn, npts = x.shape[0], mesh.num_cells * mesh.nq
    bottom, top = x[:, 2] < 1e-12, x[:, 2] > 1 - 1e-12
    fixed = np.zeros((nn, G), dtype=bool)
    fixed[bottom] = True
    fixed[top] = True
    free = torch.from_numpy(~fixed.reshape(-1)).to(dev)
    bcs = torch.from_numpy(np.flatnonzero(fixed.reshape(-1)).astype(np.int32)).to(dev)

    f64 = dict(dtype=torch.float64, device=dev)
    u = torch.zeros(nn * G, **f64)
    dP, P = (None, None) if recompute else (torch.zeros(npts * 81, **f64), torch.zeros(npts * 9, **f64))
    R, Kv, diag = (torch.zeros(nn * G, **f64) for _ in range(3))
    state = {}
    krylov = {"cg": cg, "gmres": gmres}[solver]

    def residual():
        """(dP, P) at the current u and the assembled inner(grad v, P) dx on the free dofs; with recompute, the latter from u alone"""
        if recompute:
            dm.isihara3_residual(prm, u.data_ptr(), R.data_ptr())
            return torch.where(free, R, torch.zeros_like(R))
        if net is None:
            ctx.isihara3_field(prm, dm._h, MEM_DEVICE, u.data_ptr(), dP.data_ptr(), P.data_ptr())
        else:
            ctx.icnn3_field(net, net_precision, dm._h, MEM_DEVICE, u.data_ptr(), dP.data_ptr(), P.data_ptr())
        dm.adjoint("F", G, P.data_ptr(), R.data_ptr())
        return torch.where(free, R, torch.zeros_like(R))

    def solve_assembled(b):
        if "pattern" not in state:
            state["pattern"] = dm.csr_pattern(G)
            state["values"] = torch.zeros(state["pattern"].nnz, **f64)
        A = dm.bilinear_assemble("grad", "grad", G, dP.data_ptr(), state["pattern"], values=state["values"], bcs=bcs, diagonal=1.0)
        if "amg" not in state:
            state["amg"] = A.amg(bcs, near_nullspace=rigid_body_modes(x, ctx=ctx))
        else:
            state["amg"].setup(A)
        return krylov(A, b, M=state["amg"], rtol=1e-12, maxiter=400)

    def jacobian_times(v, out):
        """out = K v with the Dirichlet rows and columns of the assembled form: identity on the fixed dofs"""
        vm = torch.where(free, v, torch.zeros_like(v))
        if recompute:
            dm.isihara3_tangent_apply(prm, u.data_ptr(), vm.data_ptr(), Kv.data_ptr())
        else:
            dm.bilinear_apply("grad", "grad", G, dP.data_ptr(), vm.data_ptr(), Kv.data_ptr())
        out.copy_(torch.where(free, Kv, v))

    def coarse_level():
        """The degree-1 matrix at the injected u and its multigrid; the objects are made at the first call"""
        if "pmg" not in state:
            if hexahedra:
                rule = gauss_tensor_rule("hexahedron", 2)
            else:
                rule = (np.array([[0.25, 0.25, 0.25]]), np.array([1.0 / 6.0]))
            mc = vertex_companion(mesh, *rule)
            transfer = dm.vertex_transfer(coordinate_element_at_nodes(mesh.cell, 2))
            state["pmg"] = PMG(transfer, G, constrained=bcs, ctx=ctx)
            state["dmc"] = dmc = dm.vertex_mesh(mc.psi, mc.dpsi, mc.weights)
            state["ctf"] = torch.from_numpy(transfer.coarse_to_fine.astype(np.int64)).to(dev)
            nptc = mesh.num_cells * mc.nq
            state["dPc"], state["Pc"] = torch.zeros(nptc * 81, **f64), torch.zeros(nptc * 9, **f64)
            state["pattern_c"] = dmc.csr_pattern(G)
            state["values_c"] = torch.zeros(state["pattern_c"].nnz, **f64)
        dmc = state["dmc"]
        uc = u.view(nn, G)[state["ctf"]].reshape(-1).contiguous()
        if net is None:
            ctx.isihara3_field(prm, dmc._h, MEM_DEVICE, uc.data_ptr(), state["dPc"].data_ptr(), state["Pc"].data_ptr())
        else:
            ctx.icnn3_field(net, net_precision, dmc._h, MEM_DEVICE, uc.data_ptr(), state["dPc"].data_ptr(), state["Pc"].data_ptr())
        Ac = dmc.bilinear_assemble("grad", "grad", G, state["dPc"].data_ptr(), state["pattern_c"], values=state["values_c"],
                                   bcs=state["pmg"].coarse_constrained, diagonal=1.0)
        if "amg_c" not in state:
            state["amg_c"] = Ac.amg(state["pmg"].coarse_constrained, near_nullspace=rigid_body_modes(mesh.x, ctx=ctx))
            amg = state["amg_c"]
            report["coarse_bytes"] = (sum(t.numel() * t.element_size() for t in (state["dPc"], state["Pc"], state["values_c"]))
                                      + sum(8 * d["block_nnz"] * d["bs"] ** 2 for d in amg.levels[1:]))
        else:
            state["amg_c"].setup(Ac)
        return state["amg_c"]

    def solve_matrix_free(b):
        if recompute:
            dm.isihara3_tangent_diagonal(prm, u.data_ptr(), diag.data_ptr())
        else:
            dm.bilinear_diagonal("grad", "grad", G, dP.data_ptr(), diag.data_ptr())
        minv = torch.where(free, 1.0 / diag, torch.ones_like(diag))
        if pc == "pmg":
            amg = coarse_level()
            return krylov(jacobian_times, b, M=state["pmg"].setup(jacobian_times, minv, amg), rtol=1e-12, maxiter=20000, ctx=ctx)
        return krylov(jacobian_times, b, M=minv, rtol=1e-12, maxiter=20000, ctx=ctx)

    report = {"cells": mesh.num_cells, "points": npts, "dofs": nn * G, "matrix_free": matrix_free, "solver": solver, "model": model, "recompute": recompute,
              "quadrature_bytes": sum(t.numel() * t.element_size() for t in (dP, P) if t is not None), "pc": pc if matrix_free else "amg",
              "coarse_bytes": 0, "steps": []}
    if verbose:
        print(f"{npts} points, quadrature data held: {report['quadrature_bytes']} bytes ({'none' if recompute else '720 per point: dP [n][9][9] and P [n][9]'})")
    prev = np.zeros_like(x)
    for k in range(1, steps + 1):
        lam = k / steps
        now = predictor(x, lam * compress, lam * twist)
        u += torch.from_numpy((now - prev).reshape(-1)).to(dev)
        prev = now
        history, lin_its, t0 = [], [], time.perf_counter()
        while True:
            res = residual()
            rn = float(torch.linalg.norm(res))
            history.append(rn)
            if not np.isfinite(rn):
                raise RuntimeError(f"load step {k}: the residual is not finite (det F <= 0 at a quadrature point)")
            if rn <= 1e-10 * history[0]:
                break
            if len(history) > MAX_NEWTON:
                raise RuntimeError(f"load step {k} did not converge in {MAX_NEWTON} Newton iterations: |R| = " + " ".join(f"{r:.2e}" for r in history))
            sol = (solve_matrix_free if matrix_free else solve_assembled)(-res)
            if not sol.converged:
                raise RuntimeError(f"load step {k}, Newton iteration {len(history)}: the linear solve did not converge "
                                   f"({sol.iterations} iterations, relative residual {sol.residual:.2e})")
            lin_its.append(sol.iterations)
            u += sol.x
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        report["steps"].append({"load": lam, "newton_residuals": history, "linear_iterations": lin_its, "seconds": dt})
        if verbose:
            print(f"load {lam:.3f}: {len(history) - 1} Newton its, residuals " + " ".join(f"{r:.2e}" for r in history)
                  + f", {solver} its {lin_its}, {dt * 1e3:.0f} ms")
    report["u"] = u.cpu().numpy()
    if net is not None:
        ctx.icnn_destroy(net)
    if "pmg" in state:
        state["pmg"].close()
        state["dmc"].close()
    dm.close()
    ctx.close()
    return report


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=6, help="cells per side")
    ap.add_argument("--steps", type=int, default=3, help="load steps")
    ap.add_argument("--hex", action="store_true", help="Q2 hexahedra with the 27-point rule instead of P2 tetrahedra")
    ap.add_argument("--matrix-free", action="store_true", help="Jacobi-preconditioned Krylov solve on bilinear_apply, nothing assembled")
    ap.add_argument("--recompute", action="store_true", help="with --matrix-free --model isihara: residual, K v and diag(K) from u alone, "
                    "no quadrature array (dP, P) is allocated")
    ap.add_argument("--solver", choices=["cg", "gmres"], default="cg")
    ap.add_argument("--pc", choices=["jacobi", "pmg"], default="jacobi", help="with --matrix-free: point Jacobi (default) or the two-level "
                    "p-multigrid on the operator")
    ap.add_argument("--model", choices=["isihara", "icnn"], default="isihara", help="the analytic energy (default) or the trained network")
    ap.add_argument("--weights", help="--model icnn: the network's state_dict (torch file or .npz)")
    ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp64", help="--model icnn: precision of the network")
    a = ap.parse_args()
    if a.recompute and not (a.matrix_free and a.model == "isihara"):
        ap.error("--recompute is valid only with --matrix-free and --model isihara")
    if a.pc == "pmg" and not a.matrix_free:
        ap.error("--pc pmg is valid only with --matrix-free")
    main(a.n, steps=a.steps, hexahedra=a.hex, matrix_free=a.matrix_free, solver=a.solver, model=a.model, weights=a.weights, precision=a.precision,
         recompute=a.recompute, pc=a.pc)
