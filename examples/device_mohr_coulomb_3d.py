#!/usr/bin/env python3
"""The Mohr-Coulomb slope of examples/device_mohr_coulomb_slope.py as a three-dimensional problem, solved on the device.

The 1.2 x 1.0 rectangle extruded by one layer of Q2 hexahedra in z (thickness one cell width; 18 Gauss points, 3 x 3 in the plane
and 2 across the layer: the 8-point rule leaves the Q2 stiffness matrix with near-zero-energy modes, and the element tables of the
27-point rule do not fit the 64 KiB of LDS the internal-force and matrix-free kernels work in), bottom and right faces clamped,
u_z = 0 on both z faces, body force q = load (0, -gamma, 0), the load raised from 5 to the demo's 22.99. The strain has six Mandel components and
the material is dxo_mohr_coulomb3. Per Newton iteration, all on the device:

    sigma, C_tang = MC3(eps(Du), sigma_n)          dxo_mohr_coulomb3_field (mem = DEVICE), C_tang [n][6][6]
    R = adjoint(eps, sigma) - adjoint(value, q)    dxo_operand_adjoint, bs = 3, zero on the constrained dofs
    assembled (the default):
      J = (eps, eps) form with C_tang at bs = 3    dxo_bilinear_assemble + Dirichlet rows and columns
      M = smoothed-aggregation multigrid           near-null space: the six rigid-body modes; symbolic phase once
      solve J dDu = -R                             gmres (C_tang is not symmetric in general)
    --matrix-free:
      K v: dxo_tangent_apply, diag(K): dxo_tangent_diagonal, Jacobi-preconditioned gmres, nothing assembled
    Du += dDu
and at the end of a load step u += Du and sigma_n <- sigma, a device-to-device copy. As in the plane-strain example every step starts
from Du = 0, where the return map has no tangent (deps = 0: zero iterations, C_tang = 0), so the first Newton iteration of a step
uses the elastic tangent. By the mirror symmetry of the one-layer mesh the solution is the plane-strain one: u_z and the out-of-plane
shears sigma_xz, sigma_yz vanish to the solver's tolerance, which tests/test_mohr_coulomb3_example_gpu.py checks.

    python3 examples/device_mohr_coulomb_3d.py [--n 12] [--steps K] [--matrix-free]
"""
import argparse
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dolfinx_external_operator_amd import MEM_DEVICE, Context, DeviceMesh, McParams, gmres, rigid_body_modes  # noqa: E402
from tools.synthetic import structured_mesh, with_rule  # noqa: E402

E, NU, COH, PHI, PSI, THETA_T = 6778.0, 0.25, 3.45, 30 * np.pi / 180, 30 * np.pi / 180, 26 * np.pi / 180
L, H, GAMMA = 1.2, 1.0, 1.0
MAX_NEWTON = 50


def layer_rule():
    """Gauss-Legendre 3 x 3 x 2 on the reference hexahedron, x fastest; symmetric about the mid-plane of the layer"""
    (t3, w3), (t2, w2) = np.polynomial.legendre.leggauss(3), np.polynomial.legendre.leggauss(2)
    t3, w3, t2, w2 = 0.5 * (t3 + 1.0), 0.5 * w3, 0.5 * (t2 + 1.0), 0.5 * w2
    pts = [[t3[i], t3[j], t2[k]] for k in range(2) for j in range(3) for i in range(3)]
    wts = [w3[i] * w3[j] * w2[k] for k in range(2) for j in range(3) for i in range(3)]
    return np.array(pts), np.array(wts)


def load_schedule():
    """The demo's loads from where this slope first yields (at about 4.1; below that the response is elastic and a load step of any
    size is exact), in steps of 0.8 up to the demo's last three loads."""
    return np.concatenate([np.linspace(5.0, 22.6, 23), np.array([22.9, 22.96, 22.99])])


def main(n: int = 12, steps: int | None = None, matrix_free: bool = False, verbose: bool = True) -> dict:
    """Returns the per-step Newton residuals and linear iteration counts, the final displacement `u` and the final stresses `sigma`
    ((points, 6) host arrays). Raises RuntimeError if a load step or a linear solve does not converge."""
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_option("consumer_overwrite", 1)      # residual pieces, matvec, diagonal and assembly SET their output
    mesh = structured_mesh("hexahedron", (n, n, 1), degree=2)
    mesh = with_rule(mesh, *layer_rule())
    thick = H / n
    for xs in (mesh.x, mesh.node_x):
        xs[:, 0] *= L
        xs[:, 2] *= thick
    dm = DeviceMesh.from_synthetic(mesh, ctx=ctx)
    prm = McParams(E, NU, COH, PHI, PSI, THETA_T, 0.26 * COH / np.tan(PHI), 1e-8, 200, 0)
    G = 3
    x = mesh.node_x
    nn, npts = x.shape[0], mesh.num_cells * mesh.nq
    fixed = np.zeros((nn, G), dtype=bool)
    fixed[np.abs(x[:, 1]) < 1e-12] = True
    fixed[np.abs(x[:, 0] - L) < 1e-12] = True
    fixed[(np.abs(x[:, 2]) < 1e-12) | (np.abs(x[:, 2] - thick) < 1e-12), 2] = True
    free = torch.from_numpy(~fixed.reshape(-1)).to(dev)
    bcs = torch.from_numpy(np.flatnonzero(fixed.reshape(-1)).astype(np.int32)).to(dev)

    f64 = dict(dtype=torch.float64, device=dev)
    u, Du = torch.zeros(nn * G, **f64), torch.zeros(nn * G, **f64)
    sigma_n, sigma = torch.zeros(npts * 6, **f64), torch.zeros(npts * 6, **f64)
    C_tang = torch.zeros(npts * 36, **f64)
    q = torch.zeros(npts * G, **f64)
    R, Rq, Kv, diag = (torch.zeros(nn * G, **f64) for _ in range(4))
    aux = [torch.zeros(npts, dtype=dt, device=dev) for dt in (torch.int32, torch.float64, torch.float64, torch.float64)]
    lam, mu = E * NU / ((1 + NU) * (1 - 2 * NU)), E / (2 * (1 + NU))
    Ce = 2 * mu * np.eye(6)
    Ce[:3, :3] += lam
    C_elas = torch.from_numpy(np.tile(Ce.reshape(-1), npts)).to(dev)
    state = {}

    def residual():
        ctx.mohr_coulomb3_field(prm, dm._h, MEM_DEVICE, Du.data_ptr(), sigma_n.data_ptr(), C_tang.data_ptr(), sigma.data_ptr(),
                                *(a.data_ptr() for a in aux))
        dm.adjoint("eps", G, sigma.data_ptr(), R.data_ptr())
        dm.adjoint("value", G, q.data_ptr(), Rq.data_ptr())
        return torch.where(free, R - Rq, torch.zeros_like(R))

    def solve_assembled(Cj, b):
        if "pattern" not in state:
            state["pattern"] = dm.csr_pattern(G)
            state["values"] = torch.zeros(state["pattern"].nnz, **f64)
        A = dm.bilinear_assemble("eps", "eps", G, Cj.data_ptr(), state["pattern"], values=state["values"], bcs=bcs, diagonal=1.0)
        if "amg" not in state:
            state["amg"] = A.amg(bcs, near_nullspace=rigid_body_modes(x, ctx=ctx))
        else:
            state["amg"].setup(A)
        return gmres(A, b, M=state["amg"], restart=30, rtol=1e-12, maxiter=3000)

    def solve_matrix_free(Cj, b):
        def jacobian_times(v, out):
            vm = torch.where(free, v, torch.zeros_like(v))
            dm.tangent_apply(Cj.data_ptr(), vm.data_ptr(), Kv.data_ptr())
            out.copy_(torch.where(free, Kv, v))

        dm.tangent_diagonal(Cj.data_ptr(), diag.data_ptr())
        minv = torch.where(free, 1.0 / diag, torch.ones_like(diag))
        return gmres(jacobian_times, b, M=minv, restart=64, rtol=1e-12, maxiter=20000, ctx=ctx)

    loads = load_schedule()[: steps if steps else None]
    report = {"cells": mesh.num_cells, "points": npts, "dofs": nn * G, "matrix_free": matrix_free, "steps": []}
    for i, load in enumerate(loads):
        q.view(-1, G)[:, 1] = -load * GAMMA
        Du.zero_()
        history, lin_its, t0 = [], [], time.perf_counter()
        while True:
            res = residual()
            rn = float(torch.linalg.norm(res))
            history.append(rn)
            if not np.isfinite(rn):
                raise RuntimeError(f"load {load:.3f} (step {i}): the residual is not finite")
            if rn <= max(1e-12, 1e-10 * history[0]):
                break
            if len(history) > MAX_NEWTON:
                raise RuntimeError(f"load {load:.3f} (step {i}) did not converge in {MAX_NEWTON} Newton iterations: |R| = "
                                   + " ".join(f"{r:.2e}" for r in history))
            Cj = C_elas if len(history) == 1 else C_tang
            sol = (solve_matrix_free if matrix_free else solve_assembled)(Cj, -res)
            if not sol.converged:
                raise RuntimeError(f"load {load:.3f} (step {i}), Newton iteration {len(history)}: the linear solve did not converge "
                                   f"({sol.iterations} iterations, relative residual {sol.residual:.2e})")
            lin_its.append(sol.iterations)
            Du += sol.x
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        u += Du
        sigma_n.copy_(sigma)          # the history variable never leaves the device
        report["steps"].append({"load": float(load), "newton_residuals": history, "linear_iterations": lin_its, "seconds": dt,
                                "plastic_points": int((aux[1] > 0).sum())})
        if verbose:
            print(f"step {i:2d} load {load:6.3f}: {len(history) - 1} Newton its, residuals " + " ".join(f"{r:.2e}" for r in history)
                  + f", gmres its {lin_its}, {report['steps'][-1]['plastic_points']} plastic points, {dt * 1e3:.0f} ms")
    report["load_reached"] = report["steps"][-1]["load"] if report["steps"] else 0.0
    report["stability_factor"] = report["load_reached"] * GAMMA * H / COH
    report["u"] = u.cpu().numpy()
    report["sigma"] = sigma_n.cpu().numpy().reshape(npts, 6)
    if verbose:
        print(f"{mesh.num_cells} Q2 hexahedra, {nn * G} dofs, {'matrix-free' if matrix_free else 'assembled + multigrid'}; "
              f"load reached {report['load_reached']:.3f}, load*H/c = {report['stability_factor']:.3f}")
    dm.close()
    ctx.close()
    return report


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=12, help="cells per side in x and y (one layer in z)")
    ap.add_argument("--steps", type=int, default=None, help="first K load steps only")
    ap.add_argument("--matrix-free", action="store_true", help="Jacobi-preconditioned gmres on tangent_apply, nothing assembled")
    a = ap.parse_args()
    main(a.n, a.steps, a.matrix_free)
