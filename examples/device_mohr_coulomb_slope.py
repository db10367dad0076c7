#!/usr/bin/env python3
"""The Mohr-Coulomb demo's global problem, a slope under gravity (demo_plasticity_mohr_coulomb.py:110-735), solved on the device.

A 1.2 x 1.0 rectangle of P2 triangles, bottom and right edges clamped, body force q = load (0, -gamma) with the demo's load schedule
(np.linspace(2, 22.9, 50), then 22.96 and 22.99). Per Newton iteration, all on the device:

    sigma, C_tang = MC(eps(Du), sigma_n)        dxo_mohr_coulomb_field (mem = DEVICE)
    R = adjoint(eps, sigma) - adjoint(value, q) dxo_operand_adjoint, zero on the clamped dofs
    J = assembled (eps, eps) form with C_tang   dxo_bilinear_assemble + dxo_csr_dirichlet (identity rows)
    solve J dDu = -R                            gmres with block Jacobi (dxo_krylov_gmres), --solver amg: gmres with the multigrid cycle (amg-rbm: with the rigid-body modes as its near-null space, amg-cheby: those modes, the power estimate of rho and Chebyshev smoothing of degree 2, amg-soc: those modes and strength-of-connection coarsening with theta 0.1, the masks of the first Newton iteration kept, amg-k: amg-rbm with the K-cycle, under flexible GMRES, amg-fp32: amg-cheby with the cycle in single precision, under flexible GMRES, amg-p: amg-cheby with the p-coarsening first level, the degree-1 space on the same cells, in front of the aggregation: the mesh here is quadratic), --solver lu: splu on the host
    Du += dDu
and at the end of a load step u += Du, sigma_n <- sigma. C_tang is the derivative through the return map and is not symmetric in
general, hence GMRES. Newton stops at |R| <= max(1e-8, 1e-8 |R_0|) (the demo's snes_atol / snes_rtol). Each step starts from
Du = 0, where the return map has no tangent: with deps = 0 its initial residual is zero, the reference's Newton loop tests
0 / 0 and runs no iteration, so jacfwd gives C_tang = 0 (demo_plasticity_mohr_coulomb.py:497-507; the demo seeds Du = 1 for
the same reason, :639-646). The first Newton iteration of a step therefore uses the elastic tangent, the others C_tang. A step
whose GMRES or Newton does not converge is reported and ends the loading.

    python3 examples/device_mohr_coulomb_slope.py [--n 25] [--steps K] [--solver gmres|amg|amg-rbm|amg-cheby|amg-soc|amg-k|amg-fp32|amg-p|lu]
        [--basis fp64|fp32]   (fp32: the Krylov basis of gmres / fgmres stored in single precision, dxo_krylov_create_basis)
"""
import argparse
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dolfinx_external_operator_amd import MEM_DEVICE, Context, DeviceMesh, McParams, fgmres, gmres, rigid_body_modes  # noqa: E402
from tools.synthetic import coordinate_element_at_nodes, structured_mesh  # noqa: E402

E, NU, COH, PHI, PSI, THETA_T = 6778.0, 0.25, 3.45, 30 * np.pi / 180, 30 * np.pi / 180, 26 * np.pi / 180
L, H, GAMMA = 1.2, 1.0, 1.0
L_LIM = 6.69            # the demo's reference stability factor (Chen and Liu)


def load_schedule():
    return np.concatenate([np.linspace(2, 22.9, 50), np.array([22.96, 22.99])])


def main(n: int = 25, steps: int | None = None, solver: str = "gmres", verbose: bool = True, restart: int = 30,
         lin_rtol: float = 1e-10, lin_maxiter: int = 3000, basis: str = "fp64") -> dict:
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_option("consumer_overwrite", 1)      # residual pieces and the assembly SET their output
    mesh = structured_mesh("triangle", (n, n), degree=2)
    mesh.x[:, 0] *= L
    mesh.node_x[:, 0] *= L
    dm = DeviceMesh.from_synthetic(mesh, ctx=ctx)
    prm = McParams(E, NU, COH, PHI, PSI, THETA_T, 0.26 * COH / np.tan(PHI), 1e-8, 200, 0)
    G = 2
    nn, npts = mesh.node_x.shape[0], mesh.num_cells * mesh.nq
    x = mesh.node_x
    fixed = np.zeros((nn, G), dtype=bool)
    fixed[np.abs(x[:, 1]) < 1e-12] = True
    fixed[np.abs(x[:, 0] - L) < 1e-12] = True
    free = torch.from_numpy(~fixed.reshape(-1)).to(dev)
    bcs = torch.from_numpy(np.flatnonzero(fixed.reshape(-1)).astype(np.int32)).to(dev)
    corner = int(np.flatnonzero((np.abs(x[:, 0]) < 1e-12) & (np.abs(x[:, 1] - H) < 1e-12))[0])

    f64 = dict(dtype=torch.float64, device=dev)
    u, Du = torch.zeros(nn * G, **f64), torch.zeros(nn * G, **f64)
    sigma_n, sigma = torch.zeros(npts * 4, **f64), torch.zeros(npts * 4, **f64)
    C_tang = torch.zeros(npts * 16, **f64)
    q = torch.zeros(npts * G, **f64)
    R, Rq = torch.zeros(nn * G, **f64), torch.zeros(nn * G, **f64)
    diag = [torch.zeros(npts, dtype=dt, device=dev) for dt in (torch.int32, torch.float64, torch.float64, torch.float64)]
    lam, mu = E * NU / ((1 + NU) * (1 - 2 * NU)), E / (2 * (1 + NU))
    Ce = np.zeros((4, 4))
    Ce[:3, :3] = lam
    Ce[np.arange(4), np.arange(4)] += 2 * mu                  # Mandel: the shear entry is 2 mu as well
    C_elas = torch.from_numpy(np.tile(Ce.reshape(-1), npts)).to(dev)
    pattern = dm.csr_pattern(G)
    values = torch.zeros(pattern.nnz, **f64)
    if solver == "lu":
        import scipy.sparse
        import scipy.sparse.linalg

        indptr, indices = pattern.indptr.cpu().numpy(), pattern.indices.cpu().numpy()

    def residual():
        ctx.mohr_coulomb_field(prm, dm._h, MEM_DEVICE, Du.data_ptr(), sigma_n.data_ptr(), C_tang.data_ptr(), sigma.data_ptr(),
                               *(d.data_ptr() for d in diag))
        dm.adjoint("eps", G, sigma.data_ptr(), R.data_ptr())
        dm.adjoint("value", G, q.data_ptr(), Rq.data_ptr())
        return torch.where(free, R - Rq, torch.zeros_like(R))

    amg = None
    loads = load_schedule()[: steps if steps else None]
    report = {"dofs": nn * G, "nnz": pattern.nnz, "solver": solver, "steps": [], "failed": None}
    for i, load in enumerate(loads):
        q.view(-1, G)[:, 1] = -load * GAMMA
        Du.zero_()
        t0 = time.perf_counter()
        history, lin_its, failed = [], [], None
        for it in range(100):
            res = residual()
            rn = float(torch.linalg.norm(res))
            history.append(rn)
            if rn <= max(1e-8, 1e-8 * history[0]):
                break
            Cj = C_elas if it == 0 else C_tang
            A = dm.bilinear_assemble("eps", "eps", G, Cj.data_ptr(), pattern, values=values, bcs=bcs, diagonal=1.0)
            rhs = -res
            if solver == "lu":
                S = scipy.sparse.csc_matrix(scipy.sparse.csr_matrix((values.cpu().numpy(), indices, indptr), shape=A.shape))
                d = torch.from_numpy(scipy.sparse.linalg.splu(S).solve(rhs.cpu().numpy())).to(dev)
            else:
                try:
                    if solver in ("amg", "amg-rbm", "amg-cheby", "amg-soc", "amg-k", "amg-fp32", "amg-p"):     # the symbolic phase once, the numeric setup at every Newton iteration
                        if amg is None:
                            relax = {"smoother": "chebyshev", "degree": 2, "rho": "power"} if solver == "amg-cheby" else {}
                            if solver == "amg-soc":
                                relax = {"strength": 0.1}
                            if solver == "amg-k":
                                relax = {"cycle": "K"}
                            if solver == "amg-fp32":
                                relax = {"smoother": "chebyshev", "degree": 2, "rho": "power", "precision": "fp32"}
                            if solver == "amg-p":    # the recommended relaxation, and level 1 the P1 space on the same triangles
                                relax = {"smoother": "chebyshev", "degree": 2, "rho": "power",
                                         "first_transfer": dm.vertex_transfer(coordinate_element_at_nodes(mesh.cell, mesh.degree))}
                            amg = A.amg(bcs, near_nullspace=rigid_body_modes(x, ctx=ctx) if solver != "amg" else None, **relax)
                        else:
                            amg.setup(A)
                        M = amg
                    else:
                        M = A.block_jacobi()
                except ValueError as e:          # DXO_E_SINGULAR: a node whose tangent blocks vanish
                    failed = f"preconditioner setup failed at load {load:.3f} (step {i}, Newton iteration {it}): {e}"
                    break
                out = (fgmres if solver in ("amg-k", "amg-fp32") else gmres)(A, rhs, M=M, restart=restart, rtol=lin_rtol, maxiter=lin_maxiter,
                                                                                    basis=basis)
                lin_its.append(out.iterations)
                if not out.converged:
                    failed = f"GMRES did not converge at load {load:.3f} (step {i}): {out.iterations} iterations, relative residual {out.residual:.2e}"
                d = out.x
            Du += d
            if failed:
                break
        else:
            failed = f"Newton did not converge at load {load:.3f} (step {i}) in 100 iterations: |R| = {history[-1]:.2e}"
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if failed:
            report["failed"] = failed
            if verbose:
                print(failed)
            break
        u += Du
        sigma_n.copy_(sigma)
        ux = float(u[corner * G])
        report["steps"].append({"load": float(load), "newton": len(history) - 1, "gmres": lin_its, "ms": ms, "u_corner": (ux, float(u[corner * G + 1])),
                                "residuals": history})
        if verbose:
            print(f"step {i:2d} load {load:6.3f}: u_x(0, H) = {ux: .6e}, {len(history) - 1} Newton its"
                  + (f", GMRES its {lin_its}" if solver != "lu" else "") + f", {ms:.0f} ms")
    done = report["steps"]
    report["load_reached"] = done[-1]["load"] if done else 0.0
    report["stability_factor"] = report["load_reached"] * GAMMA * H / COH
    report["u"] = u.cpu().numpy()
    if verbose:
        print(f"{nn * G} dofs, {pattern.nnz} nonzeros, solver {solver}; slope stability factor load*H/c = {report['stability_factor']:.3f} "
              f"(reference {L_LIM})" + (f"; stopped: {report['failed']}" if report["failed"] else ""))
    dm.close()
    ctx.close()
    return report


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=25, help="cells per side (the demo: 25)")
    ap.add_argument("--steps", type=int, default=None, help="first K load steps only")
    ap.add_argument("--solver", choices=["gmres", "amg", "amg-rbm", "amg-cheby", "amg-soc", "amg-k", "amg-fp32", "amg-p", "lu"], default="gmres",
                    help="amg-p: amg-cheby with the p-coarsening first level (quadratic meshes only; this one is)")
    ap.add_argument("--basis", choices=["fp64", "fp32"], default="fp64", help="storage of the Krylov basis of gmres / fgmres")
    a = ap.parse_args()
    main(a.n, a.steps, a.solver, basis=a.basis)
