#!/usr/bin/env python3
"""The von Mises demo's own problem (doc/demo/demo_plasticity_von_mises.py) solved on the device: a thick-walled cylinder under
internal pressure, a quarter of it with symmetry conditions, plane strain, P2 triangles and the 3-point rule.

Residual of the demo (:249-253):   F = inner(sigma, eps(v)) dx - inner(loading * -n, v) ds(inner)
Here, per Newton iteration:
    sigma, dp = von Mises(eps(Du), sigma_n, p); R = sum w|J| B^T sigma     dxo_von_mises_residual (SETs R: option consumer_overwrite)
    R += loading * sum dS phi n  over the inner arc                       dxo_facet_pressure (always accumulates)
    solve K d = -R on the free dofs, Jacobi-preconditioned CG             dxo_tangent_apply_vm / dxo_tangent_diagonal_vm
    Du += d
and at the end of a load step  p += dp, sigma_n <- sigma                  dxo_vm_commit_state (:561-565).
Load schedule of the demo: q_lim * linspace(0, 1.1, 20)^0.5 with q_lim = 2/sqrt(3) ln(R_e/R_i) sigma_0 (:542-545). Reported: u_x at
(R_i, 0) against the load, as the demo plots it (:539-592).

Starting guess. The reference kernel divides by the equivalent stress (:318-321), so a point with zero deviatoric stress gives 0/0. The
demo starts every step from Du = machine epsilon (:555). Here the step at zero load is u = 0 exactly (no solve); the first loaded step
starts from the homogeneous expansion u = c (x, y), with c from Lame's solution, which satisfies both symmetry conditions and strains
every point; each later step starts from the previous step's increment scaled by the ratio of the load increments.
Needs an MI355X.    python3 examples/device_cylinder_plasticity.py [n_r] [n_theta]
"""
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dolfinx_external_operator_amd import Context, DeviceMesh, VmParams  # noqa: E402
from tools.synthetic import facet_geometry, facet_tables, quarter_annulus  # noqa: E402

E, NU, SIGMA_0 = 70e3, 0.3, 250.0            # demo constants, :185-188
E_T = E / 100.0
H = E * E_T / (E - E_T)
R_I, R_E = 1.0, 1.3                          # :183


def lame_inner_displacement(p: float, R_i: float = R_I, R_e: float = R_E, E: float = E, nu: float = NU) -> float:
    """u_r(R_i) of the elastic thick-walled cylinder under internal pressure p, plane strain."""
    a, b = R_i, R_e
    return p * a * (1 + nu) * ((1 - 2 * nu) * a * a + b * b) / (E * (b * b - a * a))


def main(n_r: int = 16, n_theta: int = 64, n_steps: int = 20, verbose: bool = True, newton_tol: float = 1e-9, max_newton: int = 30) -> dict:
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_option("consumer_overwrite", 1)      # residual / matvec / diagonal SET their vector; the facet load adds on top
    mesh, tags = quarter_annulus(n_r, n_theta, R_I, R_E, degree=2)
    dm = DeviceMesh.from_synthetic(mesh, ctx=ctx)
    dm.set_facet_tables(*facet_tables(mesh)[:3])
    dm.set_facet_geometry(*facet_geometry("triangle"))
    inner = dm.facet_set(tags["inner"])
    G, d = 2, 4
    nn, npts = mesh.node_x.shape[0], mesh.num_cells * mesh.nq
    prm = VmParams(E, NU, SIGMA_0, H)
    x = mesh.node_x
    fixed = np.zeros((nn, G), dtype=bool)
    fixed[x[:, 1] == 0.0, 1] = True              # Lx: u_y = 0
    fixed[x[:, 0] == 0.0, 0] = True              # Ly: u_x = 0
    free = torch.from_numpy(~fixed.reshape(-1)).to(dev)
    probe = int(np.argmin(np.linalg.norm(x - [R_I, 0.0], axis=1)))      # the node at (R_i, 0)

    f64 = dict(dtype=torch.float64, device=dev)
    u, Du, Du_prev = (torch.zeros(nn * G, **f64) for _ in range(3))
    sigma_n, p = torch.zeros(npts * d, **f64), torch.zeros(npts, **f64)
    sigma, dp = torch.zeros(npts * d, **f64), torch.zeros(npts, **f64)
    R, Kv, diag, fext = (torch.zeros(nn * G, **f64) for _ in range(4))
    zero = torch.zeros(nn * G, **f64)

    def residual(loading):
        dm.von_mises_residual(prm, Du.data_ptr(), sigma_n.data_ptr(), p.data_ptr(), sigma.data_ptr(), dp.data_ptr(), R.data_ptr())
        dm.facet_pressure(inner, R.data_ptr(), scale=loading)
        return torch.where(free, R, zero)

    def K_times(v):
        dm.tangent_apply_vm(prm, sigma.data_ptr(), dp.data_ptr(), v.data_ptr(), Kv.data_ptr())
        return torch.where(free, Kv, zero)

    def cg(b, tol=1e-11, maxit=20000, check_every=8):
        dm.tangent_diagonal_vm(prm, sigma.data_ptr(), dp.data_ptr(), diag.data_ptr())
        minv = torch.where(free, 1.0 / diag, zero)
        xk, r = torch.zeros_like(b), b.clone()
        z = minv * r
        pk, rz = z.clone(), torch.dot(r, z)
        b2, its = float(torch.dot(b, b)), 0
        while its < maxit and float(torch.dot(r, r)) > tol * tol * b2:
            for _ in range(check_every):
                Ap = K_times(pk)
                pAp = torch.dot(pk, Ap)
                alpha = torch.where(pAp > 0, rz / pAp, torch.zeros_like(rz))
                xk.add_(alpha * pk)
                r.sub_(alpha * Ap)
                z = minv * r
                rz_new = torch.dot(r, z)
                pk.mul_(torch.where(rz > 0, rz_new / rz, torch.zeros_like(rz))).add_(z)
                rz = rz_new
            its += check_every
        return xk, its

    q_lim = 2.0 / np.sqrt(3.0) * np.log(R_E / R_I) * SIGMA_0           # :542
    loadings = q_lim * np.linspace(0, 1.1, n_steps, endpoint=True) ** 0.5
    expansion = torch.from_numpy(x.reshape(-1).copy()).to(dev)          # u = (x, y): both symmetry conditions hold
    report = {"points": npts, "dofs": nn * G, "q_lim": q_lim, "steps": []}
    if verbose:
        print(f"quarter cylinder {n_r} x {n_theta} P2 triangles: {nn * G} dofs, {npts} points, q_lim = {q_lim:.3f}")
        print(f"{'q/q_lim':>8} {'u_x(R_i,0)':>12} {'Newton':>6} {'final |R|/|f|':>13} {'CG its':>7} {'plastic':>8} {'ms':>8}")
    prev_load, prev_inc = 0.0, 0.0
    for loading in loadings:
        t0 = time.perf_counter()
        history, cg_its = [], 0
        if loading == 0.0:                       # u = 0 solves the unloaded step; the return map would be 0/0 there
            rel = 0.0
        else:
            fext.zero_()
            dm.facet_pressure(inner, fext.data_ptr(), scale=-loading)      # the load vector, inner(loading * -n, v) ds
            fnorm = float(torch.linalg.norm(torch.where(free, fext, zero)))
            if prev_inc > 0.0:
                Du.copy_(Du_prev * ((loading - prev_load) / prev_inc))
            else:
                Du.copy_(expansion * (lame_inner_displacement(loading) / R_I))
            for _ in range(max_newton):
                res = residual(loading)
                rn = float(torch.linalg.norm(res))
                history.append(rn)
                if rn <= newton_tol * fnorm:
                    break
                dDu, k = cg(-res)
                cg_its += k
                Du.add_(dDu)
            rel = history[-1] / fnorm
            u.add_(Du)
            ctx.vm_commit_state(d, npts, p.data_ptr(), dp.data_ptr(), sigma_n.data_ptr(), sigma.data_ptr())   # :561-565
            Du_prev.copy_(Du)
            prev_inc = loading - prev_load
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        prev_load = loading
        ux = float(u[probe * G])
        plastic = float((p > 0).double().mean())
        step = {"load": float(loading), "load_ratio": float(loading / q_lim), "u_x": ux, "newton_residuals": history,
                "newton_iterations": max(0, len(history) - 1), "relative_residual": rel, "cg_iterations": cg_its,
                "plastic_fraction": plastic, "max_dp": float(dp.max()) if loading else 0.0, "seconds": dt}
        report["steps"].append(step)
        if verbose:
            print(f"{loading / q_lim:8.3f} {ux:12.6e} {step['newton_iterations']:6d} {rel:13.2e} {cg_its:7d} {plastic:8.3f} {dt * 1e3:8.1f}")
    dm.close()
    ctx.close()
    return report


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
