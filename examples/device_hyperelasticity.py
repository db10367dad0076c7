#!/usr/bin/env python3
"""The hyperelasticity demo's tension test as a Newton-Krylov solve in which quadrature data never leaves the GPU.

The reference (doc/demo/demo_hyperelasticity.py) evaluates F = I + grad u, calls the external operator for (dP/dF, P), copies both into
coefficients and lets DOLFINx + PETSc SNES assemble the residual inner(grad v, P) dx and the Jacobian
J = derivative(inner(grad v, P) dx, u, u_hat), whose action is sum_q w|J| grad(v) : dP/dF : grad(u_hat). Here, per Newton iteration:

    dP, P = Isihara(I + grad u)                  dxo_isihara_field (operand and model in one launch, fp64)
    R = sum w|J| grad(v) : P  on the free dofs   dxo_operand_adjoint, kind "F"
    solve K d = -R by Jacobi-preconditioned CG   K v: dxo_bilinear_apply("grad", "grad", 2, dP), diag(K): dxo_bilinear_diagonal
    u += d
Only dof vectors (and a few CG scalars) are touched outside the kernels; they are torch CUDA tensors.

Problem: unit square, P2 vector field on triangles, 3-point rule; bottom edge clamped, top edge u_x = 0 and u_y prescribed, raised over
a few load steps. The analytic Isihara model is fp64, so Newton converges quadratically.
Needs an MI355X.    python3 examples/device_hyperelasticity.py [cells_per_side]
"""
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dolfinx_external_operator_amd import MEM_DEVICE, Context, DeviceMesh, IsiharaParams  # noqa: E402
from tools.synthetic import structured_mesh  # noqa: E402


def main(n_side: int = 32, steps=(0.025, 0.05, 0.075, 0.1), verbose: bool = True, c=(0.5, 1.0, 1.0, 1.5)) -> dict:
    """steps: the prescribed top displacement u_y of each load step; c: the Isihara constants (demo_hyperelasticity.py:700)."""
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_option("consumer_overwrite", 1)      # residual / matvec / diagonal calls SET their output vector
    mesh = structured_mesh("triangle", (n_side, n_side), degree=2)
    dm = DeviceMesh.from_synthetic(mesh, ctx=ctx)
    prm = IsiharaParams(*c)
    G = 2
    nn, npts = mesh.node_x.shape[0], mesh.num_cells * mesh.nq
    x = mesh.node_x
    bottom, top = x[:, 1] < 1e-12, x[:, 1] > 1 - 1e-12
    fixed = np.zeros((nn, G), dtype=bool)
    fixed[bottom] = True
    fixed[top] = True                            # top: u_x = 0, u_y = load
    free = torch.from_numpy(~fixed.reshape(-1)).to(dev)

    f64 = dict(dtype=torch.float64, device=dev)
    u = torch.zeros(nn * G, **f64)
    dP, P = torch.zeros(npts * 16, **f64), torch.zeros(npts * 4, **f64)
    R, Kv, diag = (torch.zeros(nn * G, **f64) for _ in range(3))

    def residual():
        """(dP, P) at the current u and the assembled inner(grad v, P) dx on the free dofs"""
        ctx.isihara_field(prm, dm._h, MEM_DEVICE, u.data_ptr(), dP.data_ptr(), P.data_ptr())
        dm.adjoint("F", G, P.data_ptr(), R.data_ptr())
        return torch.where(free, R, torch.zeros_like(R))

    def K_times(v):
        dm.bilinear_apply("grad", "grad", G, dP.data_ptr(), v.data_ptr(), Kv.data_ptr())
        return torch.where(free, Kv, torch.zeros_like(Kv))

    def cg(b, tol=1e-12, maxit=5000, check_every=8):
        """Jacobi-preconditioned conjugate gradients with K v and diag(K) matrix-free. Scalars stay on the device; the convergence
        test (the only host synchronisation) runs every `check_every` iterations, and the quotients are guarded for a converged system."""
        dm.bilinear_diagonal("grad", "grad", G, dP.data_ptr(), diag.data_ptr())
        minv = torch.where(free, 1.0 / diag, torch.zeros_like(diag))
        xk = torch.zeros_like(b)
        r = b.clone()
        z = minv * r
        pk = z.clone()
        rz = torch.dot(r, z)
        b2 = float(torch.dot(b, b))
        its = 0
        while its < maxit and float(torch.dot(r, r)) > tol * tol * b2:
            for _ in range(check_every):
                Ap = K_times(pk)
                pAp = torch.dot(pk, Ap)
                alpha = torch.where(pAp > 0, rz / pAp, torch.zeros_like(rz))
                xk.add_(alpha * pk)
                r.sub_(alpha * Ap)
                torch.mul(minv, r, out=z)
                rz_new = torch.dot(r, z)
                beta = torch.where(rz > 0, rz_new / rz, torch.zeros_like(rz))
                pk.mul_(beta).add_(z)
                rz = rz_new
            its += check_every
        return xk, its

    # predictor of a load step: the homogeneous stretch u_y = load * y (satisfies both Dirichlet edges)
    stretch = torch.zeros(nn * G, **f64)
    stretch[1::G] = torch.from_numpy(x[:, 1].copy()).to(dev)
    report = {"points": npts, "dofs": nn * G, "steps": []}
    prev = 0.0
    for load in steps:
        u += (load - prev) * stretch
        prev = load
        history, t0, cg_its = [], time.perf_counter(), 0
        for _ in range(25):
            res = residual()
            rn = float(torch.linalg.norm(res))
            history.append(rn)
            if rn <= 1e-10 * max(history[0], 1e-30):
                break
            du, k = cg(-res)
            cg_its += k
            u += du
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        report["steps"].append({"load": load, "newton_residuals": history, "cg_iterations": cg_its, "seconds": dt,
                                "max_uy": float(u[1::G].max())})
        if verbose:
            print(f"u_y(top) = {load:.3f}: {len(history) - 1} Newton its, residuals " + " ".join(f"{r:.2e}" for r in history)
                  + f", {cg_its} CG its, {dt * 1e3:.0f} ms")
    dm.close()
    ctx.close()
    return report


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 32)
