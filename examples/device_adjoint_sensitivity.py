#!/usr/bin/env python3
"""The gradient of a functional of a nonlinear heat problem with respect to its parameters, by ONE adjoint solve on the device.

The problem is the one of examples/device_robin_heat.py: unit square, P2 triangles, k(T) = 1 / (A + B T), q = -k(T) grad T, T = T_D on
x = 0, and on x = 1 the flux q . n = g(T) = h (T - T_inf) + c (T^4 - T_inf^4). Its Jacobian is non-symmetric (the pair
("grad", "value_grad") plus a facet term). The functional is

    J(T; h, c) = int T^2 dx + int_{x=1} g(T) ds          dxo_operand_moments("value") + dxo_facet_integrate,

the parameters theta = (h, c, A, B). With R(T; theta) = 0 solved by Newton's method, dJ/dtheta = dJ/dtheta|_T - lambda . dR/dtheta, where

    K^T lambda = dJ/dT,   dJ/dT[v] = int 2 T v dx + int g'(T) v ds         dxo_operand_adjoint + dxo_facet_adjoint, kind "value"

assembled   the Jacobian at the converged T is transposed IN PLACE (DeviceCSR.transpose(out=values), dxo_csr_transpose) and the
            multigrid of the Newton solves gets its numeric phase again (amg.setup(): the symbolic phase is reused), then gmres
--matrix-free   K^T v = dxo_bilinear_apply_t on the forward call's pair and blocks + the facet action (("value", "value"): symmetric),
            Jacobi-preconditioned gmres (the diagonal of the transpose is the diagonal)

and the four partial derivatives pair lambda with quadrature data, no new kernel:

    dR/dh . lambda = int (T - T_inf) lambda ds,  dR/dc . lambda = int (T^4 - T_inf^4) lambda ds       dxo_facet_integrate(f, g)
    dR/dA . lambda = -int k^2 sigma . grad lambda dx,  dR/dB . lambda = -int k^2 T sigma . grad lambda dx   dxo_integrate(f, g)

(dq/dA = k^2 sigma, dq/dB = k^2 T sigma with sigma = grad T). The gradient is printed next to central differences of J with steps
`rel_step` and `rel_step` / 2 times the parameter, each from two more Newton solves.
Prints one JSON line. Needs an MI355X.    python3 examples/device_adjoint_sensitivity.py [cells_per_side] [--matrix-free] [--rel-step S]
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

T_D, T_INF = 1.0, 0.2
PARAMS = ("h", "c", "A", "B")
THETA0 = {"h": 0.1, "c": 0.05, "A": 1.0, "B": 1.0}


def main(n_side: int = 8, matrix_free: bool = False, rel_step: float = 5e-3, verbose: bool = False) -> dict:
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_option("consumer_overwrite", 1)      # the cell calls SET their output; the facet calls always add on top
    mesh = structured_mesh("triangle", (n_side, n_side), degree=2)
    dm = DeviceMesh.from_synthetic(mesh, ctx=ctx)
    dm.set_facet_tables(*facet_tables(mesh)[:3])
    dm.set_facet_geometry(*facet_geometry(mesh.cell))
    G = 2
    nn, nc, nq, npts = mesh.node_x.shape[0], mesh.num_cells, mesh.nq, mesh.num_cells * mesh.nq
    fs = dm.facet_set(exterior_facets(mesh, where=lambda X: np.all(X[..., 0] == 1.0, axis=1)))
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
    Jmat = DeviceCSR(pattern, values)
    state = {}

    def residual(th):
        """R on the free dofs, and the blocks of the Jacobian at the current T: Cj (cells) and dg (facet points)"""
        dm.heat(th["A"], th["B"], T.data_ptr(), q.data_ptr(), dqdT.data_ptr(), dqds.data_ptr(), mem=MEM_DEVICE)
        torch.neg(q, out=mq)
        Cj[:, :, 0] = -dqdT.reshape(npts, G)
        Cj[:, :, 1:] = -dqds.reshape(npts, G, G)
        dm.adjoint("grad", 1, mq.data_ptr(), R.data_ptr())
        dm.evaluate_facets_device("value", 1, T, ents_d, out=Tf)
        g.copy_(th["h"] * (Tf - T_INF) + th["c"] * (Tf ** 4 - T_INF ** 4))
        dg.copy_(th["h"] + 4.0 * th["c"] * Tf ** 3)
        dm.facet_adjoint("value", 1, g.data_ptr(), fs, R.data_ptr())
        return torch.where(free, R, torch.zeros_like(R))

    def assemble():
        dm.bilinear_assemble("grad", "value_grad", 1, Cj.data_ptr(), pattern, values=values)
        dm.facet_bilinear_assemble("value", 1, dg.data_ptr(), fs, pattern, values=values, bcs=bcs, diagonal=1.0)

    def multigrid():
        if "amg" not in state:
            state["amg"] = Jmat.amg(constrained=bcs)
        else:
            state["amg"].setup()
        return state["amg"]

    def jacobian_times(v, out, transpose=False):
        """out = J v (or J^T v) with the Dirichlet rows and columns of the assembled form: identity on the fixed dofs"""
        vm = torch.where(free, v, torch.zeros_like(v))
        (dm.bilinear_apply_t if transpose else dm.bilinear_apply)("grad", "value_grad", 1, Cj.data_ptr(), vm.data_ptr(), Kv.data_ptr())
        dm.facet_bilinear_apply("value", 1, dg.data_ptr(), vm.data_ptr(), fs, Kv.data_ptr())      # ("value", "value"): its own transpose
        out.copy_(torch.where(free, Kv, v))

    def jacobi():
        dm.bilinear_diagonal("grad", "value_grad", 1, Cj.data_ptr(), diag.data_ptr())
        dm.facet_bilinear_diagonal("value", 1, dg.data_ptr(), fs, diag.data_ptr())
        return torch.where(free, 1.0 / diag, torch.ones_like(diag))

    def linear_solve(b, transpose=False):
        """J d = b, or J^T d = b, at the blocks of the last residual()"""
        if matrix_free:
            sol = gmres(lambda v, out: jacobian_times(v, out, transpose), b, M=jacobi(), restart=60, rtol=1e-12, maxiter=6000, ctx=ctx)
        else:
            assemble()
            if transpose:
                Jmat.transpose(out=values)      # in place: same pattern, Dirichlet rows and columns stay what they are
            sol = gmres(Jmat, b, M=multigrid(), restart=30, rtol=1e-12, maxiter=600)
        if not sol.converged:
            raise RuntimeError(f"a linear solve did not converge: {sol}")
        return sol.x

    def newton(th):
        """T(theta) from the start T = T_D, down to the floor of the residual; returns the history"""
        T.fill_(T_D)
        history = []
        for _ in range(40):
            res = residual(th)
            history.append(float(torch.linalg.norm(res)))
            if history[-1] <= 1e-14 * history[0] or (len(history) > 3 and history[-1] >= 0.5 * history[-2] and history[-1] <= 1e-10 * history[0]):
                return history
            T.add_(linear_solve(-res))
        raise RuntimeError(f"Newton did not converge: {history}")

    def functional(th):
        """J at the current T; g holds g(T) of the last residual()"""
        residual(th)
        return float(dm.operand_moments("value", 1, T)[1] + dm.facet_integrate(g.reshape(fs.n, dm.nq_facet, 1), fs)[0])

    def solved_functional(th):
        newton(th)
        return functional(th)

    # ---- finite differences of J: forward solves only
    fd = {}
    for step in (rel_step, 0.5 * rel_step):
        fd[step] = []
        for name in PARAMS:
            d = step * THETA0[name]
            fd[step].append((solved_functional({**THETA0, name: THETA0[name] + d}) - solved_functional({**THETA0, name: THETA0[name] - d})) / (2 * d))

    # ---- the adjoint gradient at theta0
    th = dict(THETA0)
    history = newton(th)
    J0 = functional(th)                                   # leaves Cj, dg, g, Tf at the converged T
    Tq, sig = torch.zeros(nc, nq, 1, **f64), torch.zeros(nc, nq, G, **f64)
    dm.evaluate_device("value", 1, T.data_ptr(), nc, Tq.data_ptr())
    dm.evaluate_device("grad", 1, T.data_ptr(), nc, sig.data_ptr())
    dJdT = torch.zeros(nn, **f64)
    two_T = 2.0 * Tq
    dm.adjoint("value", 1, two_T.data_ptr(), dJdT.data_ptr())
    dm.facet_adjoint("value", 1, dg.data_ptr(), fs, dJdT.data_ptr())
    lam = linear_solve(torch.where(free, dJdT, torch.zeros_like(dJdT)), transpose=True)
    lam_f = dm.evaluate_facets_device("value", 1, lam, ents_d).reshape(fs.n, dm.nq_facet, 1)
    glam = torch.zeros(nc, nq, G, **f64)
    dm.evaluate_device("grad", 1, lam.data_ptr(), nc, glam.data_ptr())
    Tfp = Tf.reshape(fs.n, dm.nq_facet, 1)
    dg_dh, dg_dc = Tfp - T_INF, Tfp ** 4 - T_INF ** 4
    k2 = 1.0 / (th["A"] + th["B"] * Tq) ** 2
    dq_dA, dq_dB = (k2 * sig).contiguous(), (k2 * Tq * sig).contiguous()
    grad = [float(dm.facet_integrate(dg_dh, fs)[0] - dm.facet_integrate(dg_dh, fs, g=lam_f)[0]),
            float(dm.facet_integrate(dg_dc, fs)[0] - dm.facet_integrate(dg_dc, fs, g=lam_f)[0]),
            float(dm.integrate(dq_dA, g=glam)[0]),
            float(dm.integrate(dq_dB, g=glam)[0])]
    torch.cuda.synchronize()
    report = {"cells_per_side": n_side, "dofs": nn, "matrix_free": matrix_free, "rel_step": rel_step, "parameters": list(PARAMS),
              "theta": [THETA0[p] for p in PARAMS], "J": J0, "newton_residuals": history, "gradient": grad,
              "fd_h": fd[rel_step], "fd_h2": fd[0.5 * rel_step]}
    if verbose:
        for i, p in enumerate(PARAMS):
            print(f"dJ/d{p}: adjoint {grad[i]: .12e}   FD(h) {fd[rel_step][i]: .12e}   FD(h/2) {fd[0.5 * rel_step][i]: .12e}", file=sys.stderr)
    dm.close()
    ctx.close()
    return report


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("cells_per_side", nargs="?", type=int, default=8)
    ap.add_argument("--matrix-free", action="store_true")
    ap.add_argument("--rel-step", type=float, default=5e-3)
    a = ap.parse_args()
    print(json.dumps(main(a.cells_per_side, a.matrix_free, a.rel_step, verbose=True)))
