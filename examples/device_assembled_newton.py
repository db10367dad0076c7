#!/usr/bin/env python3
"""The hyperelasticity demo's tension test solved the way the reference solves it: an assembled Jacobian and a direct LU solve.

The reference (doc/demo/demo_hyperelasticity.py:560-573) hands assemble_matrix(J_replaced, bcs) to PETSc with ksp_type = preonly,
pc_type = lu. Here, per Newton iteration:

    dP, P = Isihara(I + grad u)                  dxo_isihara_field (operand and model in one launch, fp64)
    R = sum w|J| grad(v) : P  on the free dofs   dxo_operand_adjoint, kind "F"
    J = assembled (grad, grad) form with dP      dxo_bilinear_assemble into the CSR pattern of the mesh (built once)
        Dirichlet rows and columns, diagonal 1   dxo_csr_dirichlet
    solve J d = -R on the host                   scipy.sparse.linalg.splu (stands in for preonly + lu); without scipy a dense
                                                 torch.linalg.solve at small sizes
    u += d
The CSR values and the right-hand side go to the host, the Newton step comes back; the pattern's index arrays are copied once.
Same mesh, boundary conditions, load steps and Isihara constants as examples/device_hyperelasticity.py (matrix-free CG).
Needs an MI355X.    python3 examples/device_assembled_newton.py [cells_per_side]
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

DENSE_MAX_DOFS = 20000      # the fallback without scipy forms the dense matrix


def direct_solver(indptr: np.ndarray, indices: np.ndarray, n: int):
    """solve(values, b) -> x for the CSR matrix (indptr, indices, values): sparse LU with scipy, else dense LU with torch."""
    try:
        import scipy.sparse
        import scipy.sparse.linalg
    except ImportError:
        if n > DENSE_MAX_DOFS:
            raise RuntimeError(f"scipy is not installed and {n} dofs are too many for the dense fallback") from None
        rows = np.repeat(np.arange(n), np.diff(indptr))

        def solve(values, b):
            A = torch.zeros((n, n), dtype=torch.float64)
            A[torch.from_numpy(rows), torch.from_numpy(indices.astype(np.int64))] = torch.from_numpy(values)
            return torch.linalg.solve(A, torch.from_numpy(b)).numpy()

        return solve, "torch.linalg.solve (dense)"

    def solve(values, b):
        A = scipy.sparse.csc_matrix(scipy.sparse.csr_matrix((values, indices, indptr), shape=(n, n)))
        return scipy.sparse.linalg.splu(A).solve(b)

    return solve, "scipy.sparse.linalg.splu"


def main(n_side: int = 32, steps=(0.025, 0.05, 0.075, 0.1), verbose: bool = True, c=(0.5, 1.0, 1.0, 1.5)) -> dict:
    """steps: the prescribed top displacement u_y of each load step; c: the Isihara constants (demo_hyperelasticity.py:700)."""
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_option("consumer_overwrite", 1)      # the residual and the assembly SET their output
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
    bcs = torch.from_numpy(np.flatnonzero(fixed.reshape(-1)).astype(np.int32)).to(dev)

    f64 = dict(dtype=torch.float64, device=dev)
    u = torch.zeros(nn * G, **f64)
    dP, P = torch.zeros(npts * 16, **f64), torch.zeros(npts * 4, **f64)
    R = torch.zeros(nn * G, **f64)
    pattern = dm.csr_pattern(G)
    values = torch.zeros(pattern.nnz, **f64)
    solve, solver_name = direct_solver(pattern.indptr.cpu().numpy(), pattern.indices.cpu().numpy(), pattern.n_rows)

    def residual():
        """(dP, P) at the current u and the assembled inner(grad v, P) dx on the free dofs"""
        ctx.isihara_field(prm, dm._h, MEM_DEVICE, u.data_ptr(), dP.data_ptr(), P.data_ptr())
        dm.adjoint("F", G, P.data_ptr(), R.data_ptr())
        return torch.where(free, R, torch.zeros_like(R))

    stretch = torch.zeros(nn * G, **f64)
    stretch[1::G] = torch.from_numpy(x[:, 1].copy()).to(dev)
    report = {"points": npts, "dofs": nn * G, "nnz": pattern.nnz, "pattern_ms": pattern.build_ms, "solver": solver_name, "steps": []}
    prev = 0.0
    for load in steps:
        u += (load - prev) * stretch
        prev = load
        history, t0, t_asm = [], time.perf_counter(), 0.0
        for _ in range(25):
            res = residual()
            rn = float(torch.linalg.norm(res))
            history.append(rn)
            if rn <= 1e-10 * max(history[0], 1e-30):
                break
            ta = time.perf_counter()
            dm.bilinear_assemble("grad", "grad", G, dP.data_ptr(), pattern, values=values, bcs=bcs, diagonal=1.0)
            torch.cuda.synchronize()
            t_asm += time.perf_counter() - ta
            du = solve(values.cpu().numpy(), (-res).cpu().numpy())        # fixed dofs: identity rows, zero right-hand side
            u += torch.from_numpy(du).to(dev)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        report["steps"].append({"load": load, "newton_residuals": history, "seconds": dt, "assemble_seconds": t_asm,
                                "max_uy": float(u[1::G].max())})
        if verbose:
            print(f"u_y(top) = {load:.3f}: {len(history) - 1} Newton its, residuals " + " ".join(f"{r:.2e}" for r in history)
                  + f", {dt * 1e3:.0f} ms ({t_asm * 1e3:.1f} ms assembling)")
    report["u"] = u.cpu().numpy()
    if verbose:
        print(f"{nn * G} dofs, {pattern.nnz} nonzeros, pattern built in {pattern.build_ms:.1f} ms, solver {solver_name}")
    dm.close()
    ctx.close()
    return report


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 32)
