#!/usr/bin/env python3
"""Scalar functionals on the device: the quantities of interest of the reference's codim tests and the error norm of its demo.

The reference assembles rank-0 forms with `fem.assemble_scalar`:

    test/test_codim_external_operator.py    u = x + y on a 5 x 5 P1 unit square;
                                            codim 0: J = f(u * u) * dx over the cells with x <= 0.2, f(s) = s sqrt(s), f'(s) = 3 s
                                                     (the test's derivative check integrates 3 u^2 over the same cells);
                                            codim 1: J = g(u) * ds over the exterior, g = cos, g' = -sin
    doc/demo/demo_hyperelasticity.py:817    sqrt(assemble_scalar((u - u_UFL)**2 * dx))

Here the quadrature data never leave the device:

    u at the points of the cell subset          dxo_eval_operand (kind "value", entity list)          DeviceMesh.evaluate_device
    f(u^2), 3 u^2                               torch, elementwise
    int f(u^2) dx, int 3 u^2 dx                 dxo_integrate                                         DeviceMesh.integrate
    u at the facet points of the exterior       dxo_eval_operand_facets                               DeviceMesh.evaluate_facets_device
    int cos(u) ds, int sin(u) ds                dxo_facet_integrate                                   DeviceMesh.facet_integrate
    ||u - u_ref||^2                             dxo_operand_moments (kind "value" of the difference)  DeviceMesh.operand_moments
    deformed volume int det F dx, affine u      dxo_operand_moments (kind "detF")

Each result is compared with the same quadrature done in NumPy on the host (assert_allclose at its default rtol, as the reference
test compares with its closed forms); host_side() is that NumPy arithmetic and needs no GPU.
Prints one JSON line. Needs an MI355X.    python3 examples/device_functionals.py
"""
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from tools.synthetic import FACETS, exterior_facets, facet_geometry, facet_tables, structured_mesh  # noqa: E402

N_SIDE = 5
X_MAX = 0.2 + 1e-12                          # the reference's marker: cells whose vertices all have x <= 0.2
ERR_SLOPE = 0.01                             # u_ref = u + ERR_SLOPE * x, so ||u - u_ref||^2 = ERR_SLOPE^2 / 3 on the unit square
L2_ERROR_SQ_EXACT = ERR_SLOPE ** 2 / 3.0
A_AFFINE = np.array([[0.1, 0.2], [-0.05, 0.3]])              # u = A x: F = I + A everywhere
DEFORMED_VOLUME_EXACT = float(np.linalg.det(np.eye(2) + A_AFFINE))


def problem():
    """(mesh, u nodal values of x + y, the cell subset, the exterior facets)."""
    mesh = structured_mesh("triangle", (N_SIDE, N_SIDE), degree=1)
    u = mesh.node_x[:, 0] + mesh.node_x[:, 1]
    cells = np.flatnonzero(np.all(mesh.x[mesh.geom_dofmap][:, :, 0] <= X_MAX, axis=1)).astype(np.int32)
    return mesh, u, cells, exterior_facets(mesh)


def host_side() -> dict:
    """The same quadrature in NumPy: what the device results are compared with."""
    mesh, u, cells, ents = problem()
    X = mesh.x[mesh.geom_dofmap]                                                 # (nc, 3, 2)
    J = np.einsum("cvj,qvk->cqjk", X, mesh.dpsi)
    dx = mesh.weights[None, :] * np.abs(np.linalg.det(J))                        # (nc, nq)
    uq = np.einsum("qa,ca->cq", mesh.phi, u[mesh.dofmap])
    s = uq[cells] ** 2
    out = {"int_u3_dx": float(np.sum(dx[cells] * s * np.sqrt(s))), "int_3u2_dx": float(np.sum(dx[cells] * 3.0 * s))}
    phi_f = facet_tables(mesh)[0]                                                # (nf, nqf, nd)
    w_f = facet_geometry(mesh.cell)[0]
    fl = np.array(FACETS[mesh.cell])
    ends = mesh.x[mesh.geom_dofmap[ents[:, 0][:, None], fl[ents[:, 1]]]]         # (n, 2, 2): the facet's two vertices
    dS = np.linalg.norm(ends[:, 1] - ends[:, 0], axis=1)[:, None] * w_f[None, :]
    uf = np.einsum("eqa,ea->eq", phi_f[ents[:, 1]], u[mesh.dofmap[ents[:, 0]]])
    out["int_cos_ds"], out["int_sin_ds"] = float(np.sum(dS * np.cos(uf))), float(np.sum(dS * np.sin(uf)))
    diff = -ERR_SLOPE * mesh.node_x[:, 0]
    dq = np.einsum("qa,ca->cq", mesh.phi, diff[mesh.dofmap])
    out["l2_error_sq"] = float(np.sum(dx * dq * dq))
    ua = mesh.node_x @ A_AFFINE.T                                                # (nn, 2)
    g = np.einsum("cai,qak,cqkj->cqij", ua[mesh.dofmap], mesh.dphi, np.linalg.inv(J))
    out["deformed_volume"] = float(np.sum(dx * np.linalg.det(np.eye(2) + g)))
    return out


def main() -> dict:
    import torch

    from dolfinx_external_operator_amd import Context, DeviceMesh

    dev = torch.device("cuda:0")
    ctx = Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    mesh, u, cells, ents = problem()
    dm = DeviceMesh.from_synthetic(mesh, ctx=ctx)
    dm.set_facet_tables(*facet_tables(mesh)[:3])
    dm.set_facet_geometry(*facet_geometry(mesh.cell))
    u_d, cells_d = torch.from_numpy(u).to(dev), torch.from_numpy(cells).to(dev)

    # codim 0: u at the points of the subset, then f(u^2) = u^2 sqrt(u^2) and f'(u^2) u^2 = 3 u^2, integrated over the subset
    uq = torch.empty((len(cells), dm.nq, 1), dtype=torch.float64, device=dev)
    dm.evaluate_device("value", 1, u_d.data_ptr(), len(cells), uq.data_ptr(), cells_d.data_ptr())
    s = uq * uq
    got = {"int_u3_dx": dm.integrate(s * torch.sqrt(s), cells=cells_d), "int_3u2_dx": dm.integrate(3.0 * s, cells=cells_d)}

    # codim 1: u at the facet points of the exterior, g = cos and -g' = sin
    fs = dm.facet_set(ents)
    uf = dm.evaluate_facets_device("value", 1, u_d, torch.from_numpy(fs.entities).to(dev))
    got["int_cos_ds"], got["int_sin_ds"] = dm.facet_integrate(torch.cos(uf), fs), dm.facet_integrate(torch.sin(uf), fs)

    # the demo's error norm: the field u - u_ref, its squared L2 norm is the last entry of the "value" moments
    diff = torch.from_numpy(-ERR_SLOPE * mesh.node_x[:, 0]).to(dev)
    got["l2_error_sq"] = dm.operand_moments("value", 1, diff)[1:]
    # the deformed volume of an affine displacement: the first entry of the "detF" moments
    ua = torch.from_numpy(np.ascontiguousarray((mesh.node_x @ A_AFFINE.T).reshape(-1))).to(dev)
    got["deformed_volume"] = dm.operand_moments("detF", 2, ua)[:1]

    got = {k: float(v.cpu()[0]) for k, v in got.items()}          # the one synchronisation
    host = host_side()
    for k, v in host.items():
        np.testing.assert_allclose(got[k], v, err_msg=k)
    np.testing.assert_allclose(got["l2_error_sq"], L2_ERROR_SQ_EXACT)
    np.testing.assert_allclose(got["deformed_volume"], DEFORMED_VOLUME_EXACT)
    got["l2_error"] = float(np.sqrt(got["l2_error_sq"]))
    fs.close()
    dm.close()
    ctx.close()
    return got


if __name__ == "__main__":
    print(json.dumps(main()))
