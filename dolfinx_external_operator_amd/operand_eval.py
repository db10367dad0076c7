"""Operand evaluation on the GPU: the device counterpart of `fem.Expression(operand, points).eval(mesh, entities)`
inside `evaluate_operands` (src/dolfinx_external_operator/external_operator.py:386-402), for operands that are
linear in the value or gradient of one Lagrange field — eps(Du), I + grad u, T, grad T: every operand of the
reference's demos.

    mesh = DeviceMesh(gdim=2, phi=..., dphi=..., dpsi=..., dofmap=V.dofmap.list, geom_dofmap=domain.geometry.dofmap,
                      x=domain.geometry.x, num_field_nodes=...)
    deps = mesh.operand("eps", Du)           # an object with .eval(entities) -> (len(entities), nq, 4)
    evaluated = evaluate_operands([sigma])   # evaluation.py mirror; or call deps.eval(cells) directly

The field holder (`fem.Function`, ndarray or zero-argument callable) is re-read at every evaluation, like the
reference's Expression re-reads the Function's vector.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from ._lib import MEM_DEVICE, MEM_HOST, Context, DxoError, _CudaArrayView, default_context

KINDS = {"value": 0, "grad": 1, "eps": 2, "F": 3, "value_grad": 4,
         # nonlinear operands of F = I + grad u (the reference's own operand test, test/test_operands_evaluation.py:32-36): forward only
         "C": 5, "I1": 6, "detF": 7,
         "div": 8}        # div u (linear: forward and adjoint), test/test_external_operators_evaluation.py:141


class MeshDesc(C.Structure):
    """dxo_mesh_desc (include/dxo.h)."""
    _fields_ = [("gdim", C.c_int32), ("nq", C.c_int32), ("ndofs", C.c_int32), ("ngeom", C.c_int32),
                ("x_stride", C.c_int32), ("_pad", C.c_int32),
                ("num_cells", C.c_int64), ("num_field_nodes", C.c_int64), ("num_geom_nodes", C.c_int64),
                ("phi", C.c_void_p), ("dphi", C.c_void_p), ("dpsi", C.c_void_p),
                ("dofmap", C.c_void_p), ("geom_dofmap", C.c_void_p), ("x", C.c_void_p)]


def _state(holder):
    if callable(holder) and not hasattr(holder, "x") and not hasattr(holder, "data_ptr"):
        holder = holder()
    xv = getattr(holder, "x", None)
    if xv is not None and hasattr(xv, "array"):
        return xv.array
    return holder


class DeviceMesh:
    """Element tables, dofmaps and coordinates resident on the GPU (uploaded once)."""

    def __init__(self, *, gdim: int, phi, dphi, dpsi, dofmap, geom_dofmap, x, num_field_nodes: int | None = None,
                 ctx: Context | None = None, device: int = 0, psi=None):
        self.ctx = ctx if ctx is not None else default_context(device)
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        dphi = np.ascontiguousarray(dphi, dtype=np.float64)
        dpsi = np.ascontiguousarray(dpsi, dtype=np.float64)
        dofmap = np.ascontiguousarray(dofmap, dtype=np.int32)
        geom_dofmap = np.ascontiguousarray(geom_dofmap, dtype=np.int32)
        x = np.ascontiguousarray(x, dtype=np.float64)
        nq, ndofs = phi.shape
        if dphi.shape != (nq, ndofs, gdim) or dpsi.shape[0] != nq or dpsi.shape[2] != gdim:
            raise ValueError("table shapes: phi (nq, ndofs), dphi (nq, ndofs, gdim), dpsi (nq, ngeom, gdim)")
        if dofmap.ndim != 2 or dofmap.shape[1] != ndofs or geom_dofmap.shape != (dofmap.shape[0], dpsi.shape[1]):
            raise ValueError("dofmap (num_cells, ndofs) and geom_dofmap (num_cells, ngeom) do not match the tables")
        if num_field_nodes is None:
            num_field_nodes = int(dofmap.max()) + 1 if dofmap.size else 0
        self.gdim, self.nq, self.num_cells, self.num_field_nodes = gdim, nq, dofmap.shape[0], int(num_field_nodes)
        d = MeshDesc(gdim, nq, ndofs, dpsi.shape[1], x.shape[1], 0, self.num_cells, self.num_field_nodes, x.shape[0],
                     phi.ctypes.data, dphi.ctypes.data, dpsi.ctypes.data, dofmap.ctypes.data, geom_dofmap.ctypes.data,
                     x.ctypes.data)
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.dxo_mesh_create(self.ctx._h, C.byref(d), C.byref(h)), "dxo_mesh_create")
        self._h = h
        self._dofmap, self._geom_dofmap = dofmap, geom_dofmap      # host arrays, for vertex_transfer
        self._x = x                                                # and for vertex_mesh
        if psi is not None:     # values of the coordinate element at the points: the operand `x` (set_coordinate_values)
            self.set_coordinate_values(psi)

    @classmethod
    def from_synthetic(cls, mesh, **kw):
        """From a `tools.synthetic.SyntheticMesh` (tests, benches, examples): any object with these attributes."""
        dm = cls(gdim=mesh.gdim, phi=mesh.phi, dphi=mesh.dphi, dpsi=mesh.dpsi, dofmap=mesh.dofmap,
                 geom_dofmap=mesh.geom_dofmap, x=mesh.x, num_field_nodes=mesh.node_x.shape[0], **kw)
        if getattr(mesh, "weights", None) is not None:
            dm.set_weights(mesh.weights)
        if getattr(mesh, "psi", None) is not None:
            dm.set_coordinate_values(mesh.psi)
        return dm

    @staticmethod
    def tables_from_dolfinx(V, quadrature_points) -> dict:
        """The constructor arguments for a DOLFINx function space `V` (blocked Lagrange) and the reference quadrature
        points the operator's quadrature element uses (`basix.make_quadrature(...)[0]`), as plain arrays.
        basix's `tabulate(1, points)` returns (1 + tdim, npoints, ndofs, value_size) with index 0 the values and
        1 + k the derivative along reference axis k; field tables and dofmap both come from `V`, geometry tables and
        geometry dofmap both from `mesh.geometry`, so basix's node numbering never has to be known here.
        Elements whose dofs need per-cell transformations (Lagrange degree >= 3 on unordered meshes) are refused: the
        kernels apply none."""
        import basix

        if getattr(V.element, "needs_dof_transformations", False):
            raise NotImplementedError("DeviceMesh: elements that need dof transformations are not supported")
        mesh = V.mesh
        gdim = mesh.geometry.dim
        quadrature_points = np.asarray(quadrature_points, dtype=np.float64)
        tab = V.element.basix_element.tabulate(1, quadrature_points)
        # the coordinate element as a basix element of the same family / degree / variant as mesh.geometry.cmap
        cmap = mesh.geometry.cmap
        cell = getattr(basix.CellType, mesh.topology.cell_name())
        cel = basix.create_element(basix.ElementFamily.P, cell, cmap.degree, basix.LagrangeVariant(int(cmap.variant)))
        ctab = cel.tabulate(1, quadrature_points)
        if tab.shape[3] != 1:
            raise ValueError("DeviceMesh: the space's basix element must be the SCALAR sub-element of a blocked space")
        n_nodes = V.dofmap.index_map.size_local + V.dofmap.index_map.num_ghosts
        return dict(gdim=gdim, phi=tab[0, :, :, 0], dphi=np.moveaxis(tab[1:, :, :, 0], 0, 2),
                    dpsi=np.moveaxis(ctab[1:, :, :, 0], 0, 2), dofmap=V.dofmap.list, geom_dofmap=mesh.geometry.dofmap,
                    x=mesh.geometry.x, num_field_nodes=n_nodes, psi=ctab[0, :, :, 0])

    @classmethod
    def from_dolfinx(cls, V, quadrature_points, **kw):
        """From a DOLFINx function space and reference quadrature points (see `tables_from_dolfinx`). DOLFINx is not
        installed on the GPU box; tests drive this with stand-in objects that follow basix's documented layouts."""
        return cls(**cls.tables_from_dolfinx(V, quadrature_points), **kw)

    def vertex_transfer(self, psi_nodes) -> "NodalTransfer":
        """The nodal interpolation from the degree-1 space on the same cells to this mesh's field space, for
        DeviceCSR.amg(first_transfer=...): host NumPy, once per mesh. `psi_nodes` (ndofs per cell, ngeom): the degree-1 coordinate
        element tabulated at the field element's reference nodes (tools.synthetic.coordinate_element_at_nodes; on DOLFINx the
        coordinate element at V.element.interpolation_points). Coarse nodes are the geometry nodes; entries with |psi| <= 1e-14 are
        dropped; a node shared by several cells must get the same row from each (ValueError otherwise). A degree-1 field, where every
        row would be a single 1, is refused."""
        return vertex_transfer(self._dofmap, self._geom_dofmap, psi_nodes, self.num_field_nodes)

    def vertex_mesh(self, psi, dpsi, weights=None) -> "DeviceMesh":
        """The degree-1 mesh on the same cells, whose nodes ARE the geometry nodes: the coarse numbering of vertex_transfer, on which
        the coarse matrix of a krylov.PMG is assembled. `psi` (nq, ngeom) and `dpsi` (nq, ngeom, gdim): the coordinate element at a
        quadrature rule of the caller's choice, which may be coarser than this mesh's (phi = psi, dphi = dpsi, dofmap = geom_dofmap);
        `weights` (nq,): the rule's weights (set_weights). A mesh whose field is already of degree 1 raises ValueError, as
        vertex_transfer does."""
        if self._dofmap.shape[1] <= self._geom_dofmap.shape[1]:
            raise ValueError("vertex_mesh: the field has no more nodes per cell than the geometry (degree 1): there is nothing to coarsen")
        psi = np.ascontiguousarray(psi, dtype=np.float64)
        dpsi = np.ascontiguousarray(dpsi, dtype=np.float64)
        ng = self._geom_dofmap.shape[1]
        if psi.ndim != 2 or psi.shape[1] != ng or dpsi.shape != (psi.shape[0], ng, self.gdim):
            raise ValueError("vertex_mesh: psi (nq, ngeom) and dpsi (nq, ngeom, gdim) of the coordinate element")
        vm = DeviceMesh(gdim=self.gdim, phi=psi, dphi=dpsi, dpsi=dpsi, dofmap=self._geom_dofmap, geom_dofmap=self._geom_dofmap, x=self._x,
                        num_field_nodes=self._x.shape[0], ctx=self.ctx, psi=psi)
        if weights is not None:
            vm.set_weights(weights)
        return vm

    def value_size(self, kind: str, bs: int) -> int:
        r = self.ctx.lib.dxo_operand_value_size(self.gdim, int(bs), KINDS[kind])
        if r < 0:
            raise ValueError(f"operand '{kind}' is not defined for gdim={self.gdim}, block size {bs}")
        return r

    def evaluate(self, kind: str, bs: int, u, entities=None, out=None) -> np.ndarray:
        """Host arrays in, host array (n_cells, nq, value_size) out."""
        D = self.value_size(kind, bs)
        u = np.ascontiguousarray(_state(u), dtype=np.float64).reshape(-1)
        if u.size != self.num_field_nodes * bs:
            raise ValueError(f"field vector has {u.size} entries, expected {self.num_field_nodes * bs}")
        cells = None if entities is None else np.ascontiguousarray(entities, dtype=np.int32)
        n = self.num_cells if cells is None else cells.size
        if out is None:
            out = np.empty((n, self.nq, D))
        rc = self.ctx.lib.dxo_eval_operand(self.ctx._h, self._h, KINDS[kind], int(bs), MEM_HOST, u.ctypes.data,
                                           None if cells is None else cells.ctypes.data, n, out.ctypes.data)
        self.ctx.check(rc, "dxo_eval_operand")
        return out

    def set_coordinate_values(self, psi) -> None:
        """Values of the coordinate element's basis at the quadrature points, (nq, ngeom): what the operand `x` (ufl.SpatialCoordinate,
        test/test_nested_ex_op.py:113-118) needs beside the gradients the mesh already holds. basix: `tabulate(0, points)[0]` of
        `mesh.geometry.cmap`."""
        psi = np.ascontiguousarray(psi, dtype=np.float64)
        if psi.ndim != 2 or psi.shape[0] != self.nq:
            raise ValueError("psi must have shape (nq, ngeom)")
        self.ctx.check(self.ctx.lib.dxo_mesh_set_coordinate_values(self.ctx._h, self._h, psi.ctypes.data), "dxo_mesh_set_coordinate_values")

    def coordinate(self, entities=None, out=None) -> np.ndarray:
        """x at every quadrature point of the cells: host array (n_cells, nq, gdim) — `Expression(SpatialCoordinate(mesh), points).eval`."""
        cells = None if entities is None else np.ascontiguousarray(entities, dtype=np.int32)
        n = self.num_cells if cells is None else cells.size
        if out is None:
            out = np.empty((n, self.nq, self.gdim))
        rc = self.ctx.lib.dxo_eval_coordinate(self.ctx._h, self._h, MEM_HOST, None if cells is None else cells.ctypes.data, n, out.ctypes.data)
        self.ctx.check(rc, "dxo_eval_coordinate")
        return out

    def coordinate_device(self, n_cells: int, out_ptr: int, cells_ptr: int | None = None) -> None:
        """The same into device memory, asynchronous on the context's stream."""
        rc = self.ctx.lib.dxo_eval_coordinate(self.ctx._h, self._h, MEM_DEVICE, None if cells_ptr is None else C.c_void_p(cells_ptr), int(n_cells),
                                              C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_eval_coordinate")

    def set_facet_tables(self, phi, dphi, dpsi) -> None:
        """Tables for codim-1 entities, one set per LOCAL facet of the cell, tabulated at the facet quadrature points
        mapped into the reference cell (what Expression.eval does with `(cell, local_facet)` entities,
        external_operator.py:402; test/test_codim_external_operator.py:76-84): phi (nf, nq, ndofs),
        dphi (nf, nq, ndofs, gdim), dpsi (nf, nq, ngeom, gdim)."""
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        dphi = np.ascontiguousarray(dphi, dtype=np.float64)
        dpsi = np.ascontiguousarray(dpsi, dtype=np.float64)
        if phi.ndim != 3 or dphi.shape != phi.shape + (self.gdim,) or dpsi.ndim != 4 or dpsi.shape[:2] != phi.shape[:2] \
                or dpsi.shape[3] != self.gdim:
            raise ValueError("facet tables: phi (nf, nq, ndofs), dphi (nf, nq, ndofs, gdim), dpsi (nf, nq, ngeom, gdim)")
        rc = self.ctx.lib.dxo_mesh_set_facet_tables(self.ctx._h, self._h, phi.shape[0], phi.shape[1], phi.ctypes.data,
                                                    dphi.ctypes.data, dpsi.ctypes.data)
        self.ctx.check(rc, "dxo_mesh_set_facet_tables")
        self.nq_facet = phi.shape[1]

    def evaluate_facets(self, kind: str, bs: int, u, entities, out=None) -> np.ndarray:
        """Host arrays in, host array (n_entities, nq_facet, value_size) out; entities (n, 2) = (cell, local facet)."""
        D = self.value_size(kind, bs)
        u = np.ascontiguousarray(_state(u), dtype=np.float64).reshape(-1)
        if u.size != self.num_field_nodes * bs:
            raise ValueError(f"field vector has {u.size} entries, expected {self.num_field_nodes * bs}")
        ents = np.ascontiguousarray(entities, dtype=np.int32)
        if ents.ndim != 2 or ents.shape[1] != 2:
            raise ValueError("codim-1 entities must have shape (n, 2): (cell, local facet)")
        if out is None:
            out = np.empty((ents.shape[0], getattr(self, "nq_facet", 0), D))
        rc = self.ctx.lib.dxo_eval_operand_facets(self.ctx._h, self._h, KINDS[kind], int(bs), MEM_HOST, u.ctypes.data,
                                                  ents.ctypes.data, ents.shape[0], out.ctypes.data)
        self.ctx.check(rc, "dxo_eval_operand_facets")
        return out

    def evaluate_facets_device(self, kind: str, bs: int, u, entities, out=None):
        """evaluate_facets on the device, asynchronous on the context's stream: u a float64 CUDA tensor of num_field_nodes * bs entries,
        entities an int32 CUDA tensor (n, 2) of (cell, local facet) pairs (e.g. a CUDA copy of FacetSet.entities; the device path does
        not range-check them, as dxo_eval_operand_facets says), out a float64 CUDA tensor of n * nq_facet * value_size entries or None
        for a new one. Returns out, shaped (n, nq_facet, value_size) when it was made here."""
        import torch

        D = self.value_size(kind, bs)
        if not hasattr(self, "nq_facet"):
            raise ValueError("evaluate_facets_device: facet tables not set (set_facet_tables)")
        dev = torch.device("cuda", self.ctx.device)

        def ok(t, dtype):
            return isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == dev and t.is_contiguous()

        if not ok(u, torch.float64) or u.numel() != self.num_field_nodes * bs:
            raise ValueError(f"evaluate_facets_device: u must be a contiguous float64 CUDA tensor of {self.num_field_nodes * bs} entries")
        if not ok(entities, torch.int32) or entities.ndim != 2 or entities.shape[1] != 2:
            raise ValueError("evaluate_facets_device: entities must be a contiguous int32 CUDA tensor of shape (n, 2): (cell, local facet)")
        n = entities.shape[0]
        if out is None:
            out = torch.empty((n, self.nq_facet, D), dtype=torch.float64, device=dev)
        if not ok(out, torch.float64) or out.numel() != n * self.nq_facet * D:
            raise ValueError(f"evaluate_facets_device: out must be a contiguous float64 CUDA tensor of {n * self.nq_facet * D} entries")
        rc = self.ctx.lib.dxo_eval_operand_facets(self.ctx._h, self._h, KINDS[kind], int(bs), MEM_DEVICE, C.c_void_p(u.data_ptr()),
                                                  C.c_void_p(entities.data_ptr()), n, C.c_void_p(out.data_ptr()))
        self.ctx.check(rc, "dxo_eval_operand_facets")
        return out

    def evaluate_device(self, kind: str, bs: int, u_ptr: int, n_cells: int, out_ptr: int, cells_ptr: int | None = None) -> None:
        """Raw device pointers, asynchronous on the context's stream."""
        rc = self.ctx.lib.dxo_eval_operand(self.ctx._h, self._h, KINDS[kind], int(bs), MEM_DEVICE, C.c_void_p(u_ptr),
                                           None if cells_ptr is None else C.c_void_p(cells_ptr), int(n_cells),
                                           C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_eval_operand")

    def operand(self, kind: str, field, bs: int | None = None, name: str | None = None, lazy: bool = False,
                snapshot: bool = True) -> "DeviceOperand":
        """lazy=True: `.eval()` over all cells returns a `LazyOperand` — an array-like that a fused consumer
        (`make_von_mises`) evaluates inside its own launch and that turns into the ndarray on `np.asarray`.
        snapshot (lazy only): True copies the field vector when the operand is "evaluated", so the value is the one at
        `evaluate_operands` time exactly as with `Expression.eval` (one host copy of the dof vector per call: 25-40 ms
        at 10^7 Q2 nodes). False keeps a reference to the live array instead — for the reference's own calling
        sequence, where `evaluate_external_operators` follows `evaluate_operands` at once (demo_plasticity_von_mises.py:
        445-456) and the field does not change in between."""
        if kind == "x":     # ufl.SpatialCoordinate(mesh): no field (pass None), codim-0 entities
            return DeviceOperand(self, "x", None, self.gdim, name or "x", False, snapshot)
        return DeviceOperand(self, kind, field, self.gdim if bs is None else bs, name or kind, lazy, snapshot)

    def von_mises(self, prm, u, sigma_n, p, C_tang, sigma, dp, mem: int = MEM_HOST) -> None:
        """dxo_von_mises_field: eps(u) + radial return + tangent in one launch (all cells of the mesh)."""
        def ptr(a):
            return a if isinstance(a, (int, np.integer)) or a is None else a.ctypes.data
        rc = self.ctx.lib.dxo_von_mises_field(self.ctx._h, C.byref(prm), self._h, int(mem), *(C.c_void_p(ptr(a)) for a in
                                              (u, sigma_n, p, C_tang, sigma, dp)))
        self.ctx.check(rc, "dxo_von_mises_field")

    def set_weights(self, weights) -> None:
        """Reference quadrature weights (nq values, `basix.make_quadrature(...)[1]`): needed by adjoint / tangent_apply."""
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.size != self.nq:
            raise ValueError(f"{w.size} weights for {self.nq} quadrature points")
        self.ctx.check(self.ctx.lib.dxo_mesh_set_weights(self.ctx._h, self._h, w.ctypes.data), "dxo_mesh_set_weights")


    def patch_info(self) -> dict:
        """The patches of the patch form of the internal force — an experiment that is NOT in the product library: the entry point
        (dxo_mesh_patch_info, scripts/exp/adjoint_patch_kernels.h) exists only in a -DDXO_EXPERIMENTS build (scripts/exp/build_variant.py,
        loaded through DXO_HIP_LIBRARY) and is bound here on demand."""
        import numpy as np

        fn = getattr(self.ctx.lib, "dxo_mesh_patch_info", None)
        if fn is None:
            raise DxoError("dxo_mesh_patch_info: the patch form is not part of this build of libdxo_hip.so (-DDXO_EXPERIMENTS only)")
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]
        info = np.zeros(8, dtype=np.int64)
        self.ctx.check(fn(self.ctx._h, self._h, info.ctypes.data), "dxo_mesh_patch_info")
        keys = ("patches", "groups_per_wave", "wave_groups", "max_patch_nodes", "patch_nodes", "shared_nodes", "shared_entry_ppm", "waves_per_patch")
        out = dict(zip(keys, (int(x) for x in info)))
        out["max_wave_nodes"] = out["groups_per_wave"] >> 32
        out["groups_per_wave"] &= 0xFFFFFFFF
        out["schedule_fill"] = out["wave_groups"] / max(1, out["patches"] * out["waves_per_patch"] * out["groups_per_wave"])
        return out

    def adjoint(self, kind: str, bs: int, S_ptr: int, out_ptr: int, n_cells: int | None = None, cells_ptr: int | None = None) -> None:
        """out += sum_q w |det J| B^T S (DEVICE pointers): the assembled vector of inner(S, operand(v)) dx."""
        rc = self.ctx.lib.dxo_operand_adjoint(self.ctx._h, self._h, KINDS[kind], int(bs), C.c_void_p(S_ptr),
                                              None if cells_ptr is None else C.c_void_p(cells_ptr),
                                              self.num_cells if n_cells is None else int(n_cells), C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_operand_adjoint")

    def tangent_apply(self, C_tang_ptr: int, v_ptr: int, out_ptr: int) -> None:
        """out += K v with K = sum_q w |det J| B^T C_tang B never formed (DEVICE pointers, eps / Mandel, bs = gdim)."""
        rc = self.ctx.lib.dxo_tangent_apply(self.ctx._h, self._h, C.c_void_p(C_tang_ptr), C.c_void_p(v_ptr), C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_tangent_apply")

    def tangent_diagonal(self, C_tang_ptr: int, out_ptr: int) -> None:
        """out += diag(K) for the same K as tangent_apply (DEVICE pointers): Jacobi preconditioner."""
        rc = self.ctx.lib.dxo_tangent_diagonal(self.ctx._h, self._h, C.c_void_p(C_tang_ptr), C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_tangent_diagonal")

    # (test, trial, bs == gdim) pairs of dxo_bilinear_apply; "F" stands for its linearisation, grad
    BILINEAR_PAIRS_VECTOR = {("grad", "grad"), ("grad", "F"), ("F", "grad"), ("F", "F"), ("eps", "eps")}
    BILINEAR_PAIRS_SCALAR = {("grad", "value_grad"), ("grad", "grad"), ("value", "value"), ("value_grad", "value_grad")}

    def _bilinear_kinds(self, test: str, trial: str, bs: int) -> tuple[int, int]:
        pairs = self.BILINEAR_PAIRS_VECTOR if int(bs) == self.gdim else self.BILINEAR_PAIRS_SCALAR if int(bs) == 1 else set()
        if (test, trial) not in pairs:
            raise ValueError(f"bilinear form: unsupported pair ({test!r}, {trial!r}) with bs = {bs} on gdim {self.gdim}; bs = gdim takes "
                             f"{sorted(self.BILINEAR_PAIRS_VECTOR)}, bs = 1 takes {sorted(self.BILINEAR_PAIRS_SCALAR)}")
        return KINDS[test], KINDS[trial]

    def bilinear_apply(self, test: str, trial: str, bs: int, C_ptr: int, v_ptr: int, out_ptr: int) -> None:
        """out += sum_q w |det J| B_test^T C B_trial v (DEVICE pointers; C [num_cells*nq][D_test][D_trial], 16-byte aligned): the action of
        the bilinear form inner(C : trial(u_hat), test(v)) dx — e.g. ("grad", "grad", gdim) with C = dP/dF, the hyperelastic Jacobian."""
        t, r = self._bilinear_kinds(test, trial, bs)
        rc = self.ctx.lib.dxo_bilinear_apply(self.ctx._h, self._h, t, r, int(bs), C.c_void_p(C_ptr), C.c_void_p(v_ptr), C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_bilinear_apply")

    def bilinear_apply_t(self, test: str, trial: str, bs: int, C_ptr: int, v_ptr: int, out_ptr: int) -> None:
        """out += sum_q w |det J| B_trial^T C^T B_test v (dxo_bilinear_apply_t): the action of the TRANSPOSE of bilinear_apply's operator,
        for adjoint solves. (test, trial), C and its layout are those of the forward call; nothing is transposed by the caller. The
        diagonal of the transpose is bilinear_diagonal. The transposed boundary-facet action has no call of its own: it composes from
        evaluate_facets_device("value", v), a pointwise C^T product and facet_adjoint of the trial kind."""
        t, r = self._bilinear_kinds(test, trial, bs)
        rc = self.ctx.lib.dxo_bilinear_apply_t(self.ctx._h, self._h, t, r, int(bs), C.c_void_p(C_ptr), C.c_void_p(v_ptr), C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_bilinear_apply_t")

    def bilinear_diagonal(self, test: str, trial: str, bs: int, C_ptr: int, out_ptr: int) -> None:
        """out += diag of the same operator as bilinear_apply (DEVICE pointers): Jacobi preconditioner."""
        t, r = self._bilinear_kinds(test, trial, bs)
        rc = self.ctx.lib.dxo_bilinear_diagonal(self.ctx._h, self._h, t, r, int(bs), C.c_void_p(C_ptr), C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_bilinear_diagonal")

    def csr_pattern(self, bs: int) -> "CsrPattern":
        """The CSR pattern of this mesh's field with block size bs (dxo_csr_create): built once per block size and kept by the mesh."""
        pats = self.__dict__.setdefault("_csr", {})
        if int(bs) not in pats:
            pats[int(bs)] = CsrPattern(self, int(bs))
        return pats[int(bs)]

    def bilinear_assemble(self, test: str, trial: str, bs: int, C_ptr: int, pattern: "CsrPattern", values=None, bcs=None,
                          diagonal: float = 1.0) -> "DeviceCSR":
        """The bilinear form of bilinear_apply ASSEMBLED on `pattern` (dxo_bilinear_assemble): values (+)= sum_cells sum_q w |det J|
        B_test^T C B_trial, C a DEVICE pointer as for bilinear_apply. `values`: a float64 CUDA tensor of pattern.nnz entries, accumulated
        into (SET with option consumer_overwrite); None: a new zero tensor. `bcs`: an int32 CUDA tensor of constrained dofs, whose rows and
        columns are then zeroed and whose diagonal is set to `diagonal` (dxo_csr_dirichlet), as assemble_matrix(J, bcs) does."""
        t, r = self._bilinear_kinds(test, trial, bs)

        def assemble(values_ptr):
            rc = self.ctx.lib.dxo_bilinear_assemble(self.ctx._h, self._h, pattern._h, t, r, int(bs), C.c_void_p(C_ptr), values_ptr)
            self.ctx.check(rc, "dxo_bilinear_assemble")

        return self._assemble_on("bilinear_assemble", pattern, values, bcs, diagonal, assemble)

    def _assemble_on(self, who: str, pattern: "CsrPattern", values, bcs, diagonal: float, assemble) -> "DeviceCSR":
        """The values / bcs half of the two *_assemble methods: `values` checked (None: a new zero tensor), assemble(pointer to them), then
        the Dirichlet pass over `bcs` (dxo_csr_dirichlet) unless it is None."""
        import torch

        if values is None:
            values = torch.zeros(pattern.nnz, dtype=torch.float64, device=torch.device("cuda", self.ctx.device))
        if not (values.dtype == torch.float64 and values.is_cuda and values.is_contiguous() and values.numel() == pattern.nnz):
            raise ValueError(f"{who}: values must be a contiguous float64 CUDA tensor of {pattern.nnz} entries")
        assemble(C.c_void_p(values.data_ptr()))
        if bcs is not None:
            if not (bcs.dtype == torch.int32 and bcs.is_cuda and bcs.is_contiguous()):
                raise ValueError(f"{who}: bcs must be a contiguous int32 CUDA tensor")
            rc = self.ctx.lib.dxo_csr_dirichlet(self.ctx._h, pattern._h, C.c_void_p(bcs.data_ptr()), int(bcs.numel()), float(diagonal),
                                                C.c_void_p(values.data_ptr()))
            self.ctx.check(rc, "dxo_csr_dirichlet")
        return DeviceCSR(pattern, values)

    def set_facet_geometry(self, weights, ref_normals, ref_jacobians) -> None:
        """Reference facet data for the boundary integrals (dxo_mesh_set_facet_geometry), one entry per LOCAL facet, matching
        set_facet_tables (call it first): weights (nq,) = basix.make_quadrature(facet_cell, deg)[1], ref_normals (nf, gdim) =
        basix.cell.facet_outward_normals(cell), ref_jacobians (nf, gdim, gdim - 1) = basix.cell.facet_jacobians(cell)."""
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        nrm = np.ascontiguousarray(ref_normals, dtype=np.float64)
        jac = np.ascontiguousarray(ref_jacobians, dtype=np.float64)
        G = self.gdim
        if nrm.ndim != 2 or nrm.shape[1] != G or jac.shape != (nrm.shape[0], G, G - 1):
            raise ValueError("facet geometry: weights (nq,), ref_normals (nf, gdim), ref_jacobians (nf, gdim, gdim - 1)")
        rc = self.ctx.lib.dxo_mesh_set_facet_geometry(self.ctx._h, self._h, nrm.shape[0], w.size, w.ctypes.data, nrm.ctypes.data,
                                                      jac.ctypes.data)
        self.ctx.check(rc, "dxo_mesh_set_facet_geometry")

    def facet_set(self, entities) -> "FacetSet":
        """The device facet set of the (cell, local facet) pairs `entities` (n, 2) (dxo_facet_set_create), e.g. the facets of one tag:
        built once and kept by the mesh, keyed by the entity array's bytes."""
        ents = np.ascontiguousarray(entities, dtype=np.int32)
        if ents.ndim != 2 or ents.shape[1] != 2:
            raise ValueError("facet entities must have shape (n, 2): (cell, local facet)")
        sets = self.__dict__.setdefault("_facet_sets", {})
        key = ents.tobytes()
        if key not in sets:
            sets[key] = FacetSet(self, ents)
        return sets[key]

    def facet_geometry(self, facet_set: "FacetSet", normals_ptr: int | None = None, dS_ptr: int | None = None) -> None:
        """FacetNormal (n, nq, gdim) and the point measure dS = w |det J_f| (n, nq) at the set's facet points (dxo_eval_facet_geometry;
        DEVICE pointers, either may be None), asynchronous on the context's stream."""
        rc = self.ctx.lib.dxo_eval_facet_geometry(self.ctx._h, self._h, facet_set._h, None if normals_ptr is None else C.c_void_p(normals_ptr),
                                                  None if dS_ptr is None else C.c_void_p(dS_ptr))
        self.ctx.check(rc, "dxo_eval_facet_geometry")

    FACET_ADJOINT_KINDS = ("value", "grad", "value_grad", "eps", "div", "F")

    def _facet_kind_check(self, who: str, what: str, form: str, kind: str, bs: int) -> None:
        """The (kind, bs) a facet form admits: a linear kind at bs = 1 or gdim, the kinds of a vector field at gdim alone."""
        if kind not in self.FACET_ADJOINT_KINDS:
            raise ValueError(f"{who}: {what} {kind!r} has no {form}; linear kinds: {self.FACET_ADJOINT_KINDS}")
        if int(bs) not in (1, self.gdim) or (kind in ("eps", "div", "F") and int(bs) != self.gdim):
            raise ValueError(f"{who}: bs = {bs} does not fit {what} {kind!r} on gdim {self.gdim} (bs = 1 or gdim; eps / div / F: gdim)")

    def facet_adjoint(self, kind: str, bs: int, S_ptr: int, facet_set: "FacetSet", out_ptr: int) -> None:
        """out += sum_e sum_q dS B^T S over the set's facets (dxo_facet_adjoint; DEVICE pointers, S (n, nq, value_size)): the assembled
        vector of inner(S, operand(v)) ds. ("value", gdim) with S = t is a traction load. Always accumulates."""
        self._facet_kind_check("facet_adjoint", "kind", "adjoint", kind, bs)
        rc = self.ctx.lib.dxo_facet_adjoint(self.ctx._h, self._h, facet_set._h, KINDS[kind], int(bs), C.c_void_p(S_ptr), C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_facet_adjoint")

    def facet_pressure(self, facet_set: "FacetSet", out_ptr: int, p_ptr: int | None = None, scale: float = 1.0) -> None:
        """out[node*gdim + i] += scale * sum_e sum_q dS p phi_a n_i (dxo_facet_pressure; DEVICE pointers, p (n, nq) or None for p = 1):
        the demo's boundary term -inner(loading * -n, v) ds is facet_pressure(scale=loading). Always accumulates."""
        rc = self.ctx.lib.dxo_facet_pressure(self.ctx._h, self._h, facet_set._h, None if p_ptr is None else C.c_void_p(p_ptr), float(scale),
                                             C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_facet_pressure")

    # ---- scalar functionals (csrc/functional.hip): CUDA tensors in, CUDA tensors out, nothing synchronised — the caller's .item() /
    # .cpu() does. Results are SET, bit-reproducible and independent of the launch shape.
    INTEGRATE_SIZES = (1, 2, 3, 4, 6, 9)

    def _functional_tensor(self, who: str, name: str, t, dtype, shape, optional: bool = False):
        """`t` checked as a contiguous CUDA tensor of this context's device with `dtype` and `shape` (None entries: any extent)."""
        import torch

        if t is None and optional:
            return None
        dev = torch.device("cuda", self.ctx.device)
        ok = isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == dev and t.is_contiguous() and t.ndim == len(shape) and \
            all(s is None or s == e for s, e in zip(shape, t.shape))
        if not ok:
            want = "(" + ", ".join("n" if s is None else str(s) for s in shape) + ("," if len(shape) == 1 else "") + ")"
            raise ValueError(f"{who}: {name} must be a contiguous {str(dtype).replace('torch.', '')} CUDA tensor of shape {want} on {dev}")
        return t

    def _functional_cells(self, who: str, cells):
        import torch

        cells = self._functional_tensor(who, "cells", cells, torch.int32, (None,), optional=True)
        return cells, (self.num_cells if cells is None else cells.shape[0]), (None if cells is None else C.c_void_p(cells.data_ptr()))

    def _functional_out(self, who: str, out, n: int):
        import torch

        if out is None:
            return torch.empty((n,), dtype=torch.float64, device=torch.device("cuda", self.ctx.device))
        return self._functional_tensor(who, "out", out, torch.float64, (n,))

    def cell_measure(self, cells=None, out=None):
        """dx = w |det J| at the quadrature points of `cells` (an int32 CUDA tensor (n,), None: all cells), a float64 CUDA tensor
        (n, nq) (dxo_eval_cell_measure): the cell counterpart of the dS of facet_geometry. Needs set_weights."""
        import torch

        cells, n, cptr = self._functional_cells("cell_measure", cells)
        if out is None:
            out = torch.empty((n, self.nq), dtype=torch.float64, device=torch.device("cuda", self.ctx.device))
        self._functional_tensor("cell_measure", "out", out, torch.float64, (n, self.nq))
        rc = self.ctx.lib.dxo_eval_cell_measure(self.ctx._h, self._h, cptr, n, C.c_void_p(out.data_ptr()))
        self.ctx.check(rc, "dxo_eval_cell_measure")
        return out

    def integrate(self, f, g=None, cells=None, out=None):
        """The integrals over `cells` (None: all) of quadrature data f, a float64 CUDA tensor (n, nq, D) indexed by position in the
        list, as evaluate / Expression.eval lay it out (dxo_integrate). g = None: the D integrals of the components, a (D,) tensor, D in
        INTEGRATE_SIZES; g shaped like f: the pairing int f : g dx, a (1,) tensor, any D (g may be f: int |f|^2 dx)."""
        import torch

        cells, n, cptr = self._functional_cells("integrate", cells)
        if isinstance(f, torch.Tensor) and f.ndim == 2:
            f = f.unsqueeze(2)
        if isinstance(g, torch.Tensor) and g.ndim == 2:
            g = g.unsqueeze(2)
        f = self._functional_tensor("integrate", "f", f, torch.float64, (n, self.nq, None))
        D = f.shape[2]
        g = self._functional_tensor("integrate", "g", g, torch.float64, (n, self.nq, D), optional=True)
        if D < 1 or (g is None and D not in self.INTEGRATE_SIZES):
            raise ValueError(f"integrate: f (n, nq, D) has D = {D}; without g the value sizes {self.INTEGRATE_SIZES} are served")
        out = self._functional_out("integrate", out, D if g is None else 1)
        # an empty tensor has no address, and a NULL g would select the per-component form: `out` stands in (nothing is read at n = 0)
        fp, gp = (out.data_ptr(), None if g is None else out.data_ptr()) if n == 0 else (f.data_ptr(), None if g is None else g.data_ptr())
        rc = self.ctx.lib.dxo_integrate(self.ctx._h, self._h, cptr, n, D, C.c_void_p(fp), None if gp is None else C.c_void_p(gp),
                                        C.c_void_p(out.data_ptr()))
        self.ctx.check(rc, "dxo_integrate")
        return out

    def facet_integrate(self, f, facet_set: "FacetSet", g=None, out=None):
        """integrate over the facets of `facet_set` with dS (dxo_facet_integrate): f a float64 CUDA tensor (n, nq_facet, D), e.g. torch
        arithmetic on evaluate_facets_device. Needs set_facet_geometry."""
        import torch

        if not hasattr(self, "nq_facet"):
            raise ValueError("facet_integrate: facet tables not set (set_facet_tables)")
        if isinstance(f, torch.Tensor) and f.ndim == 2:
            f = f.unsqueeze(2)
        if isinstance(g, torch.Tensor) and g.ndim == 2:
            g = g.unsqueeze(2)
        f = self._functional_tensor("facet_integrate", "f", f, torch.float64, (facet_set.n, self.nq_facet, None))
        D = f.shape[2]
        g = self._functional_tensor("facet_integrate", "g", g, torch.float64, (facet_set.n, self.nq_facet, D), optional=True)
        if D < 1 or (g is None and D not in self.INTEGRATE_SIZES):
            raise ValueError(f"facet_integrate: f (n, nq_facet, D) has D = {D}; without g the value sizes {self.INTEGRATE_SIZES} are served")
        out = self._functional_out("facet_integrate", out, D if g is None else 1)
        empty = facet_set.n == 0      # as in integrate: `out` stands in for the addresses of empty tensors
        fp, gp = (out.data_ptr(), None if g is None else out.data_ptr()) if empty else (f.data_ptr(), None if g is None else g.data_ptr())
        rc = self.ctx.lib.dxo_facet_integrate(self.ctx._h, self._h, facet_set._h, D, C.c_void_p(fp), None if gp is None else C.c_void_p(gp),
                                              C.c_void_p(out.data_ptr()))
        self.ctx.check(rc, "dxo_facet_integrate")
        return out

    def operand_moments(self, kind: str, bs: int, u, cells=None, out=None):
        """The fused form (dxo_operand_moments): the operand `kind` of the dofs u (a float64 CUDA tensor of num_field_nodes * bs
        entries, bs = 1 or gdim) is formed in registers and never written. Returns a (D + 1,) tensor: [int operand_k dx for k < D,
        int |operand|^2 dx]. "value": mean and squared L2 norm; "grad": squared H1 seminorm; "detF": deformed volume; "div": outflow."""
        import torch

        D = self.value_size(kind, bs)
        if bs not in (1, self.gdim):
            raise ValueError(f"operand_moments: block size {bs} has no fused form (bs = 1 or gdim = {self.gdim})")
        cells, n, cptr = self._functional_cells("operand_moments", cells)
        u = self._functional_tensor("operand_moments", "u", u, torch.float64, (self.num_field_nodes * bs,))
        out = self._functional_out("operand_moments", out, D + 1)
        rc = self.ctx.lib.dxo_operand_moments(self.ctx._h, self._h, KINDS[kind], int(bs), C.c_void_p(u.data_ptr()), cptr, n,
                                              C.c_void_p(out.data_ptr()))
        self.ctx.check(rc, "dxo_operand_moments")
        return out

    # trial kinds of the facet bilinear forms: the linear kinds, "F" standing for its linearisation, grad
    FACET_BILINEAR_TRIALS = FACET_ADJOINT_KINDS

    def _facet_bilinear_kinds(self, who: str, test: str, trial: str, bs: int) -> tuple[int, int]:
        if test != "value":
            raise ValueError(f"{who}: the test kind must be 'value' (a boundary residual g . v ds), not {test!r}")
        self._facet_kind_check(who, "trial kind", "bilinear form", trial, bs)
        return KINDS[test], KINDS[trial]

    def facet_bilinear_apply(self, trial: str, bs: int, C_ptr: int, v_ptr: int, facet_set: "FacetSet", out_ptr: int, test: str = "value") -> None:
        """out += K v with K[(a,i),(b,j)] = sum_e sum_q dS phi_a sum_r C[i][r] (B_trial)_r,(b,j) over the set's facets
        (dxo_facet_bilinear_apply; DEVICE pointers, C (n, nq_facet, bs, value_size(trial, bs))): the action of the Jacobian of a boundary
        term g(operand(u)) . v ds with C = dg/d operand — ("value", 1) with C = dg/dT is a Robin term. Always accumulates."""
        t, r = self._facet_bilinear_kinds("facet_bilinear_apply", test, trial, bs)
        rc = self.ctx.lib.dxo_facet_bilinear_apply(self.ctx._h, self._h, facet_set._h, t, r, int(bs), C.c_void_p(C_ptr), C.c_void_p(v_ptr),
                                                   C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_facet_bilinear_apply")

    def facet_bilinear_diagonal(self, trial: str, bs: int, C_ptr: int, facet_set: "FacetSet", out_ptr: int, test: str = "value") -> None:
        """out += diag of the same operator as facet_bilinear_apply (dxo_facet_bilinear_diagonal; DEVICE pointers). Always accumulates."""
        t, r = self._facet_bilinear_kinds("facet_bilinear_diagonal", test, trial, bs)
        rc = self.ctx.lib.dxo_facet_bilinear_diagonal(self.ctx._h, self._h, facet_set._h, t, r, int(bs), C.c_void_p(C_ptr), C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_facet_bilinear_diagonal")

    def facet_bilinear_assemble(self, trial: str, bs: int, C_ptr: int, facet_set: "FacetSet", pattern: "CsrPattern", values=None, bcs=None,
                                diagonal: float = 1.0, test: str = "value") -> "DeviceCSR":
        """The operator of facet_bilinear_apply ASSEMBLED on `pattern` (dxo_facet_bilinear_assemble): values += K, always accumulated.
        `values` and `bcs` as in bilinear_assemble: with values=A.values the boundary term is added to a cell matrix, and the Dirichlet
        pass (dxo_csr_dirichlet) runs after it — so assemble the cell form without bcs and pass them here."""
        t, r = self._facet_bilinear_kinds("facet_bilinear_assemble", test, trial, bs)

        def assemble(values_ptr):
            rc = self.ctx.lib.dxo_facet_bilinear_assemble(self.ctx._h, self._h, facet_set._h, pattern._h, t, r, int(bs), C.c_void_p(C_ptr), values_ptr)
            self.ctx.check(rc, "dxo_facet_bilinear_assemble")

        return self._assemble_on("facet_bilinear_assemble", pattern, values, bcs, diagonal, assemble)

    def tangent_apply_vm(self, prm, sigma_ptr: int, dp_ptr: int, v_ptr: int, out_ptr: int) -> None:
        """out += K v with the von Mises consistent tangent formed per point from the operator's returned (sigma, dp) — no C_tang
        array (dxo_tangent_apply_vm; DEVICE pointers, e.g. VmState.pointers()): 56 instead of 288 bytes per point."""
        rc = self.ctx.lib.dxo_tangent_apply_vm(self.ctx._h, self._h, C.byref(prm), C.c_void_p(sigma_ptr), C.c_void_p(dp_ptr),
                                               C.c_void_p(v_ptr), C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_tangent_apply_vm")

    def tangent_diagonal_vm(self, prm, sigma_ptr: int, dp_ptr: int, out_ptr: int) -> None:
        """out += diag(K) from the returned (sigma, dp) (dxo_tangent_diagonal_vm)."""
        rc = self.ctx.lib.dxo_tangent_diagonal_vm(self.ctx._h, self._h, C.byref(prm), C.c_void_p(sigma_ptr), C.c_void_p(dp_ptr),
                                                  C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_tangent_diagonal_vm")

    def von_mises_residual(self, prm, u_ptr: int, sigma_n_ptr: int, p_ptr: int, sigma_ptr: int, dp_ptr: int, R_ptr: int) -> None:
        """(sigma, dp) = von Mises return map of (eps(u), sigma_n, p) and R += sum_q w|J| B^T sigma in one call
        (dxo_von_mises_residual; DEVICE pointers): the residual evaluation of a Newton iteration of a matrix-free solve."""
        rc = self.ctx.lib.dxo_von_mises_residual(self.ctx._h, C.byref(prm), self._h, *(C.c_void_p(a) for a in
                                                 (u_ptr, sigma_n_ptr, p_ptr, sigma_ptr, dp_ptr, R_ptr)))
        self.ctx.check(rc, "dxo_von_mises_residual")

    def isihara3_residual(self, prm, u_ptr: int, R_ptr: int) -> None:
        """R += sum_q w|J| B^T P(I + grad u) of the 3-D Isihara model, stress formed per point from the dof vector — no P array
        (dxo_isihara3_residual; DEVICE pointers, gdim = 3): isihara3_field followed by adjoint("F", 3) without the 720 bytes per point."""
        rc = self.ctx.lib.dxo_isihara3_residual(self.ctx._h, C.byref(prm), self._h, C.c_void_p(u_ptr), C.c_void_p(R_ptr))
        self.ctx.check(rc, "dxo_isihara3_residual")

    def isihara3_tangent_apply(self, prm, u_ptr: int, v_ptr: int, out_ptr: int) -> None:
        """out += K(u) v with dP/dF : grad v formed per point from the dof vectors u and v — no dP array (dxo_isihara3_tangent_apply;
        DEVICE pointers): bilinear_apply("grad", "grad", 3, dP, v) without the 648 bytes per point read at every matvec."""
        rc = self.ctx.lib.dxo_isihara3_tangent_apply(self.ctx._h, C.byref(prm), self._h, C.c_void_p(u_ptr), C.c_void_p(v_ptr),
                                                     C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_isihara3_tangent_apply")

    def isihara3_tangent_diagonal(self, prm, u_ptr: int, out_ptr: int) -> None:
        """out += diag(K(u)) from the dof vector (dxo_isihara3_tangent_diagonal): Jacobi preconditioner of the same operator."""
        rc = self.ctx.lib.dxo_isihara3_tangent_diagonal(self.ctx._h, C.byref(prm), self._h, C.c_void_p(u_ptr), C.c_void_p(out_ptr))
        self.ctx.check(rc, "dxo_isihara3_tangent_diagonal")

    def heat(self, A: float, B: float, T_dofs, q=None, dqdT=None, dqdsigma=None, mem: int = MEM_HOST) -> None:
        """dxo_heat_field: T and grad T of a scalar field + the heat-flux kernels in one launch (all cells)."""
        def ptr(a):
            return a if isinstance(a, (int, np.integer)) or a is None else a.ctypes.data
        rc = self.ctx.lib.dxo_heat_field(self.ctx._h, float(A), float(B), self._h, int(mem),
                                         *(None if a is None else C.c_void_p(ptr(a)) for a in (T_dofs, q, dqdT, dqdsigma)))
        self.ctx.check(rc, "dxo_heat_field")

    def close(self) -> None:
        for pat in self.__dict__.pop("_csr", {}).values():
            pat.close()
        for fs in self.__dict__.pop("_facet_sets", {}).values():
            fs.close()
        if getattr(self, "_h", None) and self.ctx._h:
            self.ctx.lib.dxo_mesh_destroy(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NodalTransfer:
    """W of a nodal interpolation in CSR form: row i holds the coarse nodes `col` (ascending) and weights `w` of fine node i;
    `coarse_to_fine[v]` is the fine node that coarse node v is (its row is the single entry (v, 1)). The argument `first_transfer`
    of DeviceCSR.amg (dxo_amg_transfer)."""

    def __init__(self, n_coarse, ptr, col, w, coarse_to_fine):
        self.n_coarse = int(n_coarse)
        self.ptr = np.ascontiguousarray(ptr, dtype=np.int64)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.w = np.ascontiguousarray(w, dtype=np.float64)
        self.coarse_to_fine = np.ascontiguousarray(coarse_to_fine, dtype=np.int32)

    def to_scipy(self):
        import scipy.sparse

        return scipy.sparse.csr_matrix((self.w, self.col, self.ptr), shape=(self.ptr.size - 1, self.n_coarse))


def vertex_transfer(dofmap, geom_dofmap, psi_nodes, num_field_nodes: int | None = None) -> NodalTransfer:
    """DeviceMesh.vertex_transfer on plain arrays: dofmap (cells, ndofs), geom_dofmap (cells, ngeom), psi_nodes (ndofs, ngeom)."""
    dofmap = np.asarray(dofmap, dtype=np.int64)
    geom = np.asarray(geom_dofmap, dtype=np.int64)
    psi = np.asarray(psi_nodes, dtype=np.float64)
    nc, nd = dofmap.shape
    if psi.shape != (nd, geom.shape[1]) or geom.shape[0] != nc:
        raise ValueError("vertex_transfer: psi_nodes must have the shape (dofs per cell, geometry nodes per cell)")
    if nd <= geom.shape[1]:
        raise ValueError("vertex_transfer: the field has no more nodes per cell than the geometry (degree 1): there is nothing to coarsen")
    n = int(num_field_nodes) if num_field_nodes is not None else int(dofmap.max()) + 1
    n_coarse = int(geom.max()) + 1
    a, v = np.nonzero(np.abs(psi) > 1e-14)                    # the same local entries in every cell
    rows = dofmap[:, a].reshape(-1)
    cols = geom[:, v].reshape(-1)
    vals = np.broadcast_to(psi[a, v], (nc, a.size)).reshape(-1)
    key = rows * n_coarse + cols
    order = np.argsort(key, kind="stable")
    key, vals = key[order], vals[order]
    first = np.concatenate([[True], key[1:] != key[:-1]])
    start = np.flatnonzero(first)
    group = np.cumsum(first) - 1
    if np.abs(vals - vals[start][group]).max(initial=0.0) > 1e-12:
        raise ValueError("vertex_transfer: the cells that share a node disagree on its weights")
    ukey, w = key[start], vals[start]
    r, c = ukey // n_coarse, ukey % n_coarse
    counts = np.bincount(r, minlength=n)
    if (counts == 0).any():
        raise ValueError("vertex_transfer: a field node belongs to no cell")
    ptr = np.concatenate([[0], np.cumsum(counts)])
    single = np.flatnonzero((counts == 1) & (w[ptr[:-1]] == 1.0))       # the fine nodes that are coarse nodes
    ctf = -np.ones(n_coarse, dtype=np.int64)
    ctf[c[ptr[single]]] = single
    if (ctf < 0).any() or np.unique(ctf).size != n_coarse:
        raise ValueError("vertex_transfer: not every geometry node is a field node with the weight 1")
    return NodalTransfer(n_coarse, ptr, c, w, ctf)


class CsrPattern:
    """dxo_csr: the CSR pattern of one Lagrange field with block size bs on a DeviceMesh. Rows and columns are the blocked dofs
    node*bs + i; a row holds the columns of every node that shares a cell with its node, sorted, diagonal included (DOLFINx's layout for
    a serial blocked space). `indptr` (int64) / `indices` (int32) are device copies of the library's arrays; `build_ms` the build time."""

    def __init__(self, mesh: DeviceMesh, bs: int):
        self.ctx, self.bs, self.gdim = mesh.ctx, int(bs), mesh.gdim
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.dxo_csr_create(self.ctx._h, mesh._h, self.bs, C.byref(h)), "dxo_csr_create")
        self._h = h
        self._fin = weakref.finalize(self, CsrPattern._destroy, self.ctx, h)
        n_rows, nnz, rp, col, ms = C.c_int64(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_double()
        self.ctx.check(self.ctx.lib.dxo_csr_info(self.ctx._h, h, C.byref(n_rows), C.byref(nnz), C.byref(rp), C.byref(col), C.byref(ms)),
                       "dxo_csr_info")
        self.n_rows, self.nnz, self.build_ms = n_rows.value, nnz.value, ms.value
        self._rp, self._col = rp.value, col.value
        self._indptr = self._indices = None

    @staticmethod
    def _destroy(ctx, h):
        ctx.lib.dxo_csr_destroy(ctx._h, h)      # a closed context passes NULL: the pattern's device arrays are still freed

    def _copy(self, ptr: int, n: int, typestr: str):
        import torch

        dev = torch.device("cuda", self.ctx.device)
        if n == 0:
            return torch.empty(0, dtype=torch.int64 if typestr == "<i8" else torch.int32, device=dev)
        return torch.as_tensor(_CudaArrayView(self, ptr, n, typestr), device=dev).clone()

    @property
    def indptr(self):
        if self._indptr is None:
            self._indptr = self._copy(self._rp, self.n_rows + 1, "<i8")
        return self._indptr

    @property
    def indices(self):
        if self._indices is None:
            self._indices = self._copy(self._col, self.nnz, "<i4")
        return self._indices

    def close(self) -> None:
        self._fin()


class FacetSet:
    """dxo_facet_set: a fixed list of (cell, local facet) entities of a DeviceMesh on the device, with its element-vector scratch and
    transposed incidence (built once). `n` entities; `entities` keeps the host array."""

    def __init__(self, mesh: DeviceMesh, entities: np.ndarray):
        self.ctx, self.mesh_handle = mesh.ctx, mesh._h
        self.entities = np.ascontiguousarray(entities, dtype=np.int32)
        self.n = self.entities.shape[0]
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.dxo_facet_set_create(self.ctx._h, mesh._h, self.entities.ctypes.data, self.n, C.byref(h)),
                       "dxo_facet_set_create")
        self._h = h
        self._fin = weakref.finalize(self, FacetSet._destroy, self.ctx, h)

    @staticmethod
    def _destroy(ctx, h):
        ctx.lib.dxo_facet_set_destroy(ctx._h, h)

    def close(self) -> None:
        self._fin()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceCSR:
    """An assembled matrix: `values` (float64 CUDA tensor, nnz) on `pattern`."""

    def __init__(self, pattern: CsrPattern, values):
        self.pattern, self.values = pattern, values
        self.shape = (pattern.n_rows, pattern.n_rows)

    def to_torch(self):
        """torch.sparse_csr_tensor on the device (both index arrays int64, as torch requires one index dtype)."""
        import torch

        return torch.sparse_csr_tensor(self.pattern.indptr, self.pattern.indices.to(torch.int64), self.values, size=self.shape)

    def to_numpy(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(indptr, indices, values) copied to the host."""
        return self.pattern.indptr.cpu().numpy(), self.pattern.indices.cpu().numpy(), self.values.cpu().numpy()

    def to_scipy(self):
        """scipy.sparse.csr_matrix, copied to the host."""
        import scipy.sparse

        indptr, indices, values = self.to_numpy()
        return scipy.sparse.csr_matrix((values, indices, indptr), shape=self.shape)

    def matvec(self, x, y=None, alpha: float = 1.0, beta: float = 0.0, transpose: bool = False):
        """y = alpha A x + beta y on the device (dxo_csr_spmv, BLAS semantics: with beta == 0, y is not read); returns y.
        transpose=True: y = alpha A^T x + beta y without forming A^T (dxo_csr_spmv_t), bit for bit the product of `transpose()`'s
        matrix. `gmres(lambda v, out: A.matvec(v, out, transpose=True), ...)` is the copy-free route to an adjoint solve; a one-off
        product pays scattered reads, so many products on one matrix are better served by `transpose()` once."""
        from .krylov import csr_matvec

        return csr_matvec(self, x, y, alpha, beta, transpose)

    def transpose(self, out=None) -> "DeviceCSR":
        """A^T on the same pattern (dxo_csr_transpose): the pattern is structurally symmetric, so only the values are permuted, exactly.
        out=None: a new values tensor; out=self.values: in place; any other float64 CUDA tensor of nnz entries that does not overlap
        the values: written to. The transposed matrix keeps the row pointers, columns and Dirichlet mask, so block Jacobi and the
        multigrid apply unchanged: an in-place transpose followed by `amg.setup()` reuses the hierarchy's symbolic phase for the
        adjoint solve (strength masks stay the frozen ones). dxo_csr_dirichlet commutes with transposition: rows and columns are
        both zeroed."""
        import torch

        pat = self.pattern
        if out is None:
            out = torch.empty_like(self.values)
        if not (out.dtype == torch.float64 and out.is_cuda and out.is_contiguous() and out.numel() == pat.nnz):
            raise ValueError(f"transpose: out must be a contiguous float64 CUDA tensor of {pat.nnz} entries")
        from .krylov import _use_current_stream

        _use_current_stream(pat.ctx)
        rc = pat.ctx.lib.dxo_csr_transpose(pat.ctx._h, pat._h, C.c_void_p(self.values.data_ptr()), C.c_void_p(out.data_ptr()))
        pat.ctx.check(rc, "dxo_csr_transpose")
        return self if out is self.values else DeviceCSR(pat, out)

    def block_jacobi(self) -> "BlockJacobi":
        """The inverses of the bs x bs diagonal blocks (dxo_csr_block_jacobi) as a preconditioner for krylov.gmres / krylov.cg.
        A singular block raises ValueError (DXO_E_SINGULAR)."""
        from .krylov import BlockJacobi

        return BlockJacobi.from_csr(self)

    def amg(self, constrained=None, max_levels: int = 10, coarse_rows: int = 512, sweeps: int = 1, near_nullspace=None,
            smoother: str = "jacobi", degree: int | None = None, rho: str = "inf-norm", rho_iters: int = 10, lower: float = 0.1,
            safety: float = 1.1, strength: float = 0.0, cycle: str = "V", precision: str = "fp64", first_transfer=None) -> "AMG":
        """A smoothed-aggregation multigrid preconditioner of this matrix (krylov.AMG: the symbolic phase and the first setup), for
        krylov.gmres / krylov.cg. `constrained`: the dofs given as bcs to bilinear_assemble. `near_nullspace`: a float64 CUDA tensor
        (n_rows, k), e.g. krylov.rigid_body_modes(x) for elasticity (k = 3 for bs 2, 6 for bs 3). `smoother` ("jacobi" or "chebyshev" of `degree`), `rho`
        ("inf-norm" or "power") and rho_iters, lower, safety: the relaxation, see krylov.AMG; the defaults 10 / 0.1 / 1.1 are the
        customary rule, not measurements. `strength`: the threshold of the strength of connection in [0, 1), 0 for none
        (anisotropic operators: 0.25); the masks are made from the present values and frozen. `cycle`: "V", or "K" for the K-cycle
        (for krylov.fgmres only). `precision`: "fp64", or "fp32" for a V-cycle on single-precision copies of the levels (the setup
        stays double; krylov.fgmres is its recommended partner). `first_transfer`: a NodalTransfer (DeviceMesh.vertex_transfer) for
        matrices of quadratic elements: level 1 is then the degree-1 space on the same cells and the aggregation starts there, see
        krylov.AMG. After the values changed: `.setup()`."""
        from .krylov import AMG

        return AMG(self, constrained, max_levels, coarse_rows, sweeps, near_nullspace, smoother, degree, rho, rho_iters, lower, safety, strength, cycle,
                   precision, first_transfer)


class DeviceOperand:
    """Plays the role of a UFL operand in `evaluation.evaluate_operands`: `.eval(entities)` returns what
    `Expression.eval` returns, (len(entities), nq, *shape); for "F" the trailing shape is (gdim, gdim) like the
    tensor operand of the hyperelasticity demo, for "grad" of a vector field (bs, gdim)."""

    def __init__(self, mesh: DeviceMesh, kind: str, field, bs: int, name: str, lazy: bool = False, snapshot: bool = True):
        self.mesh, self.kind, self.field, self.bs, self.name, self.lazy, self.snapshot = mesh, kind, field, bs, name, lazy, snapshot
        self.eval_count = 0

    def eval(self, entities):
        self.eval_count += 1
        if self.lazy and (entities is None or (len(entities) == self.mesh.num_cells
                                               and np.array_equal(entities, np.arange(self.mesh.num_cells)))):
            if self.snapshot:
                u = np.array(_state(self.field), dtype=np.float64).reshape(-1)  # snapshot, like Expression.eval's result
            else:
                u = np.ascontiguousarray(_state(self.field), dtype=np.float64).reshape(-1)   # the live array (no copy if fp64)
            return LazyOperand(self.mesh, self.kind, self.bs, u)
        if self.kind == "x":
            if entities is not None and np.ndim(entities) == 2:
                raise NotImplementedError("the operand `x` is evaluated on cells; codim-1 entities go through the host array")
            return self.mesh.coordinate(entities)                                         # (n, nq, gdim), like any vector operand
        if entities is not None and np.ndim(entities) == 2:
            out = self.mesh.evaluate_facets(self.kind, self.bs, self.field, entities)    # (cell, local facet) pairs
        else:
            out = self.mesh.evaluate(self.kind, self.bs, self.field, entities)
        g = self.mesh.gdim
        if self.kind in ("F", "C"):
            return out.reshape(out.shape[0], out.shape[1], g, g)
        if self.kind == "grad" and self.bs > 1:
            return out.reshape(out.shape[0], out.shape[1], self.bs, g)
        if out.shape[2] == 1:
            return out.reshape(out.shape[0], out.shape[1])       # scalar operand is 2-D (heat demo, part2.py:220-228)
        return out

    def __repr__(self) -> str:
        return f"DeviceOperand({self.name})"


class LazyOperand:
    """The value of an operand over all cells, not yet computed: (mesh, kind, snapshot of the field vector).

    `make_von_mises` recognises it and runs dxo_von_mises_field (operand + return map in one launch, the strain
    never reaches memory). Anything else sees an array: `np.asarray(lazy)`, `.shape`, `.reshape` evaluate it once
    with dxo_eval_operand."""

    def __init__(self, mesh: DeviceMesh, kind: str, bs: int, u: np.ndarray):
        self.mesh, self.kind, self.bs, self.u = mesh, kind, bs, u
        self._value = None

    @property
    def shape(self):
        return (self.mesh.num_cells, self.mesh.nq, self.mesh.value_size(self.kind, self.bs))

    @property
    def dtype(self):
        return np.dtype(np.float64)

    def __array__(self, dtype=None, copy=None):
        if self._value is None:
            self._value = self.mesh.evaluate(self.kind, self.bs, self.u)
        return self._value if dtype is None else self._value.astype(dtype)

    def reshape(self, *shape):
        return np.asarray(self).reshape(*shape)
