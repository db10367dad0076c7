"""Linear solves on the device (csrc/krylov.hip): CSR SpMV, block Jacobi, restarted GMRES, flexible GMRES and CG.

All vectors are contiguous float64 CUDA tensors on the context's device. The calls run on torch's current stream of that device,
which they make the context's stream (the convention of the examples and tests: ctx.set_stream(torch.cuda.current_stream())), so
torch work before and after them is ordered without a synchronisation. A solve synchronises only to read its residual estimate,
every `check_every` iterations.
"""
from __future__ import annotations

import ctypes as C
import weakref
from dataclasses import dataclass

from ._lib import KRYLOV_APPLY_FN, AmgLevelInfo, KrylovCallback, KrylovInfo, KrylovOp, KrylovPc, _CudaArrayView

PC_NONE, PC_JACOBI, PC_BLOCK_JACOBI, PC_AMG, PC_CALLBACK, PC_PMG = 0, 1, 2, 3, 4, 5
_SMOOTHERS = {"jacobi": 0, "chebyshev": 1}           # DXO_AMG_SMOOTH_*
_RHO_KINDS = {"inf-norm": 0, "power": 1}             # DXO_AMG_RHO_*
_CYCLES = {"V": 0, "K": 1}                           # DXO_AMG_CYCLE_*
_PRECISIONS = {"fp64": 0, "fp32": 1}                 # DXO_AMG_PRECISION_*
_BASES = {"fp64": 0, "fp32": 1}                      # DXO_KRYLOV_BASIS_*


def _torch():
    import torch

    return torch


def _check_vec(v, n: int, dev, what: str):
    torch = _torch()
    if not (isinstance(v, torch.Tensor) and v.dtype == torch.float64 and v.is_cuda and v.is_contiguous() and v.numel() == n
            and v.device == dev):
        raise ValueError(f"{what}: expected a contiguous float64 CUDA tensor of {n} entries on {dev}")


def _use_current_stream(ctx) -> None:
    torch = _torch()
    ctx.set_stream(torch.cuda.current_stream(torch.device("cuda", ctx.device)).cuda_stream)


@dataclass
class KrylovResult:
    """What gmres / fgmres / cg return: the solution, the iterations up to the converged step, the true relative residual |b - A x| / |b|,
    whether it met the tolerance, whether the iteration broke down, the cycles started, the wall ms of the solve, the storage of the
    Krylov basis ("fp64" or "fp32") and the bytes of its rows (V alone: the second basis of fgmres, always double, is not counted;
    0 for cg, which keeps none)."""
    x: object
    iterations: int
    residual: float
    converged: bool
    breakdown: bool = False
    restarts: int = 0
    ms: float = 0.0
    basis: str = "fp64"
    basis_bytes: int = 0


class BlockJacobi:
    """Inverses of the bs x bs diagonal blocks of an assembled matrix, inv [n/bs][bs][bs] (dxo_csr_block_jacobi). bs = 1 is point
    Jacobi. `apply(r, out)` sets out = M^-1 r."""

    def __init__(self, ctx, bs: int, inv):
        self.ctx, self.bs, self.inv = ctx, int(bs), inv
        self.n = inv.numel() // self.bs

    @classmethod
    def from_csr(cls, A) -> "BlockJacobi":
        torch = _torch()
        ctx, bs = A.pattern.ctx, A.pattern.bs
        inv = torch.empty(A.pattern.n_rows * bs, dtype=torch.float64, device=A.values.device)
        _use_current_stream(ctx)
        rc = ctx.lib.dxo_csr_block_jacobi(ctx._h, A.pattern._h, C.c_void_p(A.values.data_ptr()), C.c_void_p(inv.data_ptr()))
        ctx.check(rc, "dxo_csr_block_jacobi")
        return cls(ctx, bs, inv)

    def apply(self, r, out=None):
        torch = _torch()
        _check_vec(r, self.n, self.inv.device, "BlockJacobi.apply: r")
        if out is None:
            out = torch.empty_like(r)
        _check_vec(out, self.n, self.inv.device, "BlockJacobi.apply: out")
        _use_current_stream(self.ctx)
        rc = self.ctx.lib.dxo_block_jacobi_apply(self.ctx._h, self.bs, self.n, C.c_void_p(self.inv.data_ptr()), C.c_void_p(r.data_ptr()),
                                                 C.c_void_p(out.data_ptr()))
        self.ctx.check(rc, "dxo_block_jacobi_apply")
        return out

    def _pc(self) -> KrylovPc:
        return KrylovPc(PC_BLOCK_JACOBI, self.bs, self.n, C.c_void_p(self.inv.data_ptr()))


def rigid_body_modes(x, ctx=None):
    """The rigid-body modes of node coordinates x (n_nodes, gdim), a NumPy array or a tensor: a float64 CUDA tensor
    (n_nodes * gdim, k), k = 3 in 2-D and 6 in 3-D (dxo_rigid_body_modes): the translations, then (-y, x), or (-y, x, 0), (0, -z, y),
    (z, 0, -x). The near-null space of elasticity for DeviceCSR.amg(near_nullspace=...)."""
    torch = _torch()
    import numpy as np

    if ctx is None:
        from ._lib import default_context

        ctx = default_context()
    dev = torch.device("cuda", ctx.device)
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    if x.dim() != 2 or x.shape[1] not in (2, 3):
        raise ValueError("rigid_body_modes: x must have the shape (n_nodes, 2) or (n_nodes, 3)")
    x = x.to(device=dev, dtype=torch.float64).contiguous()
    n, g = int(x.shape[0]), int(x.shape[1])
    B = torch.empty((n * g, 3 if g == 2 else 6), dtype=torch.float64, device=dev)
    _use_current_stream(ctx)
    ctx.check(ctx.lib.dxo_rigid_body_modes(ctx._h, C.c_void_p(x.data_ptr()), n, g, C.c_void_p(B.data_ptr())), "dxo_rigid_body_modes")
    return B


class AMG:
    """Smoothed-aggregation multigrid preconditioner of an assembled matrix (dxo_amg_*, csrc/amg.hip), applied as one V-cycle, or as
    one K-cycle (`cycle`, below).

    The constructor runs the symbolic phase on the host (aggregates and the patterns of every level, once per pattern) and the first
    setup(). After the values of the matrix changed (a Newton iteration: the same DeviceCSR, or another on the same pattern) call
    setup() again; it runs on the device only. `constrained`: the dofs given to bilinear_assemble(bcs=...) (an int32 CUDA tensor,
    or anything numpy converts), None for none. Pass it as M to gmres / cg (cg: symmetric positive definite A).

    `near_nullspace`: a float64 CUDA tensor (n_rows, k), k = 3 for bs 2 and 6 for bs 3 (rigid_body_modes(x) for elasticity). The
    tentative prolongator then carries these vectors, orthonormalised per aggregate, and every coarse level has block size k
    (dxo_amg_create_nns); it is made once, here, and setup() leaves it alone.

    The relaxation (dxo_amg_set_smoother). `rho`: where the estimate of the spectral radius of Dinv A comes from, which sets
    omega = (4/3) / rho of the prolongator smoothing and of the Jacobi sweeps: "inf-norm" (|Dinv A|_inf, a bound, often 2x too large
    on elasticity) or "power" (`rho_iters` steps of the power iteration on the device, times `safety`; an estimate from below, not a
    bound). `smoother`: "jacobi" (`sweeps` damped block-Jacobi sweeps) or "chebyshev" (the polynomial of `degree` in Dinv A on
    [lower rho, rho] before and after the coarse correction; `degree` None: `sweeps`, at most 8). The defaults rho_iters 10,
    lower 0.1 and safety 1.1 are the customary rule (PETSc's), not measurements on this library. With the default smoother and rho
    the object is the one of earlier versions bit for bit.

    `strength`: the threshold theta of the strength of connection, in [0, 1) (dxo_amg_create_soc). 0 (the default): every stored
    block is a connection, the object of earlier versions. theta > 0: block (i, j) is strong when
    |A_ij|_F^2 >= theta^2 |A_ii|_F |A_jj|_F for (i, j) or (j, i); the aggregates are made on the strong graph and the prolongator is
    smoothed with the filtered matrix (weak blocks lumped onto the diagonal), which is what anisotropic operators and stretched
    cells need (0.25 is customary for scalar problems). The masks, and with them the aggregates and all patterns, are made from the
    values of the matrix at construction and are frozen there: setup() reuses them for new values, and set_smoother() changes the
    relaxation but not the coarsening (the construction itself coarsens with the default relaxation).

    `cycle`: "V" (the default) or "K" (dxo_amg_set_cycle; set_cycle() changes it later, at once and without a setup, on any of the
    hierarchies above). The K-cycle solves the coarse equation of every level between the finest and the coarsest by two GCR steps
    preconditioned by the cycle of that level, so level l is visited 2^l times (`visits`). It is not a fixed linear operator: pass it
    to fgmres; gmres and cg raise ValueError (DXO_E_OPTION). With at most two levels it is the V-cycle bit for bit. It is homogeneous
    in r (apply(2^e r) == 2^e apply(r)) as long as the squares of |r| are finite and normal, |r| roughly within 2^-500 .. 2^500.

    `precision`: "fp64" (the default, the object of earlier versions bit for bit) or "fp32" (dxo_amg_set_precision;
    set_precision() changes it later, for the next setup()). setup() stays double throughout and then casts the values, the block
    inverses and the prolongator of every level but the coarsest to float; apply() runs the same V-cycle on these copies with float
    vectors and arithmetic, the coarsest dense solve in double, r and the result double as before. The cycle is then a fixed linear
    operator up to single-precision rounding (about 1e-7 relative to the fp64 cycle): it may be passed to gmres, cg and fgmres, whose
    own arithmetic stays double; fgmres is the recommended partner. `fp32_bytes`: what the copies take. A finite entry beyond the
    range of float makes setup() raise ValueError; r is narrowed to float on entry, so an |r| beyond float's range is not representable
    (scale it). Not with cycle="K" (ValueError, in either order).

    `first_transfer`: a NodalTransfer (DeviceMesh.vertex_transfer(psi_nodes)) for matrices of quadratic elements
    (dxo_amg_create_transfer). The prolongator of level 0 is then this nodal interpolation, P = W (x) I_bs without the constrained
    dofs: level 1 is the degree-1 space on the same cells (A_1 = P^T A P, recomputed by every setup()) and the aggregation, the
    near-null space and `strength` start there, on a matrix whose nodes have 27 neighbours instead of up to 125. Level 0 keeps its
    relaxation; its P is stored as block diagonals (the property `first_transfer`), frozen at construction. Every other keyword composes
    with it. None (the default): the object of earlier versions."""

    def __init__(self, A, constrained=None, max_levels: int = 10, coarse_rows: int = 512, sweeps: int = 1, near_nullspace=None,
                 smoother: str = "jacobi", degree: int | None = None, rho: str = "inf-norm", rho_iters: int = 10, lower: float = 0.1,
                 safety: float = 1.1, strength: float = 0.0, cycle: str = "V", precision: str = "fp64", first_transfer=None):
        torch = _torch()
        import numpy as np

        if cycle not in _CYCLES:
            raise ValueError(f"AMG: cycle must be one of {sorted(_CYCLES)}")
        if precision not in _PRECISIONS:
            raise ValueError(f"AMG: precision must be one of {sorted(_PRECISIONS)}")
        strength = float(strength)
        if not 0.0 <= strength < 1.0:          # NaN fails both comparisons
            raise ValueError("AMG: strength must lie in [0, 1)")
        self.strength = strength

        self.ctx, self.A, self.bs, self.n = A.pattern.ctx, A, A.pattern.bs, A.pattern.n_rows
        self.device = A.values.device
        if int(max_levels) < 1 or int(coarse_rows) < 1 or int(sweeps) < 1:
            raise ValueError("AMG: max_levels, coarse_rows and sweeps must be at least 1")
        self.sweeps = int(sweeps)
        relax = self._relaxation(smoother, degree, rho, rho_iters, lower, safety)
        if constrained is None:
            bc = torch.empty(0, dtype=torch.int32, device=self.device)
        elif isinstance(constrained, torch.Tensor):
            bc = constrained.to(device=self.device, dtype=torch.int32).contiguous()
        else:
            bc = torch.from_numpy(np.ascontiguousarray(constrained, dtype=np.int32)).to(self.device)
        h = C.c_void_p()
        _use_current_stream(self.ctx)
        bcp = C.c_void_p(bc.data_ptr()) if bc.numel() else None
        self.n_modes = 0
        if first_transfer is not None:
            from ._lib import AmgTransfer

            t, k, B = first_transfer, 0, None
            if t.ptr.size != self.n // self.bs + 1:
                raise ValueError(f"AMG: first_transfer has {t.ptr.size - 1} rows, the matrix {self.n // self.bs} nodes")
            if near_nullspace is not None:
                B, k = self._near_nullspace(near_nullspace)
            desc = AmgTransfer(t.n_coarse, t.ptr.ctypes.data, t.col.ctypes.data, t.w.ctypes.data, t.coarse_to_fine.ctypes.data)
            rc = self.ctx.lib.dxo_amg_create_transfer(self.ctx._h, A.pattern._h, C.c_void_p(A.values.data_ptr()), bcp, int(bc.numel()),
                                                      C.c_void_p(B.data_ptr()) if k else None, k, strength, C.byref(desc), int(max_levels),
                                                      int(coarse_rows), int(sweeps), C.byref(h))
            self.ctx.check(rc, "dxo_amg_create_transfer")
            self.n_modes = k
        elif near_nullspace is None and strength > 0.0:
            rc = self.ctx.lib.dxo_amg_create_soc(self.ctx._h, A.pattern._h, C.c_void_p(A.values.data_ptr()), bcp, int(bc.numel()), None, 0, strength,
                                                 int(max_levels), int(coarse_rows), int(sweeps), C.byref(h))
            self.ctx.check(rc, "dxo_amg_create_soc")
        elif near_nullspace is None:
            rc = self.ctx.lib.dxo_amg_create(self.ctx._h, A.pattern._h, bcp, int(bc.numel()), int(max_levels), int(coarse_rows), int(sweeps),
                                             C.byref(h))
            self.ctx.check(rc, "dxo_amg_create")
        else:
            B, k = self._near_nullspace(near_nullspace)
            if strength > 0.0:
                rc = self.ctx.lib.dxo_amg_create_soc(self.ctx._h, A.pattern._h, C.c_void_p(A.values.data_ptr()), bcp, int(bc.numel()),
                                                     C.c_void_p(B.data_ptr()), k, strength, int(max_levels), int(coarse_rows), int(sweeps),
                                                     C.byref(h))
                self.ctx.check(rc, "dxo_amg_create_soc")
            else:
                rc = self.ctx.lib.dxo_amg_create_nns(self.ctx._h, A.pattern._h, bcp, int(bc.numel()), C.c_void_p(B.data_ptr()), k,
                                                     int(max_levels), int(coarse_rows), int(sweeps), C.byref(h))
                self.ctx.check(rc, "dxo_amg_create_nns")
            self.n_modes = k
        self._h = h
        self._fin = weakref.finalize(self, self.ctx.lib.dxo_amg_destroy, None, h)
        self._fin.atexit = False
        nl, ms, oc = C.c_int(), C.c_double(), C.c_double()
        self.ctx.check(self.ctx.lib.dxo_amg_info(self.ctx._h, h, C.byref(nl), C.byref(ms), C.byref(oc), 0, None), "dxo_amg_info")
        self.n_levels, self.build_ms, self.operator_complexity = nl.value, ms.value, oc.value
        self._lower, self._safety = 0.1, 1.1
        if relax[0] or relax[2]:         # the defaults call nothing that earlier versions did not call
            self._set_smoother(*relax)
        if cycle != "V":
            self.set_cycle(cycle)
        if precision != "fp64":
            self.set_precision(precision)
        self.setup()

    def _near_nullspace(self, B) -> tuple:
        """(B contiguous, k) of a valid near-null space of this matrix."""
        torch = _torch()
        k = {2: 3, 3: 6}.get(self.bs)
        if not (isinstance(B, torch.Tensor) and B.dtype == torch.float64 and B.is_cuda and B.device == self.device and B.dim() == 2
                and k is not None and tuple(B.shape) == (self.n, k)):
            raise ValueError(f"AMG: near_nullspace must be a float64 CUDA tensor of shape ({self.n}, {k}) on {self.device} "
                             f"(bs 2: 3 vectors, bs 3: 6 vectors; this matrix has bs {self.bs})")
        return B.contiguous(), k

    def _relaxation(self, smoother, degree, rho, rho_iters, lower, safety) -> tuple:
        if smoother not in _SMOOTHERS or rho not in _RHO_KINDS:
            raise ValueError(f"AMG: smoother must be one of {sorted(_SMOOTHERS)} and rho one of {sorted(_RHO_KINDS)}")
        degree = self.sweeps if degree is None else int(degree)
        if smoother == "chebyshev" and not 1 <= degree <= 8:
            raise ValueError("AMG: the Chebyshev degree (sweeps if degree is None) must lie in 1..8")
        if int(rho_iters) < 1 or not 0.0 < float(lower) < 1.0 or not float(safety) >= 1.0:
            raise ValueError("AMG: rho_iters must be at least 1, lower inside (0, 1) and safety at least 1")
        return _SMOOTHERS[smoother], degree, _RHO_KINDS[rho], int(rho_iters), float(lower), float(safety)

    def _set_smoother(self, kind, degree, rho_kind, rho_iters, lower, safety) -> None:
        rc = self.ctx.lib.dxo_amg_set_smoother(self.ctx._h, self._h, kind, degree, rho_kind, rho_iters, lower, safety)
        self.ctx.check(rc, "dxo_amg_set_smoother")
        self._lower, self._safety = lower, safety

    def set_smoother(self, smoother: str = "jacobi", degree: int | None = None, rho: str = "inf-norm", rho_iters: int = 10,
                     lower: float = 0.1, safety: float = 1.1) -> "AMG":
        """Another relaxation for this hierarchy (the keywords of the constructor); allocates nothing. apply() and the solvers raise
        ValueError (DXO_E_OPTION) until the next setup()."""
        self._set_smoother(*self._relaxation(smoother, degree, rho, rho_iters, lower, safety))
        return self

    def set_cycle(self, cycle: str = "V") -> "AMG":
        """"V" or "K" (dxo_amg_set_cycle): takes effect at the next apply, no setup() needed. The first "K" allocates the vectors of
        the two GCR steps on the intermediate levels."""
        if cycle not in _CYCLES:
            raise ValueError(f"AMG: cycle must be one of {sorted(_CYCLES)}")
        self.ctx.check(self.ctx.lib.dxo_amg_set_cycle(self.ctx._h, self._h, _CYCLES[cycle]), "dxo_amg_set_cycle")
        return self

    def set_precision(self, precision: str = "fp64") -> "AMG":
        """"fp64" or "fp32" (dxo_amg_set_precision) for the next setup(): apply() and the solvers raise ValueError (DXO_E_OPTION) until
        then, unless the object already has this precision. The first "fp32" allocates the single-precision copies and vectors
        (`fp32_bytes`); they stay with the object. "fp32" on a K-cycle raises ValueError."""
        if precision not in _PRECISIONS:
            raise ValueError(f"AMG: precision must be one of {sorted(_PRECISIONS)}")
        self.ctx.check(self.ctx.lib.dxo_amg_set_precision(self.ctx._h, self._h, _PRECISIONS[precision]), "dxo_amg_set_precision")
        return self

    def _transfer_info(self) -> tuple:
        on, nc, pb, pd, ctf = C.c_int(), C.c_int64(), C.c_int64(), C.c_void_p(), C.c_void_p()
        self.ctx.check(self.ctx.lib.dxo_amg_transfer_info(self.ctx._h, self._h, C.byref(on), C.byref(nc), C.byref(pb), C.byref(pd), C.byref(ctf)),
                       "dxo_amg_transfer_info")
        return bool(on.value), int(nc.value), int(pb.value), pd.value, ctf.value

    @property
    def first_transfer(self):
        """None, or what level 0 keeps of the given transfer: {"n_coarse", "p_blocks", "p_diag"}, p_diag a float64 CUDA tensor view
        (p_blocks, bs) of the block diagonals of P (the weights without the constrained dofs; alive as long as this object)."""
        on, nc, pb, pd, _ = self._transfer_info()
        if not on:
            return None
        torch = _torch()
        view = torch.as_tensor(_CudaArrayView(self, pd, pb * self.bs, "<f8"), device=self.device).view(pb, self.bs) if pb else \
            torch.empty((0, self.bs), dtype=torch.float64, device=self.device)
        return {"n_coarse": nc, "p_blocks": pb, "p_diag": view}

    def _precision_info(self) -> tuple:
        kind, nbytes = C.c_int(), C.c_int64()
        self.ctx.check(self.ctx.lib.dxo_amg_precision_info(self.ctx._h, self._h, C.byref(kind), C.byref(nbytes)), "dxo_amg_precision_info")
        return {v: k for k, v in _PRECISIONS.items()}[kind.value], int(nbytes.value)

    @property
    def precision(self) -> str:
        """"fp64" or "fp32"."""
        return self._precision_info()[0]

    @property
    def fp32_bytes(self) -> int:
        """Bytes of the single-precision copies and vectors; 0 if "fp32" was never selected (or the hierarchy has one level)."""
        return self._precision_info()[1]

    def _cycle_info(self) -> tuple:
        kind, visits = C.c_int(), C.c_int64()
        self.ctx.check(self.ctx.lib.dxo_amg_cycle_info(self.ctx._h, self._h, C.byref(kind), C.byref(visits)), "dxo_amg_cycle_info")
        return {v: k for k, v in _CYCLES.items()}[kind.value], int(visits.value)

    @property
    def cycle(self) -> str:
        """"V" or "K"."""
        return self._cycle_info()[0]

    @property
    def visits(self) -> int:
        """Level visits of one apply: the levels for "V"; for "K" 2^l per level l but the coarsest, which is visited as often as
        the level above it."""
        return self._cycle_info()[1]

    def close(self) -> None:
        self._fin()

    def setup(self, A=None) -> "AMG":
        """The numeric phase for the current values of the matrix (dxo_amg_setup); `A`: another DeviceCSR on the same pattern.
        Synchronises once. A singular diagonal block or coarsest matrix raises ValueError (DXO_E_SINGULAR)."""
        if A is not None:
            if A.pattern is not self.A.pattern:
                raise ValueError("AMG.setup: the matrix lies on another pattern than the one this object was made for")
            self.A = A
        _use_current_stream(self.ctx)
        rc = self.ctx.lib.dxo_amg_setup(self.ctx._h, self._h, C.c_void_p(self.A.values.data_ptr()))
        self.ctx.check(rc, "dxo_amg_setup")
        return self

    def apply(self, r, out=None):
        """out = M(r), one cycle (dxo_amg_apply; V, or K after set_cycle("K")); returns out."""
        torch = _torch()
        _check_vec(r, self.n, self.device, "AMG.apply: r")
        if out is None:
            out = torch.empty_like(r)
        _check_vec(out, self.n, self.device, "AMG.apply: out")
        _use_current_stream(self.ctx)
        rc = self.ctx.lib.dxo_amg_apply(self.ctx._h, self._h, C.c_void_p(r.data_ptr()), C.c_void_p(out.data_ptr()))
        self.ctx.check(rc, "dxo_amg_apply")
        return out

    def _pc(self) -> KrylovPc:
        return KrylovPc(PC_AMG, self.bs, self.n, C.c_void_p(self._h.value))

    # ---- inspection (copies; for tests and reports)
    def _info(self, level: int) -> AmgLevelInfo:
        info = AmgLevelInfo()
        self.ctx.check(self.ctx.lib.dxo_amg_info(self.ctx._h, self._h, None, None, None, int(level), C.byref(info)), "dxo_amg_info")
        return info

    def _array(self, ptr, n: int, typestr: str):
        import numpy as np

        torch = _torch()
        if not n:
            return np.empty(0, dtype=np.dtype(typestr))
        torch.cuda.current_stream(self.device).synchronize()
        return torch.as_tensor(_CudaArrayView(self, ptr, int(n), typestr), device=self.device).cpu().numpy().copy()

    def _nns(self, level: int):
        """(bs, bs_coarse, dead columns, T pointer, B pointer) of a level (dxo_amg_nns_info)."""
        bs, bsc, dead, t, b = C.c_int(), C.c_int(), C.c_int64(), C.c_void_p(), C.c_void_p()
        self.ctx.check(self.ctx.lib.dxo_amg_nns_info(self.ctx._h, self._h, int(level), C.byref(bs), C.byref(bsc), C.byref(dead), C.byref(t),
                                                     C.byref(b)), "dxo_amg_nns_info")
        return bs.value, bsc.value, dead.value, t.value, b.value

    def _soc(self, level: int, count: bool = False):
        """(theta, mask pointer, strong blocks, unlumped nodes or None, dinv_f pointer, omega_F pointer) of a level
        (dxo_amg_soc_info)."""
        th, st, ns, nu, df, of = C.c_double(), C.c_void_p(), C.c_int64(), C.c_int64(), C.c_void_p(), C.c_void_p()
        self.ctx.check(self.ctx.lib.dxo_amg_soc_info(self.ctx._h, self._h, int(level), C.byref(th), C.byref(st), C.byref(ns),
                                                     C.byref(nu) if count else None, C.byref(df), C.byref(of)), "dxo_amg_soc_info")
        return th.value, st.value, ns.value, (nu.value if count else None), df.value, of.value

    @property
    def levels(self) -> list:
        """Per level: rows, block nonzeros, the block size, omega (None on the coarsest level) and omega_f, the omega of the filtered
        prolongator smoothing (None without strength of connection and on the coarsest level). Reading them synchronises the
        stream."""
        out = []
        for l in range(self.n_levels):
            i = self._info(l)
            om = float(self._array(i.omega, 1, "<f8")[0]) if i.omega else None
            of = self._soc(l)[5]
            out.append({"rows": int(i.n_rows), "nodes": int(i.n_nodes), "block_nnz": int(i.nnz_blocks), "omega": om, "bs": self._nns(l)[0],
                        "omega_f": float(self._array(of, 1, "<f8")[0]) if of else None})
        return out

    def strong_mask(self, level: int):
        """A NumPy bool per block of `level`, in the CSR order of its block pattern: the strong blocks, frozen at construction (all
        True without strength of connection and on the coarsest level)."""
        import numpy as np

        i = self._info(level)
        st = self._soc(level)[1]
        if not st:
            return np.ones(int(i.nnz_blocks), dtype=bool)
        return self._array(st, i.nnz_blocks, "|u1").astype(bool)

    @property
    def unlumped_nodes(self) -> list:
        """Per level but the coarsest: the nodes whose lumped diagonal block failed the singularity test at the last setup, so
        that the filtered smoothing used the inverse of A_ii for them (0 without strength of connection)."""
        return [self._soc(l, count=True)[3] for l in range(self.n_levels - 1)]

    def level_dinv_f(self, level: int):
        """The inverses of the lumped diagonal blocks of `level`, (nodes, bs, bs): those of A_ii where the lumped block failed the
        test, zero for a node without a strong neighbour. Empty without strength of connection and on the coarsest level."""
        i = self._info(level)
        bs = self._nns(level)[0]
        df = self._soc(level)[4]
        return self._array(df, i.n_nodes * bs * bs if df else 0, "<f8").reshape(-1, bs, bs)

    def _smoother_info(self, level: int):
        """(kind, degree, rho kind, rho_iters, rho pointer) of a level (dxo_amg_smoother_info)."""
        kind, degree, rk, it, rho = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_void_p()
        self.ctx.check(self.ctx.lib.dxo_amg_smoother_info(self.ctx._h, self._h, int(level), C.byref(kind), C.byref(degree), C.byref(rk),
                                                          C.byref(it), C.byref(rho)), "dxo_amg_smoother_info")
        return kind.value, degree.value, rk.value, it.value, rho.value

    @property
    def smoother(self) -> dict:
        """The relaxation: smoother, degree (the sweeps of Jacobi), rho, rho_iters, lower and safety."""
        kind, degree, rk, it, _ = self._smoother_info(0)
        return {"smoother": {v: k for k, v in _SMOOTHERS.items()}[kind], "degree": degree, "rho": {v: k for k, v in _RHO_KINDS.items()}[rk],
                "rho_iters": it, "lower": self._lower, "safety": self._safety}

    @property
    def rho(self) -> list:
        """Per level the estimate of the spectral radius of Dinv A that omega was made from at the last setup (None on the coarsest
        level). Reading it synchronises the stream."""
        ptrs = [self._smoother_info(l)[4] for l in range(self.n_levels)]
        return [float(self._array(p, 1, "<f8")[0]) if p else None for p in ptrs]

    @property
    def dead_columns(self) -> list:
        """Per level but the coarsest: the columns of the tentative prolongator that an aggregate could not carry (0 without a
        near-null space)."""
        return [self._nns(l)[2] for l in range(self.n_levels - 1)]

    def aggregates(self, level: int):
        """The aggregate of every node of `level` (-1: none), int32."""
        i = self._info(level)
        return self._array(i.aggregate, i.n_nodes if i.aggregate else 0, "<i4")

    def level_matrix(self, level: int):
        """A_level as a scipy.sparse.csr_matrix on the level's pattern (explicit zeros kept)."""
        import scipy.sparse

        i = self._info(level)
        n_rows, nnz, rp, col = C.c_int64(), C.c_int64(), C.c_void_p(), C.c_void_p()
        self.ctx.check(self.ctx.lib.dxo_csr_info(self.ctx._h, i.csr, C.byref(n_rows), C.byref(nnz), C.byref(rp), C.byref(col), None), "dxo_csr_info")
        indptr = self._array(rp.value, n_rows.value + 1, "<i8")
        return scipy.sparse.csr_matrix((self._array(i.values, nnz.value, "<f8"), self._array(col.value, nnz.value, "<i4"), indptr),
                                       shape=(n_rows.value, n_rows.value))

    def level_dinv(self, level: int):
        """The block-Jacobi inverses of `level`, (nodes, bs, bs) with the level's block size."""
        i = self._info(level)
        bs = self._nns(level)[0]
        return self._array(i.dinv, i.n_nodes * bs * bs if i.dinv else 0, "<f8").reshape(-1, bs, bs)

    def prolongator(self, level: int):
        """P_level (rows of `level`, rows of `level + 1`) as a scipy.sparse.bsr_matrix with bs x bs_coarse blocks (explicit zeros
        kept)."""
        import numpy as np
        import scipy.sparse

        i = self._info(level)
        if not i.p_ptr:
            raise ValueError(f"AMG.prolongator: level {level} is the coarsest")
        bs, bsc = self._nns(level)[:2]
        if not i.p_values:               # a given transfer: the diagonals of the blocks
            pd = self._array(self._transfer_info()[3], i.p_blocks * bs, "<f8").reshape(-1, bs)
            data = pd[:, :, None] * np.eye(bs)[None]
        else:
            data = self._array(i.p_values, i.p_blocks * bs * bsc, "<f8").reshape(-1, bs, bsc)
        return scipy.sparse.bsr_matrix((data, self._array(i.p_col, i.p_blocks, "<i4"), self._array(i.p_ptr, i.n_nodes + 1, "<i8")),
                                       shape=(i.n_rows, i.n_aggregates * bsc))

    def ap_pattern(self, level: int):
        """(indptr, indices) of the block pattern of A_level P_level."""
        i = self._info(level)
        return self._array(i.ap_ptr, i.n_nodes + 1 if i.ap_ptr else 0, "<i8"), self._array(i.ap_col, i.ap_blocks, "<i4")

    def tentative(self, level: int):
        """T_level of a hierarchy with a near-null space as a scipy.sparse.csr_matrix (rows of `level`, rows of `level + 1`): the
        bs x k block of every node in the block column of its aggregate (explicit zeros kept)."""
        import numpy as np
        import scipy.sparse

        i = self._info(level)
        bs, bsc, _, t, _ = self._nns(level)
        if not t:
            raise ValueError(f"AMG.tentative: level {level} is the coarsest, or the hierarchy has no near-null space")
        agg = self.aggregates(level)
        on = np.flatnonzero(agg >= 0)
        data = self._array(t, i.n_nodes * bs * bsc, "<f8").reshape(-1, bs, bsc)
        ptr = np.concatenate([[0], np.cumsum(agg >= 0)])
        return scipy.sparse.bsr_matrix((data[on], agg[on], ptr), shape=(i.n_rows, i.n_aggregates * bsc)).tocsr()

    def near_nullspace(self, level: int):
        """B_level (rows of `level`, k) of a hierarchy with a near-null space (level 0: the given one, rows of constrained dofs zero)."""
        i = self._info(level)
        b = self._nns(level)[4]
        if not b:
            raise ValueError("AMG.near_nullspace: the hierarchy has no near-null space")
        return self._array(b, i.n_rows * self.n_modes, "<f8").reshape(-1, self.n_modes)


class PMG:
    """Two-level p-multigrid preconditioner whose fine level is an operator, not a matrix (dxo_pmg_*, csrc/pmg.hip): for the
    matrix-free and array-free solves of quadratic elements, where DeviceCSR.amg(first_transfer=...) would need the assembled matrix.

    One apply: the Chebyshev polynomial of `degree` in Dinv A on [lower rho, rho] from zero, the residual restricted to the degree-1
    space on the same cells by `transfer` (a NodalTransfer: DeviceMesh.vertex_transfer), a preconditioner of the degree-1 matrix,
    prolongation, the same polynomial again: 2 degree operator calls (`matvecs_per_apply`). A fixed linear operator, symmetric for a
    symmetric A and coarse preconditioner: pass it as M to gmres, cg or fgmres.

    The constructor runs the symbolic part (dxo_pmg_create). `bs`: dofs per node (1, 2, 3); `constrained`: the dofs given to
    bilinear_assemble(bcs=...) (an int32 CUDA tensor, or anything numpy converts), None for none. `coarse_constrained` is then the
    Dirichlet set of the coarse matrix: assemble the degree-1 matrix on DeviceMesh.vertex_mesh(...) with bcs=pmg.coarse_constrained.
    `degree`, `rho_iters`, `lower`, `safety`: the smoother, as in AMG (dxo_pmg_set_smoother; set_smoother() changes it for the next
    setup())."""

    def __init__(self, transfer, bs: int, constrained=None, ctx=None, degree: int = 2, rho_iters: int = 10, lower: float = 0.1,
                 safety: float = 1.1):
        torch = _torch()
        import numpy as np

        from ._lib import AmgTransfer

        if ctx is None:
            from ._lib import default_context

            ctx = default_context()
        self.ctx, self.bs = ctx, int(bs)
        self.device = torch.device("cuda", ctx.device)
        self.n_nodes = int(transfer.ptr.size) - 1
        self.n = self.n_nodes * self.bs
        if constrained is None:
            bc = torch.empty(0, dtype=torch.int32, device=self.device)
        elif isinstance(constrained, torch.Tensor):
            bc = constrained.to(device=self.device, dtype=torch.int32).contiguous()
        else:
            bc = torch.from_numpy(np.ascontiguousarray(constrained, dtype=np.int32)).to(self.device)
        t = transfer
        desc = AmgTransfer(t.n_coarse, t.ptr.ctypes.data, t.col.ctypes.data, t.w.ctypes.data, t.coarse_to_fine.ctypes.data)
        h = C.c_void_p()
        _use_current_stream(ctx)
        rc = ctx.lib.dxo_pmg_create(ctx._h, self.n_nodes, self.bs, C.byref(desc), C.c_void_p(bc.data_ptr()) if bc.numel() else None,
                                    int(bc.numel()), C.byref(h))
        ctx.check(rc, "dxo_pmg_create")
        self._h = h
        self._fin = weakref.finalize(self, ctx.lib.dxo_pmg_destroy, None, h)
        self._fin.atexit = False
        self.transfer = transfer
        self._A = self._dinv = self._coarse = None
        self._keep: tuple = ()
        self._failure: list = []
        if (int(degree), int(rho_iters), float(lower), float(safety)) != (2, 10, 0.1, 1.1):
            self.set_smoother(degree, rho_iters, lower, safety)

    def set_smoother(self, degree: int = 2, rho_iters: int = 10, lower: float = 0.1, safety: float = 1.1) -> "PMG":
        """The Chebyshev degree (1..8), the steps of the power iteration, and the interval [lower rho, rho] with rho = safety times the
        estimate (dxo_pmg_set_smoother). Takes effect at the next setup(); apply() and the solvers raise ValueError (DXO_E_OPTION)
        until then."""
        rc = self.ctx.lib.dxo_pmg_set_smoother(self.ctx._h, self._h, int(degree), int(rho_iters), float(lower), float(safety))
        self.ctx.check(rc, "dxo_pmg_set_smoother")
        return self

    def _callback(self, f, n: int):
        """A C callback (v, out) -> f(tensor view of v, tensor view of out) on vectors of n entries; an exception is kept for
        _raise()."""
        torch = _torch()
        views: dict = {}
        ctx, dev, failure = self.ctx, self.device, self._failure

        def view(ptr: int):
            t = views.get(ptr)
            if t is None:
                t = views[ptr] = torch.as_tensor(_CudaArrayView(ctx, ptr, n, "<f8"), device=dev)
            return t

        def cb(_user, v, out):
            try:
                f(view(v), view(out))
                return 0
            except BaseException as e:      # noqa: BLE001 — re-raised when the call into the library has returned
                failure.append(e)
                return 1

        return KRYLOV_APPLY_FN(cb)

    def _raise(self) -> None:
        if self._failure:
            e = self._failure[0]
            self._failure.clear()
            raise e

    def setup(self, A, dinv, coarse) -> "PMG":
        """The numeric part (dxo_pmg_setup): rho of Dinv A by `rho_iters` operator calls and the Chebyshev pairs, both left on the
        device (no synchronisation). `A`: a DeviceCSR, or a callable (v, out) that sets out = A v, the identity on constrained dofs.
        `dinv`: a float64 CUDA tensor, the inverse diagonal with 1 on constrained dofs. `coarse`: an AMG (V-cycle), a BlockJacobi, or
        a callable (r, out) on the n_coarse vectors. The object keeps references to all three; call setup() again when the operator
        changed (a Newton iteration)."""
        from .operand_eval import DeviceCSR

        _check_vec(dinv, self.n, self.device, "PMG.setup: dinv")
        keep = []
        if isinstance(A, DeviceCSR):
            op = KrylovOp(A.pattern.n_rows, A.pattern._h, C.c_void_p(A.values.data_ptr()), KRYLOV_APPLY_FN(), None)
        elif callable(A):
            cb = self._callback(A, self.n)
            keep.append(cb)
            op = KrylovOp(self.n, None, None, cb, None)
        else:
            raise TypeError("PMG.setup: A must be a DeviceCSR or a callable (v, out) that sets out = A v")
        if isinstance(coarse, (AMG, BlockJacobi)):
            pc = coarse._pc()
        elif callable(coarse):
            ccb = self._callback(coarse, self.n_coarse)
            cstruct = KrylovCallback(ccb, None)
            keep += [ccb, cstruct]
            pc = KrylovPc(PC_CALLBACK, 1, self.n_coarse, C.cast(C.pointer(cstruct), C.c_void_p))
        else:
            raise TypeError("PMG.setup: coarse must be an AMG, a BlockJacobi or a callable (r, out)")
        _use_current_stream(self.ctx)
        rc = self.ctx.lib.dxo_pmg_setup(self.ctx._h, self._h, C.byref(op), C.c_void_p(dinv.data_ptr()), C.byref(pc))
        self._raise()
        self.ctx.check(rc, "dxo_pmg_setup")
        self._A, self._dinv, self._coarse, self._keep = A, dinv, coarse, tuple(keep)
        return self

    def _call(self, name: str, fn, a, na: int, out, nout: int):
        torch = _torch()
        _check_vec(a, na, self.device, f"PMG.{name}: input")
        if out is None:
            out = torch.empty(nout, dtype=torch.float64, device=self.device)
        _check_vec(out, nout, self.device, f"PMG.{name}: out")
        _use_current_stream(self.ctx)
        rc = fn(self.ctx._h, self._h, C.c_void_p(a.data_ptr()), C.c_void_p(out.data_ptr()))
        self._raise()
        self.ctx.check(rc, "dxo_pmg_" + name)
        return out

    def apply(self, r, out=None):
        """out = M r, one cycle (dxo_pmg_apply); out may be r. Returns out."""
        return self._call("apply", self.ctx.lib.dxo_pmg_apply, r, self.n, out, self.n)

    def restrict(self, r, out=None):
        """out = P^T r on the n_coarse vector (dxo_pmg_restrict): sums over the fine nodes in ascending order."""
        return self._call("restrict", self.ctx.lib.dxo_pmg_restrict, r, self.n, out, self.n_coarse)

    def prolong(self, e, out=None):
        """out = P e on the fine vector (dxo_pmg_prolong): sums over the coarse nodes in ascending order."""
        return self._call("prolong", self.ctx.lib.dxo_pmg_prolong, e, self.n_coarse, out, self.n)

    def _info(self) -> dict:
        nc, pb, pd, cb, ncb, rho, pairs, deg, mv = (C.c_int64(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p(),
                                                    C.c_int(), C.c_int64())
        rc = self.ctx.lib.dxo_pmg_info(self.ctx._h, self._h, C.byref(nc), C.byref(pb), C.byref(pd), C.byref(cb), C.byref(ncb), C.byref(rho),
                                       C.byref(pairs), C.byref(deg), C.byref(mv))
        self.ctx.check(rc, "dxo_pmg_info")
        return {"n_coarse": int(nc.value), "p_blocks": int(pb.value), "p_diag": pd.value, "c_bc": cb.value, "n_c_bc": int(ncb.value),
                "rho": rho.value, "pairs": pairs.value, "degree": int(deg.value), "matvecs": int(mv.value)}

    def _tensor(self, ptr, n: int, typestr: str, dtype):
        torch = _torch()
        if not n:
            return torch.empty(0, dtype=dtype, device=self.device)
        return torch.as_tensor(_CudaArrayView(self, ptr, int(n), typestr), device=self.device)

    @property
    def n_coarse(self) -> int:
        """Rows of the coarse space: coarse nodes times bs (dxo_pmg_info)."""
        return self._info()["n_coarse"]

    @property
    def degree(self) -> int:
        return self._info()["degree"]

    @property
    def matvecs_per_apply(self) -> int:
        """Operator calls of one apply: 2 degree."""
        return self._info()["matvecs"]

    @property
    def coarse_constrained(self):
        """The constrained dofs of the coarse space, an int32 CUDA tensor (a view, alive as long as this object): dof (v, c) iff the
        fine dof (coarse_to_fine[v], c) is constrained. The `bcs` of the coarse assembly."""
        torch = _torch()
        i = self._info()
        return self._tensor(i["c_bc"], i["n_c_bc"], "<i4", torch.int32)

    @property
    def p_diag(self):
        """(p_blocks, bs): the diagonals of the blocks of P, a float64 CUDA tensor view."""
        torch = _torch()
        i = self._info()
        return self._tensor(i["p_diag"], i["p_blocks"] * self.bs, "<f8", torch.float64).view(-1, self.bs)

    @property
    def pairs(self):
        """(degree, 2): the pairs (c1, c2) of the Chebyshev steps of the last setup, a float64 CUDA tensor view (no synchronisation)."""
        torch = _torch()
        i = self._info()
        return self._tensor(i["pairs"], 2 * i["degree"], "<f8", torch.float64).view(-1, 2)

    @property
    def rho(self) -> float:
        """The estimate of the spectral radius of Dinv A of the last setup, times `safety`. Reading it synchronises."""
        torch = _torch()
        return float(self._tensor(self._info()["rho"], 1, "<f8", torch.float64).cpu()[0])

    def _pc(self) -> KrylovPc:
        return KrylovPc(PC_PMG, self.bs, self.n, C.c_void_p(self._h.value))

    def close(self) -> None:
        """Frees the device memory (dxo_pmg_destroy)."""
        self._fin()


def csr_matvec(A, x, y=None, alpha: float = 1.0, beta: float = 0.0, transpose: bool = False):
    """y = alpha A x + beta y on the device (dxo_csr_spmv); with beta == 0, y is not read. Returns y. transpose=True:
    y = alpha A^T x + beta y (dxo_csr_spmv_t), bit for bit the product with DeviceCSR.transpose()'s matrix."""
    torch = _torch()
    ctx, n = A.pattern.ctx, A.pattern.n_rows
    _check_vec(x, n, A.values.device, "matvec: x")
    if y is None:
        if beta != 0.0:
            raise ValueError("matvec: beta != 0 needs y")
        y = torch.empty_like(x)
    _check_vec(y, n, A.values.device, "matvec: y")
    _use_current_stream(ctx)
    spmv, name = (ctx.lib.dxo_csr_spmv_t, "dxo_csr_spmv_t") if transpose else (ctx.lib.dxo_csr_spmv, "dxo_csr_spmv")
    rc = spmv(ctx._h, A.pattern._h, C.c_void_p(A.values.data_ptr()), float(alpha), C.c_void_p(x.data_ptr()), float(beta),
              C.c_void_p(y.data_ptr()))
    ctx.check(rc, name)
    return y


class _Workspace:
    """dxo_krylov of one (n, restart) and kind of basis. The context keeps a few of them (Context._krylov_ws) for later solves of the same
    size; Context.close() frees them. The finalizer holds the library and the raw context handle, not the Context."""

    def __init__(self, ctx, n: int, restart: int, basis: str = "fp64"):
        h = C.c_void_p()
        ctx.check(ctx.lib.dxo_krylov_create_basis(ctx._h, int(n), int(restart), _BASES[basis], C.byref(h)), "dxo_krylov_create_basis")
        self._h = h
        self.ctx, self.n, self.restart = ctx, int(n), int(restart)
        self._fin = weakref.finalize(self, ctx.lib.dxo_krylov_destroy, C.c_void_p(ctx._h.value), h)
        self._fin.atexit = False   # at interpreter exit the device memory goes with the process

    def close(self) -> None:
        self._fin()

    def basis_info(self) -> tuple:
        """(kind, bytes of the basis rows, device pointer of row 0, row stride in elements) (dxo_krylov_basis_info)."""
        kind, nbytes, rows, ld = C.c_int(), C.c_int64(), C.c_void_p(), C.c_int64()
        self.ctx.check(self.ctx.lib.dxo_krylov_basis_info(self.ctx._h, self._h, C.byref(kind), C.byref(nbytes), C.byref(rows), C.byref(ld)),
                       "dxo_krylov_basis_info")
        return {v: k for k, v in _BASES.items()}[kind.value], int(nbytes.value), rows.value, int(ld.value)


def _ws_key(n: int, restart: int, basis: str) -> tuple:
    """The cache key of a workspace: (n, restart) for the fp64 basis, as before the basis could be chosen, (n, restart, basis) for
    any other."""
    return (int(n), int(restart)) if basis == "fp64" else (int(n), int(restart), basis)


def _workspace(ctx, n: int, restart: int, basis: str = "fp64") -> _Workspace:
    cache = ctx.__dict__.setdefault("_krylov_ws", {})
    key = _ws_key(n, restart, basis)
    if key not in cache:
        if len(cache) >= 4:    # a few sizes per context: the oldest basis is freed
            cache.pop(next(iter(cache))).close()
        cache[key] = _Workspace(ctx, n, restart, basis)
    return cache[key]


def krylov_basis_rows(ctx, n: int, restart: int, basis: str = "fp32"):
    """The stored basis of the last solve on the context's (n, restart, basis) workspace as a NumPy array (restart + 1, ld), float32
    or float64 by the kind: row j is v_j in its first n entries, the padding up to the row stride ld is zero. Rows beyond the last
    cycle's steps hold what earlier cycles left. A copy; synchronises the stream. For tests and reports."""
    torch = _torch()
    ws = ctx.__dict__.get("_krylov_ws", {}).get(_ws_key(n, restart, basis))
    if ws is None:
        raise ValueError(f"krylov_basis_rows: no solve with n = {n}, restart = {restart}, basis = {basis!r} on this context")
    kind, _, rows, ld = ws.basis_info()
    dev = torch.device("cuda", ctx.device)
    torch.cuda.current_stream(dev).synchronize()
    view = _CudaArrayView(ws, rows, (int(restart) + 1) * ld, "<f4" if kind == "fp32" else "<f8")
    return torch.as_tensor(view, device=dev).cpu().numpy().copy().reshape(int(restart) + 1, ld)


def _solve(entry: str, A, b, x, M, restart: int, rtol: float, atol: float, maxiter, check_every: int, ctx=None,
           basis: str = "fp64") -> KrylovResult:
    torch = _torch()
    if not isinstance(basis, str) or basis not in _BASES:
        raise ValueError(f"{entry}: basis must be one of {sorted(_BASES)}")
    from .operand_eval import DeviceCSR

    if isinstance(A, DeviceCSR):
        ctx, n = A.pattern.ctx, A.pattern.n_rows
        op = KrylovOp(n, A.pattern._h, C.c_void_p(A.values.data_ptr()), KRYLOV_APPLY_FN(), None)
        failure: list = []
        cb = None
    elif callable(A):
        if ctx is None:
            from ._lib import default_context

            ctx = default_context()
        if not isinstance(b, torch.Tensor):
            raise ValueError(f"{entry}: b must be a float64 CUDA tensor")
        n = b.numel()
        views: dict = {}
        failure = []

        def view(ptr: int):
            t = views.get(ptr)
            if t is None:
                t = views[ptr] = torch.as_tensor(_CudaArrayView(ctx, ptr, n, "<f8"), device=torch.device("cuda", ctx.device))
            return t

        def cb(_user, v, out):
            try:
                A(view(v), view(out))
                return 0
            except BaseException as e:      # noqa: BLE001 — re-raised after the solve returns
                failure.append(e)
                return 1

        cb = KRYLOV_APPLY_FN(cb)
        op = KrylovOp(n, None, None, cb, None)
    else:
        raise TypeError(f"{entry}: A must be a DeviceCSR or a callable (v, out) that sets out = A v")
    dev = torch.device("cuda", ctx.device)
    _check_vec(b, n, dev, f"{entry}: b")
    if x is None:
        x = torch.zeros_like(b)
    _check_vec(x, n, dev, f"{entry}: x")
    if M is None:
        pc = KrylovPc(PC_NONE, 1, n, None)
    elif isinstance(M, BlockJacobi):
        if M.n != n or M.inv.device != dev:
            raise ValueError(f"{entry}: the preconditioner covers {M.n} rows on {M.inv.device}, the operator has {n} on {dev}")
        pc = M._pc()
    elif isinstance(M, AMG):      # on a callable A (matrix-free, or a lagged matrix behind M) the block size is the multigrid's
        if M.n != n or M.device != dev or (isinstance(A, DeviceCSR) and A.pattern.bs != M.bs):
            raise ValueError(f"{entry}: the multigrid preconditioner covers {M.n} rows (bs {M.bs}) on {M.device}, the operator has {n} on {dev}")
        pc = M._pc()
    elif isinstance(M, PMG):
        if M.n != n or M.device != dev:
            raise ValueError(f"{entry}: the p-multigrid preconditioner covers {M.n} rows on {M.device}, the operator has {n} on {dev}")
        pc = M._pc()
    elif isinstance(M, torch.Tensor):
        _check_vec(M, n, dev, f"{entry}: M (inverse diagonal)")
        pc = KrylovPc(PC_JACOBI, 1, n, C.c_void_p(M.data_ptr()))
    elif callable(M):
        mviews: dict = {}

        def mview(ptr: int):
            t = mviews.get(ptr)
            if t is None:
                t = mviews[ptr] = torch.as_tensor(_CudaArrayView(ctx, ptr, n, "<f8"), device=dev)
            return t

        def mcb(_user, r, out):
            try:
                M(mview(r), mview(out))
                return 0
            except BaseException as e:      # noqa: BLE001 — re-raised after the solve returns
                failure.append(e)
                return 1

        mcb = KRYLOV_APPLY_FN(mcb)
        mstruct = KrylovCallback(mcb, None)      # both stay referenced until the solve has returned
        pc = KrylovPc(PC_CALLBACK, 1, n, C.cast(C.pointer(mstruct), C.c_void_p))
    else:
        raise TypeError(f"{entry}: M must be None, a BlockJacobi, an AMG, a PMG, a tensor holding an inverse diagonal or a callable (r, out)")
    if maxiter is None:
        maxiter = max(1000, 10 * restart)
    ws = _workspace(ctx, n, restart, basis)
    info = KrylovInfo()
    _use_current_stream(ctx)
    rc = getattr(ctx.lib, entry)(ctx._h, ws._h, C.byref(op), C.byref(pc), C.c_void_p(b.data_ptr()), C.c_void_p(x.data_ptr()), float(rtol),
                                 float(atol), int(maxiter), int(check_every), C.byref(info))
    if failure:
        raise failure[0]
    if isinstance(M, PMG):
        M._raise()
    ctx.check(rc, entry)
    return KrylovResult(x=x, iterations=int(info.iterations), residual=float(info.residual), converged=bool(info.converged),
                        breakdown=bool(info.breakdown), restarts=int(info.restarts), ms=float(info.ms), basis=basis,
                        basis_bytes=0 if entry == "dxo_krylov_cg" else ws.basis_info()[1])


def gmres(A, b, x=None, M=None, restart: int = 30, rtol: float = 1e-10, atol: float = 0.0, maxiter: int | None = None,
          check_every: int = 8, ctx=None, basis: str = "fp64") -> KrylovResult:
    """Solve A x = b by restarted GMRES(restart) with right preconditioning on the device (dxo_krylov_gmres).

    A: a DeviceCSR, or a callable (v, out) that sets out = A v on the device (e.g. DeviceMesh.bilinear_apply with option
    consumer_overwrite = 1; `ctx` then names the context, default_context() otherwise). M: None, a BlockJacobi, an AMG (one V-cycle
    per iteration; with a callable A the multigrid of an assembled, possibly lagged, matrix of the same size), a float64 CUDA tensor
    holding an inverse diagonal (1 / bilinear_diagonal for the matrix-free path), a PMG after its setup() (the p-multigrid of the
    matrix-free path, DXO_PC_PMG), or a callable (r, out) that sets out = M r on the
    device; an exception in it is re-raised after the solve. M must be a fixed linear operator here, the same at every call: M is
    applied once more to the combination at the end of a cycle. One that varies (an inner iteration, an AMG with the K-cycle,
    which raises ValueError here) belongs to fgmres. An AMG with precision="fp32" is a fixed linear operator up to single-precision
    rounding and is accepted; it may cost one more restart to reach tolerances below about 1e-7. x: the initial guess, overwritten with the
    solution (zeros if None). Converged when |b - A x| <= max(rtol |b|, atol); not converging within maxiter gives converged False,
    not an exception.

    basis: "fp64" (the default, the solver of earlier versions bit for bit) or "fp32", a compressed basis (dxo_krylov_create_basis):
    the Krylov vectors are stored in float, half the bytes the orthogonalisation reads and half the basis memory, while every dot
    product, update, Hessenberg entry, rotation and x stay double, and M and A are given exactly the vector that was stored. What it
    guarantees: the stopping test is on the double true residual b - A x, formed at every restart, so a converged result meets the
    tolerance as with "fp64"; a solve is bit-reproducible. What it may cost: the Hessenberg estimate inside a cycle is trustworthy
    to about 2^-24 relative to the cycle's starting residual, so one cycle cannot gain much more than seven digits on its own
    estimate: expect at most one extra cycle at tight tolerances. Anything else raises ValueError."""
    return _solve("dxo_krylov_gmres", A, b, x, M, restart, rtol, atol, maxiter, check_every, ctx, basis)


def fgmres(A, b, x=None, M=None, restart: int = 30, rtol: float = 1e-10, atol: float = 0.0, maxiter: int | None = None,
           check_every: int = 8, ctx=None, basis: str = "fp64") -> KrylovResult:
    """Solve A x = b by flexible GMRES(restart) on the device (dxo_krylov_fgmres), with the arguments and the stopping rule of gmres.

    M need not be a fixed linear operator: it may differ from step to step (a callable that runs an inner solve, an AMG with the
    K-cycle). The preconditioned vectors z_j = M v_j are kept in a second basis (restart more vectors, allocated at the first
    flexible solve of a size) and the solution is updated with them, so M is called once per iteration and never at the update.
    With a fixed M it takes the iterations of gmres. It is the recommended partner of an AMG with precision="fp32": the update uses the
    stored z_j, so the single-precision rounding of the cycle never enters the solution a second time.

    basis: as in gmres, with its guarantees (the stopping test on the double true residual) and its cost (a cycle's own estimate is
    good to about 2^-24 of its starting residual: at most one extra cycle at tight tolerances). "fp32" compresses V only. The second
    basis Z stays double: the z_j = M v_j are not normalised, so their range is the caller's, and Z is written once and read once
    per cycle. `basis_bytes` of the result counts V alone."""
    return _solve("dxo_krylov_fgmres", A, b, x, M, restart, rtol, atol, maxiter, check_every, ctx, basis)


def cg(A, b, x=None, M=None, rtol: float = 1e-10, atol: float = 0.0, maxiter: int | None = None, check_every: int = 8,
       ctx=None) -> KrylovResult:
    """Preconditioned conjugate gradients for symmetric positive definite A and M, same arguments as gmres (dxo_krylov_cg). M must
    be a fixed linear operator (a callable that varies between calls, or an AMG with the K-cycle, has no place here: fgmres). An AMG
    with precision="fp32" is accepted: it is symmetric up to single-precision rounding, and the residual is recomputed at the end."""
    return _solve("dxo_krylov_cg", A, b, x, M, 1, rtol, atol, maxiter, check_every, ctx)


__all__ = ["AMG", "PMG", "BlockJacobi", "KrylovResult", "krylov_basis_rows", "cg", "csr_matvec", "fgmres", "gmres", "rigid_body_modes"]
