"""What the tests of the solver stack share (the form layer's assembly, the Krylov methods, the multigrid): the named systems on the
CPU and on the device, the hierarchy builders, the helpers around torch and the cross-file constants. Not a test module; the
references themselves are in oracle/."""
import numpy as np
import pytest

from oracle.amg_oracle import Level, amg_ref, node_graph, rigid_body_modes_ref
from oracle.form_oracle import apply_bcs, dense_ref, heat_setting, pattern_ref
from oracle.krylov_oracle import (F2_C, F2_D, F2_S, MARGIN, REF_F1_RES, REF_F1_X, REF_F2_RES, REF_F2_X, bottom_dofs, boundary_dofs,
                                  cycle_rhs, cyclic_shift_src, elastic_C, elastic_C3, eps_matrix, heat_matrix, precond_diagonal,
                                  to_pattern_csr)
from tools.synthetic import structured_mesh

# ---- the form layer: cells and pairs of the bilinear and assembly tests
CELLS = {"triangle": (4, 3), "quadrilateral": (3, 3), "tetrahedron": (2, 2, 1), "hexahedron": (2, 1, 2)}
# (test, trial, bs is gdim)
PAIRS = [("grad", "grad", True), ("F", "grad", True), ("grad", "F", True), ("F", "F", True), ("eps", "eps", True),
         ("grad", "value_grad", False), ("grad", "grad", False), ("value", "value", False), ("value_grad", "value_grad", False)]


def _value_size(kind, G, bs):
    return {"value": bs, "grad": bs * G, "F": G * G, "value_grad": bs * (1 + G), "eps": 4 if G == 2 else 6}[kind]


# ---- the CPU systems of the multigrid oracles
THETA = 0.25
GPU_THETAS = {"aniso_quad": THETA, "aniso_tri": THETA, "p2_tri_rbm": 0.1, "hex_rbm": 0.1}
COARSE_ROWS = 60         # of the p-coarsening experiment and its device tests
_CACHE = {}


def eps_spd(n, degree=2, clamp="bottom", distort=0.15, seed=5):
    """(mesh, S on the device pattern, constrained dofs): eps/eps with the isotropic C on triangles, SPD."""
    m = structured_mesh("triangle", n, degree, distort=distort, seed=seed)
    if clamp == "bottom":
        dofs = bottom_dofs(m, 2)
    else:                                                  # the left edge: a cantilever
        on = np.flatnonzero(np.abs(m.node_x[:, 0] - m.node_x[:, 0].min()) < 1e-12)
        dofs = (on[:, None] * 2 + np.arange(2)).reshape(-1)
    A = apply_bcs(dense_ref(m, "eps", "eps", 2, elastic_C(m)), dofs, 1.0)
    return m, to_pattern_csr(m, A, 2), dofs


# the dead-column case: P1 triangles 6 x 5, rollers (the vertical component) on the bottom, the horizontal component held on the left
# edge, and the neighbours of one interior node clamped. Rollers alone cannot give a singleton: a partly constrained node stays active,
# so the aggregates are those of the unconstrained mesh, and these structured meshes have no singleton aggregate
# (test_dead_column_case_has_a_singleton checks the sizes 3..8 per side). Clamped neighbours leave the node alone in the graph, so it
# founds an aggregate of one node: 2 rows, 3 vectors, the rotation is dead.
DEAD_CASE = (6, 5)
DEAD_NODE = 14


def dead_case():
    m = structured_mesh("triangle", DEAD_CASE, 1, distort=0.1, seed=2)
    indptr, indices = pattern_ref(m, 2)
    ptr, nb = node_graph(indptr, indices, 2)
    ring = nb[ptr[DEAD_NODE]:ptr[DEAD_NODE + 1]]
    ring = ring[ring != DEAD_NODE]
    rollers = bottom_dofs(m, 2)[1::2]
    left = np.flatnonzero(np.abs(m.node_x[:, 0] - m.node_x[:, 0].min()) < 1e-12) * 2
    dofs = np.unique(np.concatenate([rollers, left, (ring[:, None] * 2 + np.arange(2)).reshape(-1)]))
    A = dense_ref(m, "eps", "eps", 2, elastic_C(m))
    return m, to_pattern_csr(m, apply_bcs(A, dofs, 1.0), 2), dofs


def aniso_system(cell, n=24, eps=1e-3):
    """(mesh, S on the device pattern, constrained dofs): grad/grad with C = diag(1, eps), Dirichlet boundary; the quadrilaterals
    uniform, the triangles distorted by 0.1 (seed 2)."""
    m = structured_mesh(cell, (n, n), 1, distort=0.0 if cell == "quadrilateral" else 0.1, seed=2)
    C = np.broadcast_to(np.diag([1.0, eps]), (m.num_cells * m.nq, 2, 2)).copy()
    dofs = boundary_dofs(m, 1)
    return m, to_pattern_csr(m, apply_bcs(dense_ref(m, "grad", "grad", 1, C), dofs, 1.0), 1), dofs


def cached_aniso(cell, n=24, eps=1e-3):
    if (cell, n, eps) not in _CACHE:
        _CACHE[(cell, n, eps)] = aniso_system(cell, n, eps)
    return _CACHE[(cell, n, eps)]


def system(which):
    """(S, b, levels): "p2_rbm" P2 eps/eps 14 x 14 with rigid-body modes, "heat" the P1 heat Jacobian 16 x 16, "nonsym" the
    non-symmetric eps_matrix((14, 14)), "aniso" the anisotropic 24 x 24 quadrilaterals with strength 0.25, "heat48" the scalar P1
    system of 2401 rows on four levels: the systems of the earlier oracle tests, coarsened far enough for three levels and more."""
    if which not in _CACHE:
        if which == "p2_rbm":
            m, S, dofs = eps_spd((14, 14))
            levels = amg_ref(S, 2, dofs, near_nullspace=rigid_body_modes_ref(m.node_x), coarse_rows=20)
        elif which in ("heat", "heat48"):
            m, A = heat_matrix(16 if which == "heat" else 48)
            S = to_pattern_csr(m, A, 1)
            levels = amg_ref(S, 1, boundary_dofs(m, 1), coarse_rows=10)
        elif which == "nonsym":
            m, A = eps_matrix((14, 14))
            S = to_pattern_csr(m, A, 2)
            levels = amg_ref(S, 2, bottom_dofs(m, 2), coarse_rows=20)
        else:
            m, S, dofs = cached_aniso("quadrilateral")
            levels = amg_ref(S, 1, dofs, strength=THETA, coarse_rows=10)
        b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
        _CACHE[which] = (S, b, levels)
    return _CACHE[which]


# ---- torch and the device
def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).cuda()


def _zeros(n):
    import torch

    return torch.zeros(n, dtype=torch.float64, device="cuda")


def _torch(ctx):
    import torch

    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    return torch


def _assemble(ctx, dm, test, trial, bs, Cb, bcs=None):
    torch = _torch(ctx)
    bt = None if bcs is None else torch.from_numpy(np.asarray(bcs, dtype=np.int32)).cuda()
    Cd = _cuda(Cb)                  # kept alive until the assembly has run
    A = dm.bilinear_assemble(test, trial, bs, Cd.data_ptr(), dm.csr_pattern(bs), bcs=bt)
    torch.cuda.synchronize()
    return A


@pytest.fixture
def meshes(ctx):
    from dolfinx_external_operator_amd import DeviceMesh

    made = []

    def make(m):
        dm = DeviceMesh.from_synthetic(m, ctx=ctx)
        made.append(dm)
        return dm

    yield make
    for dm in made:
        dm.close()


# ---- the device systems
def _heat(ctx, meshes, nx):
    m, dqdT, dqds, _ = heat_setting(nx)
    Cb = np.concatenate([dqdT[..., None], dqds], axis=-1).reshape(m.num_cells * m.nq, 2, 3)
    bcs = boundary_dofs(m, 1)
    return _assemble(ctx, meshes(m), "grad", "value_grad", 1, -Cb, bcs=bcs), bcs


def _assembled_system(ctx, meshes, which):
    """(DeviceCSR, bs, constrained dofs), with Dirichlet rows: "heat", "hyperelastic", "hex_eps" (a non-symmetric coupling) and the
    SPD system "spd_quad" of the CG tests."""
    torch = _torch(ctx)
    if which == "heat":
        A, bcs = _heat(ctx, meshes, 16)
        return A, 1, bcs
    if which == "hyperelastic":
        from dolfinx_external_operator_amd import MEM_DEVICE, IsiharaParams

        m = structured_mesh("triangle", (10, 10), 2, distort=0.1, seed=3)
        dm = meshes(m)
        npts = m.num_cells * m.nq
        u = torch.from_numpy((0.08 * m.node_x * m.node_x[:, 1:2]).reshape(-1).copy()).cuda()
        dP, P = torch.zeros(npts * 16, dtype=torch.float64, device="cuda"), torch.zeros(npts * 4, dtype=torch.float64, device="cuda")
        ctx.isihara_field(IsiharaParams(0.5, 1.0, 1.0, 1.5), dm._h, MEM_DEVICE, u.data_ptr(), dP.data_ptr(), P.data_ptr())
        torch.cuda.synchronize()
        bcs = bottom_dofs(m, 2)
        return _assemble(ctx, dm, "grad", "grad", 2, dP.cpu().numpy().reshape(npts, 4, 4), bcs=bcs), 2, bcs
    if which == "hex_eps":
        m = structured_mesh("hexahedron", (4, 3, 3), 1, distort=0.1, seed=2)
        Cb = elastic_C3(m.num_cells * m.nq)
        Cb[:, :3, 3:] += 0.2
        bcs = bottom_dofs(m, 3)
        return _assemble(ctx, meshes(m), "eps", "eps", 3, Cb, bcs=bcs), 3, bcs
    m = structured_mesh("quadrilateral", (12, 10), 2, distort=0.1, seed=1)
    bcs = bottom_dofs(m, 2)
    return _assemble(ctx, meshes(m), "eps", "eps", 2, elastic_C(m), bcs=bcs), 2, bcs


def _krylov_system(ctx, meshes, which):
    """(DeviceCSR, bs) of _assembled_system."""
    return _assembled_system(ctx, meshes, which)[:2]


def _nns_system(ctx, meshes, which):
    """(DeviceCSR, bs, constrained dofs, node coordinates, SPD?)"""
    if which == "p2_eps":
        m = structured_mesh("triangle", (14, 14), 2, distort=0.15, seed=5)
        bcs = bottom_dofs(m, 2)
        return _assemble(ctx, meshes(m), "eps", "eps", 2, elastic_C(m), bcs=bcs), 2, bcs, m.node_x, True
    if which == "hyperelastic":
        A, bs, bcs = _assembled_system(ctx, meshes, "hyperelastic")
        return A, bs, bcs, structured_mesh("triangle", (10, 10), 2, distort=0.1, seed=3).node_x, False
    if which in ("hex_eps", "hex_bar"):      # the bar: 22 nodes and 3 aggregates on the level of block size 6 (the cube: 8 and 1)
        m = structured_mesh("hexahedron", (4, 4, 4) if which == "hex_eps" else (32, 3, 3), 1, distort=0.1, seed=2)
        bcs = bottom_dofs(m, 3)
        return _assemble(ctx, meshes(m), "eps", "eps", 3, elastic_C3(m.num_cells * m.nq), bcs=bcs), 3, bcs, m.node_x, True
    m, _, bcs = dead_case()
    return _assemble(ctx, meshes(m), "eps", "eps", 2, elastic_C(m), bcs=bcs), 2, bcs, m.node_x, True


def _aniso(ctx, meshes, cell, n=24, eps=1e-3, distort=None):
    m = structured_mesh(cell, (n, n), 1, distort=(0.0 if cell == "quadrilateral" else 0.1) if distort is None else distort, seed=2)
    Cb = np.broadcast_to(np.diag([1.0, eps]), (m.num_cells * m.nq, 2, 2)).copy()
    bcs = boundary_dofs(m, 1)
    return _assemble(ctx, meshes(m), "grad", "grad", 1, Cb, bcs=bcs), bcs


def _soc_system(ctx, meshes, which):
    """(DeviceCSR, bs, constrained dofs, near-null space or None, coarse_rows): the systems of GPU_THETAS, assembled on the device."""
    from dolfinx_external_operator_amd.krylov import rigid_body_modes

    if which in ("aniso_quad", "aniso_tri"):
        A, bcs = _aniso(ctx, meshes, "quadrilateral" if which == "aniso_quad" else "triangle")
        return A, 1, bcs, None, 60
    if which == "p2_tri_rbm":
        m = structured_mesh("triangle", (6, 5), 2, distort=0.1, seed=2)
        bcs = bottom_dofs(m, 2)
        return _assemble(ctx, meshes(m), "eps", "eps", 2, elastic_C(m), bcs=bcs), 2, bcs, rigid_body_modes(m.node_x, ctx=ctx), 20
    m = structured_mesh("hexahedron", (3, 2, 3), 1, distort=0.1, seed=2)
    bcs = bottom_dofs(m, 3)
    return _assemble(ctx, meshes(m), "eps", "eps", 3, elastic_C3(m.num_cells * m.nq), bcs=bcs), 3, bcs, rigid_body_modes(m.node_x, ctx=ctx), 20


# ---- the hierarchies of the cycle tests
# which -> (levels, block sizes): a scalar P1 system of 2401 rows on four levels (a K solve calls a K solve), P2 triangles 14 x 14
# eps/eps with rigid-body modes, the 32 x 3 x 3 hexahedron bar, Chebyshev degree 2 on the power estimate, strength of connection 0.25
CASES = {"heat48": (4, [1, 1, 1, 1]), "p2_rbm": (3, [2, 3, 3]), "hex_bar": (3, [3, 6, 6]), "heat48_cheby": (4, [1, 1, 1, 1]),
         "aniso_soc": (4, [1, 1, 1, 1])}


def _case_system(ctx, meshes, which):
    """(DeviceCSR, constrained dofs, the keywords of its hierarchy) of a case."""
    from dolfinx_external_operator_amd import rigid_body_modes

    if which in ("heat48", "heat48_cheby"):
        A, bcs = _heat(ctx, meshes, 48)
        return A, bcs, dict(coarse_rows=10, **(dict(smoother="chebyshev", degree=2, rho="power") if which == "heat48_cheby" else {}))
    if which == "aniso_soc":
        A, bcs = _aniso(ctx, meshes, "quadrilateral")
        return A, bcs, dict(coarse_rows=10, strength=0.25)
    A, bs, bcs, x, _ = _nns_system(ctx, meshes, "p2_eps" if which == "p2_rbm" else "hex_bar")
    return A, bcs, dict(coarse_rows=20 if which == "p2_rbm" else 40, near_nullspace=rigid_body_modes(x, ctx=ctx))


def _case_hierarchy(ctx, meshes, which, **kw):
    """(DeviceCSR, AMG): the hierarchy of a case with the keywords of the constructor on top (cycle=...)."""
    A, bcs, base = _case_system(ctx, meshes, which)
    return A, A.amg(bcs, **base, **kw)


def _device_levels(amg):
    """The hierarchy on the device as the Level list the oracle cycles walk."""
    dev, rhos, sm = amg.levels, amg.rho, amg.smoother
    levels = []
    for l in range(amg.n_levels):
        L = Level()
        L.A, L.n_rows, L.bs, L.sweeps = amg.level_matrix(l), dev[l]["rows"], dev[l]["bs"], amg.sweeps
        L.smoother, L.degree, L.lower = sm["smoother"], sm["degree"], sm["lower"]
        if l + 1 < amg.n_levels:
            L.Dinv, L.omega, L.rho, L.P = amg.level_dinv(l), dev[l]["omega"], rhos[l], amg.prolongator(l).tocsr()
        levels.append(L)
    levels[-1].dense_inverse = np.linalg.inv(levels[-1].A.toarray())
    return levels


def _soc_snapshot(amg):
    return ([amg.level_matrix(l) for l in range(amg.n_levels)], [amg.prolongator(l) for l in range(amg.n_levels - 1)],
            [amg.strong_mask(l) for l in range(amg.n_levels)], [amg.aggregates(l) for l in range(amg.n_levels - 1)],
            [(d["omega"], d["omega_f"]) for d in amg.levels])


# the cycle against the oracle cycle, relative to |z|. Not derivable; measured on the four systems of tests/test_amg_gpu.py on an
# MI355X: 8.6e-16 (heat), 1.0e-15 (hyperelastic), 2.1e-15 (hex_eps), 1.4e-15 (spd_quad). 100 x the largest, and far below the 1e-10 the
# feature was specified with.
CYCLE_TOL = 2e-13
# The K-cycle against the oracle's K-cycle on the device's own levels, relative to |z|. Not derivable: the coefficients divide by rho1
# and rho2, sums that the device adds in another order. The rule is 100 x the largest K_CYCLE_SEEN the first test of
# tests/test_amg_kcycle_gpu.py prints on an MI355X (the rule of CYCLE_TOL). Measured on an MI355X with the ratio form of the
# coefficients: heat48 5.2e-16, heat48_cheby 8.6e-16, aniso_soc 1.3e-15, p2_rbm 5.2e-15, hex_bar 4.5e-14 (4.471e-14). That is more
# than the V-cycle's 2e-13 that stood here before the first run, and it comes from hex_bar alone: on the hierarchies with rigid-body
# modes the V-cycle itself is up to 1.3e-14 |z| from its oracle (test_amg_nns_gpu.py; rows of 6 x 6 blocks summed in another order),
# the K solve of level 1 runs that body twice, the second time on r1 = r - alpha1 v1, which is smaller than its two terms, so what the
# first body deviates by arrives magnified by |r| / |r1|, and x1 = alpha1 - (g / rho1) x2 is a difference again
K_CYCLE_TOL = 4.5e-12
# e_dev <= SAME_FORMULAS e_ref: the device and the oracle evaluate the same formulas in float32 in different summation orders (a rule
# for that reordering, not a measurement); e_dev >= NOT_DOUBLE e_ref: a cycle that silently ran in double would sit orders below
SAME_FORMULAS, NOT_DOUBLE = 8.0, 0.05


# ---- the known-answer families on the device
# The device against the closed forms and the float64 oracle. Not derivable as one constant (the device adds its dot products over
# nb partials with FMA, in another order than NumPy), so: MARGIN = 100 x the oracle's own deviation from the long-double answers,
# REF_* in oracle/krylov_oracle.py, measured by tests/test_krylov_oracle_cpu.py as 4.5e-16 max|b| / 3.6e-16 (F1: x, residual at
# termination) and 6.5e-16 relative / 5.2e-16 max|x| (F2: residual, x_k) and rounded up to 6e-16 / 4e-16 / 1e-15 / 1e-15. Measured on an
# MI355X (256 CUs), the largest over all cases the tests of tests/test_krylov_known_answers_gpu.py print: F1 x 4.4e-16 max|b|,
# F1 residual 3.1e-16, F2 residual 7.0e-16 relative, F2 x_k 5.2e-16 max|x|. One wrong rotation or Hessenberg entry changes these by O(1).
F1_X_TOL, F1_RES_TOL = MARGIN * REF_F1_X, MARGIN * REF_F1_RES
F2_RES_TOL, F2_X_TOL = MARGIN * REF_F2_RES, MARGIN * REF_F2_X


def _grid_cap(torch):
    """Rows that one trip of the row kernels covers: nb = min(ceil(n / 256), 4 CUs) workgroups of 256."""
    return 256 * 4 * torch.cuda.get_device_properties(0).multi_processor_count


def _index(torch, src):
    return torch.from_numpy(src.astype(np.int64)).cuda()


def _shift(torch, src):
    s = _index(torch, src)
    return lambda v, out: torch.index_select(v, 0, s, out=out)


def _shifted(torch, src, D=None):
    """c I + s P, or (c I + s P) diag(D), rounded as shifted_op of oracle/krylov_oracle.py rounds it."""
    s = _index(torch, src)
    tmp = torch.empty(src.size, dtype=torch.float64, device="cuda")

    def apply(v, out):
        if D is not None:
            v = torch.mul(v, D, out=tmp)
        torch.index_select(v, 0, s, out=out)
        out.mul_(F2_S).add_(v, alpha=F2_C)

    return apply


def _reorth(ctx, value):
    class Scope:
        def __enter__(self):
            ctx.set_option("krylov_reorth", value)

        def __exit__(self, *exc):
            ctx.set_option("krylov_reorth", 1)

    return Scope()


def _f2(torch, q, t, precond=False):
    src, b = cyclic_shift_src(F2_D, q, t), cycle_rhs(F2_D, q, t, seed=q)
    D = precond_diagonal(b.size) if precond else None
    dev = _shifted(torch, src, None if D is None else _cuda(D))
    return src, b, D, dev
