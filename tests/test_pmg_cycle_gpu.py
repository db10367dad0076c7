"""dxo_pmg_setup and dxo_pmg_apply on the device against tests/pmg_reference.py: rho and the Chebyshev pairs, the cycle against the
long-double reference, its algebraic properties, the Krylov methods with it and a graph capture."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle.amg_oracle import cheby_pairs, power_rho_ref, vertex_transfer_ref
from oracle.form_oracle import apply_bcs, dense_ref
from oracle.krylov_oracle import cg_ref, elastic_C3, fgmres_ref, gmres_ref, to_pattern_csr
from pmg_reference import PmgRef, diagonal_case, exact_inverse
from solver_cases import _assemble, _cuda, _torch, meshes  # noqa: F401  (meshes is a fixture)
from tools.synthetic import gauss_tensor_rule, structured_mesh, vertex_companion, with_rule

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
# cell, boxes, block size, form, 27-point rule
CASES = {"tri6_s": ("triangle", (6, 6), 1, "grad", False), "tri6_v": ("triangle", (6, 6), 2, "grad", False),
         "tet3": ("tetrahedron", (3, 3, 3), 3, "eps", False), "hex2": ("hexahedron", (2, 2, 2), 3, "eps", True)}
_HOST = {}


def _transfer(W, ctf):
    from dolfinx_external_operator_amd import NodalTransfer

    return NodalTransfer(W.shape[1], W.indptr, W.indices, W.data, ctf)


def _host(which):
    if which not in _HOST:
        cell, n, bs, form, rule27 = CASES[which]
        m = structured_mesh(cell, n, 2, distort=0.1, seed=2)
        if rule27:
            m = with_rule(m, *gauss_tensor_rule(cell, 3))
        on = np.flatnonzero(np.abs(m.node_x[:, -1]) < 1e-12)                      # the face x_last = 0 clamped
        dofs = (on[:, None] * bs + np.arange(bs)).reshape(-1)
        _HOST[which] = (m, vertex_companion(m), dofs) + vertex_transfer_ref(m)
    return _HOST[which]


def _blocks(m, bs, form):
    if form == "grad":
        D = bs * m.gdim
        return np.broadcast_to(np.eye(D), (m.num_cells * m.nq, D, D)).copy()
    return elastic_C3(m.num_cells * m.nq)


class System:
    """The fine matrix (assembled on the device), its inverse diagonal, the PMG object, and the coarse matrix assembled on
    DeviceMesh.vertex_mesh with the coarse constrained list."""

    def __init__(self, ctx, meshes, which, **smoother):
        from dolfinx_external_operator_amd import PMG
        from dolfinx_external_operator_amd.operand_eval import DeviceCSR

        torch = _torch(ctx)
        cell, n, bs, form, _ = CASES[which]
        m, mc, dofs, W, ctf = _host(which)
        self.which, self.bs, self.m, self.dofs, self.W, self.ctf = which, bs, m, dofs, W, ctf
        dm = meshes(m)
        try:
            self.A = _assemble(ctx, dm, form, form, bs, _blocks(m, bs, form), bcs=dofs)
        except ValueError as e:      # the Q2 hexahedron with 27 points may not fit the assembly's LDS budget: the oracle's values
            assert which == "hex2" and "DXO_E_SIZE" in str(e), e
            S = to_pattern_csr(m, apply_bcs(dense_ref(m, form, form, bs, _blocks(m, bs, form)), dofs, 1.0), bs)
            pat = dm.csr_pattern(bs)
            assert np.array_equal(pat.indptr.cpu().numpy(), S.indptr) and np.array_equal(pat.indices.cpu().numpy(), S.indices)
            self.A = DeviceCSR(pat, torch.from_numpy(S.data.copy()).cuda())
        self.S = self.A.to_scipy()
        self.dinv_h = 1.0 / self.S.diagonal()
        self.dinv = _cuda(self.dinv_h)
        self.pmg = PMG(_transfer(W, ctf), bs, constrained=dofs, ctx=ctx, **smoother)
        dmc = dm.vertex_mesh(mc.psi, mc.dpsi, mc.weights)
        self._dmc = dmc
        self.Ac = _assemble(ctx, dmc, form, form, bs, _blocks(mc, bs, form), bcs=self.pmg.coarse_constrained.cpu().numpy())
        self.Sc = self.Ac.to_scipy()
        self.ref = PmgRef(W, ctf, bs, dofs)

    def dense_amg(self):
        amg = self.Ac.amg(self.pmg.coarse_constrained, coarse_rows=10 ** 6)       # one level: the dense inverse
        assert amg.n_levels == 1
        return amg

    def close(self):
        self.pmg.close()
        self._dmc.close()


@pytest.fixture
def systems(ctx, meshes):
    made = []

    def make(which, **smoother):
        s = System(ctx, meshes, which, **smoother)
        made.append(s)
        return s

    yield make
    for s in made:
        s.close()


# ---- rho and the pairs
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_rho_and_pairs_on_a_diagonal_operator(ctx, n):
    """A v = a v through a callback, Dinv A = diag(q), identity transfer. rho against power_rho_ref, relative to EPS rho_iters C_RHO.
    Per step and side an entry is rounded three times (the scale, A, Dinv): 3 EPS per step for both sides together. The last norm: the
    device adds the squares over a depth of at most 1 (a thread's entries, n <= 1024 * 256) + 6 (butterfly) + 3 (waves), the same again
    for the partials with up to 4 per thread: 23; NumPy's pairwise sum 16 + 3 inside a block of 128 and ceil(log2(n / 128)) above: 25
    at n = 4097; the square roots halve both, and sqrt, 1 / |w| and the factor `safety` add 3 roundings a side: (23 + 25) / 2 u / 2 + 6 u
    <= 9 EPS. Together EPS (3 m + 9) <= 12 EPS m: C_RHO = 12. Earlier norms only scale w, which the next normalisation removes."""
    from dolfinx_external_operator_amd import PMG, BlockJacobi

    C_RHO = 12
    torch = _torch(ctx)
    rng = np.random.Generator(np.random.PCG64(n))
    a, q = rng.uniform(0.5, 2.0, size=n), rng.uniform(0.25, 4.0, size=n)
    dinv = q / a
    ad, calls = _cuda(a), [0]

    def A(v, out):
        calls[0] += 1
        torch.mul(ad, v, out=out)

    W, ctf = diagonal_case(n)
    coarse = BlockJacobi(ctx, 1, _cuda(1.0 / a))
    for iters, degree, lower, safety in ((10, 2, 0.1, 1.1), (3, 8, 0.3, 1.0), (1, 1, 0.1, 1.1)):
        pmg = PMG(_transfer(W, ctf), 1, ctx=ctx, degree=degree, rho_iters=iters, lower=lower, safety=safety)
        calls[0] = 0
        pmg.setup(A, _cuda(dinv), coarse)
        assert calls[0] == iters                                                   # setup costs rho_iters operator calls
        rho = pmg.rho
        want = power_rho_ref(sp.diags(a).tocsr(), dinv.reshape(-1, 1, 1), iters=iters, safety=safety)
        print(f"n {n} iters {iters}: rho {rho:.17g}, reference {want:.17g}, deviation {abs(rho - want) / want / EPS:.2f} EPS")
        assert abs(rho - want) <= EPS * iters * C_RHO * want
        pairs = pmg.pairs.cpu().numpy()
        ref = np.array(cheby_pairs(rho, lower, degree))
        assert pairs.shape == (degree, 2) and pmg.degree == degree
        assert (np.abs(pairs - ref) <= 4 * EPS * np.abs(ref)).all(), (pairs, ref)  # a few ulp: the same recurrence
        assert pairs[0, 0] == 0.0
        # and the cycle on it against the reference (the odd sizes end in the one-entry tail of the 16-byte kernel). Every step is
        # entrywise: 2 degree steps of at most 8 roundings a side, each on a term of at most c2 |dinv r| (the residual of a step is
        # at most |r|: q lies below rho), so 2 * 16 degree EPS of scale = max |dinv r| sum c2 bounds the difference
        r = rng.normal(size=n)
        R = PmgRef(W, ctf, 1).setup(sp.diags(a).tocsr(), dinv, lambda rc: rc / a, degree=degree, lower=lower, rho=rho)
        z, zr = pmg.apply(_cuda(r)).cpu().numpy(), R.apply(r)
        scale = np.abs(dinv * r).max() * 2 * ref[:, 1].sum() + np.abs(r / a).max()
        assert np.abs(z - zr).max() <= 32 * degree * EPS * scale
        pmg.close()


def test_zero_operator_gives_zero_pairs_and_a_zero_result(ctx):
    """rho = 0: no relaxation, as omega = 0 in the multigrid. With the coarse operator zero as well (its pseudo-inverse: zero) z = 0."""
    from dolfinx_external_operator_amd import PMG, BlockJacobi

    _torch(ctx)
    n = 65
    W, ctf = diagonal_case(n)
    pmg = PMG(_transfer(W, ctf), 1, ctx=ctx, degree=3)
    pmg.setup(lambda v, out: out.zero_(), _cuda(np.ones(n)), BlockJacobi(ctx, 1, _cuda(np.zeros(n))))
    assert pmg.rho == 0.0 and not pmg.pairs.cpu().numpy().any()
    z = pmg.apply(_cuda(np.random.Generator(np.random.PCG64(0)).normal(size=n)))
    assert not z.cpu().numpy().any()
    pmg.close()


# ---- apply
def _accuracy(S, r, z_dev, coarse64, coarse_ld, tag):
    """e_dev <= 8 max(e_ref, 2^-52 |z|_inf): the device and the float64 reference against the long-double reference."""
    ref = S.ref
    z64 = ref.setup(S.S, S.dinv_h, coarse64, degree=S.pmg.degree, rho=S.pmg.rho).apply(r)
    ref.coarse = coarse_ld
    z_ld = ref.apply(r, dtype=np.longdouble)
    e_ref = float(np.abs(z64 - z_ld).max())
    e_dev = float(np.abs(z_dev - z_ld).max())
    floor = EPS * float(np.abs(z_ld).max())
    print(f"{tag}: e_dev {e_dev:.3e}, e_ref {e_ref:.3e}, 2^-52 |z| {floor:.3e}, PMG_SEEN ratio {e_dev / max(e_ref, floor):.3f}")
    assert e_dev <= 8 * max(e_ref, floor), (tag, e_dev, e_ref, floor)


@pytest.mark.parametrize("degree", [1, 2, 3, 8])
@pytest.mark.parametrize("which", list(CASES))
def test_cycle_against_the_long_double_reference(ctx, systems, which, degree):
    from dolfinx_external_operator_amd.krylov import csr_matvec

    torch = _torch(ctx)
    S = systems(which, degree=degree)
    amg = S.dense_amg()
    r = np.random.Generator(np.random.PCG64(12)).normal(size=S.S.shape[0])
    rd = _cuda(r)
    z = S.pmg.setup(S.A, S.dinv, amg).apply(rd).clone()
    assert S.pmg.matvecs_per_apply == 2 * degree
    # the same matrix behind a callable: the same kernel, the same bits
    z_cb = S.pmg.setup(lambda v, out: csr_matvec(S.A, v, out), S.dinv, amg).apply(rd)
    assert torch.equal(z, z_cb)
    inv64 = np.linalg.inv(S.Sc.toarray())
    inv_ld = exact_inverse(S.Sc, np.longdouble)
    _accuracy(S, r, z.cpu().numpy(), lambda rc: inv64 @ rc, lambda rc: inv_ld @ rc, f"{which} degree {degree}")


@pytest.mark.parametrize("coarse", ["amg_levels", "block_jacobi"])
def test_cycle_with_other_coarse_preconditioners(ctx, systems, coarse):
    """A multi-level AMG (rigid-body modes) and block Jacobi as the coarse step; the references call the device object for it."""
    from dolfinx_external_operator_amd import rigid_body_modes

    _torch(ctx)
    S = systems("tet3")
    if coarse == "amg_levels":
        M = S.Ac.amg(S.pmg.coarse_constrained, coarse_rows=30, near_nullspace=rigid_body_modes(S.m.x, ctx=ctx))
        assert M.n_levels >= 2
    else:
        M = S.Ac.block_jacobi()
    r = np.random.Generator(np.random.PCG64(13)).normal(size=S.S.shape[0])
    z = S.pmg.setup(S.A, S.dinv, M).apply(_cuda(r)).cpu().numpy()

    def dev(rc):
        return M.apply(_cuda(np.asarray(rc, dtype=np.float64))).cpu().numpy()

    _accuracy(S, r, z, dev, dev, f"tet3 {coarse}")


# ---- properties
def test_properties_of_the_cycle(ctx, systems):
    from dolfinx_external_operator_amd import BlockJacobi
    from dolfinx_external_operator_amd.krylov import csr_matvec

    torch = _torch(ctx)
    S = systems("tri6_v", degree=3, rho_iters=7)
    pmg, amg = S.pmg, S.dense_amg()
    n = S.S.shape[0]
    rng = np.random.Generator(np.random.PCG64(3))
    r, s = _cuda(rng.normal(size=n)), _cuda(rng.normal(size=n))
    with pytest.raises(ValueError, match="DXO_E_OPTION"):
        pmg.apply(r)                                                               # before any setup
    calls = [0]

    def A(v, out):
        calls[0] += 1
        csr_matvec(S.A, v, out)

    pmg.setup(A, S.dinv, amg)
    assert calls[0] == 7                                                           # exactly rho_iters
    calls[0] = 0
    z = pmg.apply(r).clone()
    assert calls[0] == pmg.matvecs_per_apply == 6                                  # 2 degree
    assert torch.equal(pmg.apply(r), z)                                            # two applies, the same bits
    buf = r.clone()
    pmg.apply(buf, out=buf)                                                        # r == z
    assert torch.equal(buf, z)
    for e in (-40, 3, 37):                                                         # M(2^e r) = 2^e M(r) bit for bit
        assert torch.equal(pmg.apply(r * 2.0 ** e), z * 2.0 ** e)
    Ms = pmg.apply(s)
    asym = abs(float(z @ s) - float(r @ Ms)) / (float(torch.linalg.norm(z)) * float(torch.linalg.norm(s)))
    print(f"tri6_v: |<M r, s> - <r, M s>| = {asym:.3e} |M r| |s|")
    assert asym <= 1e-12
    # a new smoother needs a new setup
    pmg.set_smoother(degree=2)
    with pytest.raises(ValueError, match="DXO_E_OPTION"):
        pmg.apply(r)
    from dolfinx_external_operator_amd import cg

    with pytest.raises(ValueError, match="DXO_E_OPTION"):
        cg(S.A, r, M=pmg, rtol=1e-8)
    pmg.setup(S.A, S.dinv, amg)
    assert pmg.matvecs_per_apply == 4 and not torch.equal(pmg.apply(r), z)
    for bad in (dict(degree=0), dict(degree=9), dict(rho_iters=0), dict(lower=0.0), dict(lower=1.0), dict(safety=0.9)):
        with pytest.raises(ValueError, match="DXO_E_OPTION"):
            pmg.set_smoother(**bad)
    assert torch.isfinite(pmg.apply(r)).all()                                      # a refused setting changes nothing
    # what setup refuses
    with pytest.raises(ValueError, match="DXO_E_OPTION"):
        pmg.setup(S.A, S.dinv, S.Ac.amg(pmg.coarse_constrained, coarse_rows=10 ** 6, cycle="K"))
    with pytest.raises(ValueError, match="DXO_E_OPTION"):
        pmg.apply(r)                                                               # a failed setup leaves no valid one
    with pytest.raises(ValueError, match="DXO_E_SIZE"):
        pmg.setup(S.A, S.dinv, S.A.amg(S.dofs, coarse_rows=10 ** 6))                # a preconditioner of the fine size
    with pytest.raises(ValueError, match="DXO_E_SIZE"):
        pmg.setup(S.Ac, S.dinv, amg)                                               # an operator of the coarse size
    with pytest.raises(ValueError, match="DXO_E_DIM"):
        pmg.setup(S.A, S.dinv, BlockJacobi(ctx, 1, _cuda(np.ones(pmg.n_coarse))))  # block Jacobi of another block size
    other = systems("tri6_s")
    with pytest.raises(ValueError, match="DXO_E_(SIZE|DIM)"):
        pmg.setup(other.A, S.dinv, amg)
    with pytest.raises(TypeError):
        pmg.setup(S.A, S.dinv, None)
    # an exception in a callable comes back as it is
    def broken(v, out):
        raise KeyError("broken operator")

    with pytest.raises(KeyError, match="broken operator"):
        pmg.setup(broken, S.dinv, amg)
    pmg.setup(S.A, S.dinv, amg)
    assert torch.equal(pmg.apply(r), PMG_twin(ctx, S, amg).apply(r))               # two objects, the same bits


def PMG_twin(ctx, S, amg):
    from dolfinx_external_operator_amd import PMG

    return PMG(_transfer(S.W, S.ctf), S.bs, constrained=S.dofs, ctx=ctx).setup(S.A, S.dinv, amg)


# ---- Krylov
def test_krylov_with_the_cycle(ctx, systems):
    """cg, gmres and fgmres on the tetrahedron case to 1e-8: at most the reference's count (the same algorithm with the reference
    cycle, on the CPU) plus 2 for the order of rounding; CG below a fifth of its count under Jacobi."""
    from dolfinx_external_operator_amd import cg, fgmres, gmres

    _torch(ctx)
    S = systems("tet3")
    amg = S.dense_amg()
    S.pmg.setup(S.A, S.dinv, amg)
    inv64 = np.linalg.inv(S.Sc.toarray())
    ref = S.ref.setup(S.S, S.dinv_h, lambda rc: inv64 @ rc, rho=S.pmg.rho)
    b = np.random.Generator(np.random.PCG64(1)).normal(size=S.S.shape[0])
    bd = _cuda(b)
    want = {"cg": cg_ref(S.S, b, inv=ref.apply, rtol=1e-8, maxiter=200)[1],
            "gmres": gmres_ref(S.S, b, inv=ref.apply, m=30, rtol=1e-8, maxiter=200)[1],
            "fgmres": fgmres_ref(S.S, b, M=lambda r, j: ref.apply(r), m=30, rtol=1e-8, maxiter=200)[1]}
    got = {}
    for name, solver, kw in (("cg", cg, {}), ("gmres", gmres, dict(restart=30)), ("fgmres", fgmres, dict(restart=30))):
        out = solver(S.A, bd, M=S.pmg, rtol=1e-8, maxiter=200, check_every=1, **kw)
        got[name] = out.iterations
        assert out.converged, name
        assert np.linalg.norm(b - S.S @ out.x.cpu().numpy()) <= 1.01e-8 * np.linalg.norm(b), name
    jac = cg(S.A, bd, M=S.dinv, rtol=1e-8, maxiter=2000, check_every=1)
    print(f"tet3: iterations with the p-multigrid {got}, reference {want}; CG with Jacobi {jac.iterations}")
    for name in want:
        assert got[name] <= want[name] + 2, (name, got[name], want[name])
    assert jac.converged and got["cg"] < jac.iterations / 5, (got["cg"], jac.iterations)
    # the operator behind a callable, matrix-free style
    from dolfinx_external_operator_amd.krylov import csr_matvec

    def A(v, out):
        csr_matvec(S.A, v, out)

    S.pmg.setup(A, S.dinv, amg)
    out = cg(A, bd, M=S.pmg, rtol=1e-8, maxiter=200, check_every=1, ctx=ctx)
    assert out.converged and out.iterations == got["cg"]


# ---- capture
def test_capture_and_replay_of_apply(ctx, systems):
    torch = _torch(ctx)
    S = systems("tri6_v")
    amg = S.dense_amg()
    S.pmg.setup(S.A, S.dinv, amg)
    r = _cuda(np.random.Generator(np.random.PCG64(1)).normal(size=S.S.shape[0]))
    z_first = S.pmg.apply(r).clone()
    z = torch.zeros_like(r)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ctx.set_stream(s.cuda_stream)
            S.pmg.apply(r, out=z)
    torch.cuda.current_stream().wait_stream(s)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        z.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(z, z_first)
