"""The scaling laws of the multigrid (csrc/amg.hip), which need no oracle: every operation of the setup and of a cycle commutes exactly
with a power of two while nothing leaves the range of its number format, so on every variant of the hierarchy

    the matrix law           2^e A has the omega, rho, strength masks, aggregates and P of A, its coarse matrices times 2^e and its
                             Dinv, Dinv_F and z times 2^-e, bit for bit;
    the right-hand-side law  apply(2^e r) == 2^e apply(r), bit for bit and finite. The K-cycle is not linear, but its coefficients are
                             ratios of dot products: it is homogeneous of degree one all the same;

and a closed form: a right-hand side on the constrained dofs alone never reaches a coarse level (their rows of P are zero), so z is
the smoother's polynomial on a decoupled dof, and every K solve below takes its rho1 == 0 branch inside a non-trivial apply.

The reference of every law is the same object at scale 1; all comparisons are exact but the closed form, whose bound is counted."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle.amg_oracle import U, cheby_pairs, cheby_ref
from solver_cases import (CASES, GPU_THETAS, _case_hierarchy, _case_system, _cuda, _soc_snapshot, _soc_system, _torch,
                          meshes)  # noqa: F401  (meshes is a fixture)

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
WIDE = (996, -900)                     # about 1e300 and 1e-271: the ends of double
BREAKS = (996, -900, 520, -540)        # and where squared block norms first overflow / underflow
CHEBY_INF = dict(smoother="chebyshev", degree=2)
CHEBY_POWER = dict(smoother="chebyshev", degree=2, rho="power")

# (variant, system, keywords on top of the system's own, exponents). The fp32 exponents stay inside float's range
MATRIX_LAW = (
    [("cheby_power", "heat48_cheby", {}, WIDE)]
    + [("cheby_inf", w, CHEBY_INF, WIDE) for w in ("heat48", "hex_bar")]
    + [("soc", w, {}, BREAKS) for w in ("aniso_soc", "aniso_tri", "p2_tri_rbm", "hex_rbm")]
    + [("soc_cheby_power", "aniso_tri", CHEBY_POWER, WIDE)]
    + [("k", w, dict(cycle="K"), WIDE) for w in ("heat48", "hex_bar", "aniso_soc")]
    + [("fp32", w, dict(precision="fp32"), (40, -40)) for w in ("heat48", "hex_bar", "heat48_cheby")])


def _case(ctx, meshes, which):
    """(DeviceCSR, constrained dofs, keywords): the cases of test_amg_kcycle_gpu.py and the systems of test_amg_soc_gpu.py."""
    if which in CASES:
        return _case_system(ctx, meshes, which)
    A, bs, bcs, B, cr = _soc_system(ctx, meshes, which)
    return A, bcs, dict(coarse_rows=cr, near_nullspace=B, strength=GPU_THETAS[which])


def _state(amg, r):
    nl = amg.n_levels
    dev = amg.levels
    return dict(snapshot=_soc_snapshot(amg), shape=[(d["rows"], d["bs"]) for d in dev], rho=amg.rho, unlumped=amg.unlumped_nodes,
                dinv=[amg.level_dinv(l) for l in range(nl - 1)], dinv_f=[amg.level_dinv_f(l) for l in range(nl - 1)],
                z=amg.apply(r).clone())


def _same_pattern(a, b):
    return a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)


@pytest.mark.parametrize("variant,which,kw,exponents", MATRIX_LAW, ids=[f"{v}-{w}" for v, w, _, _ in MATRIX_LAW])
def test_matrix_law(ctx, meshes, variant, which, kw, exponents):
    from dolfinx_external_operator_amd.operand_eval import DeviceCSR

    torch = _torch(ctx)
    A, bcs, base = _case(ctx, meshes, which)
    r = _cuda(np.random.Generator(np.random.PCG64(4)).normal(size=A.shape[0]))
    one = A.amg(bcs, **base, **kw)
    ref = _state(one, r)
    mats, Ps, masks, aggs, omegas = ref["snapshot"]
    assert one.n_levels >= 3 and torch.isfinite(ref["z"]).all().item()
    if "strength" in base:
        assert not masks[0].all() and all(d.size for d in ref["dinv_f"])           # a mask that can be lost
    for e in exponents:
        # a new object: a strength hierarchy freezes its masks at creation
        two = DeviceCSR(A.pattern, A.values * 2.0 ** e).amg(bcs, **base, **kw)
        got = _state(two, r)
        mats2, Ps2, masks2, aggs2, omegas2 = got["snapshot"]
        where = (variant, which, e)
        assert two.n_levels == one.n_levels and got["shape"] == ref["shape"], where
        assert omegas2 == omegas and got["rho"] == ref["rho"], (where, omegas2, omegas, got["rho"], ref["rho"])
        for l, (m1, m2) in enumerate(zip(masks, masks2)):
            assert np.array_equal(m1, m2), (where, l, int(m1.sum()), int(m2.sum()), m1.size)
        assert all(np.array_equal(a1, a2) for a1, a2 in zip(aggs, aggs2)), where
        assert got["unlumped"] == ref["unlumped"], where
        for l, (p1, p2) in enumerate(zip(Ps, Ps2)):
            assert _same_pattern(p1, p2) and np.array_equal(p1.data, p2.data), (where, l)
        for l, (a1, a2) in enumerate(zip(mats, mats2)):
            assert _same_pattern(a1, a2) and np.array_equal(a2.data, np.ldexp(a1.data, e)), (where, l)
        for key in ("dinv", "dinv_f"):
            for l, (d1, d2) in enumerate(zip(ref[key], got[key])):
                assert d1.shape == d2.shape and np.array_equal(d2, np.ldexp(d1, -e)), (where, key, l)
        assert torch.equal(got["z"], ref["z"] * 2.0 ** -e), where


RHS_LAW = ([("jacobi", w, {}, (900, -900)) for w in ("heat48", "p2_rbm", "hex_bar", "aniso_soc")]
           + [("cheby", "heat48_cheby", {}, (900, -900))]
           + [("fp32", w, dict(precision="fp32"), (40, -40)) for w in ("heat48", "hex_bar")]
           + [("k", w, dict(cycle="K"), (300, -300, 400, -400)) for w in ("heat48", "hex_bar", "aniso_soc", "heat48_cheby")])


@pytest.mark.parametrize("variant,which,kw,exponents", RHS_LAW, ids=[f"{v}-{w}" for v, w, _, _ in RHS_LAW])
def test_right_hand_side_law(ctx, meshes, variant, which, kw, exponents):
    torch = _torch(ctx)
    A, amg = _case_hierarchy(ctx, meshes, which, **kw)
    assert amg.n_levels >= 3
    r = _cuda(np.random.Generator(np.random.PCG64(6)).normal(size=A.shape[0]))
    z = amg.apply(r).clone()
    assert torch.isfinite(z).all().item() and z.any().item()
    for e in exponents:
        ze = amg.apply(r * 2.0 ** e)
        assert torch.isfinite(ze).all().item(), (variant, which, e)
        worst = ((ze * 2.0 ** -e - z).abs().max() / z.abs().max()).item()
        assert torch.equal(ze, z * 2.0 ** e), (variant, which, e, f"largest deviation {worst:.3e} of max |z|")


def _decoupled(A, bcs):
    """The diagonal entries of the constrained dofs, after checking that their rows and columns hold nothing else."""
    S = A.to_scipy().tocsr()
    D = S.diagonal()
    off = (S - sp.diags(D)).tocsr()
    assert abs(off[bcs]).sum() == 0.0 and abs(off[:, bcs]).sum() == 0.0
    assert (D[bcs] != 0.0).all()
    return D[bcs]


@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("which", ["heat48", "aniso_soc", "p2_rbm"])
def test_right_hand_side_on_the_constrained_dofs_jacobi(ctx, meshes, which, sweeps):
    """r is non-zero on the constrained dofs alone. Their rows and columns hold the diagonal entry d only and their rows of P are
    zero, so the residual restricted to level 1 is exactly 0, every K solve returns through rho1 == 0, and z is zero but for
    z_b = (1 - (1 - omega)^(2 nu)) r_b / d, the 2 nu damped Jacobi steps on a decoupled dof.

    The bound, counted. A step is acc = d x (1 rounding), res = r - acc (1), s = dinv res (1, and 1 for dinv = 1 / d itself),
    x = fma(omega, s, x) (1): 5 roundings, 2 nu steps. omega = (4/3) / rho with rho >= 1 (the row of a constrained dof alone gives
    |Dinv A|_inf >= 1), so |1 - omega| <= 1: an error made in x is not amplified by the later steps, |res| <= |r| and
    |x| <= (4/3) |r / d|, and each rounding adds at most (4/3) u |r / d|. The closed form evaluated here in double adds 6 more
    (1 - omega, the power, 1 - it, the product and the quotient, the power counted twice). Under fp32 the same count in units of
    2^-24, with 4 for the narrowing of r, omega, dinv and d and 2 nu for the narrowed omega acting in every step."""
    torch = _torch(ctx)
    A, bcs, base = _case_system(ctx, meshes, which)
    bcs = np.asarray(bcs)
    d = _decoupled(A, bcs)
    rb = np.random.Generator(np.random.PCG64(8)).normal(size=bcs.size)
    r = np.zeros(A.shape[0])
    r[bcs] = rb
    interior = np.ones(A.shape[0], dtype=bool)
    interior[bcs] = False
    amg = A.amg(bcs, sweeps=sweeps, **base)
    assert amg.n_levels >= 3 and amg.cycle == "V"
    omega = amg.levels[0]["omega"]
    assert 0.0 < omega <= 4.0 / 3.0
    exact = (1.0 - (1.0 - omega) ** (2 * sweeps)) * rb / d
    count = 5 * 2 * sweeps + 6
    z_v = amg.apply(_cuda(r)).clone()
    z = z_v.cpu().numpy()
    err = np.abs(z[bcs] - exact) / np.abs(rb / d)
    print(f"{which} sweeps {sweeps}: closed form missed by {err.max() / U:.2f} u at most (bound {4.0 / 3.0 * count:.0f} u)")
    assert not z[interior].any() and z[bcs].all()
    assert (err <= (4.0 / 3.0) * count * U).all(), (which, sweeps, err.max() / U)
    z_k = amg.set_cycle("K").apply(_cuda(r))
    assert amg.cycle == "K" and torch.equal(z_k, z_v)
    if which == "heat48":
        z32 = amg.set_cycle("V").set_precision("fp32").setup().apply(_cuda(r)).cpu().numpy()
        err = np.abs(z32[bcs] - exact) / np.abs(rb / d)
        count32 = count + 4 + 2 * sweeps
        print(f"{which} sweeps {sweeps} fp32: closed form missed by {err.max() / U32:.2f} 2^-24 at most (bound {4.0 / 3.0 * count32:.0f})")
        assert amg.precision == "fp32" and not z32[interior].any()
        assert (err <= (4.0 / 3.0) * count32 * U32).all(), (which, sweeps, err.max() / U32)


@pytest.mark.parametrize("degree", [1, 2])
def test_right_hand_side_on_the_constrained_dofs_chebyshev(ctx, meshes, degree):
    """The same with the Chebyshev smoother: z_b = (1 - p(1)^2) r_b / d, p the polynomial of one smoothing at the eigenvalue 1 of
    Dinv A on a decoupled dof. It is taken from the scalar recurrence of cheby_ref on the 1 x 1 system (d), run as the cycle runs it
    (from zero, then again from its result) with the device's rho and lower.

    The bound, counted. A step is acc = d x, res = r - acc, s = dinv res (and dinv's own rounding), c1 d_k, the fma with c2, x + d_k:
    7 roundings, and 2 for the device's pair (c1, c2) against the oracle's: 9, in 2 degree steps, and as many in the recurrence
    evaluated here. 1 lies in [lower rho, rho] (asserted), so |p_k(1)| <= 1, |res| <= |r|, |x| <= 2 |r / d| and a direction is at most
    c |r / d| with c = max(1, max c2): a rounding adds at most 2 c u |r / d|. A perturbation of x_k reaches the end through a
    polynomial of degree at most the remaining steps, which a three-term recurrence bounds on its interval by that number of
    steps: a factor 2 degree at most."""
    torch = _torch(ctx)
    A, bcs, base = _case_system(ctx, meshes, "heat48_cheby")
    base = dict(base, degree=degree)
    bcs = np.asarray(bcs)
    d = _decoupled(A, bcs)
    rb = np.random.Generator(np.random.PCG64(8)).normal(size=bcs.size)
    r = np.zeros(A.shape[0])
    r[bcs] = rb
    interior = np.ones(A.shape[0], dtype=bool)
    interior[bcs] = False
    amg = A.amg(bcs, **base)
    sm = amg.smoother
    rho, lower = amg.rho[0], sm["lower"]
    assert amg.n_levels >= 3 and sm["smoother"] == "chebyshev" and sm["degree"] == degree
    assert lower * rho <= 1.0 <= rho, (rho, lower)
    exact = np.empty(bcs.size)
    for i in range(bcs.size):
        S1, D1, r1 = np.array([[d[i]]]), np.array([[[1.0 / d[i]]]]), np.array([rb[i]])
        exact[i] = cheby_ref(S1, D1, rho, lower, degree, r1, cheby_ref(S1, D1, rho, lower, degree, r1))[0]
    c = max(1.0, max(c2 for _, c2 in cheby_pairs(rho, lower, degree)))
    bound = 2 * degree * 2 * c * (2 * 9 * 2 * degree) * U
    z_v = amg.apply(_cuda(r)).clone()
    z = z_v.cpu().numpy()
    err = np.abs(z[bcs] - exact) / np.abs(rb / d)
    print(f"heat48_cheby degree {degree}: closed form missed by {err.max() / U:.2f} u at most (bound {bound / U:.0f} u)")
    assert not z[interior].any() and z[bcs].all()
    assert (err <= bound).all(), (degree, err.max() / U)
    assert torch.equal(amg.set_cycle("K").apply(_cuda(r)), z_v)
