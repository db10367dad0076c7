"""3-D Mohr-Coulomb on the CPU (not gpu): the host build of the six-component lane math (csrc/mc3_core.h) against the
reference-pinned plane-strain oracle (embedded and rotated), against the reference's algorithm restated for six components with
dual numbers (tests/helpers/mc3_referee.cpp, double and long double), and against finite differences of the frozen-count iterate."""
import ctypes as C

import numpy as np
import pytest

import mc3_cases as m3
from conftest import mc_compare_all, mc_path_increment, mc_tracing_inputs
from tools.mc_inputs import mc_elastic_matrices


@pytest.fixture(scope="module")
def aids(tmp_path_factory):
    """(lane math, referee, long-double referee, lane math library): test aids only, never shipped."""
    return m3.build_aids(tmp_path_factory.mktemp("mc3"))


@pytest.fixture(scope="module")
def rotated(oracle):
    return {(2, 0.0): m3.rotated_plane_strain(oracle, 6000, 2), (5, 0.3): m3.rotated_plane_strain(oracle, 6000, 5, shear=0.3)}


@pytest.mark.parametrize("seed,shear", [(2, 0.0), (5, 0.3)])
def test_plane_strain_embedded_gives_the_plane_strain_oracle(oracle, aids, seed, shear):
    """Zeros in components 4 and 5: counts, yielding, dlambda, sigma[:4] and C_tang[:4, :4] are the 2-D oracle's under mc_compare's
    bounds (mc_compare_all: the slowly converging points of the sheared set included), and the cross blocks are exactly zero."""
    lane = aids[0]
    deps, sn = mc_tracing_inputs(oracle, 6000, seed=seed, shear=shear)
    ref = oracle.mohr_coulomb(deps, sn, nthreads=8)
    Ct, s, it, y, nr, dl = lane(m3.embed(deps), m3.embed(sn))
    got = (np.ascontiguousarray(Ct[:, :4, :4]), np.ascontiguousarray(s[:, :4]), it, y, nr, dl)
    mc_compare_all(got, ref, f"mc3_core embedded vs 2-D oracle (seed {seed})", sn)
    assert np.all(Ct[:, :4, 4:] == 0.0) and np.all(Ct[:, 4:, :4] == 0.0)
    assert np.all(s[:, 4:] == 0.0)
    assert (ref[3] > 0).mean() > 0.2


@pytest.mark.parametrize("seed,shear", [(2, 0.0), (5, 0.3)])
def test_rotated_plane_strain_gives_the_rotated_oracle(aids, rotated, seed, shear):
    """R(Q) embed(deps), R(Q) embed(sigma_n) with a random Q per point must give R(Q) embed(sigma_2D) and R(Q) C R(Q)^T: all six
    components pinned to the 2-D oracle. Compared in the plane-strain frame (R^T C R, R^T sigma): the in-plane block against the
    oracle, the cross blocks against zero. Kept points (plastic, 2-D count the same at tol 2e-8 / 1e-8 / 5e-9): at least 85 % of the
    plastic ones, counts exact, tangent and stress under BOUND_*_ROTATED. The rest: counts within one, stress to 1e-7 of its scale.
    Measured (host lane math against the rotated long-double 2-D referee, n = 6000): kept 92.6 % (seed 2) and 87.8 % (seed 5);
    tangent 1.4e-14 / 1.8e-14 of its scale, stress 2.4e-15 / 2.0e-15 -> bounds 1.8e-13 and 2.4e-14 (mc3_cases.BOUND_*_ROTATED)."""
    lane = aids[0]
    c = rotated[(seed, shear)]
    ref, ld, kept, plastic = c["ref"], c["ld"], c["kept"], c["plastic"]
    share = kept.sum() / plastic.sum()
    print(f"kept {share:.4f} of {plastic.sum()} plastic points")
    assert share >= 0.85
    got = lane(c["deps6"], c["sn6"])
    Cb, sb = m3.back_rotated(c["R"], got)
    assert np.array_equal(got[2][kept], ref[2][kept])
    assert np.array_equal(ld[2][kept], ref[2][kept])               # the referee's own count is as robust there
    el = ~plastic
    assert np.array_equal(got[2][el], ref[2][el])
    scale_C, scale_s = np.max(np.abs(ld[0])), max(np.max(np.abs(ld[1])), 1.0)
    sel = kept | el
    errC = max(np.max(np.abs(Cb[sel][:, :4, :4] - ld[0][sel])), np.max(np.abs(Cb[sel][:, :4, 4:])), np.max(np.abs(Cb[sel][:, 4:, :4]))) / scale_C
    errS = max(np.max(np.abs(sb[sel][:, :4] - ld[1][sel])), np.max(np.abs(sb[sel][:, 4:]))) / scale_s
    print(f"measured: tangent {errC:.3e}, stress {errS:.3e}")
    assert errC <= m3.BOUND_C_ROTATED <= 1e-9 and errS <= m3.BOUND_S_ROTATED <= 1e-9
    # the double oracle itself, under mc_compare's 1e-9
    assert np.max(np.abs(Cb[sel][:, :4, :4] - ref[0][sel])) <= 1e-9 * scale_C
    rest = plastic & ~kept & (ref[2] < 30)
    assert np.max(np.abs(got[2][rest].astype(int) - ref[2][rest].astype(int))) <= 1
    assert np.max(np.abs(sb[rest][:, :4] - ref[1][rest])) <= 1e-7 * scale_s


@pytest.fixture(scope="module")
def general(aids):
    out = {}
    for name, kw in (("associated", {}), ("non_associated", m3.NON_ASSOCIATED)):
        deps, sn = m3.general_states(6000)
        out[name] = (deps, sn, kw, aids[1](deps, sn, nthreads=8, **kw), aids[2](deps, sn, nthreads=8, **kw))
    return out


@pytest.mark.parametrize("name", ["associated", "non_associated"])
def test_general_states_against_the_six_component_referee(aids, general, name):
    """deps and sigma_n with no common principal axis (the pool's points, each tensor under a rotation of its own), kept where the
    long-double referee converges in fewer than 30 iterations (at least 90 %). Counts exact against the double and the long-double
    referee; tangent and stress entry by entry under BOUND_*_GENERAL.
    Measured (host lane math against the long-double referee, n = 6000): kept 100 %; tangent 1.1e-14 (associated) / 1.8e-15
    (phi != psi) of its scale, stress 1.7e-15 / 5.7e-16 -> bounds 1.1e-13 and 1.7e-14 (mc3_cases.BOUND_*_GENERAL). The double referee
    itself is 1.8e-13 away from the long-double one on the tangent (the reference's asin chain), so against it the lane math is held
    to mc_compare's bounds, 1e-9 and 1e-12."""
    lane = aids[0]
    deps, sn, kw, rd, rl = general[name]
    keep = rl[2] < 30
    print(f"kept {keep.mean():.4f}; plastic {(rl[3] > 0).mean():.3f}; iterations {np.bincount(rl[2][keep])}")
    assert keep.mean() >= 0.90 and (rl[3] > 0).mean() > 0.1
    got = lane(deps, sn, **kw)
    assert np.array_equal(got[2][keep], rl[2][keep]) and np.array_equal(got[2][keep], rd[2][keep])
    eC, eS = m3.rel_errors(got, rl, keep)
    dC, dS = m3.rel_errors(rd, rl, keep)
    print(f"measured: lane math tangent {eC:.3e}, stress {eS:.3e}; double referee tangent {dC:.3e}, stress {dS:.3e}")
    assert eC <= m3.BOUND_C_GENERAL <= 1e-9 and eS <= m3.BOUND_S_GENERAL <= 1e-9
    gC, gS = m3.rel_errors(got, rd, keep)
    assert gC <= 1e-9 and gS <= 1e-12
    assert np.max(np.abs(got[5][keep] - rd[5][keep])) <= 1e-12
    fin = np.isfinite(rd[3])
    assert np.array_equal(fin, np.isfinite(got[3])) and np.max(np.abs(got[3][fin] - rd[3][fin])) <= 1e-12 * max(np.max(np.abs(rd[3][fin])), 1.0)


def test_tangent_is_the_derivative_of_the_K_th_newton_iterate(aids):
    """Forward mode through the loop differentiates the ITERATES: where the loop ends after K steps, C_tang is the derivative of the
    K-th iterate with the count frozen. The frozen map is the referee with tol = 0 and nitermax = K; its central difference in each
    of the six strain directions must give the lane math's tangent. Bound 2e-8 as in the plane-strain test.
    Measured differencing noise in six dimensions: 2.4e-10 (below the bound, which therefore stands)."""
    lane, ref = aids[0], aids[1]
    deps, sn = m3.general_states(400, seed=11)
    Ct, s, it, y, nr, dl = lane(deps, sn)
    pick = np.flatnonzero((y > 0) & (it >= 2) & (it <= 6))[:30]
    assert pick.size >= 20
    worst = 0.0
    for i in pick:
        K = int(it[i])
        fd = np.empty((6, 6))
        for j in range(6):
            h = 1e-6 * max(1e-3, abs(deps[i, j]))
            dp_, dm_ = deps[i].copy(), deps[i].copy()
            dp_[j] += h
            dm_[j] -= h
            sp = ref(dp_[None], sn[i][None], tol=0.0, nitermax=K)
            sm = ref(dm_[None], sn[i][None], tol=0.0, nitermax=K)
            assert sp[2][0] == K and sm[2][0] == K
            fd[:, j] = (sp[1][0] - sm[1][0]) / (2 * h)
        err = np.max(np.abs(fd - Ct[i])) / np.max(np.abs(Ct[i]))
        worst = max(worst, err)
        assert err < 2e-8, (i, K, err)
    print(f"measured: worst {worst:.3e}")
    assert worst > 0.0


def test_dense_matrices_against_the_structured_operators(aids):
    """hess(g) and T(t) as dense symmetric 6x6 matrices against the literal chain-rule operators kept beside them: the same H v and
    T(t) v to rounding, non-associated flow, both Abbo-Sloan branches, every one of the six components non-zero."""
    from oracle.loader import mc_params

    lib = aids[3]
    lib.mc3_dense_vs_structured.argtypes = [C.c_void_p] * 5
    _, sn = m3.general_states(400, seed=21)
    prm = mc_params(psi=20 * np.pi / 180)
    rng = np.random.default_rng(3)
    worst, branches = 0.0, set()
    for i in range(sn.shape[0]):
        sig = np.ascontiguousarray(sn[i] + rng.normal(size=6) * 0.3)
        assert np.all(sig != 0.0)
        t, v = rng.normal(size=6), rng.normal(size=6)
        out = np.zeros(24)
        lib.mc3_dense_vs_structured(C.byref(prm), sig.ctypes.data, t.ctypes.data, v.ctypes.data, out.ctypes.data)
        if not np.all(np.isfinite(out)):
            continue
        T = m3.to_tensor(sig)
        dv = T - np.trace(T) / 3.0 * np.eye(3)
        arg = -(3.0 * np.sqrt(3.0) * np.linalg.det(dv)) / (2.0 * (0.5 * np.sum(dv * dv)) ** 1.5)
        branches.add(bool(abs(np.arcsin(np.clip(arg, -1, 1)) / 3.0) > 26 * np.pi / 180))
        for a, b in ((out[0:6], out[6:12]), (out[12:18], out[18:24])):
            worst = max(worst, np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300))
    assert branches == {False, True}
    assert worst < 1e-11, worst


def test_returned_stress_lies_on_the_surface_of_the_numpy_tensor_function(aids):
    """A 3-D tracing path: the demo's nine loads turned by a fixed rotation per path. After the return the stress sits on f = 0, with
    f evaluated in NumPy from the 3x3 tensor (J2 = tr s^2 / 2, J3 = det s), independently of the component formulas of mc3_core.h."""
    lane = aids[0]
    _, S = mc_elastic_matrices()
    n_angles = 50
    theta = np.linspace(-np.pi / 6 + 1e-5, np.pi / 6 - 1e-5, n_angles)
    R = m3.mandel_rotation(m3.rotations(n_angles, 77))
    tr = np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0])
    sn = np.zeros((n_angles, 6))
    sn[:, :3] = 0.1
    saw_plastic = False
    for load in range(9):
        d = m3.rotate_vec(R, m3.embed(mc_path_increment(theta, 0.7) @ S.T))
        _, s, it, y, nr, dl = lane(d, sn)
        plastic = y > 0
        saw_plastic |= plastic.any()
        assert np.all(np.abs(s[:, 3:]).max(axis=0) > 0.0)            # all three shears are in play
        assert np.all(np.abs(m3.surface_np(s[plastic])) < 1e-7)
        assert np.allclose(m3.surface_np(d @ m3.c_elas6().T + sn), y, rtol=0, atol=1e-10)
        assert np.all(it[~plastic] == 1) and it.max() <= 6
        sn = s - np.outer(s @ tr / 3.0 - 0.1, tr)
    assert saw_plastic


def test_elastic_zero_and_hydrostatic_points(aids):
    lane, ref = aids[0], aids[1]
    Cel = m3.c_elas6()
    rng = np.random.default_rng(0)
    deps = rng.normal(0, 1e-6, (200, 6))
    sn = np.tile([-1.0, -1.2, -0.8, 0.1, 0.05, -0.07], (200, 1))
    for run in (lane, ref):
        Ct, s, it, y, nr, dl = run(deps, sn)
        assert np.all(it == 1) and np.all(y < 0) and np.all(dl == 0)
        assert np.array_equal(Ct, np.broadcast_to(Cel, Ct.shape))
        assert np.allclose(s, sn + deps @ Cel.T, rtol=0, atol=1e-15)
        # deps == 0: 0/0 > tol is false, zero iterations, C_tang = 0
        Ct, s, it, y, nr, dl = run(np.zeros((1, 6)), np.array([[0.1, 0.2, 0.1, 0.01, 0.0, 0.02]]))
        assert it[0] == 0 and np.all(Ct == 0.0) and np.array_equal(s[0], [0.1, 0.2, 0.1, 0.01, 0.0, 0.02])
        # hydrostatic trial stress: J2 = 0, f = NaN, the plastic branch
        with np.errstate(all="ignore"):
            Ct, s, it, y, nr, dl = run(np.array([[1e-3, 1e-3, 1e-3, 0, 0, 0]]), np.array([[1.0, 1.0, 1.0, 0, 0, 0]]))
        assert np.isnan(y[0])
