"""The NumPy / SciPy yardstick of dxo_amg_set_smoother (csrc/amg.hip): the power-iteration estimate of rho and Chebyshev smoothing,
pinned on the CPU (oracle/amg_oracle.py).

power_rho_ref: rho = safety |w_m| after m steps w_k = Dinv A (w_{k-1} / |w_{k-1}|) from the fixed start vector
w_0[i] = 0.5 + ((uint32)(i * 2654435761) >> 8) * 2^-24, which is exact in float64. cheby_ref: the polynomial of degree k in Dinv A on
[lower rho, rho], by the recurrence of the device. amg_ref(rho="power") takes rho (and with it omega of the prolongator smoothing)
from the selected estimate; cycle_ref runs the selected smoother before and after the coarse correction."""
import numpy as np
import pytest
import scipy.sparse.linalg

from oracle.amg_oracle import (LOWER, U, amg_ref, apply_block, block_diag, cg_with_cycle, cheby_ref, cycle_ref, gmres_with_cycle,
                               power_rho_ref, rho_ref, rigid_body_modes_ref, start_vector)
from oracle.krylov_oracle import bottom_dofs, boundary_dofs, eps_matrix, heat_matrix, to_pattern_csr
from solver_cases import eps_spd


def eps_system(nonsym_seed):
    m, A = eps_matrix((14, 14), nonsym_seed=nonsym_seed)
    return to_pattern_csr(m, A, 2), 2, bottom_dofs(m, 2)


# ---- tests
def test_start_vector_is_exact_and_fixed():
    v = start_vector(5000)
    assert (v >= 0.5).all() and (v < 1.5).all() and np.unique(v).size > 4000
    assert np.array_equal((v - 0.5) * 2.0 ** 24, np.round((v - 0.5) * 2.0 ** 24))          # 24 bits below the point: exact
    assert v[0] == 0.5 and v[1] == 0.5 + (2654435761 >> 8) * 2.0 ** -24
    assert v[3] == 0.5 + (((3 * 2654435761) % 2 ** 32) >> 8) * 2.0 ** -24                  # the product wraps as a uint32


def test_jacobi_with_the_inf_norm_is_the_cycle_of_today():
    S, bs, dofs = eps_system(3)
    r = np.random.Generator(np.random.PCG64(4)).normal(size=S.shape[0])
    for sweeps in (1, 2):
        levels = amg_ref(S, bs, dofs, smoother="jacobi", rho="inf-norm", coarse_rows=60, sweeps=sweeps)
        assert np.array_equal(cycle_ref(levels, r), cycle_ref(amg_ref(S, bs, dofs, coarse_rows=60, sweeps=sweeps), r))


def test_degree_one_is_a_damped_jacobi_sweep():
    """theta = (1 + lower) rho / 2, so degree 1 is x += omega Dinv (r - A x) with omega = 2 / ((1 + lower) rho)."""
    S, bs, dofs = eps_system(3)
    rng = np.random.Generator(np.random.PCG64(6))
    r, x0 = rng.normal(size=(2, S.shape[0]))
    L = amg_ref(S, bs, dofs, smoother="chebyshev", rho="power", coarse_rows=60)[0]
    for lower in (0.1, 0.3):
        omega = 2.0 / ((1.0 + lower) * L.rho)
        for start in (None, x0):
            x = np.zeros_like(r) if start is None else start
            want = x + omega * apply_block(L.Dinv, r - L.A @ x)
            got = cheby_ref(L.A, L.Dinv, L.rho, lower, 1, r, start)
            assert np.linalg.norm(got - want) <= 8 * U * np.linalg.norm(want), lower
    # and the whole cycle of degree 1 is the Jacobi cycle with that omega
    levels = amg_ref(S, bs, dofs, smoother="chebyshev", rho="power", degree=1, coarse_rows=60)
    jac = amg_ref(S, bs, dofs, rho="power", smoother="jacobi", coarse_rows=60)
    for Lj in jac[:-1]:
        Lj.omega = 2.0 / ((1.0 + LOWER) * Lj.rho)       # the sweeps only: P keeps the omega it was built with
    z, zj = cycle_ref(levels, r), cycle_ref(jac, r)
    assert np.linalg.norm(z - zj) <= 1e-13 * np.linalg.norm(zj)


def test_polynomial_damps_the_interval():
    """On a diagonal matrix the error after degree k is the Chebyshev polynomial: at most 1 / T_k(sigma) on [lower rho, rho]."""
    lam = np.linspace(0.05, 2.0, 400)
    A = scipy.sparse.diags(lam).tocsr()
    Dinv = np.ones((lam.size, 1, 1))
    rho, lower = 2.0, 0.1
    sigma = (1 + lower) / (1 - lower)
    r = lam.copy()                                       # the solution is the vector of ones
    for k in (1, 2, 3, 5, 8):
        err = np.abs(1.0 - cheby_ref(A, Dinv, rho, lower, k, r))
        bound = 1.0 / np.cosh(k * np.arccosh(sigma))
        inside = lam >= lower * rho
        assert err[inside].max() <= bound * (1 + 1e-12), k
        assert err[inside].max() >= 0.99 * bound and (err[~inside] < 1.0).all(), k


def test_cycle_is_linear_and_symmetric_for_an_spd_matrix():
    rng = np.random.Generator(np.random.PCG64(11))
    m, A = eps_matrix(nonsym_seed=None)
    S = to_pattern_csr(m, A, 2)
    for degree in (1, 2, 3):
        levels = amg_ref(S, 2, bottom_dofs(m, 2), smoother="chebyshev", rho="power", degree=degree, coarse_rows=30)
        assert len(levels) >= 2
        r1, r2 = rng.normal(size=(2, S.shape[0]))
        z1, z2 = cycle_ref(levels, r1), cycle_ref(levels, r2)
        z = cycle_ref(levels, 2.5 * r1 + r2)
        assert np.linalg.norm(z - (2.5 * z1 + z2)) <= 1e-13 * np.linalg.norm(z)
        assert abs(r2 @ z1 - r1 @ z2) <= 1e-12 * (np.linalg.norm(r1) * np.linalg.norm(z2))
        assert r1 @ z1 > 0 and r2 @ z2 > 0
        x, its, conv = cg_with_cycle(S, r1, levels, rtol=1e-10)
        assert conv
        assert np.linalg.norm(x - scipy.sparse.linalg.spsolve(S.tocsc(), r1)) <= 1e-8 * np.linalg.norm(x)


def _radius_cases():
    m, A = heat_matrix(32)
    yield "heat32", to_pattern_csr(m, A, 1), 1, boundary_dofs(m, 1), 60
    m, A = heat_matrix(64)
    yield "heat64", to_pattern_csr(m, A, 1), 1, boundary_dofs(m, 1), 300
    yield ("eps14",) + eps_system(3) + (60,)
    yield ("eps14_spd",) + eps_system(None) + (60,)


def test_power_estimate_against_the_true_radius():
    """0.9 rho_true <= rho_power <= 1.1 |Dinv A|_inf on every level of at most 3000 rows. The estimate comes from below: ten steps
    times 1.1 can stay under the true radius (the smallest ratio here is 0.917, heat 32 x 32 level 1), which is why the lower
    factor is 0.9 and not 1."""
    smallest = np.inf
    for name, S, bs, dofs, coarse_rows in _radius_cases():
        levels = amg_ref(S, bs, dofs, smoother="chebyshev", rho="power", coarse_rows=coarse_rows)
        assert len(levels) >= 3, name
        checked = 0
        for l, L in enumerate(levels[:-1]):
            assert L.rho == power_rho_ref(L.A, L.Dinv) and L.omega == (4.0 / 3.0) / L.rho
            if L.n_rows > 3000:
                continue
            true = np.abs(np.linalg.eigvals((block_diag(L.Dinv) @ L.A).toarray())).max()
            inf_norm, _ = rho_ref(L.A, L.Dinv)
            print(f"{name} level {l}: rows {L.n_rows}, rho true {true:.4f}, power {L.rho:.4f} ({L.rho / true:.3f}), inf-norm {inf_norm:.4f}")
            assert 0.9 * true <= L.rho <= 1.1 * inf_norm, (name, l, true, L.rho, inf_norm)
            smallest = min(smallest, L.rho / true)
            checked += 1
        assert checked >= 1, name
    print(f"smallest rho_power / rho_true: {smallest:.3f}")


@pytest.mark.parametrize("spd", [False, True])
def test_chebyshev_with_the_power_estimate_needs_fewer_iterations(spd):
    """P2 eps/eps 14 x 14, rtol 1e-8, coarse_rows 60: degree 3 on the power estimate against 3 Jacobi sweeps on the infinity norm,
    the same SpMV work per cycle."""
    S, bs, dofs = eps_system(None if spd else 3)
    b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
    ref = scipy.sparse.linalg.spsolve(S.tocsc(), b)
    cheb = amg_ref(S, bs, dofs, smoother="chebyshev", rho="power", degree=3, coarse_rows=60)
    jac = amg_ref(S, bs, dofs, smoother="jacobi", rho="inf-norm", sweeps=3, coarse_rows=60)
    jac_power = amg_ref(S, bs, dofs, rho="power", smoother="jacobi", sweeps=3, coarse_rows=60)
    counts = []
    for levels in (cheb, jac_power, jac):
        if spd:
            x, its, conv = cg_with_cycle(S, b, levels, rtol=1e-8, maxiter=3000)
        else:
            x, its, conv, _ = gmres_with_cycle(S, b, levels, m=30, rtol=1e-8, maxiter=3000)
        assert conv and np.linalg.norm(x - ref) <= 1e-5 * np.linalg.norm(ref)
        counts.append(its)
    print(f"eps 14 x 14 {'CG' if spd else 'GMRES(30)'}: Chebyshev 3 / power {counts[0]}, Jacobi 3 / power {counts[1]}, "
          f"Jacobi 3 / inf-norm {counts[2]} iterations")
    assert counts[0] < counts[2], counts


def test_near_nullspace_levels_take_the_same_smoother():
    """Rigid-body modes: coarse levels of block size 3; the estimate and the polynomial run on them as on any level."""
    m, S, dofs = eps_spd((10, 10))
    B = rigid_body_modes_ref(m.node_x)
    levels = amg_ref(S, 2, dofs, smoother="chebyshev", rho="power", near_nullspace=B, degree=2, coarse_rows=40)
    assert len(levels) >= 3 and [L.bs for L in levels] == [2] + [3] * (len(levels) - 1)
    for L in levels[:-1]:
        assert L.rho == power_rho_ref(L.A, L.Dinv) and L.Dinv.shape[1] == L.bs
    b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
    _, its, conv = cg_with_cycle(S, b, levels, rtol=1e-8, maxiter=2000)
    plain = amg_ref(S, 2, dofs, near_nullspace=B, coarse_rows=40, sweeps=2)
    _, its_plain, conv_plain = cg_with_cycle(S, b, plain, rtol=1e-8, maxiter=2000)
    print(f"eps 10 x 10 with rigid-body modes, CG: Chebyshev 2 / power {its}, Jacobi 2 / inf-norm {its_plain} iterations")
    assert conv and conv_plain and its < its_plain
