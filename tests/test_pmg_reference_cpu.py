"""The algorithm behind dxo_pmg_* on the CPU, with the NumPy oracles and tests/pmg_reference.py (not gpu).

(1) The coarse matrix of the p-multigrid is a rediscretisation on the degree-1 element. For nested Lagrange spaces, the same rule and
the same coefficients it is P^T A P: phi1_v = sum_i W_iv phi2_i holds on the reference cell, so both are the same sums up to rounding.
(2) The reference cycle is a symmetric operator. (3) The CG counts of the experiment the feature was specified with (P2 tetrahedra 3^3,
eps / eps, isotropic C, the face z = 0 clamped, Chebyshev degree 2 on [0.1 rho, rho], rho from 10 power steps x 1.1, exact coarse
solve, tolerance 1e-8, a random right-hand side): 171 with Jacobi, 15 with the two-level cycle."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle.amg_oracle import U, forward_bound, vertex_transfer_ref
from oracle.form_oracle import apply_bcs, dense_ref
from oracle.krylov_oracle import cg_ref, elastic_C3
from pmg_reference import PmgRef, exact_inverse
from tools.synthetic import gauss_tensor_rule, structured_mesh, vertex_companion, with_rule

CASES = {"p2_tet3": ("tetrahedron", (3, 3, 3), False, 0.0), "q2_hex2": ("hexahedron", (2, 2, 2), True, 0.1)}
_CACHE = {}


def z0_dofs(m, bs=3):
    on = np.flatnonzero(np.abs(m.node_x[:, 2]) < 1e-12)
    return (on[:, None] * bs + np.arange(bs)).reshape(-1)


def case(name):
    """(mesh, companion, A raw, A_c raw, W, coarse_to_fine): eps / eps bs 3 on the mesh and on its degree-1 companion at the SAME rule."""
    if name not in _CACHE:
        cell, n, rule27, distort = CASES[name]
        m = structured_mesh(cell, n, 2, distort=distort, seed=2)
        if rule27:
            m = with_rule(m, *gauss_tensor_rule(cell, 3))
        mc = vertex_companion(m)
        C = elastic_C3(m.num_cells * m.nq)
        _CACHE[name] = (m, mc, dense_ref(m, "eps", "eps", 3, C), dense_ref(mc, "eps", "eps", 3, C)) + vertex_transfer_ref(m)
    return _CACHE[name]


def system(name):
    """(A with the face z = 0 clamped, its inverse diagonal, the reference object, the exact inverse of the rediscretised coarse matrix)"""
    m, mc, A, Ac, W, ctf = case(name)
    dofs = z0_dofs(m)
    ref = PmgRef(W, ctf, 3, dofs)
    Ab = apply_bcs(A, dofs, 1.0)
    assert np.array_equal(ref.coarse_constrained, z0_dofs(mc))                     # the clamped vertices are the clamped coarse nodes
    Acb = apply_bcs(Ac, ref.coarse_constrained, 1.0)
    return sp.csr_matrix(Ab), 1.0 / np.diag(Ab), ref, exact_inverse(Acb), Acb


@pytest.mark.parametrize("name", list(CASES))
def test_rediscretised_coarse_matrix_is_the_galerkin_product(name):
    """|A_c - P^T A P| entrywise against the rounding of three sums, each at most 4 K u (the same sum over absolute values)
    (forward_bound): (a) the triple product, K_c terms, absolute sum |P|^T |A| |P|; (b), (c) the two assemblies, (c) carried through
    |P|: an entry is a sum over at most `cells` cells, nq points and D^2 products B_k C_kl B_l; C is symmetric positive definite with
    non-negative entries, so per point |B_i|^T C |B_j| <= kappa sqrt((B_i^T C B_i)(B_j^T C B_j)), kappa = lambda_max / lambda_min of
    C, and by Cauchy-Schwarz over points and cells the absolute sum of entry (i, j) is at most kappa sqrt(A_ii A_jj). Altogether
    4 u (K_c |P|^T |A| |P| + K_asm kappa (sqrt(a_c a_c^T) + |P|^T (sqrt(a a^T) on the pattern of A) |P|)), a and a_c the diagonals."""
    m, mc, A, Ac, W, ctf = case(name)
    P = sp.kron(W, sp.identity(3), format="csr")
    G = (P.T @ sp.csr_matrix(A) @ P).toarray()
    Ce = elastic_C3(1)[0]
    ev = np.linalg.eigvalsh(Ce)
    kappa = ev[-1] / ev[0]
    cells = {"tetrahedron": 24, "hexahedron": 8}[m.cell]                         # cells around an interior vertex: the most of any node
    K_asm = cells * m.nq * Ce.size
    K_c = int((A != 0).sum(axis=1).max()) * int(np.diff(P.tocsc().indptr).max()) + 2
    aP = abs(P)
    S2 = kappa * np.sqrt(np.outer(np.diag(A), np.diag(A))) * (A != 0)
    S1 = kappa * np.sqrt(np.outer(np.diag(Ac), np.diag(Ac)))
    tol = forward_bound(K_c, (aP.T @ sp.csr_matrix(np.abs(A)) @ aP).toarray()) + forward_bound(K_asm, S1) + (aP.T @ sp.csr_matrix(forward_bound(K_asm, S2)) @ aP).toarray()
    diff = np.abs(Ac - G)
    print(f"{name}: max |A_c - P^T A P| {diff.max():.3e} of {np.abs(Ac).max():.3e}, the bound there {tol.reshape(-1)[diff.argmax()]:.3e}, u {U:.3e}")
    assert (diff <= tol).all(), (name, (diff - tol).max())
    assert tol.max() <= 1e-8 * np.abs(Ac).max()                                  # and the bound is tight enough to mean something
    # with the constraints: the masked P of the cycle gives the clamped rediscretisation but for the unit diagonal
    Ab, _, ref, _, Acb = system(name)
    Gb = (ref.P.T @ Ab @ ref.P).toarray()
    free = np.setdiff1d(np.arange(Acb.shape[0]), ref.coarse_constrained)
    assert (np.abs(Gb - Acb)[np.ix_(free, free)] <= tol[np.ix_(free, free)]).all()
    assert not Gb[ref.coarse_constrained].any() and not Gb[:, ref.coarse_constrained].any()


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_reference_cycle_is_symmetric(name, degree):
    Ab, dinv, ref, inv, _ = system(name)
    ref.setup(Ab, dinv, lambda rc: inv @ rc, degree=degree)
    rng = np.random.Generator(np.random.PCG64(3))
    r, s = rng.normal(size=Ab.shape[0]), rng.normal(size=Ab.shape[0])
    Mr, Ms = ref.apply(r), ref.apply(s)
    asym = abs(Mr @ s - r @ Ms) / (np.linalg.norm(Mr) * np.linalg.norm(s))
    print(f"{name} degree {degree}: |<M r, s> - <r, M s>| = {asym:.3e} |M r| |s|, rho {ref.rho:.4f}")
    assert asym <= 1e-12
    assert ref.calls == 2 * 2 * degree                                            # 2 degree operator calls per apply


def test_cg_counts_of_the_experiment():
    Ab, dinv, ref, inv, _ = system("p2_tet3")
    assert Ab.shape[0] == 1029
    ref.setup(Ab, dinv, lambda rc: inv @ rc)
    b = np.random.Generator(np.random.PCG64(1)).normal(size=Ab.shape[0])
    _, jac, jconv = cg_ref(Ab, b, inv=dinv, rtol=1e-8, maxiter=2000)
    x, its, conv = cg_ref(Ab, b, inv=ref.apply, rtol=1e-8, maxiter=200)
    print(f"p2_tet3: CG iterations with Jacobi {jac}, with the two-level cycle {its} (rediscretised coarse matrix, exact solve)")
    assert jconv and conv and np.linalg.norm(b - Ab @ x) <= 1.01e-8 * np.linalg.norm(b)
    assert jac >= 100 and its <= 20, (jac, its)
    # the Galerkin coarse matrix in its place: the same count to within one
    G = (ref.P.T @ Ab @ ref.P).toarray()
    G[ref.coarse_constrained, ref.coarse_constrained] = 1.0
    ginv = np.linalg.inv(G)
    ref.setup(Ab, dinv, lambda rc: ginv @ rc)
    _, gits, gconv = cg_ref(Ab, b, inv=ref.apply, rtol=1e-8, maxiter=200)
    print(f"p2_tet3: with the Galerkin coarse matrix {gits}")
    assert gconv and abs(gits - its) <= 1


def test_long_double_cycle_is_the_referee():
    """The float64 reference cycle against the same cycle in long double: the rounding of the reference itself, far below anything a
    wrong step would cause."""
    Ab, dinv, ref, inv, Acb = system("q2_hex2")
    inv_ld = exact_inverse(Acb, np.longdouble)
    r = np.random.Generator(np.random.PCG64(4)).normal(size=Ab.shape[0])
    ref.setup(Ab, dinv, lambda rc: inv @ rc)
    z = ref.apply(r)
    ref.coarse = lambda rc: inv_ld @ rc
    z_ld = ref.apply(r, dtype=np.longdouble)
    assert z_ld.dtype == np.longdouble
    err = float(np.abs(z - z_ld).max() / np.abs(z_ld).max())
    print(f"q2_hex2: float64 reference against long double {err:.3e} |z|_inf")
    assert err <= 1e-11
