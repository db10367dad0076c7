"""The NumPy yardstick of the compressed Krylov basis (dxo_krylov_create_basis, DXO_KRYLOV_BASIS_FP32), pinned on the CPU.

gmres_cb_ref is gmres_ref of tests/test_krylov_oracle_cpu.py with every stored basis vector passed through float32: the vector is
rounded once, the rounded vector is what is stored, what the preconditioner and the operator are given at the next step and what the
update combines. Everything else (dot products, updates, the Hessenberg matrix, the rotations, x, the true residual at a restart)
stays float64. On a family whose basis vectors are unit vectors it must be gmres_ref bit for bit; elsewhere it converges on the true
residual with at most one cycle more. Its own deviation from the long-double answers of F2 is measured here and recorded as
REF_CB_F2_*; tests/test_krylov_fp32_basis_gpu.py holds the device to MARGIN x these."""
import numpy as np

from oracle.krylov_oracle import (F2_D, F2_MAIN, REF_CB_F2_RES, REF_CB_F2_X, SHIFT_D, U, block_jacobi_ref, cyclic_shift_src, eps_matrix,
                                  f2_problem, gmres_cb_ref, gmres_ref, heat_matrix, same, shift_op, shifted_op, shifted_residual,
                                  to_pattern_csr, unit_rhs, xdev)

U32 = 2.0 ** -24                                        # unit roundoff of float32


def test_unit_vector_bases_give_gmres_ref_bit_for_bit():
    for d in SHIFT_D:
        for q, t in ((1, 0), (31, 0), (3, 2)):
            src = cyclic_shift_src(d, q, t)
            n = src.size
            for s in (t, n - 1):                               # on the first cycle and on the last one
                b, P = unit_rhs(n, s), shift_op(src)
                for m, reorth, maxiter in ((64, True, 1000), (d, True, 1000), (64, False, 1000), (max(d - 1, 1), True, 3 * d)):
                    ref = gmres_ref(P, b, m=m, reorth=reorth, maxiter=maxiter, full=True)
                    rows = []
                    got = gmres_cb_ref(P, b, m=m, reorth=reorth, maxiter=maxiter, full=True, basis=rows)
                    assert same(got, ref), (d, q, t, s, m, reorth)
                    if m >= d:
                        assert ref[1:4] == (d, True, 0.0)
                        pos = s                                # row j is P^j e_s = e_i with src[i] the position of row j - 1
                        for j in range(d):
                            e = np.zeros(n, np.float32)
                            e[pos] = 1.0
                            assert np.array_equal(rows[0][j], e), (d, s, j)
                            pos = int(np.flatnonzero(src == pos)[0])


def _systems():
    yield "heat", 1, *heat_matrix()
    yield "eps", 2, *eps_matrix()


def test_it_converges_on_the_true_residual_with_at_most_one_cycle_more():
    rtol = 1e-10
    src, b, A = f2_problem(*F2_MAIN)
    for m in (30, 64):
        x, its, conv, res = gmres_cb_ref(A, b, m=m, rtol=rtol, maxiter=2000)
        _, its64, conv64, _ = gmres_ref(A, b, m=m, rtol=rtol, maxiter=2000)
        true = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
        print(f"F2 restart {m}: iterations fp32 / fp64 basis {its} / {its64}, |b - A x| / |b| {true:.3e}")
        assert conv and conv64 and true <= rtol and res == true
        assert its <= its64 + m, (m, its, its64)
    bounded = 0
    for name, bs, mesh, Ad in _systems():
        S = to_pattern_csr(mesh, Ad, bs)
        b = np.random.Generator(np.random.PCG64(1)).normal(size=S.shape[0])
        for inv in (None, block_jacobi_ref(S, bs)):
            for m in (5, 30):
                x, its, conv, res = gmres_cb_ref(S, b, inv=inv, m=m, rtol=rtol, maxiter=10000)
                _, its64, conv64, _ = gmres_ref(S, b, inv=inv, m=m, rtol=rtol, maxiter=10000)
                true = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
                print(f"{name} restart {m}, M {'none' if inv is None else 'block Jacobi'}: iterations fp32 / fp64 basis {its} / {its64}, "
                      f"|b - A x| / |b| {true:.3e}")
                assert conv and conv64 and true <= rtol * (1 + 1e-6), (name, m, true)
                # One cycle more at the most, wherever a cycle gains digits. A solve that creeps over more than 20 cycles does not:
                # GMRES(5) on the (eps, eps) matrix takes 260 to 670 cycles at a few per cent each, a history that any perturbation
                # reshapes (measured here: 5181 iterations against 3327 without a preconditioner, 1405 against 1296 with block
                # Jacobi, 773 against 797 for GMRES(30) without one). There the count is printed and only the convergence is asserted.
                creeping = its64 > 20 * m
                bounded += not creeping
                assert creeping or its <= its64 + m, (name, m, its, its64)
    assert bounded >= 5                                       # heat: all four; (eps, eps): GMRES(30) with block Jacobi


def test_reference_deviation_of_the_compressed_basis():
    """gmres_cb_ref against the closed form (residual) and against gmres_ref in long double (x_k) on F2: what REF_CB_F2_* bound."""
    L = np.longdouble
    src, b, A = f2_problem(*F2_MAIN)
    worst_r = worst_x = 0.0
    for k in range(1, 65):
        x, its, conv, res, brk, cycles = gmres_cb_ref(A, b, m=64, rtol=0.0, maxiter=k, full=True)
        assert (its, conv, brk, cycles) == (k, False, False, 1)
        xl, _, _, resl = gmres_ref(shifted_op(src), b.astype(L), m=64, rtol=0.0, maxiter=k, dtype=L)
        f = shifted_residual(k)
        assert abs(resl - f) <= 1e-17 * f
        worst_r, worst_x = max(worst_r, float(abs(res - f) / f)), max(worst_x, xdev(x, xl.astype(float)))
    print(f"F2 compressed-basis reference deviation: residual {worst_r:.2e} relative, x {worst_x:.2e} max|x|")
    assert worst_r <= REF_CB_F2_RES and worst_x <= REF_CB_F2_X
    assert worst_x >= 0.01 * U32 > 100 * U                    # the rounding of the basis is what it measures, not float64's
    assert F2_D > 64
