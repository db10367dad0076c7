"""The NumPy yardstick of dxo_csr_create / dxo_bilinear_assemble, pinned on the CPU.

The pattern oracle is the definition: row node*bs + i holds the columns m*bs + j of every node m that shares a cell with the
row's node, sorted. The dense matrix oracle is built from the pinned composition of tests/test_bilinear_oracle_cpu.py: column j
of A is bilinear_ref(e_j), taken many columns at a time by probes over a distance-2 colouring of the nodes (two nodes of one
colour share no neighbour, so every row sees at most one of them). These tests pin the oracles against each other and against
what the reference's assembled Jacobians mean: symmetry for the Isihara tangent (demo_hyperelasticity.py) and, for the heat pair,
the dense matrix of the explicit Jacobian form (demo_nonlinear_heat_equation_part2.py:324-335)."""
import numpy as np

from oracle.form_oracle import apply_bcs, bilinear_ref, csr_to_dense, dense_by_probes, dense_ref, heat_setting, pattern_ref
from oracle.icnn_oracle import isihara_stress_tangent
from oracle.operand_oracle import DEFGRAD, eval_operand
from tools.synthetic import structured_mesh


def test_pattern_oracle_layout():
    for cell, n in (("triangle", (3, 2)), ("hexahedron", (2, 1, 1))):
        m = structured_mesh(cell, n, 2)
        for bs in (1, m.gdim):
            indptr, indices = pattern_ref(m, bs)
            nrows = m.node_x.shape[0] * bs
            assert indptr.size == nrows + 1 and indptr[-1] == indices.size
            dense = np.zeros((nrows, nrows), dtype=bool)
            for r in range(nrows):
                row = indices[indptr[r]:indptr[r + 1]]
                assert np.all(np.diff(row) > 0) and r in row
                dense[r, row] = True
            assert np.array_equal(dense, dense.T)             # one field: the pattern is symmetric
            # every (a, b) pair of every cell is in it
            for nodes in m.dofmap:
                for a in nodes:
                    for b in nodes:
                        assert dense[a * bs:(a + 1) * bs, b * bs:(b + 1) * bs].all()


def test_probes_equal_unit_columns():
    m = structured_mesh("quadrilateral", (2, 2), 2, distort=0.2, seed=1)
    rng = np.random.Generator(np.random.PCG64(1))
    C = rng.normal(size=(m.num_cells * m.nq, 4, 4))
    n = m.node_x.shape[0] * 2
    A = dense_ref(m, "grad", "grad", 2, C)
    full = np.stack([bilinear_ref(m, "grad", "grad", 2, C, np.eye(n)[j]) for j in range(n)], axis=1)
    assert np.array_equal(A, full)


def test_dense_oracle_lies_in_the_pattern():
    for cell, n, pair in (("triangle", (3, 3), ("grad", "value_grad", 1)), ("tetrahedron", (1, 1, 1), ("eps", "eps", 3))):
        m = structured_mesh(cell, n, 2, distort=0.2, seed=3)
        test, trial, bs = pair
        d = {"grad": bs * m.gdim, "value_grad": bs * (1 + m.gdim), "eps": 4 if m.gdim == 2 else 6}
        rng = np.random.Generator(np.random.PCG64(3))
        C = rng.normal(size=(m.num_cells * m.nq, d[test], d[trial]))
        A = dense_ref(m, test, trial, bs, C)
        indptr, indices = pattern_ref(m, bs)
        inside = csr_to_dense(indptr, indices, np.ones(indices.size), A.shape[0]) > 0
        assert np.count_nonzero(A[~inside]) == 0
        assert np.count_nonzero(A[inside]) > 0.5 * inside.sum()


def test_isihara_tangent_matrix_is_symmetric():
    m = structured_mesh("triangle", (3, 3), degree=2, distort=0.2, seed=0)
    rng = np.random.Generator(np.random.PCG64(0))
    u = 0.01 * rng.normal(size=m.node_x.shape[0] * 2)
    F = eval_operand(DEFGRAD, 2, u, m.dofmap, m.geom_dofmap, m.x, m.phi, m.dphi, m.dpsi).reshape(-1, 4)
    dP, _ = isihara_stress_tangent(F)
    A = dense_ref(m, "grad", "grad", 2, dP)
    assert np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max()


def test_heat_matrix_is_the_explicit_jacobian_matrix():
    m, dqdT, dqds, explicit = heat_setting()
    Cb = np.concatenate([dqdT[..., None], dqds], axis=-1).reshape(-1, 2, 3)     # [g][1 + g]
    A = dense_ref(m, "grad", "value_grad", 1, Cb)
    E = dense_by_probes(explicit, m, 1)
    assert np.abs(A - E).max() <= 1e-13 * np.abs(E).max()
    assert np.abs(A - A.T).max() > 1e-3 * np.abs(A).max()                 # the heat Jacobian is not symmetric


def test_bcs_oracle():
    A = np.arange(16.0).reshape(4, 4)
    B = apply_bcs(A, [1, 3], 2.5)
    assert B[1].tolist() == [0, 2.5, 0, 0] and B[:, 3].tolist() == [0, 0, 0, 2.5] and B[0, 0] == 0 and B[2, 2] == 10
