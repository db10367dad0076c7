"""The NumPy yardstick of dxo_csr_create / dxo_bilinear_assemble, pinned on the CPU.

The pattern oracle is the definition: row node*bs + i holds the columns m*bs + j of every node m that shares a cell with the
row's node, sorted. The dense matrix oracle is built from the pinned composition of tests/test_bilinear_oracle_cpu.py: column j
of A is bilinear_ref(e_j), taken many columns at a time by probes over a distance-2 colouring of the nodes (two nodes of one
colour share no neighbour, so every row sees at most one of them). These tests pin the oracles against each other and against
what the reference's assembled Jacobians mean: symmetry for the Isihara tangent (demo_hyperelasticity.py) and, for the heat pair,
the dense matrix of the explicit Jacobian form (demo_nonlinear_heat_equation_part2.py:324-335)."""
import numpy as np

from oracle.icnn_oracle import isihara_stress_tangent
from oracle.operand_oracle import DEFGRAD, GRAD, VALUE, eval_operand, operand_adjoint
from test_bilinear_oracle_cpu import bilinear_ref
from tools.synthetic import structured_mesh


def node_neighbours(m):
    """Sorted neighbour nodes (sharing a cell, the node itself included) of every field node."""
    nn = m.node_x.shape[0]
    nb = [{n} for n in range(nn)]
    for nodes in m.dofmap:
        s = set(int(a) for a in nodes)
        for a in nodes:
            nb[a] |= s
    return [np.array(sorted(x), dtype=np.int64) for x in nb]


def pattern_ref(m, bs):
    """(indptr int64, indices int32) of the blocked pattern."""
    indptr, indices = [0], []
    for nbrs in node_neighbours(m):
        cols = (nbrs[:, None] * bs + np.arange(bs)[None, :]).reshape(-1)
        for _ in range(bs):
            indices.append(cols)
            indptr.append(indptr[-1] + cols.size)
    return np.array(indptr, dtype=np.int64), np.concatenate(indices).astype(np.int32)


def distance2_colours(m):
    """Greedy colouring of the field nodes in which two nodes with a common neighbour never share a colour."""
    nb = node_neighbours(m)
    colour = -np.ones(len(nb), dtype=np.int64)
    for a in range(len(nb)):
        taken = {colour[c] for b in nb[a] for c in nb[b]}
        k = 0
        while k in taken:
            k += 1
        colour[a] = k
    return colour, nb


def dense_by_probes(apply, m, bs):
    """Dense matrix of a linear map on the blocked dofs from probes over a distance-2 colouring."""
    colour, nb = distance2_colours(m)
    nn = len(nb)
    A = np.zeros((nn * bs, nn * bs))
    owner = np.zeros(nn, dtype=np.int64)
    for k in range(colour.max() + 1):
        sel = np.flatnonzero(colour == k)
        for n in sel:
            owner[nb[n]] = n          # every row node has at most one neighbour of colour k
        rows_hit = np.unique(np.concatenate([nb[n] for n in sel]))
        for j in range(bs):
            v = np.zeros((nn, bs))
            v[sel, j] = 1.0
            y = apply(v.reshape(-1)).reshape(nn, bs)
            for r in rows_hit:
                A[r * bs:(r + 1) * bs, owner[r] * bs + j] = y[r]
    return A


def dense_ref(m, test, trial, bs, C):
    return dense_by_probes(lambda v: bilinear_ref(m, test, trial, bs, C, v), m, bs)


def csr_to_dense(indptr, indices, values, n):
    A = np.zeros((n, n))
    for r in range(n):
        A[r, indices[indptr[r]:indptr[r + 1]]] += values[indptr[r]:indptr[r + 1]]
    return A


def apply_bcs(A, dofs, diagonal):
    """assemble_matrix(a, bcs, diagonal): constrained rows and columns zero, their diagonal entries `diagonal`."""
    B = A.copy()
    B[dofs, :] = 0.0
    B[:, dofs] = 0.0
    B[dofs, dofs] = diagonal
    return B


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


def heat_setting(nx=6):
    """Unit square, P1, T = x^2 + y, k = 1 / (A + B T) (demo_nonlinear_heat_equation_part2.py:209-210)."""
    m = structured_mesh("triangle", (nx, nx), degree=1)
    A_, B_ = 1.0, 1.0
    tab = (m.dofmap, m.geom_dofmap, m.x, m.phi, m.dphi, m.dpsi)
    T = m.node_x[:, 0] ** 2 + m.node_x[:, 1]
    Tq = eval_operand(VALUE, 1, T, *tab)[..., 0]
    s = eval_operand(GRAD, 1, T, *tab)
    k = 1.0 / (A_ + B_ * Tq)
    dqdT = B_ * k[..., None] ** 2 * s                                    # q = -k sigma
    dqds = -k[..., None, None] * np.eye(2)

    def explicit(That):
        # J_explicit = inner(B k^2 sigma T_hat, grad T~) dx + inner(-k grad T_hat, grad T~) dx (part2.py:324-335)
        S = B_ * k[..., None] ** 2 * s * eval_operand(VALUE, 1, That, *tab) - k[..., None] * eval_operand(GRAD, 1, That, *tab)
        return operand_adjoint(GRAD, 1, S, m.weights, *tab, m.node_x.shape[0])

    return m, dqdT, dqds, explicit


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
