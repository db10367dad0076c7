"""The NumPy yardstick of the form layer (dxo_bilinear_apply / dxo_bilinear_diagonal / dxo_csr_create / dxo_bilinear_assemble), as
compositions of the operand oracle. Pinned by tests/test_bilinear_oracle_cpu.py and tests/test_assemble_oracle_cpu.py.

The bilinear action is K v = operand_adjoint(test, C : eval_operand(trial, v)), its diagonal the probes e_i . K e_i. The pattern
oracle is the definition: row node*bs + i holds the columns m*bs + j of every node m that shares a cell with the row's node, sorted.
Column j of the dense matrix is bilinear_ref(e_j), taken many columns at a time by probes over a distance-2 colouring of the nodes
(two nodes of one colour share no neighbour, so every row sees at most one of them)."""
import numpy as np

from oracle.operand_oracle import DEFGRAD, EPS_MANDEL, GRAD, VALUE, VALUE_GRAD, eval_operand, operand_adjoint
from tools.synthetic import structured_mesh

KIND_ID = {"value": VALUE, "grad": GRAD, "eps": EPS_MANDEL, "F": DEFGRAD, "value_grad": VALUE_GRAD}


def tables(m):
    return m.dofmap, m.geom_dofmap, m.x, m.phi, m.dphi, m.dpsi


# ---- the action and its diagonal
def bilinear_ref(m, test, trial, bs, C, v):
    """sum_q w |det J| B_test^T C B_trial v, C of shape (n_points, D_test, D_trial). "F" is taken as its linearisation, grad."""
    trial_id = GRAD if trial == "F" else KIND_ID[trial]
    e = eval_operand(trial_id, bs, v, *tables(m))                                  # (nc, nq, D_trial)
    nc, nq, dr = e.shape
    t = np.einsum("cqrs,cqs->cqr", np.asarray(C).reshape(nc, nq, -1, dr), e)
    return operand_adjoint(KIND_ID[test], bs, t, m.weights, *tables(m), m.node_x.shape[0])


def node_colours(m):
    """Greedy colouring of the field nodes: two nodes of one cell never share a colour."""
    nn = m.node_x.shape[0]
    cells_of = [[] for _ in range(nn)]
    for c, nodes in enumerate(m.dofmap):
        for a in nodes:
            cells_of[a].append(c)
    colour = -np.ones(nn, dtype=np.int64)
    for a in range(nn):
        taken = {colour[b] for c in cells_of[a] for b in m.dofmap[c]}
        k = 0
        while k in taken:
            k += 1
        colour[a] = k
    return colour


def diagonal_by_probes(apply, n_nodes, bs, colour):
    """diag(K) from K applied to sums of unit vectors: the nodes of one colour share no cell, so (K sum_j e_j)_i = K_ii on them."""
    diag = np.zeros((n_nodes, bs))
    for k in range(colour.max() + 1):
        sel = colour == k
        for i in range(bs):
            v = np.zeros((n_nodes, bs))
            v[sel, i] = 1.0
            diag[sel, i] = apply(v.reshape(-1)).reshape(n_nodes, bs)[sel, i]
    return diag.reshape(-1)


def bilinear_diag_ref(m, test, trial, bs, C):
    return diagonal_by_probes(lambda v: bilinear_ref(m, test, trial, bs, C, v), m.node_x.shape[0], bs, node_colours(m))


# ---- the pattern and the assembled matrix
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


def heat_setting(nx=6):
    """Unit square, P1, T = x^2 + y, k = 1 / (A + B T) (demo_nonlinear_heat_equation_part2.py:209-210)."""
    m = structured_mesh("triangle", (nx, nx), degree=1)
    A_, B_ = 1.0, 1.0
    tab = tables(m)
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
