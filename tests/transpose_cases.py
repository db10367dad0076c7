"""What the tests of the transposed operators share: the NumPy mirror map of a blocked pattern, the meshes of the form tests and the
random non-symmetric blocks. Not a test module."""
import numpy as np

from solver_cases import CELLS, _value_size
from tools.synthetic import structured_mesh


def mirror_ref(indptr, indices, bs):
    """For a pattern in the layout of dxo_csr_create (rows node * bs + i of a node share their columns, the columns come in runs
    m * bs + j): perm with values_t = values[perm], i.e. for the entry ((n, i), (m, j)) the index of the entry ((m, j), (n, i)).
    Raises ValueError where an entry has no mirrored entry (a pattern that is not structurally symmetric)."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n_rows = indptr.size - 1
    perm = np.empty(indices.size, dtype=np.int64)
    for r in range(n_rows):
        for e in range(indptr[r], indptr[r + 1]):
            c = indices[e]
            row = indices[indptr[c]:indptr[c + 1]]
            k = np.searchsorted(row, r)
            if k >= row.size or row[k] != r:
                raise ValueError(f"entry ({r}, {c}) has no mirrored entry")
            perm[e] = indptr[c] + k
    return perm


def form_mesh(cell, degree):
    """The smallest meshes of the form tests: CELLS of solver_cases.py, distorted by 0.2."""
    return structured_mesh(cell, CELLS[cell], degree, distort=0.2, seed=7)


def random_blocks(m, test, trial, bs, rng):
    """Random, non-symmetric [points][D_test][D_trial]."""
    G = m.gdim
    return rng.normal(size=(m.num_cells * m.nq, _value_size(test, G, bs), _value_size(trial, G, bs)))


def some_dirichlet_dofs(n_rows):
    """A few constrained dofs, spread over the rows."""
    return np.unique(np.array([0, n_rows // 3, n_rows // 2 + 1, n_rows - 1], dtype=np.int32))
