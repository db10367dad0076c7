"""The NumPy yardsticks of the transposed operators, pinned on the CPU: the mirror map of a blocked pattern against scipy's transpose,
and the transposed action as the forward reference with the kinds swapped and the blocks transposed, against the dense matrix."""
import numpy as np
import pytest
import scipy.sparse

from oracle.form_oracle import bilinear_ref, dense_ref, pattern_ref
from solver_cases import CELLS, PAIRS
from transpose_cases import form_mesh, mirror_ref, random_blocks


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("degree", [1, 2])
def test_mirror_map_is_an_involution_and_is_scipys_transpose(cell, degree):
    m = form_mesh(cell, degree)
    rng = np.random.Generator(np.random.PCG64(3))
    for bs in (1, m.gdim):
        indptr, indices = pattern_ref(m, bs)
        perm = mirror_ref(indptr, indices, bs)
        assert np.array_equal(perm[perm], np.arange(perm.size))
        values = rng.normal(size=indices.size)
        n = indptr.size - 1
        A = scipy.sparse.csr_matrix((values, indices, indptr), shape=(n, n))
        T = A.T.tocsr()
        T.sort_indices()
        assert np.array_equal(T.indptr, indptr) and np.array_equal(T.indices, indices)      # structurally symmetric
        assert np.array_equal(T.data, values[perm])


def test_mirror_map_refuses_an_unsymmetric_pattern():
    indptr, indices = np.array([0, 2, 3]), np.array([0, 1, 1])
    with pytest.raises(ValueError, match="no mirrored entry"):
        mirror_ref(indptr, indices, 1)


@pytest.mark.parametrize("cell", list(CELLS))
def test_transposed_action_reference_is_the_dense_transpose(cell):
    m = form_mesh(cell, 1)
    G, nn = m.gdim, m.node_x.shape[0]
    rng = np.random.Generator(np.random.PCG64(5))
    for test, trial, vector in PAIRS:
        bs = G if vector else 1
        Cb = random_blocks(m, test, trial, bs, rng)
        w = rng.normal(size=nn * bs)
        ref = bilinear_ref(m, trial, test, bs, np.ascontiguousarray(Cb.transpose(0, 2, 1)), w)
        dense = dense_ref(m, test, trial, bs, Cb).T @ w
        err = np.abs(ref - dense).max() / np.abs(dense).max()
        print(f"{cell} {test}/{trial} bs {bs}: {err:.2e}")
        assert err <= 1e-13
