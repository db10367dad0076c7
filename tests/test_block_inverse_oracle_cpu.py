"""The yardstick of tests/test_block_inverse_gpu.py, pinned on the CPU: an exact inverse, blocks made to go wrong, and the dense
systems that force the coarsest Gauss-Jordan to exchange rows.

exact_inverse eliminates over fractions.Fraction on the float entries (floats are rationals), so its inverse is the true one rounded
once, and the quantity of the device's singularity rule, |det| / prod |row|_2 (accepted above 1e-14), is known exactly.
adversarial_blocks makes what the finite-element blocks of the rest of the suite never are: pivots off the diagonal at every step,
nonsymmetric and indefinite entries, rows 80 binades apart, blocks a little above the threshold of the rule and blocks below it,
NaN and Inf. The tests here check the yardstick and the conditions on the inputs that the device tests rely on: no block lies in
the band where the rounding of the determinant, not the rule, decides; the blocks meant to exchange rows do so in a transcription
of the device's pivot search."""
import math

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse

from oracle.block_inverse_oracle import (ACCEPTED, BAND, BLOCK_SIZES, DENSE_CASES, DENSE_COND, NEAR, RULE, U, adversarial_blocks, block_ratio,
                                         cofactor_bound, exact_inverse, gj_exchanges, node_blocks, refined_solve, values_with_blocks,
                                         zero_diagonal_system)
from oracle.form_oracle import pattern_ref
from oracle.krylov_oracle import diagonal_blocks
from tools.synthetic import structured_mesh


# ---- tests
SEEDS = (0, 1)


@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_exact_inverse_agrees_with_numpy_on_the_well_conditioned_families(bs):
    for seed in SEEDS:
        fam = adversarial_blocks(bs, seed)
        for name in ("perm", "dense", "rowscaled"):
            for a in fam[name]:
                inv, ratio, kappa = exact_inverse(a)
                ref = np.linalg.inv(a)
                # rows 80 binades apart: column j of the inverse carries 1 / (scale of row j), compare column by column
                err = np.max(np.abs(inv - ref) / np.max(np.abs(inv), axis=0))
                assert err <= 8 * bs * U * kappa, (bs, name, err, kappa)
                assert abs(kappa - np.linalg.cond(a, np.inf)) <= 1e-6 * kappa
                prod = np.prod(np.linalg.norm(a / np.max(np.abs(a), axis=1, keepdims=True), axis=1))
                det = abs(np.linalg.det(a / np.max(np.abs(a), axis=1, keepdims=True)))
                assert abs(ratio - det / prod) <= 1e-10 * ratio, (bs, name)
                if name == "perm":
                    assert ratio == pytest.approx(1.0, abs=1e-15) and np.count_nonzero(inv) == bs
    assert exact_inverse(np.array([[1.0, 2.0], [2.0, 4.0]])) == (None, 0.0, math.inf)
    inv, ratio, kappa = exact_inverse(np.array([[0.0, 2.0], [0.5, 0.0]]))
    assert np.array_equal(inv, [[0.0, 2.0], [0.5, 0.0]]) and ratio == 1.0 and kappa == 4.0


@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_no_block_lies_in_the_band_where_rounding_decides(bs):
    for seed in SEEDS:
        fam = adversarial_blocks(bs, seed)
        assert set(fam) == ({"perm", "dense", "rowscaled", "rejected"} | ({"near"} if bs >= 2 else set()))
        for name in ACCEPTED:
            for a in fam.get(name, ()):
                r = block_ratio(a)
                assert r >= BAND[1] > RULE, (bs, name, r)
                if name == "near":
                    assert NEAR[0] <= r <= NEAR[1] and exact_inverse(a)[2] > 1e10
                if name == "rowscaled":              # the rule does not see the scaling of the rows
                    assert r == pytest.approx(block_ratio(a / np.max(np.abs(a), axis=1, keepdims=True)), rel=1e-12)
        rej = fam["rejected"]
        assert set(rej) == ({"zero", "nan", "inf"} | ({"tiny", "duplicate"} if bs >= 2 else set()))
        assert not rej["zero"].any() and np.isnan(rej["nan"]).sum() == 1 and np.isposinf(rej["inf"]).sum() == 1
        if bs >= 2:
            assert 0.0 < block_ratio(rej["tiny"]) <= BAND[0] < RULE
            assert exact_inverse(rej["duplicate"]) == (None, 0.0, math.inf) and rej["duplicate"].all()
    e = np.log2(np.max(np.abs(adversarial_blocks(max(bs, 2), 0)["rowscaled"][0]), axis=1))
    assert e.min() < -36 and e.max() > 36             # both ends of the 2^+-40 scaling are there


@pytest.mark.parametrize("bs", BLOCK_SIZES[1:])
def test_the_blocks_reach_the_row_exchange(bs):
    for seed in SEEDS:
        fam = adversarial_blocks(bs, seed)
        for a in fam["perm"]:
            assert a[0, 0] == 0.0 and gj_exchanges(a) == list(range(bs - 1)), (bs, gj_exchanges(a))
        if bs == 6:                                      # the register Gauss-Jordan: at least half of the dense blocks too
            swapping = sum(bool(gj_exchanges(a)) for a in fam["dense"])
            assert 2 * swapping >= len(fam["dense"]), (bs, swapping)
    blocks, names = node_blocks(6, 22, 0)                # what the device test of block size 6 inverts
    assert sum(bool(gj_exchanges(a)) for a in blocks) >= 11 and names[:5] == ["perm", "dense", "rowscaled", "near", "perm"]


@pytest.mark.parametrize("bs", (1, 2, 3))
def test_inputs_keep_the_first_order_bound_valid(bs):
    """cofactor_bound is a first-order bound with 1 % for the rest: the relative error of the device's det stays below 1e-2 on
    every accepted block, and the bound holds for the same formulas evaluated in float64 by NumPy."""
    worst = 0.0
    for seed in SEEDS:
        for name in ACCEPTED:
            for a in adversarial_blocks(bs, seed).get(name, ()):
                bound, rel = cofactor_bound(a)
                assert rel < 1e-2, (bs, name, rel)
                exact = exact_inverse(a)[0]
                got = _closed_form(a)
                assert (np.abs(got - exact) <= bound).all(), (bs, name)
                worst = max(worst, float(np.max(np.abs(got - exact)[bound > 0] / bound[bound > 0])))
    assert bs == 1 or worst > 1e-3       # not vacuous: NumPy's own error comes within 1000 x of it (bs 1: one division, error 0)


def _closed_form(a):
    """invert_block's formulas for bs <= 3 in float64."""
    n = a.shape[0]
    if n == 1:
        return 1.0 / a
    if n == 2:
        idet = 1.0 / (a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0])
        return np.array([[a[1, 1] * idet, -a[0, 1] * idet], [-a[1, 0] * idet, a[0, 0] * idet]])
    c00 = a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]
    c01 = a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2]
    c02 = a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0]
    idet = 1.0 / (a[0, 0] * c00 + a[0, 1] * c01 + a[0, 2] * c02)
    return np.array([[c00, a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2], a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]],
                     [c01, a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0], a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]],
                     [c02, a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1], a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]]]) * idet


def test_values_with_blocks_puts_the_blocks_on_the_diagonal():
    for cell, n, bs in (("triangle", (3, 3), 2), ("tetrahedron", (2, 2, 2), 3), ("triangle", (17, 16), 2)):
        m = structured_mesh(cell, n, 1)
        indptr, indices = pattern_ref(m, bs)
        n_nodes = (indptr.size - 1) // bs
        assert n_nodes == {(3, 3): 16, (2, 2, 2): 27, (17, 16): 306}[n]
        blocks, _ = node_blocks(bs, n_nodes, 3)
        vals = values_with_blocks(indptr, indices, bs, blocks, 4)
        S = scipy.sparse.csr_matrix((vals, indices, indptr))
        assert np.array_equal(diagonal_blocks(S, bs), blocks)
        plain = np.random.Generator(np.random.PCG64(4)).normal(size=indices.size)
        assert (vals != plain).sum() <= n_nodes * bs * bs and (vals == plain).sum() >= indices.size - n_nodes * bs * bs


@pytest.mark.parametrize("which", list(DENSE_CASES))
def test_zero_diagonal_systems_are_regular_and_exchange_rows(which):
    indptr, indices, vals, seed = zero_diagonal_system(which)
    A = scipy.sparse.csr_matrix((vals, indices, indptr)).toarray()
    n = A.shape[0]
    assert n == {"p1_306": 306, "p1_bs2": 32}[which] and not np.diag(A).any()
    assert np.linalg.cond(A) < DENSE_COND
    steps = gj_exchanges(A)
    assert steps[0] == 0 and 2 * len(steps) >= n, (which, len(steps))          # the first step, and most of them
    R = np.random.Generator(np.random.PCG64(100 + seed)).normal(size=(n, 3))
    X, res = refined_solve(A, R)
    assert res <= 2 * U, (which, res)                                          # the residual of a solution rounded once
    assert np.max(np.abs(X - np.linalg.solve(A, R))) <= 1e-6 * np.max(np.abs(X))
