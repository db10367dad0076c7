"""The yardstick of tests/test_block_inverse_gpu.py, pinned on the CPU: an exact inverse, blocks made to go wrong, and the dense
systems that force the coarsest Gauss-Jordan to exchange rows.

exact_inverse eliminates over fractions.Fraction on the float entries (floats are rationals), so its inverse is the true one rounded
once, and the quantity of the device's singularity rule, |det| / prod |row|_2 (accepted above 1e-14), is known exactly.
adversarial_blocks makes what the finite-element blocks of the rest of the suite never are: pivots off the diagonal at every step,
nonsymmetric and indefinite entries, rows 80 binades apart, blocks a little above the threshold of the rule and blocks below it,
NaN and Inf. tests/test_block_inverse_oracle_cpu.py checks the yardstick and the conditions on the inputs that the device tests rely
on: no block lies in the band where the rounding of the determinant, not the rule, decides; the blocks meant to exchange rows do so
in a transcription of the device's pivot search."""
import math
from fractions import Fraction

import numpy as np
import scipy.linalg
import scipy.sparse

from oracle.form_oracle import pattern_ref
from tools.synthetic import structured_mesh

U = 2.0 ** -53
RULE = 1e-14                   # invert_block / gj6 (csrc/krylov_internal.h): a block is accepted when |det| > RULE * prod |row|_2
BAND = (1e-16, 1e-12)          # no generated block has its exact ratio strictly inside: there the rounding of det decides
NEAR = (1e-12, 1e-11)          # the exact ratio of the `near` family
ACCEPTED = ("perm", "dense", "rowscaled", "near")
BLOCK_SIZES = (1, 2, 3, 6)


# ---- the exact reference
def _fractions(a):
    return [[Fraction(float(v)) for v in row] for row in np.asarray(a, dtype=np.float64)]


def exact_inverse(a):
    """(inverse rounded once to float64, |det| / prod |row|_2, kappa_inf) of a square float block, by Gauss-Jordan over Fractions.
    A singular block: (None, 0.0, inf); a zero row makes the ratio 0 / 0, taken as 0."""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0]
    assert a.shape == (n, n) and np.isfinite(a).all()
    A = _fractions(a)
    M = [row[:] + [Fraction(int(i == j)) for j in range(n)] for i, row in enumerate(A)]
    det = Fraction(1)
    for k in range(n):
        p = next((i for i in range(k, n) if M[i][k] != 0), None)
        if p is None:
            return None, 0.0, math.inf
        if p != k:
            M[k], M[p] = M[p], M[k]
            det = -det
        piv = M[k][k]
        det *= piv
        M[k] = [v / piv for v in M[k]]
        for i in range(n):
            if i != k and M[i][k] != 0:
                f = M[i][k]
                M[i] = [v - f * w for v, w in zip(M[i], M[k])]
    inv = [row[n:] for row in M]
    had2 = Fraction(1)
    for row in A:
        had2 *= sum(v * v for v in row)
    ratio = math.sqrt(det * det / had2)                  # Fraction / Fraction -> float is rounded correctly
    kappa = float(max(sum(abs(v) for v in row) for row in A) * max(sum(abs(v) for v in row) for row in inv))
    return np.array([[float(v) for v in row] for row in inv]), ratio, kappa


def cofactor_bound(a):
    """(bound on |device - exact| entry by entry, relative error bound of the device's det) for the closed forms of invert_block,
    bs <= 3: first order in u, with 1 % for the higher orders (test_inputs_keep_the_first_order_bound_valid holds the relative
    error of det below 1e-2).

    Every p1 - p2 of two products (with or without a fused multiply-add) errs by at most 2 u (|p1| + |p2|). bs 2: det is one such
    expression and b_ij = a_kl * fl(1 / det), so |db_ij| <= |b_ij| (2 u P / |det| + 2 u), P = |a00 a11| + |a01 a10|. bs 3: a
    cofactor errs by 2 u C_ij (C: the cofactors of |a| with every sign +); det = sum_j a0j c0j adds 3 u per term for its products
    and sums, so |ddet| <= 5 u perm(|a|), and |db_ij| <= 2 u C_ij / |det| + |b_ij| (5 u perm / |det| + 2 u). bs 1: one division.
    Half a unit more for the one rounding of the reference. Exact arithmetic throughout, rounded at the end."""
    A = _fractions(a)
    n = len(A)
    if n == 1:
        return np.array([[1.01 * U * 1.5 * abs(1.0 / float(A[0][0]))]]), U
    if n == 2:
        det = abs(A[0][0] * A[1][1] - A[0][1] * A[1][0])
        P = abs(A[0][0] * A[1][1]) + abs(A[0][1] * A[1][0])
        adj = [[A[1][1], A[0][1]], [A[1][0], A[0][0]]]
        rel = 2 * P / det
        return np.array([[1.01 * U * float(abs(adj[i][j]) / det * (rel + Fraction(5, 2))) for j in range(2)] for i in range(2)]), U * float(rel)
    assert n == 3
    cof = [[None] * 3 for _ in range(3)]                   # the entry b_ij is (cofactor of a_ji) / det
    cab = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != j]
            c = [k for k in range(3) if k != i]
            p1, p2 = A[r[0]][c[0]] * A[r[1]][c[1]], A[r[0]][c[1]] * A[r[1]][c[0]]
            cof[i][j] = (p1 - p2) * (-1) ** (i + j)
            cab[i][j] = abs(p1) + abs(p2)
    det = abs(sum(A[0][j] * cof[j][0] for j in range(3)))
    perm = sum(abs(A[0][j]) * cab[j][0] for j in range(3))
    rel = 5 * perm / det
    bound = [[1.01 * U * float(2 * cab[i][j] / det + abs(cof[i][j]) / det * (rel + Fraction(5, 2))) for j in range(3)] for i in range(3)]
    return np.array(bound), U * float(rel)


def gj_exchanges(a):
    """The steps at which the device's Gauss-Jordan (gj6, and amg_dense_step) exchanges rows: its pivot rule, the largest
    |M[i][k]| over i >= k and the lowest row among equals, transcribed into NumPy."""
    M = np.array(a, dtype=np.float64)
    n = M.shape[0]
    steps = []
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))             # argmax returns the first of equals
        if p != k:
            M[[k, p]] = M[[p, k]]
            steps.append(k)
        M[k] = M[k] / M[k, k]
        for i in range(n):
            if i != k:
                M[i] = M[i] - M[i, k] * M[k]
    return steps


# ---- the blocks
def block_ratio(a):
    return exact_inverse(a)[1]


def _near_block(rng, bs, band):
    """A dense block whose row j is row i plus eps times noise, eps adjusted until the exact ratio lies in `band`."""
    a = rng.normal(size=(bs, bs))
    i, j = rng.choice(bs, size=2, replace=False)
    noise = rng.normal(size=bs)
    target = math.sqrt(band[0] * band[1])
    eps = target
    for _ in range(40):
        b = a.copy()
        b[j] = a[i] + eps * noise
        r = block_ratio(b)
        if band[0] <= r <= band[1]:
            return b
        eps *= target / r if r > 0 else 2.0
    raise AssertionError("no eps puts the ratio into the band")


def _tiny_block(rng, bs):
    """A regular block whose exact ratio is positive and at most 1e-16: two rows that differ in the last bit of one entry."""
    for _ in range(100):
        a = rng.normal(size=(bs, bs))
        i, j = rng.choice(bs, size=2, replace=False)
        c = int(np.argmin(np.abs(a[i])))
        a[j] = a[i]
        a[j, c] = np.nextafter(a[i, c], np.inf)
        if 0.0 < block_ratio(a) <= BAND[0]:
            return a
    raise AssertionError("no block with a ratio in (0, 1e-16]")


def adversarial_blocks(bs, seed, count=6):
    """{family: (count, bs, bs)} for the accepted families that exist at `bs`, and "rejected": {name: block}. All from PCG64(seed).

    perm       a cyclic permutation times a diagonal of distinct magnitudes: a zero leading entry, and an exchange at every step
               of the elimination but the last (bs >= 2)
    dense      normal entries: nonsymmetric, indefinite
    rowscaled  a dense block with row i times 2^e_i, e_i in [-40, 40] (exact; the first block has both ends): the rule is invariant
    near       a dense block with one row replaced by another plus eps * noise, the exact ratio in [1e-12, 1e-11] (bs >= 2)
    rejected   tiny (ratio in (0, 1e-16]), duplicate (two equal rows), zero, nan, inf (one entry)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    perm = np.zeros((count, bs, bs))
    for q in range(count):
        mag = np.sort(rng.uniform(0.5, 1.0, size=bs) * 2.0 ** rng.permutation(np.arange(bs) - bs // 2))
        d = rng.permutation(mag) * rng.choice([-1.0, 1.0], size=bs)
        shift = 1 if q % 2 == 0 else bs - 1
        perm[q, np.arange(bs), (np.arange(bs) + shift) % bs] = d
    out["perm"] = perm
    out["dense"] = rng.normal(size=(count, bs, bs))
    e = rng.integers(-40, 41, size=(count, bs))
    e[0, 0] = -40
    e[0, -1] = 40 if bs > 1 else e[0, -1]
    out["rowscaled"] = rng.normal(size=(count, bs, bs)) * (2.0 ** e)[:, :, None]
    rejected = {}
    if bs >= 2:
        out["near"] = np.stack([_near_block(rng, bs, NEAR) for _ in range(count)])
        rejected["tiny"] = _tiny_block(rng, bs)
        dup = rng.normal(size=(bs, bs))
        dup[bs - 1] = dup[0]
        rejected["duplicate"] = dup
    rejected["zero"] = np.zeros((bs, bs))
    for name, bad in (("nan", np.nan), ("inf", np.inf)):
        a = rng.normal(size=(bs, bs))
        a[tuple(rng.integers(0, bs, size=2))] = bad
        rejected[name] = a
    out["rejected"] = rejected
    return out


def node_blocks(bs, n_nodes, seed):
    """(blocks (n_nodes, bs, bs), family name per node): node i gets the block i // F of family i mod F, F the accepted families
    that exist at bs."""
    names = [f for f in ACCEPTED if bs >= 2 or f != "near"]
    fam = adversarial_blocks(bs, seed, count=-(-n_nodes // len(names)))
    return (np.stack([fam[names[i % len(names)]][i // len(names)] for i in range(n_nodes)]), [names[i % len(names)] for i in range(n_nodes)])


def values_with_blocks(indptr, indices, bs, blocks, seed):
    """Values on a blocked pattern (the bs rows of a node share their sorted columns): seeded normal noise everywhere, the
    diagonal block of node i replaced by blocks[i]."""
    vals = np.random.Generator(np.random.PCG64(seed)).normal(size=indices.size)
    for node, blk in enumerate(blocks):
        for i in range(bs):
            r = node * bs + i
            cols = indices[indptr[r]:indptr[r + 1]]
            k = int(np.searchsorted(cols, node * bs))
            assert np.array_equal(cols[k:k + bs], node * bs + np.arange(bs))
            vals[indptr[r] + k:indptr[r] + k + bs] = blk[i]
    return vals


# ---- the dense systems of the coarsest level: a zero diagonal, so that the first step exchanges rows, and most that follow
DENSE_CASES = {"p1_306": ("triangle", (17, 16), 1), "p1_bs2": ("triangle", (3, 3), 2)}
DENSE_COND = 1e8


def zero_diagonal_system(which):
    """(indptr, indices, values, seed) on the pattern of the named case: every diagonal entry exactly zero, the rest seeded normal,
    the first seed whose 2-norm condition number is below DENSE_COND."""
    cell, n, bs = DENSE_CASES[which]
    indptr, indices = pattern_ref(structured_mesh(cell, n, 1), bs)
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    for seed in range(20):
        vals = np.random.Generator(np.random.PCG64(seed)).normal(size=indices.size)
        vals[rows == indices] = 0.0
        A = scipy.sparse.csr_matrix((vals, indices, indptr)).toarray()
        if np.linalg.cond(A) < DENSE_COND:
            return indptr, indices, vals, seed
    raise AssertionError("no seed below the condition number")


def refined_solve(A, R):
    """A^-1 R by a float64 LU and two steps of iterative refinement, the residual formed in np.longdouble. Returns (X, the largest
    |R - A X| / (|A| |X| + |R|), entrywise, in longdouble)."""
    lu = scipy.linalg.lu_factor(A)
    X = scipy.linalg.lu_solve(lu, R)
    Al, Rl = A.astype(np.longdouble), R.astype(np.longdouble)
    for _ in range(2):
        X = X + scipy.linalg.lu_solve(lu, (Rl - Al @ X.astype(np.longdouble)).astype(np.float64))
    Xl = X.astype(np.longdouble)
    return X, float(np.max(np.abs(Rl - Al @ Xl) / (np.abs(Al) @ np.abs(Xl) + np.abs(Rl))))
