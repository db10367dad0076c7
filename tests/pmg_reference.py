"""A NumPy restatement of dxo_pmg_create / dxo_pmg_setup / dxo_pmg_apply (csrc/pmg.hip) from the pieces of oracle.amg_oracle
(vertex_transfer_ref, p_diag_ref, start_vector, cheby_pairs): the reference of the p-multigrid tests. Not a test module.

The transfers accumulate SEQUENTIALLY in the order the header states (restriction: the fine nodes of a coarse node ascending;
prolongation: the coarse nodes of a fine node ascending), one entry of every row per pass, so that with weights that are powers of
two the device must reproduce them bit for bit. `dtype=np.longdouble` runs the cycle in extended precision as the referee of the
float64 runs (the matrix is then a dense long-double array; the pairs are made from the rho it is given)."""
import numpy as np
import scipy.sparse as sp

from oracle.amg_oracle import cheby_pairs, p_diag_ref, start_vector


def diagonal_case(n):
    """(W, coarse_to_fine) of the identity transfer on n nodes: every node is its own coarse node."""
    return sp.identity(n, format="csr", dtype=np.float64), np.arange(n, dtype=np.int32)


def _rounds(ptr):
    """The passes of a sequential sum over CSR rows: pass k holds (rows with more than k entries, their k-th entry)."""
    counts = np.diff(ptr)
    out = []
    for k in range(int(counts.max(initial=0))):
        rows = np.flatnonzero(counts > k)
        out.append((rows, ptr[rows] + k))
    return out


class PmgRef:
    """create: p_diag, the transposed incidence and the coarse constrained list of a transfer W (scipy CSR with sorted rows),
    coarse_to_fine, the block size and the constrained fine dofs."""

    def __init__(self, W, ctf, bs, constrained=()):
        W = sp.csr_matrix(W)
        self.bs, self.n_nodes, self.n_coarse_nodes = int(bs), W.shape[0], W.shape[1]
        self.n, self.nc = self.n_nodes * self.bs, self.n_coarse_nodes * self.bs
        self.ptr, self.col = W.indptr.astype(np.int64), W.indices.astype(np.int64)
        self.ctf = np.asarray(ctf, dtype=np.int64)
        self.mask = np.zeros(self.n, dtype=bool)
        dofs = np.asarray(() if constrained is None else constrained, dtype=np.int64).reshape(-1)
        self.mask[dofs[(dofs >= 0) & (dofs < self.n)]] = True
        self.p_diag = p_diag_ref(W, self.ctf, self.mask, self.bs)                         # (blocks, bs)
        self.coarse_constrained = np.flatnonzero(self.mask.reshape(-1, self.bs)[self.ctf].reshape(-1)).astype(np.int32)
        # the transposed incidence: the blocks of a coarse node with their fine nodes ascending (a stable sort of the blocks by column)
        rows = np.repeat(np.arange(self.n_nodes), np.diff(self.ptr))
        order = np.argsort(self.col, kind="stable")
        self.pt_blk, self.pt_row = order, rows[order]
        self.pt_ptr = np.concatenate([[0], np.cumsum(np.bincount(self.col, minlength=self.n_coarse_nodes))]).astype(np.int64)
        self._p_rounds, self._pt_rounds = _rounds(self.ptr), _rounds(self.pt_ptr)
        self.P = sp.csr_matrix(sp.bsr_matrix((self.p_diag[:, :, None] * np.eye(self.bs)[None], W.indices, W.indptr), shape=(self.n, self.nc)))
        self.ready = False

    # ---- the transfers
    def restrict(self, r, t=None, dtype=np.float64):
        """r_c[v, c] = sum over the fine nodes i of column v, ascending, of p_diag (r[i, c] - t[i, c]) (t None: of p_diag r[i, c])."""
        res = np.asarray(r, dtype=dtype) if t is None else np.asarray(r, dtype=dtype) - np.asarray(t, dtype=dtype)
        res = res.reshape(self.n_nodes, self.bs)
        pd = self.p_diag.astype(dtype)
        out = np.zeros((self.n_coarse_nodes, self.bs), dtype=dtype)
        for cols, e in self._pt_rounds:
            out[cols] = out[cols] + pd[self.pt_blk[e]] * res[self.pt_row[e]]
        return out.reshape(-1)

    def prolong(self, e_c, x=None, dtype=np.float64):
        """x[i, c] (+)= sum over the coarse nodes v of row i, ascending, of p_diag e_c[v, c]: the sum is formed first, then added."""
        ec = np.asarray(e_c, dtype=dtype).reshape(self.n_coarse_nodes, self.bs)
        pd = self.p_diag.astype(dtype)
        acc = np.zeros((self.n_nodes, self.bs), dtype=dtype)
        for rows, e in self._p_rounds:
            acc[rows] = acc[rows] + pd[e] * ec[self.col[e]]
        acc = acc.reshape(-1)
        return acc if x is None else np.asarray(x, dtype=dtype) + acc

    # ---- setup
    def setup(self, A, dinv, coarse, degree=2, rho_iters=10, lower=0.1, safety=1.1, rho=None):
        """A: a matrix (scipy or dense) or a callable v -> A v; dinv: the inverse diagonal; coarse: a callable r_c -> e_c. rho: taken
        as given (the device's), else the power estimate in float64."""
        self.A, self.dinv, self.coarse = A, np.asarray(dinv, dtype=np.float64), coarse
        self._A_ld = None
        self.degree, self.lower = int(degree), float(lower)
        self.rho = self.power_rho(rho_iters, safety) if rho is None else float(rho)
        self.pairs = cheby_pairs(self.rho, self.lower, self.degree)
        self.calls = 0
        self.ready = True
        return self

    def _mul(self, v, dtype=np.float64):
        self.calls += 1
        if callable(self.A):
            return np.asarray(self.A(v), dtype=dtype)
        if dtype is np.float64:
            return self.A @ v
        if getattr(self, "_A_ld", None) is None:
            self._A_ld = np.asarray(self.A.toarray() if sp.issparse(self.A) else self.A).astype(dtype)
        return self._A_ld @ v

    def power_rho(self, iters, safety):
        """safety |w_iters| of w_k = Dinv A (w_{k-1} / |w_{k-1}|) from start_vector: power_rho_ref for a diagonal Dinv and any A."""
        self.calls = 0
        w = start_vector(self.n)
        lam = np.sqrt(w @ w)
        for _ in range(iters):
            s = 1.0 / lam if lam > 0.0 else 0.0
            w = self.dinv * self._mul(s * w)
            lam = np.sqrt(w @ w)
        return safety * lam

    # ---- apply
    def apply(self, r, dtype=np.float64):
        """z = M r: the five steps of dxo_pmg_apply."""
        assert self.ready
        r = np.asarray(r, dtype=dtype)
        dinv = self.dinv.astype(dtype)
        pairs = [(dtype(c1), dtype(c2)) for c1, c2 in self.pairs]
        d = pairs[0][1] * (dinv * r)
        x = d.copy()
        for c1, c2 in pairs[1:]:
            d = c1 * d + c2 * (dinv * (r - self._mul(x, dtype)))
            x = x + d
        rc = self.restrict(r, self._mul(x, dtype), dtype)
        ec = np.asarray(self.coarse(rc), dtype=dtype)
        x = self.prolong(ec, x, dtype)
        for c1, c2 in pairs:
            d = c1 * d + c2 * (dinv * (r - self._mul(x, dtype)))
            x = x + d
        return x


def exact_inverse(Ac, dtype=np.float64):
    """The inverse of a small dense matrix; in long double: the float64 inverse improved by two Newton-Schulz steps
    X <- X + X (I - A X) in extended precision (each squares the residual I - A X)."""
    Ac = np.asarray(Ac.toarray() if sp.issparse(Ac) else Ac, dtype=np.float64)
    X = np.linalg.inv(Ac)
    if dtype is np.float64:
        return X
    A, X = Ac.astype(dtype), X.astype(dtype)
    eye = np.eye(A.shape[0], dtype=dtype)
    for _ in range(2):
        X = X + X @ (eye - A @ X)
    return X
