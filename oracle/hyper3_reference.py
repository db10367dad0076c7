"""Long-double closed form of the 3-D hyperelastic operators (dxo_isihara3, dxo_icnn3_eval and their fused forms) — TEST
INFRASTRUCTURE ONLY, NumPy only.

    isihara3_ref(F, c)            W = c1 K1 + c2 K2 + c3 K1^2 + c4 K3          (the energy of tests/hyper3_cases.py)
    icnn3_ref(F, weights, net)    W = ICNN(K1, K2, K3) + the H correction      (tests/icnn3_cases.py)
    K1 = I1 J^(-2/3) - 3,  K2 = I2 J^(-4/3) - 3,  K3 = (J - 1)^2,  I1 = tr C,  I2 = (I1^2 - tr C^2) / 2,  C = F^T F,  J = |det F|

Both are written in the invariants x = (I1, I2, D), D = det F by cofactors, not in the generators (F:F, C:C, det F) of the kernels:

    P  = sum_k y_k dK_k                                        dK_k  = sum_x K_k,x dx
    dP = sum_k y_k d2K_k + sum_kl y_kl dK_k (x) dK_l           d2K_k = sum_x K_k,x d2x + sum_xy K_k,xy dx (x) dy
    dI1 = 2 F                   d2I1 = 2 d_ij d_ab
    dI2 = 2 I1 F - 2 F C        d2I2 = 4 F_ia F_jb + 2 I1 d_ij d_ab - 2 d_ij C_ab - 2 F_ib F_ja - 2 (F F^T)_ij d_ab
    dD  = cof F                 d2D  = e_ijk e_abc F_kc

with y_k, y_kl the first and second derivatives of the energy in the features: (c1 + 2 c3 K1, c2, c4) and y_11 = 2 c3 for the
analytic model, the network's gradient and Hessian in its input for the ICNN. Every quantity is carried as a pair (value, mag) of the
class Q: mag is the same expression with the absolute value of every additive term, so EVERY subtraction enters it with a plus — the
two products of a cofactor, the six of det F, the - 3 of K1 and K2, the - 1 of (J - 1), I1^2 - tr C^2, and every sum above. A power
J^p is charged the cancellation of det F itself: mag = |J^p| * mag(D) / |D|. The network's derivatives enter with |y_k|, |y_kl|; the H
correction (H = -P_NN(I), analytically zero in 3-D) with the mag of the sum it is, sum_k |y_k(I)| mag dK_k(I), which is not zero. A
float64 evaluation of either operator, in any order and with or without fused multiply-adds, then stays within a small multiple of
2^-53 * mag[k] in EVERY entry k (tests/hyper3_reference_cases.py measures the multiple on the float64 twin: the same code with
dtype = np.float64). An entry whose every term vanishes (the out-of-plane shears of a plane-strain F) has mag = 0 and is an exact 0.
"""
from __future__ import annotations

import numpy as np

from oracle.consumer_reference import LD, worst_ratio  # noqa: F401  (worst_ratio: re-exported for the tests)
from oracle.icnn_oracle import network_jets

assert np.finfo(LD).eps <= 2.0 ** -63, f"np.longdouble has eps = {np.finfo(LD).eps}: no extended precision on this platform"


class Q:
    """value and mag of one quantity; +, - and * of two of them, where - adds the mags"""
    __slots__ = ("v", "m")

    def __init__(self, v, m=None):
        self.v = v
        self.m = np.abs(v) if m is None else m

    def _other(self, o):
        return o if isinstance(o, Q) else Q(self.v.dtype.type(o))

    def __add__(self, o):
        o = self._other(o)
        return Q(self.v + o.v, self.m + o.m)

    def __sub__(self, o):
        o = self._other(o)
        return Q(self.v - o.v, self.m + o.m)

    def __mul__(self, o):
        o = self._other(o)
        return Q(self.v * o.v, self.m * o.m)

    __radd__, __rmul__ = __add__, __mul__

    def __neg__(self):
        return Q(-self.v, self.m)

    def __getitem__(self, idx):
        return Q(self.v[idx], self.m[idx])


def qsum(spec, *qs):
    """einsum of products, every one of them added: the same contraction on the values and on the mags"""
    return Q(np.einsum(spec, *(q.v for q in qs)), np.einsum(spec, *(q.m for q in qs)))


def total(terms):
    """the sum of a list of named terms [(name, Q)]"""
    out = terms[0][1]
    for _, q in terms[1:]:
        out = out + q
    return out


def _col(q, nd):
    """a per-point scalar against a per-point tensor of nd further axes"""
    return q[(slice(None),) + (None,) * nd]


def _outer(a, b):
    return Q(a.v[:, :, None] * b.v[:, None, :], a.m[:, :, None] * b.m[:, None, :])


def _power(aD, p):
    """|D|^p, charged the relative cancellation of D"""
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.power(aD.v, p)
        return Q(v, np.abs(v) * (aD.m / aD.v))


def invariants(F, dtype=LD):
    """F (n, 9) -> the invariants x = (I1, I2, D) of every point with their first (n, 9) and second (n, 9, 9) derivatives in F, each
    a list of named terms. Returns (x, dx, d2x, F3) with x = {"I1": Q, ...}, dx = {"I1": [(name, Q)], ...}, d2x likewise."""
    F3 = Q(np.asarray(F, dtype=dtype).reshape(-1, 3, 3))
    n = F3.v.shape[0]
    two, four, half = dtype(2), dtype(4), dtype(1) / dtype(2)
    C = qsum("nia,nib->nab", F3, F3)
    B = qsum("nia,nja->nij", F3, F3)
    I1 = qsum("nia,nia->n", F3, F3)
    I2 = (I1 * I1 - qsum("nab,nab->n", C, C)) * half
    FC = qsum("nib,nba->nia", F3, C)
    cv, cm = np.zeros((n, 3, 3), dtype=dtype), np.zeros((n, 3, 3), dtype=dtype)
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            q = F3[:, j, b] * F3[:, k, c] - F3[:, j, c] * F3[:, k, b]
            cv[:, i, a], cm[:, i, a] = q.v, q.m
    cof = Q(cv, cm)
    D = qsum("na,na->n", F3[:, 0, :], cof[:, 0, :])
    eye = Q(np.eye(3, dtype=dtype))
    eps = np.zeros((3, 3, 3), dtype=dtype)
    for i, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        eps[i, j, k], eps[i, k, j] = 1, -1
    eps = Q(eps)

    def flat(q):
        return Q(q.v.reshape(n, 9), q.m.reshape(n, 9))

    def flat2(spec, *qs):
        q = qsum(spec, *qs)
        return Q(q.v.reshape(n, 9, 9), q.m.reshape(n, 9, 9))

    one = Q(np.ones(n, dtype=dtype))
    I9 = flat2("n,ij,ab->niajb", one, eye, eye)
    Ff = flat(F3)
    x = {"I1": I1, "I2": I2, "D": D}
    dx = {"I1": [("2 F", Ff * two)],
          "I2": [("2 I1 F", _col(I1, 1) * Ff * two), ("- 2 F C", -(flat(FC) * two))],
          "D": [("cof F", flat(cof))]}
    d2x = {"I1": [("2 I", I9 * two)],
           "I2": [("4 F (x) F", _outer(Ff, Ff) * four), ("2 I1 I", _col(I1, 2) * I9 * two),
                  ("- 2 d_ij C_ab", -(flat2("ij,nab->niajb", eye, C) * two)),
                  ("- 2 F_ib F_ja", -(flat2("nib,nja->niajb", F3, F3) * two)),
                  ("- 2 (F F^T)_ij d_ab", -(flat2("nij,ab->niajb", B, eye) * two))],
           "D": [("e e F", flat2("ijk,abc,nkc->niajb", eps, eps, F3))]}
    return x, dx, d2x, F3


def features_ref(F, dtype=LD):
    """K (3 x Q (n,)), dK (3 x Q (n, 9)), d2K (3 x Q (n, 9, 9)) of the features K1, K2, K3 with J = |det F|, and F3 = Q (n, 3, 3)"""
    x, dx, d2x, F3 = invariants(F, dtype)
    I1, I2, D = x["I1"], x["I2"], x["D"]
    c = lambda p, q: dtype(p) / dtype(q)                                      # noqa: E731
    aD, sg = Q(np.abs(D.v), D.m), Q(np.sign(D.v))
    pw = lambda p, q: _power(aD, c(p, q))                                     # noqa: E731
    m, nn = pw(-2, 3), pw(-4, 3)
    K = [m * I1 - 3, nn * I2 - 3, (aD - 1) * (aD - 1)]
    # partials in (I1, I2, D); d|D|/dD = sign D
    first = [{"I1": m, "D": I1 * pw(-5, 3) * sg * c(-2, 3)},
             {"I2": nn, "D": I2 * pw(-7, 3) * sg * c(-4, 3)},
             {"D": (aD - 1) * sg * 2}]
    second = [{("I1", "D"): pw(-5, 3) * sg * c(-2, 3), ("D", "D"): I1 * pw(-8, 3) * c(10, 9)},
              {("I2", "D"): pw(-7, 3) * sg * c(-4, 3), ("D", "D"): I2 * pw(-10, 3) * c(28, 9)},
              {("D", "D"): Q(np.full(aD.v.shape, 2, dtype=dtype))}]
    g = {k: total(v) for k, v in dx.items()}
    dK, d2K = [], []
    for k in range(3):
        dK.append(total([(f"K{k + 1},{a} d{a}", _col(q, 1) * g[a]) for a, q in first[k].items()]))
        terms = [(f"K{k + 1},{a} d2{a}", _col(q, 2) * total(d2x[a])) for a, q in first[k].items()]
        for (a, b), q in second[k].items():
            terms.append((f"K{k + 1},{a}{b} d{a} (x) d{b}", _col(q, 2) * _outer(g[a], g[b])))
            if a != b:
                terms.append((f"K{k + 1},{a}{b} d{b} (x) d{a}", _col(q, 2) * _outer(g[b], g[a])))
        d2K.append(total(terms))
    return K, dK, d2K, F3


def _chain(y1, y2, dK, d2K):
    """P = sum_k y_k dK_k, dP = sum_k y_k d2K_k + sum_kl y_kl dK_k (x) dK_l; y1[k], y2[(k, l)] are Q (n,), a missing y2 entry is 0"""
    P = total([(f"y{k} dK{k}", _col(y1[k], 1) * dK[k]) for k in range(3)])
    terms = [(f"y{k} d2K{k}", _col(y1[k], 2) * d2K[k]) for k in range(3)]
    terms += [(f"y{k}{l} dK{k} (x) dK{l}", _col(q, 2) * _outer(dK[k], dK[l])) for (k, l), q in y2.items()]
    return P, total(terms)


def _symmetrised(dP):
    """the tangent is a Hessian: the mean of the two mirrored entries, which differ by the rounding of `dtype` alone"""
    return Q((dP.v + dP.v.transpose(0, 2, 1)) / 2, (dP.m + dP.m.transpose(0, 2, 1)) / 2)


def isihara3_ref(F, c, dtype=LD):
    """-> (P (n, 9), dP (n, 9, 9), magP, magdP) of F (n, 9) for the coefficients c = (c1, c2, c3, c4); det F <= 0: NaN in all 90"""
    F = np.asarray(F, dtype=dtype).reshape(-1, 9)
    c1, c2, c3, c4 = (dtype(x) for x in c)
    n = F.shape[0]
    K, dK, d2K, _ = features_ref(F, dtype)
    const = lambda x: Q(np.full(n, x, dtype=dtype))                           # noqa: E731
    y1 = [K[0] * (2 * c3) + c1, const(c2), const(c4)]
    P, dP = _chain(y1, {(0, 0): const(2 * c3)}, dK, d2K)
    dP = _symmetrised(dP)
    x = invariants(F, dtype)[0]
    bad = ~(x["D"].v > 0)
    for a in (P.v, dP.v):
        a[bad] = np.nan
    return P.v, dP.v, P.m, dP.m


_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def _softplus(x):
    """torch.nn.functional.softplus (beta = 1, threshold = 20) in the dtype of x"""
    with np.errstate(over="ignore"):
        return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20))))


def network_jets_wide(x, w, dtype=LD):
    """y (n,), dy/dx (n, 3), d2y/dx2 (n, 3, 3) of the ICNN (icnn3_cases.network_energy_torch) at x (n, 3), every step in `dtype`:
    each neuron carries its value, its 3 first and its 6 distinct second derivatives in x through the layers
        a = softplus(W) z + S x + c,   z' = softplus(a)^2 / 12."""
    x = np.asarray(x, dtype=dtype)
    n = x.shape[0]
    get = lambda k: np.asarray(w[k], dtype=dtype)                             # noqa: E731
    W0 = get("layers__0__weight")
    z = x @ W0.T + get("layers__0__bias")
    dz = np.broadcast_to(W0.T[None], (n, 3, W0.shape[0]))
    d2z = np.zeros((n, 6, W0.shape[0]), dtype=dtype)
    for layer in (1, 2):
        Wp, S = _softplus(get(f"layers__{layer}__weights")).T, get(f"skip_layers__{layer}__weight")
        a = z @ Wp + x @ S.T + get(f"skip_layers__{layer}__bias")
        da = np.tensordot(dz, Wp, axes=([2], [0])) + S.T[None]
        d2a = np.tensordot(d2z, Wp, axes=([2], [0]))
        sp = _softplus(a)
        with np.errstate(over="ignore"):
            s1 = np.where(a > 20, 1, 1 / (1 + np.exp(-a)))
        s2 = np.where(a > 20, 0, s1 * (1 - s1))
        p1, p2 = sp * s1 / 6, (s1 * s1 + sp * s2) / 6                        # first and second derivative of softplus(a)^2 / 12
        z = sp * sp / 12
        dz = p1[:, None, :] * da
        d2z = p1[:, None, :] * d2a + p2[:, None, :] * np.stack([da[:, k] * da[:, l] for k, l in _PAIRS], axis=1)
    W3, S3 = _softplus(get("layers__3__weights"))[0], _softplus(get("skip_layers__3__weights"))[0]
    h = d2z @ W3
    d2y = np.zeros((n, 3, 3), dtype=dtype)
    for c, (k, l) in enumerate(_PAIRS):
        d2y[:, k, l] = d2y[:, l, k] = h[:, c]
    return z @ W3 + x @ S3, dz @ W3 + S3[None], d2y


def _jets(K, weights, net, dtype):
    """(y1, y2) as Q lists of the network at the features K (3 x Q): in `dtype`, or in float32 (net = "fp32") and widened; net may
    also be a function x (n, 3) -> (dy (n, 3), d2y (n, 3, 3)), which is how the tests feed the chain rule derivatives of their own"""
    x = np.stack([k.v for k in K], axis=1)
    if callable(net):
        dy, d2y = net(x)
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            _, dy, d2y = network_jets(x, weights, np.float32) if net == "fp32" else network_jets_wide(x, weights, dtype)
    dy, d2y = np.asarray(dy).astype(dtype), np.asarray(d2y).astype(dtype)
    return [Q(dy[:, k]) for k in range(3)], {(k, l): Q(d2y[:, k, l]) for k in range(3) for l in range(3)}


def icnn3_ref(F, weights, net="fp64", dtype=LD):
    """-> (P, dP, magP, magdP) of F (n, 9) for the network `weights` (the golden's dict). net = "fp64": the network's value,
    gradient and Hessian in `dtype`; net = "fp32": from the float32 network of oracle.icnn_oracle, everything else in `dtype`.
    P = sum_k y_k dK_k + F H, H = -(sum_k y_k dK_k)(F = I) as in icnn3_cases.icnn3_stress_tangent."""
    F = np.asarray(F, dtype=dtype).reshape(-1, 9)
    K, dK, d2K, F3 = features_ref(F, dtype)
    P, dP = _chain(*_jets(K, weights, net, dtype), dK, d2K)
    K0, dK0, _, _ = features_ref(np.eye(3, dtype=dtype).reshape(1, 9), dtype)
    y0, _ = _jets(K0, weights, net, dtype)
    H = -total([(f"y{k} dK{k} at I", _col(y0[k], 1) * dK0[k]) for k in range(3)])
    H = Q(H.v.reshape(3, 3), H.m.reshape(3, 3))
    n = F.shape[0]
    FH = qsum("nic,ca->nia", F3, H)
    P = P + Q(FH.v.reshape(n, 9), FH.m.reshape(n, 9))
    eye = Q(np.eye(3, dtype=dtype))
    T = qsum("ij,ca->iajc", eye, H)
    dP = _symmetrised(dP + Q(T.v.reshape(1, 9, 9), T.m.reshape(1, 9, 9)))
    return P.v, dP.v, P.m, dP.m
