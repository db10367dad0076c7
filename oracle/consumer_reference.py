"""Long-double restatement of the consumer side (csrc/adjoint.hip) — TEST INFRASTRUCTURE ONLY, NumPy only.

    internal force   f    = sum_cells sum_q w |det J| B^T S                 ref_adjoint_eps
    tangent action   K v  = sum_cells sum_q w |det J| B^T C B v             ref_tangent_apply
    its diagonal     K_kk = sum_cells sum_q w |det J| B[:, k]^T C B[:, k]   ref_tangent_diagonal
    C from the returned von Mises state (sigma, dp)                        vm_tangent_from_state

B is the strain operator of the eps / Mandel operand (oracle/operand_oracle.py EPS_MANDEL; in 2D the vector keeps its zero zz slot).
Every function returns, next to the value, `mag`: the same sum formed with the absolute value of every factor. A float64 evaluation
of the sum, in any order and with or without fused multiply-adds, stays within a small multiple of 2^-53 * mag[k] in EVERY entry k,
so mag is the scale a componentwise bound is stated in (tests/test_consumer_reference_*.py). All arithmetic runs in `dtype`
(np.longdouble: 64-bit mantissa on x86-64); dtype = np.float64 gives the float64 twin of the same statements, which the tests use to
measure what float64 NumPy itself loses against long double.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
# the reference has to be more precise than what it judges: 11 more bits than float64. Fail loudly where long double is double.
assert np.finfo(LD).eps <= 2.0 ** -63, f"np.longdouble has eps = {np.finfo(LD).eps}: no extended precision on this platform"


def inverse_and_det(J):
    """(..., G, G) -> (J^-1, det J) by cofactors (np.linalg has no long double)."""
    G = J.shape[-1]
    if G == 2:
        det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
        adj = np.empty_like(J)
        adj[..., 0, 0], adj[..., 1, 1] = J[..., 1, 1], J[..., 0, 0]
        adj[..., 0, 1], adj[..., 1, 0] = -J[..., 0, 1], -J[..., 1, 0]
        return adj / det[..., None, None], det
    cof = np.empty_like(J)
    for i in range(3):
        r = [k for k in range(3) if k != i]
        for j in range(3):
            c = [k for k in range(3) if k != j]
            minor = J[..., r[0], c[0]] * J[..., r[1], c[1]] - J[..., r[0], c[1]] * J[..., r[1], c[0]]
            cof[..., i, j] = minor if (i + j) % 2 == 0 else -minor
    det = (J[..., 0, :] * cof[..., 0, :]).sum(-1)
    return np.swapaxes(cof, -1, -2) / det[..., None, None], det


def mandel_B(gphys):
    """Physical gradients d phi_a / d x_j, (nc, nq, nd, G) -> B[c, q, d, a, i] with eps_mandel = sum_{a, i} B[..., a, i] v[a, i]."""
    nc, nq, nd, G = gphys.shape
    D = 4 if G == 2 else 6
    B = np.zeros((nc, nq, D, nd, G), dtype=gphys.dtype)
    r = np.sqrt(gphys.dtype.type(2)) / 2
    for i in range(G):
        B[:, :, i, :, i] = gphys[..., i]
    pairs = [(0, 1)] if G == 2 else [(0, 1), (0, 2), (1, 2)]
    for s, (i, j) in enumerate(pairs):
        B[:, :, 3 + s, :, i] = r * gphys[..., j]
        B[:, :, 3 + s, :, j] = r * gphys[..., i]
    return B


def strain_operator(mesh, dtype=LD):
    """-> (B (nc, nq, D, nd, G), scale (nc, nq) = w |det J|) of a tools.synthetic mesh."""
    G = mesh.gdim
    X = np.asarray(mesh.x, dtype=dtype)[:, :G][mesh.geom_dofmap]
    J = np.einsum("cvj,qvk->cqjk", X, np.asarray(mesh.dpsi, dtype=dtype))       # dx_j / dxi_k
    K, det = inverse_and_det(J)                                                  # dxi_k / dx_j
    gphys = np.einsum("qak,cqkj->cqaj", np.asarray(mesh.dphi, dtype=dtype), K)
    return mandel_B(gphys), np.asarray(mesh.weights, dtype=dtype)[None, :] * np.abs(det)


def _assemble(mesh, fe, fa):
    nn, G = mesh.node_x.shape[0], mesh.gdim
    out, mag = np.zeros((nn, G), fe.dtype), np.zeros((nn, G), fe.dtype)
    np.add.at(out, mesh.dofmap, fe)
    np.add.at(mag, mesh.dofmap, fa)
    return out.reshape(-1), mag.reshape(-1)


def _tangents(mesh, C, B, dtype):
    return np.asarray(C, dtype=dtype).reshape(B.shape[0], B.shape[1], B.shape[2], B.shape[2])


def ref_tangent_apply(mesh, C, v, dtype=LD, C_mag=None):
    """-> (Kv, mag). C: (num_cells * nq * D * D) entries in any shape. C_mag: the magnitudes to use for |C| where C is itself a
    sum that cancels (vm_tangent_from_state returns one); default |C|."""
    B, scale = strain_operator(mesh, dtype)
    Cl = _tangents(mesh, C, B, dtype)
    Ca = np.abs(Cl) if C_mag is None else _tangents(mesh, C_mag, B, dtype)
    V = np.asarray(v, dtype=dtype).reshape(-1, mesh.gdim)[mesh.dofmap]
    Ba = np.abs(B)
    fe = np.einsum("cq,cqdai,cqd->cai", scale, B, np.einsum("cqrs,cqs->cqr", Cl, np.einsum("cqdai,cai->cqd", B, V)))
    fa = np.einsum("cq,cqdai,cqd->cai", scale, Ba, np.einsum("cqrs,cqs->cqr", Ca, np.einsum("cqdai,cai->cqd", Ba, np.abs(V))))
    return _assemble(mesh, fe, fa)


def ref_tangent_diagonal(mesh, C, dtype=LD, C_mag=None):
    """-> (diag K, mag), formed directly from the columns of B (no probing with unit vectors)."""
    B, scale = strain_operator(mesh, dtype)
    Cl = _tangents(mesh, C, B, dtype)
    Ca = np.abs(Cl) if C_mag is None else _tangents(mesh, C_mag, B, dtype)
    Ba = np.abs(B)
    fe = np.einsum("cq,cqrai,cqrai->cai", scale, B, np.einsum("cqrs,cqsai->cqrai", Cl, B))
    fa = np.einsum("cq,cqrai,cqrai->cai", scale, Ba, np.einsum("cqrs,cqsai->cqrai", Ca, Ba))
    return _assemble(mesh, fe, fa)


def ref_adjoint_eps(mesh, S, dtype=LD):
    """-> (f, mag): the internal force of the Mandel stresses S (num_cells * nq * D entries in any shape)."""
    B, scale = strain_operator(mesh, dtype)
    Sl = np.asarray(S, dtype=dtype).reshape(B.shape[:3])
    fe = np.einsum("cq,cqdai,cqd->cai", scale, B, Sl)
    fa = np.einsum("cq,cqdai,cqd->cai", scale, np.abs(B), np.abs(Sl))
    return _assemble(mesh, fe, fa)


def vm_tangent_from_state(prm, sigma, dp, dtype=LD):
    """The consistent von Mises tangent from the RETURNED state, the closed form csrc/vm_core.h states (vm_tangent_state,
    vm_tangent_times): s = dev sigma, sigma_eq = sqrt(3/2 s.s), beta = 3 mu dp / (sigma_eq + 3 mu dp), n = s / sigma_eq [dp > 0],
    a = 3 mu (3 mu / (3 mu + H) - beta), b = 2 mu beta, C = C_elas - a n(x)n - b Dev on the Mandel vector. The producer's mark
    dp = -0.0 (the reference's 0/0 point) gives a = NaN. prm: anything with E, nu, H. sigma (..., d), dp (...) ->
    (C (n, d, d), C_mag (n, d, d)) with C_mag = |C_elas| + |a| |n(x)n| + |b| |Dev|."""
    E, nu, H = (dtype(float(getattr(prm, k))) for k in ("E", "nu", "H"))
    lmbda, mu = E * nu / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu))
    dp = np.asarray(dp, dtype=dtype).reshape(-1)
    d = np.asarray(sigma).size // dp.size
    sig = np.asarray(sigma, dtype=dtype).reshape(-1, d)
    one = np.zeros(d, dtype)
    one[:3] = 1
    C_el = lmbda * np.outer(one, one) + 2 * mu * np.eye(d, dtype=dtype)
    dev = np.eye(d, dtype=dtype) - np.outer(one, one) / dtype(3)
    s = sig @ dev.T
    seq = np.sqrt(dtype(3) / 2 * np.sum(s * s, axis=1))
    with np.errstate(all="ignore"):
        beta = 3 * mu * dp / (seq + 3 * mu * dp)
        n = s / seq[:, None] * (dp > 0)[:, None]
        a = 3 * mu * (3 * mu / (3 * mu + H) - beta)
        a = np.where((dp == 0) & np.signbit(dp), dtype(np.nan), a)
        b = 2 * mu * beta
        nn = n[:, :, None] * n[:, None, :]
        C = C_el[None] - a[:, None, None] * nn - b[:, None, None] * dev[None]
        C_mag = np.abs(C_el)[None] + np.abs(a)[:, None, None] * np.abs(nn) + np.abs(b)[:, None, None] * np.abs(dev)[None]
    return C, C_mag


def numpy_expand_tangent(sigma, dp, d, E=70e3, nu=0.3):
    """Float64 NumPy statement of the tangent-from-state formulas (dxo_vm_expand_tangent), the dp = -0.0 mark of the reference's
    0/0 point included: stand-in for the HIP rebuild kernel in the CPU-only gather test (tests/test_sharding.py), itself checked
    against the oracle's tangent there."""
    lmbda, mu = E * nu / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu))
    Et = E / 100.0
    H = E * Et / (E - Et)
    sigma = sigma.reshape(-1, d)
    one = np.zeros(d)
    one[:3] = 1.0
    C_el = lmbda * np.outer(one, one) + 2 * mu * np.eye(d)
    dev = np.eye(d) - np.outer(one, one) / 3.0
    s = sigma @ dev.T
    seq = np.sqrt(1.5 * np.sum(s * s, axis=1))
    with np.errstate(all="ignore"):
        beta = 3 * mu * dp / (seq + 3 * mu * dp)
        n = s / seq[:, None] * (dp > 0)[:, None]
    a = 3 * mu * (3 * mu / (3 * mu + H) - beta)
    a = np.where((dp == 0.0) & np.signbit(dp), np.nan, a)     # the producer's mark -> the reference's NaN tangent
    return C_el[None] - a[:, None, None] * n[:, :, None] * n[:, None, :] - (2 * mu * beta)[:, None, None] * dev[None]


def worst_ratio(got, ref, mag, extra=None):
    """max_k |got[k] - ref[k]| / (2^-53 * mag[k] (+ extra[k])) in long double; entries with a zero scale must agree exactly (-> inf
    if one does not). The componentwise figure every bound of the consumer tests is stated in."""
    err = np.abs(np.asarray(got, dtype=LD) - np.asarray(ref, dtype=LD))
    scale = LD(2.0) ** -53 * np.asarray(mag, dtype=LD) + (0 if extra is None else np.asarray(extra, dtype=LD))
    zero = scale == 0
    if np.any(err[zero] != 0):
        return float("inf")
    return float(np.max(err[~zero] / scale[~zero], initial=0.0))
