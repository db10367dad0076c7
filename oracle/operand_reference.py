"""Long-double restatement of the producer side (csrc/operand.hip, operand_facet.hip, operand_core.h, operand_cell.h) — TEST
INFRASTRUCTURE ONLY, NumPy only.

    operand of a Lagrange field at the quadrature points of cells        ref_operand          (dxo_eval_operand)
    the same at the facet points of (cell, local facet) pairs           ref_operand_facets   (dxo_eval_operand_facets)
    the operand x = SpatialCoordinate                                   ref_coordinate       (dxo_eval_coordinate)

The statements are those of oracle/operand_oracle.py (grad u = sum_a u_a (x) (dphi_a K), K = J^-1 from the coordinate element, then
the operand's shape), with K by cofactors because np.linalg has no long double. Every function returns, next to the value, `mag`:
the same expression with the absolute value of every factor,

    value                 sum_a |u_a| |phi_a|
    gradient  g_ij        sum_a |u_a,i| sum_k |dphi_a,k| |K_kj|                      (K formed in `dtype`)
    eps, div              their sums of gradient entries, on the gradient's mag; the zz slot of 2-D eps is an exact 0 with mag 0
    F                     |delta_ij| + the gradient's mag
    C, I1, detF           their own formulas on F_mag, every product and every term of the cofactor expansion taken positive

so that a float64 evaluation, in any order and with or without fused multiply-adds, stays within a small multiple of 2^-53 * mag[k]
in EVERY entry k (tests/test_operand_reference_*.py; the figure is oracle.consumer_reference.worst_ratio). What mag does not contain
is the rounding of J itself, a difference of vertex coordinates: every float64 evaluation loses that alike, and the constants of
tests/operand_cases.py measure it. All arithmetic runs in `dtype` (np.longdouble: 64-bit mantissa on x86-64); dtype = np.float64
gives the float64 twin of the same statements.
"""
from __future__ import annotations

import itertools

import numpy as np

from oracle.consumer_reference import LD, inverse_and_det, worst_ratio  # noqa: F401  (worst_ratio: re-exported for the tests)
from oracle.operand_oracle import CAUCHY_GREEN, DEFGRAD, DETF, DIV, EPS_MANDEL, GRAD, I1, VALUE, VALUE_GRAD

# the reference has to be more precise than what it judges (the rule of oracle/consumer_reference.py, restated where it is relied on)
assert np.finfo(LD).eps <= 2.0 ** -63, f"np.longdouble has eps = {np.finfo(LD).eps}: no extended precision on this platform"

KIND_ID = {"value": VALUE, "grad": GRAD, "eps": EPS_MANDEL, "F": DEFGRAD, "value_grad": VALUE_GRAD, "C": CAUCHY_GREEN, "I1": I1,
           "detF": DETF, "div": DIV}
NEEDS_VECTOR = (EPS_MANDEL, DEFGRAD, CAUCHY_GREEN, I1, DETF, DIV)


def value_size(kind, bs, gdim):
    kind = KIND_ID.get(kind, kind)
    if kind in NEEDS_VECTOR and bs != gdim:
        raise ValueError("eps / F / C / I1 / detF / div need a vector field with bs = gdim")
    return {VALUE: bs, GRAD: bs * gdim, VALUE_GRAD: bs * (1 + gdim), EPS_MANDEL: 4 if gdim == 2 else 6, DEFGRAD: gdim * gdim,
            CAUCHY_GREEN: gdim * gdim, I1: 1, DETF: 1, DIV: 1}[kind]


def _shape(kind, val, val_mag, g, g_mag):
    """(value, mag) of the operand from the field's value (nc, nq, bs) and gradient (nc, nq, bs, G), each with its mag."""
    nc, nq, bs, G = g.shape
    dtype = g.dtype
    if kind == VALUE:
        return val, val_mag
    if kind == GRAD:
        return g.reshape(nc, nq, bs * G), g_mag.reshape(nc, nq, bs * G)
    if kind == VALUE_GRAD:
        return (np.concatenate([val, g.reshape(nc, nq, bs * G)], axis=2),
                np.concatenate([val_mag, g_mag.reshape(nc, nq, bs * G)], axis=2))
    if kind == EPS_MANDEL:
        r = np.sqrt(dtype.type(2)) / 2
        pairs = [(0, 1)] if G == 2 else [(0, 1), (0, 2), (1, 2)]
        out = []
        for a in (g, g_mag):
            e = np.zeros((nc, nq, 4 if G == 2 else 6), dtype=dtype)          # 2-D: slot 2 (zz) stays an exact zero
            for i in range(G):
                e[..., i] = a[..., i, i]
            for s, (i, j) in enumerate(pairs):
                e[..., 3 + s] = r * (a[..., i, j] + a[..., j, i])
            out.append(e)
        return tuple(out)
    if kind == DIV:
        return np.einsum("cqii->cq", g)[..., None], np.einsum("cqii->cq", g_mag)[..., None]
    eye = np.eye(G, dtype=dtype)
    F, Fm = g + eye, g_mag + eye
    if kind == DEFGRAD:
        return F.reshape(nc, nq, G * G), Fm.reshape(nc, nq, G * G)
    if kind == CAUCHY_GREEN:
        return (np.einsum("cqki,cqkj->cqij", F, F).reshape(nc, nq, G * G), np.einsum("cqki,cqkj->cqij", Fm, Fm).reshape(nc, nq, G * G))
    if kind == I1:
        return np.einsum("cqij,cqij->cq", F, F)[..., None], np.einsum("cqij,cqij->cq", Fm, Fm)[..., None]
    if kind == DETF:
        det, per = np.zeros((nc, nq), dtype=dtype), np.zeros((nc, nq), dtype=dtype)
        for p in itertools.permutations(range(G)):
            sign = np.linalg.det(np.eye(G)[list(p)])                        # +1 / -1 exactly
            term, term_mag = np.ones((nc, nq), dtype=dtype), np.ones((nc, nq), dtype=dtype)
            for i in range(G):
                term, term_mag = term * F[..., i, p[i]], term_mag * Fm[..., i, p[i]]
            det = det + (term if sign > 0 else -term)
            per = per + term_mag
        return det[..., None], per[..., None]
    raise ValueError(kind)


def _evaluate(kind, U, X, phi, dphi, dpsi):
    """U (nc, nd, bs) dofs, X (nc, ng, G) vertices of the cells, tables of ONE point set: phi (nq, nd), dphi (nq, nd, G),
    dpsi (nq, ng, G) -> (value, mag), each (nc, nq, value_size)."""
    Ua, pa, da = np.abs(U), np.abs(phi), np.abs(dphi)
    val, val_mag = np.einsum("cai,qa->cqi", U, phi), np.einsum("cai,qa->cqi", Ua, pa)
    J = np.einsum("cvj,qvk->cqjk", X, dpsi)                                      # dx_j / dxi_k
    K, _ = inverse_and_det(J)                                                    # dxi_k / dx_j
    g = np.einsum("cqik,cqkj->cqij", np.einsum("cai,qak->cqik", U, dphi), K)     # du_i / dx_j
    g_mag = np.einsum("cai,cqaj->cqij", Ua, np.einsum("qak,cqkj->cqaj", da, np.abs(K)))
    return _shape(kind, val, val_mag, g, g_mag)


def _cells(mesh, cells):
    return np.arange(mesh.num_cells) if cells is None else np.asarray(cells, dtype=np.int64).reshape(-1)


def ref_operand(mesh, kind, bs, u, cells=None, dtype=LD):
    """-> (value, mag), each (n_cells, nq, value_size). kind: a name of KIND_ID or the oracle's integer; u: the blocked field vector
    (num_field_nodes * bs); cells: an entity list (repeats allowed, may be empty) or None for all cells of a tools.synthetic mesh."""
    kind = KIND_ID.get(kind, kind)
    G = mesh.gdim
    value_size(kind, bs, G)
    cells = _cells(mesh, cells)
    U = np.asarray(u, dtype=dtype).reshape(-1, bs)[mesh.dofmap[cells]]
    X = np.asarray(mesh.x, dtype=dtype)[:, :G][mesh.geom_dofmap[cells]]
    with np.errstate(invalid="ignore", over="ignore"):                          # non-finite dofs are legitimate input (confinement tests)
        return _evaluate(kind, U, X, *(np.asarray(t, dtype=dtype) for t in (mesh.phi, mesh.dphi, mesh.dpsi)))


def ref_operand_facets(mesh, kind, bs, u, phi_f, dphi_f, dpsi_f, entities, dtype=LD):
    """-> (value, mag), each (n_entities, nq_facet, value_size), for (cell, local facet) pairs and the per-facet tables that
    eval_operand_facets / DeviceMesh.set_facet_tables take: phi_f (nf, nq, nd), dphi_f (nf, nq, nd, G), dpsi_f (nf, nq, ng, G)."""
    kind = KIND_ID.get(kind, kind)
    G = mesh.gdim
    D = value_size(kind, bs, G)
    ents = np.asarray(entities, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((ents.shape[0], np.asarray(phi_f).shape[1], D), dtype=dtype)
    mag = np.zeros_like(out)
    ud = np.asarray(u, dtype=dtype).reshape(-1, bs)
    xd = np.asarray(mesh.x, dtype=dtype)[:, :G]
    for f in np.unique(ents[:, 1]):
        sel = np.flatnonzero(ents[:, 1] == f)
        c = ents[sel, 0]
        with np.errstate(invalid="ignore", over="ignore"):
            out[sel], mag[sel] = _evaluate(kind, ud[mesh.dofmap[c]], xd[mesh.geom_dofmap[c]],
                                           *(np.asarray(t[f], dtype=dtype) for t in (phi_f, dphi_f, dpsi_f)))
    return out, mag


def ref_coordinate(mesh, cells=None, dtype=LD):
    """The operand x: -> (x_q, mag), each (n_cells, nq, gdim), x_q = sum_v psi_v(xi_q) X_v and mag the same with |psi_v| |X_v|."""
    G = mesh.gdim
    X = np.asarray(mesh.x, dtype=dtype)[:, :G][mesh.geom_dofmap[_cells(mesh, cells)]]
    psi = np.asarray(mesh.psi, dtype=dtype)
    return np.einsum("qv,cvj->cqj", psi, X), np.einsum("qv,cvj->cqj", np.abs(psi), np.abs(X))
