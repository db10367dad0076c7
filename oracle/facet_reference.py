"""Long-double restatement of the boundary-facet layer (csrc/facet_form.hip) — TEST INFRASTRUCTURE ONLY, NumPy only.

    normals and point measures       n = J^-T n_ref / |.|,  dS = w sqrt(det(J_f^T J_f))          ref_facet_geometry
    pressure load                    f[a, i] = scale sum_e sum_q dS p phi_a n_i                   ref_facet_pressure
    facet adjoint                    f = sum_e sum_q dS B^T S  (F as its linear part, grad)       ref_facet_adjoint
    bilinear form, value test side   K[(a,i),(b,j)] = sum_e sum_q dS phi_a sum_r C[i][r] (B_trial)_r,(b,j)
        its action K v               ref_facet_bilinear_apply
        its diagonal                 ref_facet_bilinear_diagonal   (from the columns of B, no probing)
        its element matrices         ref_facet_bilinear_elements   (scatter_dense / scatter_csr put them into a matrix)

The statements are those in the header comment of facet_form.hip: J = sum_v X_v dpsi_f,v from the facet dpsi table, K = J^-1 by
cofactors, J_f = J J_ref_f. `tabs` = (phi_f, dphi_f, dpsi_f) and `geom` = (weights, ref_normals, ref_jacobians) are the arrays
DeviceMesh.set_facet_tables / set_facet_geometry take, of any facet rule. Every function returns, next to the value, `mag`: the same
expression with the absolute value of every factor and term,

    K          K_mag = |K| + |K| J_mag |K|,  J_mag = sum_v |X_v| |dpsi_f,v|      (see below)
    n_j        sum_k K_mag,kj |n_ref,k| / |J^-T n_ref|
    dS         w sqrt(.) with J_f = J_mag |J_ref_f| and, in 3-D, both products of every cross-product component taken positive
    the sums   dS (one positive factor, formed in `dtype`) times |phi_a|, sum_k |dphi_a,k| K_mag,kj, |S|, |C|, |v|, |p|, |scale|, n's mag

so that a float64 evaluation, in any order and with or without fused multiply-adds, stays within a small multiple of 2^-53 * mag[k]
in EVERY entry k (tests/test_facet_reference_*.py). mag does not contain the rounding of dS where dS is a factor of a sum: every
float64 evaluation loses that alike, and the constants of tests/facet_reference_cases.py measure it.

Unlike oracle/consumer_reference.py and oracle/operand_reference.py, mag DOES contain the rounding of J, to first order: J is a sum
that cancels (a difference of vertex coordinates), a float64 evaluation leaves 2^-53 * J_mag in it, and K = J^-1 moves by K dJ K. On
the facets this cannot be left to the constants, because whole entries consist of nothing else: on a boundary face that lies in a
coordinate plane the tangential components of the normal, and with them of the pressure load and of the gradient kinds' results,
vanish identically, |K| alone gives them mag = 0 (or the 1e-17 the tables carry where they should hold a zero), and what a float64
evaluation leaves there depends on the order in which the four vertex terms of a hexahedron's face cancel. No multiple of such a
mag bounds two correct float64 evaluations against each other; with K_mag those entries are held to the size of J's rounding. The
price: K_mag exceeds |K| by about (coordinate / cell size), so the bound is that much wider on fine meshes far from the origin.

All arithmetic runs in `dtype`
(np.longdouble: 64-bit mantissa on x86-64); dtype = np.float64 gives the float64 twin of the same statements. This module imports none
of the float64 oracles it is used to judge.
"""
from __future__ import annotations

import types

import numpy as np

from oracle.consumer_reference import LD, inverse_and_det, worst_ratio  # noqa: F401  (worst_ratio: re-exported for the tests)

# the reference has to be more precise than what it judges (the rule of oracle/consumer_reference.py, restated where it is relied on)
assert np.finfo(LD).eps <= 2.0 ** -63, f"np.longdouble has eps = {np.finfo(LD).eps}: no extended precision on this platform"

KINDS = ("value", "grad", "value_grad", "eps", "div", "F")
NEEDS_VECTOR = ("eps", "div", "F")


def value_size(kind, G, bs):
    if kind not in KINDS:
        raise ValueError(f"unknown linear operand kind {kind!r}")
    if bs not in (1, G) or (kind in NEEDS_VECTOR and bs != G):
        raise ValueError(f"bs = {bs} does not fit kind {kind!r} on gdim {G}")
    return {"value": bs, "grad": bs * G, "value_grad": bs * (1 + G), "eps": 4 if G == 2 else 6, "div": 1, "F": G * G}[kind]


def _entities(ents):
    return np.asarray(ents, dtype=np.int64).reshape(-1, 2)


def _points(mesh, tabs, geom, ents, dtype):
    """Everything the sums need at the facet points of the entities, value and mag side by side."""
    G = mesh.gdim
    ents = _entities(ents)
    c, f = ents[:, 0], ents[:, 1]
    phi_f, dphi_f, dpsi_f = (np.asarray(t, dtype=dtype) for t in tabs)
    w, nref, jref = (np.asarray(t, dtype=dtype) for t in geom)
    w = w.reshape(-1)
    X = np.asarray(mesh.x, dtype=dtype)[:, :G][mesh.geom_dofmap[c]]
    J = np.einsum("evj,eqvk->eqjk", X, dpsi_f[f])                                # dx_j / dxi_k
    K, _ = inverse_and_det(J)                                                    # dxi_k / dx_j
    Jm = np.einsum("evj,eqvk->eqjk", np.abs(X), np.abs(dpsi_f[f]))               # the sum J with every term positive
    Ka = np.abs(K)
    Ka = Ka + np.einsum("eqkj,eqjl,eqlm->eqkm", Ka, Jm, Ka)                      # |K| + |K| J_mag |K|: K's mag (module docstring)
    nv = np.einsum("eqkj,ek->eqj", K, nref[f])                                   # J^-T n_ref
    nv_mag = np.einsum("eqkj,ek->eqj", Ka, np.abs(nref[f]))
    norm = np.sqrt(np.sum(nv * nv, axis=2, keepdims=True))
    Jf = np.einsum("eqjk,ekl->eqjl", J, jref[f])
    Jfa = np.einsum("eqjk,ekl->eqjl", Jm, np.abs(jref[f]))
    if G == 2:
        under, under_mag = np.sum(Jf[..., 0] ** 2, axis=2), np.sum(Jfa[..., 0] ** 2, axis=2)
    else:
        under, under_mag = np.zeros(J.shape[:2], dtype), np.zeros(J.shape[:2], dtype)
        for i, j in ((1, 2), (2, 0), (0, 1)):                                    # |a x b|^2 of the columns of J_f
            under = under + (Jf[..., i, 0] * Jf[..., j, 1] - Jf[..., j, 0] * Jf[..., i, 1]) ** 2
            under_mag = under_mag + (Jfa[..., i, 0] * Jfa[..., j, 1] + Jfa[..., j, 0] * Jfa[..., i, 1]) ** 2
    phi, dphi = phi_f[f], dphi_f[f]
    return types.SimpleNamespace(
        G=G, cells=c, n=nv / norm, n_mag=nv_mag / norm, dS=w[None, :] * np.sqrt(under), dS_mag=np.abs(w)[None, :] * np.sqrt(under_mag),
        phi=phi, phi_mag=np.abs(phi), gphys=np.einsum("eqak,eqkj->eqaj", dphi, K),          # d phi_a / d x_j
        gphys_mag=np.einsum("eqak,eqkj->eqaj", np.abs(dphi), Ka))


def _node_sum(mesh, cells, bs, fe, fa):
    nn = mesh.node_x.shape[0]
    out, mag = np.zeros((nn, bs), fe.dtype), np.zeros((nn, bs), fe.dtype)
    np.add.at(out, mesh.dofmap[cells], fe)
    np.add.at(mag, mesh.dofmap[cells], fa)
    return out.reshape(-1), mag.reshape(-1)


def _dual(kind, G, bs, S):
    """The value part vh (n, nq, bs) and the dual tensor gh (n, nq, bs, G) of operand values S (n, nq, D): the pairing
    S . operand(v) = vh . v + gh : grad v. Every coefficient is positive, so the same call on |S| gives the mags."""
    ne, nq = S.shape[:2]
    vh, gh = np.zeros((ne, nq, bs), S.dtype), np.zeros((ne, nq, bs, G), S.dtype)
    if kind == "value":
        vh = S
    elif kind in ("grad", "F"):
        gh = S.reshape(ne, nq, bs, G)
    elif kind == "value_grad":
        vh, gh = S[..., :bs], S[..., bs:].reshape(ne, nq, bs, G)
    elif kind == "div":
        for i in range(G):
            gh[..., i, i] = S[..., 0]
    else:                                                                         # eps, Mandel: the zz slot of 2-D pairs with nothing
        r = np.sqrt(S.dtype.type(2)) / 2
        for i in range(G):
            gh[..., i, i] = S[..., i]
        for s, (i, j) in enumerate([(0, 1)] if G == 2 else [(0, 1), (0, 2), (1, 2)]):
            gh[..., i, j] = gh[..., j, i] = r * S[..., 3 + s]
    return vh, gh


def _trial_operator(kind, G, bs, phi, gphys):
    """B (n, nq, D, nd, bs) with operand_r = sum_{b, j} B[r, b, j] v[b, j] (F: its linear part). Every coefficient is positive, so the
    same call on (|phi|, the gradient's mag) gives B's mag."""
    ne, nq, nd = phi.shape
    B = np.zeros((ne, nq, value_size(kind, G, bs), nd, bs), phi.dtype)
    row = 0
    if kind in ("value", "value_grad"):
        for i in range(bs):
            B[:, :, i, :, i] = phi
        row = bs
    if kind in ("grad", "F", "value_grad"):
        for i in range(bs):
            for l in range(G):
                B[:, :, row + i * G + l, :, i] = gphys[..., l]
    elif kind == "div":
        for i in range(G):
            B[:, :, 0, :, i] = gphys[..., i]
    elif kind == "eps":
        r = np.sqrt(phi.dtype.type(2)) / 2
        for i in range(G):
            B[:, :, i, :, i] = gphys[..., i]
        for s, (i, j) in enumerate([(0, 1)] if G == 2 else [(0, 1), (0, 2), (1, 2)]):
            B[:, :, 3 + s, :, i] = r * gphys[..., j]
            B[:, :, 3 + s, :, j] = r * gphys[..., i]
    return B


def ref_facet_geometry(mesh, tabs, geom, ents, dtype=LD):
    """-> (n, n_mag (n_entities, nq, G), dS, dS_mag (n_entities, nq))."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = _points(mesh, tabs, geom, ents, dtype)
    return p.n, p.n_mag, p.dS, p.dS_mag


def ref_facet_pressure(mesh, tabs, geom, ents, p=None, scale=1.0, dtype=LD):
    """-> (f, mag), each (num_nodes * G,). p (n_entities, nq) in any shape, or None for p = 1."""
    with np.errstate(invalid="ignore", over="ignore"):
        g = _points(mesh, tabs, geom, ents, dtype)
        pv = np.ones(g.dS.shape, dtype) if p is None else np.asarray(p, dtype=dtype).reshape(g.dS.shape)
        sc = dtype(scale)
        fe = np.einsum("eq,eqi,eqa->eai", sc * g.dS * pv, g.n, g.phi)
        fa = np.einsum("eq,eqi,eqa->eai", np.abs(sc) * g.dS * np.abs(pv), g.n_mag, g.phi_mag)
        return _node_sum(mesh, g.cells, g.G, fe, fa)


def ref_facet_adjoint(mesh, tabs, geom, ents, kind, bs, S, dtype=LD):
    """-> (f, mag), each (num_nodes * bs,). S (n_entities, nq, value_size) in any shape."""
    with np.errstate(invalid="ignore", over="ignore"):
        g = _points(mesh, tabs, geom, ents, dtype)
        Sl = np.asarray(S, dtype=dtype).reshape(g.dS.shape + (value_size(kind, g.G, bs),))
        vh, gh = _dual(kind, g.G, bs, Sl)
        va, ga = _dual(kind, g.G, bs, np.abs(Sl))
        fe = np.einsum("eq,eqi,eqa->eai", g.dS, vh, g.phi) + np.einsum("eq,eqij,eqaj->eai", g.dS, gh, g.gphys)
        fa = np.einsum("eq,eqi,eqa->eai", g.dS, va, g.phi_mag) + np.einsum("eq,eqij,eqaj->eai", g.dS, ga, g.gphys_mag)
        return _node_sum(mesh, g.cells, bs, fe, fa)


def _form(mesh, tabs, geom, ents, trial, bs, C, dtype):
    g = _points(mesh, tabs, geom, ents, dtype)
    D = value_size(trial, g.G, bs)
    Cl = np.asarray(C, dtype=dtype).reshape(g.dS.shape + (bs, D))
    return g, Cl, _trial_operator(trial, g.G, bs, g.phi, g.gphys), _trial_operator(trial, g.G, bs, g.phi_mag, g.gphys_mag)


def ref_facet_bilinear_apply(mesh, tabs, geom, ents, trial, bs, C, v, dtype=LD):
    """-> (K v, mag), each (num_nodes * bs,). C (n_entities, nq, bs, value_size(trial)) in any shape."""
    with np.errstate(invalid="ignore", over="ignore"):
        g, Cl, B, Ba = _form(mesh, tabs, geom, ents, trial, bs, C, dtype)
        V = np.asarray(v, dtype=dtype).reshape(-1, bs)[mesh.dofmap[g.cells]]
        fe = np.einsum("eq,eqa,eqi->eai", g.dS, g.phi, np.einsum("eqir,eqr->eqi", Cl, np.einsum("eqrbj,ebj->eqr", B, V)))
        fa = np.einsum("eq,eqa,eqi->eai", g.dS, g.phi_mag,
                       np.einsum("eqir,eqr->eqi", np.abs(Cl), np.einsum("eqrbj,ebj->eqr", Ba, np.abs(V))))
        return _node_sum(mesh, g.cells, bs, fe, fa)


def ref_facet_bilinear_diagonal(mesh, tabs, geom, ents, trial, bs, C, dtype=LD):
    """-> (diag K, mag), each (num_nodes * bs,), formed directly from the columns of B (no probing with unit vectors)."""
    with np.errstate(invalid="ignore", over="ignore"):
        g, Cl, B, Ba = _form(mesh, tabs, geom, ents, trial, bs, C, dtype)
        fe = np.einsum("eq,eqa,eqai->eai", g.dS, g.phi, np.einsum("eqir,eqrai->eqai", Cl, B))
        fa = np.einsum("eq,eqa,eqai->eai", g.dS, g.phi_mag, np.einsum("eqir,eqrai->eqai", np.abs(Cl), Ba))
        return _node_sum(mesh, g.cells, bs, fe, fa)


def ref_facet_bilinear_elements(mesh, tabs, geom, ents, trial, bs, C, dtype=LD):
    """-> (Ke, mag), each (n_entities, nd * bs, nd * bs): the element matrix of every entity, rows a * bs + i, columns b * bs + j."""
    with np.errstate(invalid="ignore", over="ignore"):
        g, Cl, B, Ba = _form(mesh, tabs, geom, ents, trial, bs, C, dtype)
        ne, _, nd = g.phi.shape
        Ke = np.einsum("eqa,eqibj->eaibj", g.dS[..., None] * g.phi, np.einsum("eqir,eqrbj->eqibj", Cl, B))
        Ka = np.einsum("eqa,eqibj->eaibj", g.dS[..., None] * g.phi_mag, np.einsum("eqir,eqrbj->eqibj", np.abs(Cl), Ba))
        return Ke.reshape(ne, nd * bs, nd * bs), Ka.reshape(ne, nd * bs, nd * bs)


def element_dofs(mesh, ents, bs):
    """(n_entities, nd * bs): the blocked dofs node * bs + i of the entities' cells, in the order of the element matrices."""
    nodes = mesh.dofmap[_entities(ents)[:, 0]].astype(np.int64)
    return (nodes[:, :, None] * bs + np.arange(bs)[None, None, :]).reshape(nodes.shape[0], nodes.shape[1] * bs)


def scatter_dense(mesh, ents, bs, Ke):
    """The element matrices (or their mags) added into the dense (N, N) matrix, in Ke's dtype."""
    N = mesh.node_x.shape[0] * bs
    dofs = element_dofs(mesh, ents, bs)
    K = np.zeros((N, N), Ke.dtype)
    np.add.at(K, (dofs[:, :, None], dofs[:, None, :]), Ke)
    return K


def scatter_csr(mesh, ents, bs, Ke, indptr, indices):
    """The element matrices (or their mags, or ones: the number of entity contributions to an entry) added into the `values` array of
    a CSR pattern with sorted rows, in Ke's dtype. An entry outside the pattern is an error."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    N = indptr.size - 1
    keys = np.repeat(np.arange(N, dtype=np.int64), np.diff(indptr)) * N + indices
    assert np.all(np.diff(keys) > 0), "the pattern's rows are not sorted"
    dofs = element_dofs(mesh, ents, bs)
    want = (dofs[:, :, None] * N + dofs[:, None, :]).reshape(-1)
    pos = np.searchsorted(keys, want)
    assert want.size == 0 or (pos.max() < keys.size and np.array_equal(keys[pos], want)), "an element entry lies outside the pattern"
    values = np.zeros(keys.size, Ke.dtype)
    np.add.at(values, pos, np.asarray(Ke).reshape(-1))
    return values
