"""What the tests of the boundary-facet bilinear forms share (dxo_facet_bilinear_apply / _diagonal / _assemble): the NumPy oracle, a
composition of the facet oracles of tests/test_facet_oracle_cpu.py and oracle/operand_oracle.py, and the case lists. Not a test module.

The form is K[(a,i),(b,j)] = sum_e sum_q dS phi_a sum_r C[i][r] (B_trial)_r,(b,j). Its action on v is the facet adjoint of the VALUE
kind of S = C . operand_facets(trial, v); column c of the dense matrix is the action on the unit vector e_c. The columns are formed
one operand evaluation at a time and scattered by ONE call of facet_adjoint_ref, which takes the columns as extra components of a
VALUE load (the adjoint of VALUE treats every component alike). "F" is taken as its linearisation: its value at u = 0 is subtracted.
"""
import numpy as np

from oracle.operand_oracle import DEFGRAD, DIV, EPS_MANDEL, GRAD, VALUE, VALUE_GRAD, eval_operand_facets
from test_facet_oracle_cpu import CELLS, facet_adjoint_ref
from tools.synthetic import FACETS, exterior_facets, facet_tables, structured_mesh

KIND_ID = {"value": VALUE, "grad": GRAD, "eps": EPS_MANDEL, "F": DEFGRAD, "value_grad": VALUE_GRAD, "div": DIV}
# trial kinds and whether they take bs = 1 beside bs = gdim
TRIALS = [("value", True), ("grad", True), ("value_grad", True), ("eps", False), ("div", False), ("F", False)]
DEGREES = (1, 2)
ENTITY_LISTS = ("exterior", "subset", "all")
_CACHE = {}

__all__ = ["CELLS", "DEGREES", "ENTITY_LISTS", "KIND_ID", "TRIALS", "trial_cases", "value_size", "mesh_case", "entity_list", "random_block",
           "facet_operand_ref", "facet_bilinear_apply_ref", "facet_bilinear_dense_ref", "cached_dense_ref"]


def trial_cases(G):
    """[(trial, bs)]: every trial kind with every block size it takes on gdim G."""
    return [(k, bs) for k, scalar in TRIALS for bs in ((1, G) if scalar else (G,))]


def value_size(trial, G, bs):
    return {"value": bs, "grad": bs * G, "value_grad": bs * (1 + G), "eps": 4 if G == 2 else 6, "div": 1, "F": G * G}[trial]


def mesh_case(cell, degree, distort=0.2, seed=11, n=None):
    key = ("mesh", cell, degree, distort, seed, n)
    if key not in _CACHE:
        _CACHE[key] = structured_mesh(cell, CELLS[cell] if n is None else n, degree, distort=distort, seed=seed)
    return _CACHE[key]


def entity_list(m, which):
    """"exterior": the whole boundary in (cell, facet) order; "subset": two thirds of it, shuffled; "all": every local facet of every
    cell, interior facets included, so that a cell carries several entities."""
    if which == "exterior":
        return exterior_facets(m)
    if which == "subset":
        ents = exterior_facets(m)
        rng = np.random.Generator(np.random.PCG64(31))
        return np.ascontiguousarray(ents[rng.permutation(len(ents))[: max(3, len(ents) * 2 // 3)]])
    if which == "all":
        return np.array([(c, f) for c in range(m.num_cells) for f in range(len(FACETS[m.cell]))], dtype=np.int32)
    raise ValueError(which)


def random_block(m, ents, trial, bs, seed=17):
    """C (n, nq_facet, bs, D_trial), standard normal."""
    nq = facet_tables(m)[0].shape[1]
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.normal(size=(len(ents), nq, bs, value_size(trial, m.gdim, bs)))


def facet_operand_ref(m, ents, trial, bs, u):
    """(n, nq, D): the LINEAR part of the trial operand of u at the facet points."""
    phi_f, dphi_f, dpsi_f, _ = facet_tables(m)
    args = (m.dofmap, m.geom_dofmap, m.x, phi_f, dphi_f, dpsi_f, ents)
    e = eval_operand_facets(KIND_ID[trial], bs, u, *args)
    if trial == "F":
        e = e - eval_operand_facets(DEFGRAD, bs, np.zeros_like(u), *args)
    return e


def facet_bilinear_apply_ref(m, ents, trial, bs, C, v):
    """K v (num_nodes * bs,)."""
    e = facet_operand_ref(m, ents, trial, bs, v)
    S = np.einsum("eqir,eqr->eqi", np.asarray(C).reshape(e.shape[0], e.shape[1], bs, -1), e)
    return facet_adjoint_ref(m, ents, VALUE, bs, S)


def facet_bilinear_dense_ref(m, ents, trial, bs, C):
    """K (num_nodes * bs, num_nodes * bs). Column c is facet_adjoint_ref(m, ents, VALUE, bs, C . eval_operand_facets(trial, bs, e_c));
    only the columns of the entities' cells can be nonzero."""
    ents = np.asarray(ents, dtype=np.int64)
    nn = m.node_x.shape[0]
    N = nn * bs
    K = np.zeros((N, N))
    if len(ents) == 0:
        return K
    phi_f, dphi_f, dpsi_f, _ = facet_tables(m)
    args = (m.dofmap, m.geom_dofmap, m.x, phi_f, dphi_f, dpsi_f, ents)
    nq = phi_f.shape[1]
    Cb = np.asarray(C, dtype=np.float64).reshape(len(ents), nq, bs, -1)
    nodes = np.unique(m.dofmap[ents[:, 0]])
    cols = (nodes[:, None] * bs + np.arange(bs)[None, :]).reshape(-1)
    zero = eval_operand_facets(DEFGRAD, bs, np.zeros(N), *args) if trial == "F" else 0.0
    S = np.empty((len(ents), nq, bs, cols.size))
    u = np.zeros(N)
    for k, c in enumerate(cols):
        u[c] = 1.0
        S[..., k] = np.einsum("eqir,eqr->eqi", Cb, eval_operand_facets(KIND_ID[trial], bs, u, *args) - zero)
        u[c] = 0.0
    # the columns as extra components of a VALUE load: component i * ncols + k
    out = facet_adjoint_ref(m, ents, VALUE, bs * cols.size, S.reshape(len(ents), nq, -1))
    K[:, cols] = out.reshape(nn, bs, cols.size).reshape(N, cols.size)
    return K


def cached_dense_ref(cell, degree, which, trial, bs):
    """(mesh, entities, C, K) of the named case, computed once per session and not to be written to."""
    key = ("dense", cell, degree, which, trial, bs)
    if key not in _CACHE:
        m = mesh_case(cell, degree)
        ents = entity_list(m, which)
        Cb = random_block(m, ents, trial, bs)
        K = facet_bilinear_dense_ref(m, ents, trial, bs, Cb)
        for a in (Cb, K):
            a.setflags(write=False)
        _CACHE[key] = (m, ents, Cb, K)
    return _CACHE[key]
