"""The p-multigrid on an operator in the C ABI and the Python layer: every dxo_pmg_* function declared with its arity, exported, bound,
refusing a NULL context; DXO_PC_PMG in the header; the Python surface and its docstrings (not gpu)."""
import inspect
import re

from abi_header import HEADER, header_functions

# name -> number of parameters in include/dxo.h
ARITY = {"dxo_pmg_create": 7, "dxo_pmg_destroy": 2, "dxo_pmg_set_smoother": 6, "dxo_pmg_setup": 5, "dxo_pmg_apply": 4,
         "dxo_pmg_restrict": 4, "dxo_pmg_prolong": 4, "dxo_pmg_info": 11}


def _declarations():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def test_declared_with_their_arity():
    text = _declarations()
    for name, arity in ARITY.items():
        assert name in header_functions(), name
        found = re.findall(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert len(found) == 1, name
        params = [p.strip() for p in found[0].split(",")]
        assert len(params) == arity, (name, params)
        assert params[0] == "dxo_ctx* ctx", (name, params)
    assert re.search(r"#define\s+DXO_PC_PMG\s+5\b", text)
    assert "typedef struct dxo_pmg dxo_pmg;" in text
    assert re.search(r"#define\s+DXO_ABI_VERSION\s+2\b", text)                     # no existing struct changed


def test_exported_and_bound(hip_library):
    from dolfinx_external_operator_amd._lib import declared_symbols

    for name, arity in ARITY.items():
        assert hasattr(hip_library, name), name
        assert name in declared_symbols(), name
        assert len(getattr(hip_library, name).argtypes) == arity, name
    assert hip_library.dxo_abi_version() == 2


def test_null_context_is_refused_before_any_hip_call(hip_library):
    import ctypes as C

    for name in ARITY:
        fn = getattr(hip_library, name)
        args = [0 if t in (C.c_int, C.c_int64) else 0.0 if t is C.c_double else None for t in fn.argtypes]      # NULL pointers, zero scalars
        assert fn(*args) == -1, name


def test_python_surface():
    import dolfinx_external_operator_amd as pkg
    from dolfinx_external_operator_amd import PMG, DeviceMesh
    from dolfinx_external_operator_amd import krylov

    assert "PMG" in pkg.__all__ and "PMG" in krylov.__all__ and krylov.PC_PMG == 5
    assert list(inspect.signature(PMG.__init__).parameters) == ["self", "transfer", "bs", "constrained", "ctx", "degree", "rho_iters", "lower",
                                                               "safety"]
    defaults = {k: v.default for k, v in inspect.signature(PMG.__init__).parameters.items()}
    assert (defaults["degree"], defaults["rho_iters"], defaults["lower"], defaults["safety"]) == (2, 10, 0.1, 1.1)
    assert list(inspect.signature(PMG.setup).parameters) == ["self", "A", "dinv", "coarse"]
    assert list(inspect.signature(PMG.apply).parameters) == ["self", "r", "out"]
    assert list(inspect.signature(DeviceMesh.vertex_mesh).parameters) == ["self", "psi", "dpsi", "weights"]
    assert "dxo_pmg_create" in PMG.__doc__
    for fn, entry in ((PMG.setup, "dxo_pmg_setup"), (PMG.apply, "dxo_pmg_apply"), (PMG.restrict, "dxo_pmg_restrict"),
                      (PMG.prolong, "dxo_pmg_prolong"), (PMG.set_smoother, "dxo_pmg_set_smoother"), (PMG.close, "dxo_pmg_destroy")):
        assert fn.__doc__ and entry in fn.__doc__, entry
    for prop in ("rho", "pairs", "n_coarse", "coarse_constrained", "matvecs_per_apply"):
        assert isinstance(getattr(PMG, prop), property), prop
    for solver in (krylov.gmres, krylov.cg, krylov.fgmres):
        assert "M" in inspect.signature(solver).parameters
    assert "PMG" in krylov.gmres.__doc__


def test_synthetic_companion_is_the_degree_one_mesh():
    import numpy as np

    from tools.synthetic import LagrangeElement, structured_mesh, vertex_companion

    m = structured_mesh("tetrahedron", (2, 2, 2), 2, distort=0.1, seed=2)
    pts, w = np.array([[0.25, 0.25, 0.25]]), np.array([1.0 / 6.0])
    c = vertex_companion(m, pts, w)
    assert c.degree == 1 and c.dofmap is m.geom_dofmap and c.node_x is m.x and c.nq == 1
    psi, dpsi = LagrangeElement("tetrahedron", 1).tabulate(pts)
    assert np.array_equal(c.phi, psi) and np.array_equal(c.dphi, dpsi) and np.array_equal(c.dpsi, dpsi) and np.array_equal(c.weights, w)
    same = vertex_companion(m)
    assert np.array_equal(same.points, m.points) and np.array_equal(same.weights, m.weights) and np.array_equal(same.dpsi, m.dpsi)
