"""The array-free 3-D hyperelastic consumers in the C ABI and the Python layer: declared with their arity, exported, bound, refusing a
NULL context (not gpu)."""
import inspect
import re

from abi_header import HEADER, header_functions

# name -> number of parameters in include/dxo.h
ARITY = {"dxo_isihara3_residual": 5, "dxo_isihara3_tangent_apply": 6, "dxo_isihara3_tangent_diagonal": 5}


def test_declared_with_their_arity():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name, arity in ARITY.items():
        assert name in header_functions(), name
        found = re.findall(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert len(found) == 1, name
        params = [p.strip() for p in found[0].split(",")]
        assert len(params) == arity, (name, params)
        assert params[0] == "dxo_ctx* ctx" and params[1] == "const dxo_isihara_params* prm" and params[2] == "dxo_mesh* mesh", (name, params)
        assert all(p.startswith("const double*") for p in params[3:-1]) and params[-1].startswith("double*"), (name, params)


def test_exported_and_bound(hip_library):
    from dolfinx_external_operator_amd._lib import declared_symbols

    for name, arity in ARITY.items():
        assert hasattr(hip_library, name), name
        assert name in declared_symbols(), name
        assert len(getattr(hip_library, name).argtypes) == arity, name
    assert hip_library.dxo_abi_version() == 2


def test_null_context_is_refused_before_any_hip_call(hip_library):
    for name, arity in ARITY.items():
        assert getattr(hip_library, name)(*([None] * arity)) == -1, name


def test_python_surface():
    from dolfinx_external_operator_amd import DeviceMesh

    assert list(inspect.signature(DeviceMesh.isihara3_residual).parameters) == ["self", "prm", "u_ptr", "R_ptr"]
    assert list(inspect.signature(DeviceMesh.isihara3_tangent_apply).parameters) == ["self", "prm", "u_ptr", "v_ptr", "out_ptr"]
    assert list(inspect.signature(DeviceMesh.isihara3_tangent_diagonal).parameters) == ["self", "prm", "u_ptr", "out_ptr"]
    for fn in (DeviceMesh.isihara3_residual, DeviceMesh.isihara3_tangent_apply, DeviceMesh.isihara3_tangent_diagonal):
        assert fn.__doc__ and "dxo_" + fn.__name__ in fn.__doc__
