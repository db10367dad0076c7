"""The entry points of the compressed Krylov basis in the built library, the header and the binding (not gpu)."""
import ctypes as C
import inspect
import re

from abi_header import header_functions

NEW = ("dxo_krylov_create_basis", "dxo_krylov_basis_info")


def test_library_header_and_binding_carry_the_new_symbols(hip_library):
    from dolfinx_external_operator_amd._lib import declared_symbols

    for name in NEW:
        assert name in header_functions(), name
        assert hasattr(hip_library, name), f"{name} is not exported"
        assert name in declared_symbols(), name
    assert hip_library.dxo_abi_version() == 2                      # symbols were added, no struct changed
    blob = __import__("dolfinx_external_operator_amd._lib", fromlist=["LIB_PATH"]).LIB_PATH.read_bytes()
    # the float instantiations of the four row kernels, <T = float, FW> in their mangled names: kr_multidot<KMAX, f, FW> for some
    # KMAX and FW, the other three as <f, FW>
    for kernel in (rb"11kr_multidotILi\d+EfLi\d+EE", rb"9kr_updateIfLi\d+EE", rb"10kr_combineIfLi\d+EE", rb"14kr_scale_storeIfLi\d+EE"):
        assert re.search(kernel, blob), kernel


def test_argument_errors_without_a_device(hip_library):
    lib, h = hip_library, C.c_void_p()
    assert lib.dxo_krylov_create_basis(None, 10, 5, 1, C.byref(h)) == -1        # DXO_E_NULL before any HIP call
    assert lib.dxo_krylov_basis_info(None, None, None, None, None, None) == -1


def test_python_interface():
    from dolfinx_external_operator_amd import KrylovResult, cg, fgmres, gmres, krylov_basis_rows  # noqa: F401

    for f in (gmres, fgmres):
        assert inspect.signature(f).parameters["basis"].default == "fp64"
    assert "basis" not in inspect.signature(cg).parameters
    r = KrylovResult(None, 3, 0.5, True, False, 1, 2.0)            # the positional form of earlier versions
    assert (r.basis, r.basis_bytes, r.ms) == ("fp64", 0, 2.0)
