"""The transposed operators in the C ABI and the Python layer: declared, exported, bound, refusing a NULL context (not gpu)."""
import inspect

from abi_header import header_functions

NAMES = ("dxo_csr_transpose", "dxo_csr_spmv_t", "dxo_bilinear_apply_t")


def test_declared_exported_and_bound(hip_library):
    from dolfinx_external_operator_amd._lib import declared_symbols

    for name in NAMES:
        assert name in header_functions(), name
        assert hasattr(hip_library, name), name
        assert name in declared_symbols(), name
    assert hip_library.dxo_abi_version() == 2


def test_null_context_is_refused_before_any_hip_call(hip_library):
    lib = hip_library
    assert lib.dxo_csr_transpose(None, None, None, None) == -1
    assert lib.dxo_csr_spmv_t(None, None, None, 1.0, None, 0.0, None) == -1
    assert lib.dxo_bilinear_apply_t(None, None, 1, 1, 1, None, None, None) == -1


def test_python_surface():
    from dolfinx_external_operator_amd import DeviceMesh, krylov
    from dolfinx_external_operator_amd.operand_eval import DeviceCSR

    for fn in (DeviceCSR.matvec, krylov.csr_matvec):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "transpose" and params[-1].default is False
    assert list(inspect.signature(DeviceCSR.transpose).parameters) == ["self", "out"]
    assert inspect.signature(DeviceCSR.transpose).parameters["out"].default is None
    assert list(inspect.signature(DeviceMesh.bilinear_apply_t).parameters) == ["self", "test", "trial", "bs", "C_ptr", "v_ptr", "out_ptr"]
