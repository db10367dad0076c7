"""AddressSanitizer + UBSan over the symbolic part of dxo_pmg_create (not gpu): csrc/pmg_symbolic.h, the transfer checks, the
transposed incidence and the coarse constrained list, is plain host C++. A stand-alone program with its own main
(tests/helpers/pmg_symbolic_main.cpp) runs it on small transfers, valid and malformed; nothing is loaded into Python and no call
reaches a device."""
import pathlib
import shutil
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_symbolic_part_is_clean_under_asan_ubsan(tmp_path):
    from dolfinx_external_operator_amd._build import CSRC, INCLUDE

    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "pmg_symbolic"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{INCLUDE}", f"-I{CSRC}", str(ROOT / "tests" / "helpers" / "pmg_symbolic_main.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert res.returncode == 0, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "ERROR: AddressSanitizer" not in res.stderr, res.stderr
    assert "pmg symbolic harness: ok" in res.stdout
