"""AddressSanitizer + UBSan over the host side of csrc/functional.hip (not gpu): the argument checks its four entry points make
before their first HIP call. A stand-alone program with its own main (tests/helpers/functional_args_main.cpp) fills a context, a mesh
and facet sets in by hand and calls the entry points with NULL, misaligned, unsized and foreign arguments; only the HOST code is
instrumented (-Xarch_host), nothing is loaded into Python, and no call reaches a device."""
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_argument_checks_are_clean_under_asan_ubsan(tmp_path):
    from dolfinx_external_operator_amd._build import ARCH, CSRC, INCLUDE, _hipcc, build_library

    lib = build_library()          # the other translation units' symbols (dxo_operand_value_size, dxo_device_begin, ...)
    exe = tmp_path / "functional_args"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd = [_hipcc(), f"--offload-arch={ARCH}", "-x", "hip", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wno-cuda-compat",
           "-Wno-option-ignored", *(a for f in san for a in ("-Xarch_host", f)), f"-I{INCLUDE}", f"-I{CSRC}", str(CSRC / "functional.hip"),
           str(ROOT / "tests" / "helpers" / "functional_args_main.cpp"), "-o", str(exe), san[0], f"-L{lib.parent}", f"-l:{lib.name}",
           f"-Wl,-rpath,{lib.parent}"]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert res.returncode == 0, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "ERROR: AddressSanitizer" not in res.stderr, res.stderr
    assert "functional argument harness: ok" in res.stdout
