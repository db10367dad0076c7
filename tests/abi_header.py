"""The functions include/dxo.h declares, for the ABI tests. Not a test module."""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "dxo.h"


def header_functions():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(dxo_[a-z_0-9]+)\s*\(", text)))
