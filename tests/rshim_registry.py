"""What the .Call shim registers, against the reference's table, the shim's source and the overlay's list.  Kept apart
from tests/rshim_cases.py so that a host test which only asks whether a routine is carried loads no fixture and no
other test module.  Test infrastructure only."""
import os
import re

import rcall

_PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "matrixextra_amd")


def overlay_routines():
    """the names in .mxgpu_hot_routines of matrixextra_amd/R/mxgpu_overlay.R"""
    with open(os.path.join(_PKG, "R", "mxgpu_overlay.R")) as f:
        text = f.read()
    body = text[text.index(".mxgpu_hot_routines <- c(") + len(".mxgpu_hot_routines <- c("):]
    body = re.sub(r"#[^\n]*", "", body)
    return re.findall(r'"(\w+)"', body[:body.index(")")])


def defined_routines():
    """name -> number of parameters of every `SEXP _MatrixExtra_<name>(...)` definition in r_shim.cpp"""
    with open(os.path.join(_PKG, "csrc", "r_shim.cpp")) as f:
        text = f.read()
    return {name: len(params.split(",")) for name, params in re.findall(r"^SEXP _MatrixExtra_(\w+)\(([^)]*)\)", text, flags=re.M)}


def assert_shim_and_overlay_carry(name, arity):
    """`name` is registered by R_init_mxgpu_r with `arity` arguments under the exported symbol _MatrixExtra_<name>,
    that is the reference's arity, the definition takes that many parameters, and the overlay rebinds it"""
    shim = rcall.load(fake=True)
    assert name in shim.routines, f"R_init_mxgpu_r registers no _MatrixExtra_{name}"
    addr, n = shim.routines[name]
    assert n == arity == rcall.SIGNATURES[name]["arity"], f"{name}: registered with {n} arguments"
    assert addr == shim.symbol("_MatrixExtra_" + name), f"{name}: registered under another function"
    assert defined_routines()[name] == arity, f"{name}: the definition's parameter count"
    assert name in overlay_routines(), f"{name} is not in the overlay's .mxgpu_hot_routines"
