"""The .Call shim's own refusals (matrixextra_amd/csrc/r_shim.cpp), on the CPU over the fake C-ABI of
tests/test_rshim_host.py: every length or type check the shim makes before it calls the library.

Each case takes the recorded call of rshim_cases.first_cases() for a routine and spoils one argument: a vector one
element short ("short"), empty ("empty": an indptr of length 0), one element long ("long": the recorded
sort_coo_indices_* triplets are empty, so nothing can be taken away), passed as a vector of another R type ("as"), or a
scalar that disagrees with the indptr ("set").  The call must end in Rf_error with exactly the message below, before
any C-ABI call, with no handle begun, nothing left protected or preserved, and the arguments as they were; plain and
under the gctorture-like mode.

REFUSALS lists every refusal of the shim (the messages are the literals of r_shim.cpp; test_every_refusal_is_listed
reads the source to hold the table to that), every disjunct of a compound condition, through every registered routine
that can reach it.  Everything is exact; there is no tolerance to choose."""
import os
import re

import numpy as np
import pytest

import rcall
import rshim_cases as RC
from test_rshim_host import fresh, ledger, shim  # noqa: F401  (fixtures)

CASES = RC.first_cases()
LGL, INT, REAL = rcall.LGLSXP, rcall.INTSXP, rcall.REALSXP


def short(k):
    return (f"arg{k} short", ("short", k))


def empty(k):
    return (f"arg{k} empty", ("empty", k))


def longer(k):
    return (f"arg{k} long", ("long", k))


def as_type(k, sxp):
    return (f"arg{k} as {({LGL: 'logical', INT: 'integer', REAL: 'double'})[sxp]}", ("as", k, sxp))


def both(a, b):
    return (a[0] + ", " + b[0],) + a[1:] + b[1:]


def kinds(stem, *which):
    return [f"{stem}_{k}" for k in which]


CSC_DENSE = (kinds("multiply_csc_by_dense_ignore_NAs", "numeric", "float32", "integer", "logical")
             + kinds("multiply_csc_by_dense_keep_NAs", "numeric", "float32", "integer", "logical")
             + ["logicaland_csc_by_dense_ignore_NAs"])
CSR_BY_COO = ["multiply_csr_by_coo_elemwise", "logicaland_csr_by_coo_elemwise"]
CSR_BY_SVEC = ["multiply_csr_by_svec_no_NAs", "multiply_csr_by_svec_keep_NAs"]
ASSIGN_SMAT = ["set_rowseq_to_smat", "set_arbitrary_rows_to_smat"]
ASSIGN_SCALAR = [n for n in RC.AM.ORDER if n not in ASSIGN_SMAT]
NVL = ("numeric", "logical")
NLB = ("numeric", "logical", "binary")

# (the shim's message, the routines that can reach it, the spoils: one for each side or disjunct of the condition)
REFUSALS = [
    ("reverse_columns_inplace: integer index vectors required", kinds("reverse_columns_inplace", *NLB),
     [as_type(0, REAL), as_type(1, REAL)]),
    ("multiply_csr_by_dvec_with_NAs: indices and values have different length", ["multiply_csr_by_dvec_with_NAs"],
     [short(2), short(1)]),
    ("mxgpu_csr_transpose: values must be double, logical or NULL", ["mxgpu_csr_transpose"], [as_type(2, INT)]),
    ("mxgpu_coo_to_csr: row and column indices have different length", ["mxgpu_coo_to_csr"], [short(1), short(0)]),
    ("mxgpu_coo_to_csr: values must be double, logical or NULL", ["mxgpu_coo_to_csr"], [as_type(2, INT)]),
    ("mxgpu_coo_to_csr: values and indices have different length", ["mxgpu_coo_to_csr"],
     [short(2), both(short(2), as_type(2, LGL))]),
    ("multiply_csr_by_coo: indptr does not match max_row_X", CSR_BY_COO,
     [("max_row_X one more", ("set", 6, 16)), short(0)]),
    ("multiply_csr_by_coo: bad COO lengths", CSR_BY_COO, [short(4), short(5)]),
    ("slice_coo_single: row and column indices have different length", kinds("slice_coo_single", *NLB),
     [short(1), short(0)]),
    ("slice_coo_single: values and indices have different length", kinds("slice_coo_single", *NVL), [short(2)]),
    ("slice_coo_arbitrary: row and column indices have different length", kinds("slice_coo_arbitrary", *NLB),
     [short(1), short(0)]),
    ("slice_coo_arbitrary: values and indices have different length", kinds("slice_coo_arbitrary", *NVL), [short(2)]),
    ("remove_zero_valued_csr: indices and values have different length", kinds("remove_zero_valued_csr", *NVL),
     [short(2), short(1)]),
    ("remove_zero_valued_coo: bad lengths", kinds("remove_zero_valued_coo", *NVL), [short(1), short(2)]),
    ("remove_zero_valued_svec: indices and values have different length",
     kinds("remove_zero_valued_svec", "numeric", "integer", "logical"), [short(1), short(0)]),
    ("check_valid_coo_matrix: row and column indices have different length", ["check_valid_coo_matrix"],
     [short(1), short(0)]),
    ("multiply_csc_by_dense: indices and values have different length", CSC_DENSE, [short(2), short(1)]),
    # the dense operand's rows are its own, so only its column count can disagree: with the index pointer
    ("multiply_csc_by_dense: dense matrix does not match", CSC_DENSE, [short(0)]),
    ("multiply_csr_by_svec: indices and values have different length", CSR_BY_SVEC, [short(2), short(1)]),
    ("multiply_csr_by_svec: vector indices and values differ", CSR_BY_SVEC, [short(4), short(3)]),
    ("matmul_colvec_by_scolvecascsr: values shorter than the index pointer says",
     ["matmul_colvec_by_scolvecascsr", "matmul_colvec_by_scolvecascsr_f32"], [empty(1), short(3)]),
    ("matmul_spcolvec_by_scolvecascsr: vector indices and values differ",
     kinds("matmul_spcolvec_by_scolvecascsr", "numeric", "integer", "logical"), [short(4), short(3)]),
    ("matmul_spcolvec_by_scolvecascsr: values shorter than the index pointer says",
     kinds("matmul_spcolvec_by_scolvecascsr", "numeric", "integer", "logical", "binary"), [empty(0), short(2)]),
    ("matmul_rowvec_by_csc: indices / values shorter than the index pointer says", ["matmul_rowvec_by_csc"],
     [empty(1), short(2), short(3)]),
    ("matmul_rowvec_by_csc: indices / values shorter than the index pointer says", ["matmul_rowvec_by_cscbin"],
     [empty(1), short(2)]),
    ("sort_vector_indices: indices must be an integer vector",
     kinds("sort_vector_indices", "numeric", "integer", "logical", "binary"), [as_type(0, REAL)]),
    ("sort_vector_indices: values do not match", ["sort_vector_indices_numeric"], [as_type(1, LGL), short(1)]),
    ("sort_vector_indices: values do not match", ["sort_vector_indices_integer"], [as_type(1, LGL), short(1)]),
    ("sort_vector_indices: values do not match", ["sort_vector_indices_logical"], [as_type(1, INT), short(1)]),
    ("sort_coo_indices: indices must be integer vectors", kinds("sort_coo_indices", *NLB),
     [as_type(0, REAL), as_type(1, REAL)]),
    ("sort_coo_indices: indices do not match", kinds("sort_coo_indices", *NLB), [longer(1), longer(0)]),
    ("sort_coo_indices: values do not match", ["sort_coo_indices_numeric"], [as_type(2, LGL), longer(2)]),
    ("sort_coo_indices: values do not match", ["sort_coo_indices_logical"], [as_type(2, REAL), longer(2)]),
    ("assignment: indices and values have different length", ASSIGN_SCALAR, [short(2), short(1)]),
    # X's values against its indices, the assigned matrix's values against its indices, an assigned indptr of length 0
    ("assignment: indices and values have different length", ["set_rowseq_to_smat"], [short(2), short(7), empty(5)]),
    ("assignment: indices and values have different length", ["set_arbitrary_rows_to_smat"],
     [short(2), short(6), empty(4)]),
]
PARAMS = [pytest.param(name, spoil[1:], message, id=f"{name}-{spoil[0]}")
          for message, names, spoils in REFUSALS for name in names for spoil in spoils]


def spoiled(case, ops):
    """the recorded arguments with `ops` applied, and the as_types of rcall's call"""
    live, as_types = case.live(), {}
    for op in ops:
        kind, k = op[0], op[1]
        if kind == "as":
            as_types[k] = op[2]
        elif kind == "set":
            assert live[k] != op[2]
            live[k] = op[2]
        else:
            a = live[k]
            assert isinstance(a, np.ndarray) and a.ndim == 1, f"{case.name}: argument {k} is no vector"
            if kind == "short":
                assert a.size >= 1, f"{case.name}: argument {k} is empty already"
                live[k] = a[:-1].copy()
            elif kind == "empty":
                live[k] = a[:0].copy()
            else:
                live[k] = np.concatenate([a, np.zeros(1, dtype=a.dtype)])
    return live, as_types


@pytest.mark.parametrize("name, ops, message", PARAMS)
def test_refusal(fresh, name, ops, message):  # noqa: F811
    case = CASES[name]
    for torture in (False, True):
        fresh.lib.fake_reset()
        fresh.reset()
        fresh.torture(torture)
        live, as_types = spoiled(case, ops)
        kept = [a.copy() if isinstance(a, np.ndarray) else a for a in live]
        what = f"{name} {ops} torture={torture}"
        with pytest.raises(rcall.RError) as err:
            fresh.call(name, live, as_types=as_types)
        assert str(err.value) == message, what
        assert fresh.lib.fake_calls() == 0, f"{what}: a C-ABI call was made before the refusal"
        led = ledger(fresh)
        assert all(v == 0 for v in led.values()), f"{what}: {led}"
        fresh.assert_clean(what)
        assert fresh.arguments_after() == fresh.last["before"], f"{what}: an argument changed"
        assert not any(fresh.lib.rstub_dead(s) for s in fresh.last["sexps"]), f"{what}: an argument was collected"
        for a, b in zip(live, kept):
            assert not isinstance(a, np.ndarray) or a.tobytes() == b.tobytes(), what


def test_every_refusal_is_listed(shim):  # noqa: F811
    """the table holds every "<family>: <text>" literal of the shim's source and nothing else, and names registered
    routines only"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "matrixextra_amd", "csrc",
                        "r_shim.cpp")
    with open(path) as f:
        code = re.sub(r"//[^\n]*", "", f.read())
    literals = set(re.findall(r'"(\w+: [^"]*)"', code))
    assert literals == {message for message, _, _ in REFUSALS}
    assert len(literals) == 30
    for _, names, _ in REFUSALS:
        for name in names:
            assert name in shim.routines, name
