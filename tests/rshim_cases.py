"""One recorded call for every routine the .Call shim registers, and what its fixture implies about the R types of
the result.  Shared by tests/test_rshim_host.py (lifecycle over the fake C-ABI) and tests/test_gpu_rshim.py.

Sources: tests/golden/reference_golden.npz (reference-run, 70 routines), assign_golden.npz (22), coo_sort_golden.npz
(3), the cases of tests/test_gpu_outer.py (the 8 matmul_rowvec / colvec / spcolvec routines) and two small operands
for the shim's own mxgpu_csr_transpose / mxgpu_coo_to_csr.  Test infrastructure only.
"""
import numpy as np

import assign_model as AM
import coo_sort_model as CM
import rcall
import refpin
from rshim_registry import assert_shim_and_overlay_carry, defined_routines, overlay_routines  # noqa: F401
import test_gpu_outer as TO

# routines with records in reference_golden.npz that the shim deliberately does not carry: the gap
# may shrink, it must not grow unseen
NOT_IN_SHIM = sorted([
    "cbind_csr_numeric", "cbind_csr_logical", "cbind_csr_binary", "concat_csr_batch", "concat_indptr2",
    "matmul_csr_svec_numeric", "matmul_csr_svec_integer", "matmul_csr_svec_logical", "matmul_csr_svec_binary",
    "matmul_csr_svec_float32",
    "multiply_csr_by_dense_elemwise_double", "multiply_csr_by_dense_elemwise_float32",
    "multiply_csr_by_dense_elemwise_int", "multiply_csr_by_dense_elemwise_bool", "logicaland_csr_by_dense_cpp",
    "sort_sparse_indices_numeric", "sort_sparse_indices_logical", "sort_sparse_indices_binary",
    "check_indices_are_sorted",
])
# the sort_* and reverse_columns_inplace_* routines work on the caller's vectors where they are, so the shim coerces
# nothing there: an index vector of another type is refused with the family's message; so is a values vector of
# another type by the sort routines, while reverse_columns_inplace_* takes it as absent (only the indices move, as
# when Rcpp hands the reference a coerced copy of the values)
NO_COERCION = sorted(["sort_vector_indices_numeric", "sort_vector_indices_integer", "sort_vector_indices_logical",
                      "sort_vector_indices_binary", "sort_coo_indices_numeric", "sort_coo_indices_logical",
                      "sort_coo_indices_binary", "reverse_columns_inplace_numeric", "reverse_columns_inplace_logical",
                      "reverse_columns_inplace_binary"])
NO_COERCION_MESSAGE = {"sort_vector_indices": "sort_vector_indices: indices must be an integer vector",
                       "sort_coo_indices": "sort_coo_indices: indices must be integer vectors",
                       "reverse_columns_inplace": "reverse_columns_inplace: integer index vectors required"}
NO_COERCION_VALUES_MESSAGE = {"sort_vector_indices": "sort_vector_indices: values do not match",
                              "sort_coo_indices": "sort_coo_indices: values do not match"}
OUTER = ["matmul_rowvec_by_csc", "matmul_rowvec_by_cscbin", "matmul_colvec_by_scolvecascsr",
         "matmul_colvec_by_scolvecascsr_f32", "matmul_spcolvec_by_scolvecascsr_numeric",
         "matmul_spcolvec_by_scolvecascsr_integer", "matmul_spcolvec_by_scolvecascsr_logical",
         "matmul_spcolvec_by_scolvecascsr_binary"]
OWN = ["mxgpu_csr_transpose", "mxgpu_coo_to_csr"]

GOLDEN, _ = refpin.load()
ASSIGN, _ = AM.load()
COO_SORT, _ = CM.load()


class Case:
    """args as the caller passes them (fresh arrays), `same` as in a refpin record, and `out`: what the fixture holds
    for the call (only its kinds and shapes are used here)"""

    def __init__(self, name, args, out, same=None):
        self.name, self.args, self.out = name, list(args), out
        self.same = list(range(len(self.args))) if same is None else list(same)

    def live(self):
        live = [a.copy() if isinstance(a, np.ndarray) else a for a in self.args]
        for k, s in enumerate(self.same):
            live[k] = live[s]
        return live

    def __repr__(self):
        return self.name


def outer_case(name):
    """a small case of tests/test_gpu_outer.py for one of the eight routines, with its model's result"""
    p, j, x = TO.one_column(9, "mixed", 3)
    if name.startswith("matmul_colvec"):
        f32 = name.endswith("_f32")
        v = TO.dense_vector(5, 2)
        with np.errstate(invalid="ignore", over="ignore"):
            v = v.astype(np.float32) if f32 else v
        return Case(name, [v, p, j, x], TO.model_dense(v, p, x, f32))
    if name.startswith("matmul_spcolvec"):
        kind = name.rsplit("_", 1)[1]
        yi = np.array([1, 4, 7], dtype=np.int32)
        yv = TO.svec_values(kind, yi.size, 5)
        args = [p, j, x, yi, 7] if kind == "binary" else [p, j, x, yi, yv, 7]
        return Case(name, args, TO.model_svec(p, x, yi, yv, 7, kind))
    rng = np.random.default_rng(4)
    lens = np.array([0, 1, 3, 6])
    cp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.permutation(6)[:n]) for n in lens]).astype(np.int32)
    cx = rng.normal(size=ci.size)
    v = rng.normal(size=6).astype(np.float32)
    if name == "matmul_rowvec_by_csc":
        return Case(name, [v, cp, ci, cx], TO.model_rowvec(v, cp, ci, cx))
    return Case(name, [v, cp, ci], TO.model_rowvec(v, cp, ci, None))


def own_case(name):
    p = np.array([0, 2, 2, 3], dtype=np.int32)
    j = np.array([3, 0, 1], dtype=np.int32)
    x = np.array([1.5, -2.0, 4.0])
    out = dict(indptr=np.zeros(5, np.int32), indices=np.zeros(3, np.int32), values=np.zeros(3))
    if name == "mxgpu_csr_transpose":
        return Case(name, [p, j, x, 4], out)
    return Case(name, [np.array([0, 0, 2], dtype=np.int32), j, x, 3, 4], out)


def first_cases():
    """routine -> Case, for every routine that has a record somewhere"""
    cases = {}
    for rec in GOLDEN:
        if rec.err is None and rec.fn not in cases:
            cases[rec.fn] = Case(rec.fn, rec.args, rec.out, rec.same)
    for r in ASSIGN:
        if r["name"] not in cases and r["sorted"]:
            out = dict(indptr=r["out_p"], indices=r["out_j"], values=r["out_x"])
            cases[r["name"]] = Case(r["name"], [r["p"], r["j"], r["x"]] + AM.call_args(r["name"], r["args"]), out)
    for r in COO_SORT:
        name = "sort_coo_indices_" + r["kind"]
        if name not in cases:
            cases[name] = Case(name, [r["i"], r["j"]] + ([] if r["x"] is None else [r["x"]]), None)
    for name in OUTER:
        cases[name] = outer_case(name)
    for name in OWN:
        cases[name] = own_case(name)
    return cases


def expected_types(name, out):
    """The SEXP types the shim must return, by the routine's declared return type and the fixture's result: logical
    values stay LGLSXP, an integer sparse vector's values INTSXP, float32 results are INTSXP, the values of a
    pattern matrix an empty REALSXP.  remove_zero_valued_svec_numeric keeps its doubles where the
    reference truncates them into an integer vector."""
    ret = rcall.signature(name)["ret"]
    if ret == "void":
        return rcall.NILSXP
    if ret in rcall.SXP_OF:
        return rcall.SXP_OF[ret]
    assert ret == "List" and isinstance(out, dict), name
    types = {}
    for key, v in out.items():
        if isinstance(v, str):
            types[key] = rcall.STRSXP
        elif key in ("values", "val", "xx"):
            if name == "remove_zero_valued_svec_integer":
                types[key] = rcall.INTSXP
            elif name == "remove_zero_valued_svec_numeric" or v is None or v.dtype == np.float64:
                types[key] = rcall.REALSXP
            else:
                types[key] = rcall.LGLSXP
        else:
            types[key] = rcall.INTSXP
    return types

