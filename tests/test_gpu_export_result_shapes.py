"""Every *_begin export reports the mx_result_info and hands out, through mx_result_finish, the three vectors that it
did before mx_result got its shaping members, bit for bit: a non-empty result, an empty one, a call without values
and the aliasing paths of each export, at the small shapes where the sizing branches differ.  The record,
tests/golden/export_result_shapes.json, was taken once on an MI355X from the earlier build
(tests/golden/make_export_result_shapes.py) and is never regenerated from the code under test.  Values are compared
as uint64 / uint32 bit patterns, so NaN payloads count; a vector that finish must leave alone (an aliased
structure) keeps the sentinel it was filled with."""
import json
import os

import pytest

from export_calls import run_call

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "export_result_shapes.json")) as f:
    RECORD = json.load(f)

BEGIN_EXPORTS = """
mx_csr_elemwise_begin mx_copy_csr_rows_begin mx_copy_csr_rows_col_seq_begin mx_copy_csr_arbitrary_begin
mx_reverse_rows_begin mx_multiply_csr_by_svec_begin mx_multiply_elemwise_dense_by_svec_begin
mx_matmul_colvec_by_scolvecascsr_begin mx_matmul_spcolvec_by_scolvecascsr_begin
mx_multiply_csr_by_dvec_with_NAs_begin mx_cbind_csr_begin mx_concat_csr_batch_begin mx_csr_transpose_begin
mx_coo_to_csr_begin mx_multiply_csr_by_coo_begin mx_slice_coo_arbitrary_begin mx_filter_sparse_begin
mx_multiply_csc_by_dense_keep_NAs_numeric mx_multiply_csc_by_dense_keep_NAs_integer
mx_multiply_csc_by_dense_keep_NAs_logical mx_multiply_csc_by_dense_keep_NAs_float32
mx_remove_zero_valued_csr_numeric mx_remove_zero_valued_csr_logical mx_remove_zero_valued_coo_numeric
mx_remove_zero_valued_coo_logical mx_remove_zero_valued_svec_numeric mx_remove_zero_valued_svec_integer
mx_remove_zero_valued_svec_logical
""".split()


def test_every_begin_export_is_recorded_in_each_shape():
    by_fn = {}
    for e in RECORD.values():
        by_fn.setdefault(e["call"][0], []).append(e["result"]["info"])
    assert set(by_fn) == set(BEGIN_EXPORTS)
    for fn in BEGIN_EXPORTS[:17]:                        # (indptr_len, nnz, values_len, values_dtype, alias_structure)
        assert any(i[1] > 0 for i in by_fn[fn]) and any(i[1] == 0 for i in by_fn[fn]), fn
    aliased = {e["call"][0]: e["result"]["info"][4] for e in RECORD.values() if e["result"]["info"][4]}
    assert aliased["mx_csr_elemwise_begin"] == 1 and aliased["mx_multiply_csr_by_dvec_with_NAs_begin"] == 1
    assert {aliased[f"mx_remove_zero_valued_{k}"] for k in ("csr_numeric", "coo_numeric", "svec_logical")} == {2}
    assert RECORD["elemwise_sub_self"]["result"]["info"] == [5, 0, 0, 0, 0]
    assert RECORD["gather_empty"]["result"]["info"][:3] == [0, 0, 0]              # three EMPTY vectors
    assert RECORD["reverse_rows_empty"]["result"]["info"][:3] == [5, 0, 0]        # a full-length indptr
    assert RECORD["gather_none"]["result"]["info"][2:4] == [0, 4]                 # no values: MX_NONE
    layouts = [RECORD[f"filter_{k}"]["result"]["info"] for k in ("csr", "coo", "svec")]
    assert [i[0] for i in layouts] == [5, layouts[1][1], 0] and layouts[1][1] > 0  # COO: row ids in the indptr vector


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RECORD))
def test_result_is_that_of_the_record(name):
    e = RECORD[name]
    got = run_call(*e["call"])
    assert got == e["result"]
