"""Every mx_* export of csrc/api.hip does before its first device call what it did before the export layer got its
typed device arrays: the same argument checks in the same order with the same texts, and the same early returns,
including what they write (the zeroed C of an SpMM with nothing to multiply, the zeroed `out` of mx_matmul_csr_svec
with an empty vector) and what they leave alone.  The record, tests/golden/export_host_behaviour.json, was taken
once from the earlier build (tests/golden/make_export_host_behaviour.py, which also names the checks that can only
be reached after a device call) and is never regenerated from the code under test.  No device is needed: every
recorded call ends before the first device call, so it replays alike with and without one."""
import json
import os

import pytest

from export_calls import run_call

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "export_host_behaviour.json")) as f:
    RECORD = json.load(f)

# every function defined in api.hip that checks an argument or returns before its first device call
FUNCTIONS = """
mx_device_count
mx_tcrossprod_csr_dense_numeric mx_tcrossprod_csr_dense_float32 mx_matmul_dense_csc_numeric
mx_matmul_dense_csc_float32 mx_tcrossprod_dense_csr_numeric mx_tcrossprod_dense_csr_float32
mx_matmul_csr_dvec_numeric mx_matmul_csr_dvec_integer mx_matmul_csr_dvec_logical mx_matmul_csr_dvec_float32
mx_csr_elemwise_begin mx_copy_csr_rows_begin mx_copy_csr_rows_col_seq_begin mx_copy_csr_arbitrary_begin
mx_reverse_rows_begin mx_reverse_columns_inplace mx_matmul_csr_svec mx_multiply_csr_by_dense_elemwise
mx_multiply_csc_by_dense_ignore_NAs_numeric mx_multiply_csc_by_dense_ignore_NAs_float32
mx_multiply_csc_by_dense_ignore_NAs_integer mx_multiply_csc_by_dense_ignore_NAs_logical
mx_logicaland_csc_by_dense_ignore_NAs mx_multiply_csc_by_dense_keep_NAs_numeric
mx_multiply_csc_by_dense_keep_NAs_integer mx_multiply_csc_by_dense_keep_NAs_logical
mx_multiply_csc_by_dense_keep_NAs_float32 mx_multiply_csr_by_svec_begin mx_dense_by_svec_route
mx_multiply_elemwise_dense_by_svec_begin mx_multiply_elemwise_dense_by_svec_dense
mx_multiply_coo_by_dense_numeric mx_multiply_coo_by_dense_integer mx_multiply_coo_by_dense_logical
mx_multiply_coo_by_dense_float32 mx_logicaland_coo_by_dense_logical
mx_matmul_colvec_by_scolvecascsr_begin mx_matmul_spcolvec_by_scolvecascsr_begin mx_matmul_rowvec_by_csc
mx_multiply_csr_by_dvec_no_NAs_numeric mx_multiply_csr_by_dvec_with_NAs_begin mx_logicaland_csr_by_dvec_internal
mx_cbind_csr_begin mx_concat_csr_batch_begin mx_csr_transpose_begin mx_coo_to_csr_begin mx_csr_to_coo
mx_multiply_csr_by_coo_begin mx_multiply_coo_by_dense_ignore_NAs_numeric mx_multiply_coo_by_dense_ignore_NAs_logical
mx_slice_coo_arbitrary_begin mx_slice_coo_single
mx_remove_zero_valued_csr_numeric mx_remove_zero_valued_csr_logical mx_remove_zero_valued_coo_numeric
mx_remove_zero_valued_coo_logical mx_remove_zero_valued_svec_numeric mx_remove_zero_valued_svec_integer
mx_remove_zero_valued_svec_logical mx_filter_sparse_begin mx_rebuild_indptr_after_filter
mx_check_valid_csr_matrix mx_check_valid_coo_matrix mx_check_valid_svec mx_result_finish mx_result_discard
mx_check_is_seq mx_check_is_rev_seq mx_check_indices_are_sorted mx_sort_sparse_indices mx_sort_vector_indices
mx_sort_coo_indices
""".split()


def _defined_in_api_hip():
    import re
    from matrixextra_amd import _lib
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "api.hip")
    with open(path) as f:
        return set(re.findall(r"^(?:int|const char \*)\s*(mx_\w+)\(", f.read(), flags=re.M))


def test_every_checking_export_is_recorded():
    recorded = {e["call"][0] for e in RECORD}
    assert recorded == set(FUNCTIONS) and len(FUNCTIONS) == len(set(FUNCTIONS)) == 73
    # the others that api.hip defines go straight to the device, or only report
    assert _defined_in_api_hip() - recorded == {
        "mx_last_error", "mx_abi_version", "mx_set_device", "mx_device_name", "mx_dev_malloc", "mx_dev_free",
        "mx_dev_memset", "mx_memcpy_h2d", "mx_memcpy_d2h", "mx_stream_sync", "mx_host_register", "mx_host_unregister"}


def test_the_record_holds_outcomes_of_each_kind():
    status = [e["result"]["status"] for e in RECORD]
    assert len(RECORD) >= 450 and status.count(0) >= 60 and sum(s != 0 for s in status) >= 380
    assert all(e["result"]["error"] for e in RECORD if e["result"]["status"] not in (0, 2, 3)
               and e["call"][0] != "mx_dense_by_svec_route")
    assert sorted({e["result"]["status"] for e in RECORD if e["call"][0] == "mx_dense_by_svec_route"}) == [-1, 0, 1, 2, 3]


@pytest.mark.parametrize("name", FUNCTIONS)
def test_calls_end_as_recorded(name):
    calls = [e for e in RECORD if e["call"][0] == name]
    assert calls
    wrong = []
    for k, e in enumerate(calls):
        got = run_call(*e["call"])
        if got != e["result"]:
            wrong.append((k, e["call"][1], got, e["result"]))
    assert not wrong, f"{name}: {len(wrong)} of {len(calls)} calls differ, first (index, args, got, recorded): {wrong[0]}"
