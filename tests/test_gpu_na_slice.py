"""What finishes `[` on the device (csrc/coona.hip, csrc/api_slice.hip, matrixextra_amd/slice.py):
NA injection into a COO, the CSR scalar lookup, the recycled selector indices, the drop to a vector, and the mirror's
NA selectors end to end.

References: tests/golden/na_slice_golden.npz holds what the reference's own compiled routines returned and is compared
bit for bit; tests/na_slice_model.py (checked against those records when they were written) stands in at the sizes the
records do not hold.  The device level runs between guards (tests/devmem.py): every input, every output and the
workspace, exactly as long as the library says."""
import ctypes as C

import numpy as np
import pytest

import devmem as D
import na_slice_model as NM
from matrixextra_amd import _lib, exports as G
from matrixextra_amd._lib import MxError, check

pytestmark = pytest.mark.gpu

RECORDS, META = NM.load()
OTHER_NAN = np.frombuffer(np.uint64(0x7FF8000000000000).tobytes(), dtype=np.float64)[0]


def _b(a):
    a = np.asarray(a)
    return NM.bits(a) if a.dtype == np.float64 else a


def _same_triplets(got, want):
    for g, w, what in zip(got, want, ("ii", "jj", "xx")):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {g.dtype}{g.shape} for {w.dtype}{w.shape}"
        assert np.array_equal(_b(g), _b(w)), f"{what} differs, first at {int(np.flatnonzero(_b(g) != _b(w))[0])}"


# ---- every golden record through exports.py, bit for bit ------------------------------------------------------------
def _records(prefix):
    return [pytest.param(r, id=f"{r['name'].rsplit('_', 1)[-1]}-{r['label']}") for r in RECORDS
            if r["name"].startswith(prefix)]


def test_the_golden_file_holds_every_routine():
    names = {r["name"] for r in RECORDS}
    assert names == {"inject_NAs_inplace_coo_numeric", "inject_NAs_inplace_coo_logical",
                     "extract_single_val_csr_numeric", "extract_single_val_csr_logical",
                     "extract_single_val_csr_binary", "repeat_indices_n_times"}
    inj = [r for r in RECORDS if r["name"].startswith("inject")]
    rel = {np.sign(r["arrays"]["rows_na"].size - r["arrays"]["cols_na"].size) for r in inj}
    assert rel == {-1, 0, 1} and len(inj) >= 200
    assert any(r["arrays"]["rows_na"].size == 0 for r in inj) and any(r["arrays"]["cols_na"].size == 0 for r in inj)
    assert any(r["arrays"]["rows_na"].size == r["scalars"]["nrows"] > 1 for r in inj)
    assert any(NM.NA_INT in r["arrays"]["xx"] for r in inj if "xx" in r["arrays"])


def test_inject_NAs_matches_every_golden_record():
    for r in RECORDS:
        if not r["name"].startswith("inject"):
            continue
        A, S = r["arrays"], r["scalars"]
        lgl = r["name"].endswith("logical")
        xx, want_x = (A["xx"], A["out_xx"]) if lgl else (A["xx_f64"], A["out_xx_f64"])
        got = getattr(G, r["name"])(A["ii"], A["jj"], xx, A["rows_na"], A["cols_na"], S["nrows"], S["ncols"])
        try:
            _same_triplets((got["ii"], got["jj"], got["xx"]), (A["out_ii"], A["out_jj"], want_x))
        except AssertionError as e:
            raise AssertionError(f"{r['name']} {r['label']}: {e}") from None


@pytest.mark.parametrize("r", _records("extract_single_val_csr"))
def test_extract_single_val_csr_matches_the_golden_record(r):
    A, S = r["arrays"], r["scalars"]
    if r["name"].endswith("binary"):
        got = G.extract_single_val_csr_binary(A["indptr"], A["indices"], S["row"], S["col"])
    else:
        vals = A["values_f64"] if r["name"].endswith("numeric") else A["values"]
        got = getattr(G, r["name"])(A["indptr"], A["indices"], vals, S["row"], S["col"])
    assert NM.scalar_bits(r["name"], got) == r["result_bits"]


@pytest.mark.parametrize("r", _records("repeat_indices"))
def test_repeat_indices_n_times_matches_the_golden_record(r):
    A, S = r["arrays"], r["scalars"]
    got = G.repeat_indices_n_times(A["indices"], A["remainder"], S["ix_length"], S["desired_length"])
    assert got.dtype == np.int32 and np.array_equal(got, A["out"])


def test_inject_NAs_with_both_lists_empty_is_the_empty_list():
    none = np.zeros(0, dtype=np.int32)
    assert G.inject_NAs_inplace_coo_numeric([0, 1], [1, 0], [1.0, 2.0], none, none, 2, 2) == {}
    res, info = C.c_void_p(), _lib.ResultInfo()
    i = np.array([0, 1], dtype=np.int32)
    x = np.array([1.0, 2.0])
    check(_lib.load().mx_inject_NAs_inplace_coo_begin(_lib.ptr(i), _lib.ptr(i), _lib.ptr(x), _lib.MX_F64, 2, None, 0,
                                                      None, 0, 2, 2, C.byref(res), C.byref(info)))
    assert (info.indptr_len, info.nnz, info.values_len) == (0, 0, 0)
    check(_lib.load().mx_result_discard(res))


# ---- the device level between guards, against the model -------------------------------------------------------------
def dev_inject(i, j, x, m, n, rna, cna):
    """mxd_coo_inject_na_count + _fill: (rows, cols, values) of the result"""
    lib = _lib.load()
    gi, gj, gx = D.GuardedVec(np.int32, data=i), D.GuardedVec(np.int32, data=j), D._vec(x)
    gr, gc = D.GuardedVec(np.int32, data=rna), D.GuardedVec(np.int32, data=cna)
    nnz = gi.n
    gws, total = D._ws(lib.mxd_compact_workspace_bytes(nnz)), C.c_int64(-1)
    gmaps = D.GuardedVec(np.int32, n=4 + m + n + max(m, n))           # exactly what the header asks for
    check(lib.mxd_coo_inject_na_count(m, n, gi.ptr, gj.ptr, nnz, gr.ptr, gr.n, gc.ptr, gc.n, gws.ptr, gmaps.ptr,
                                      C.byref(total), None))
    gws._download(), gmaps._download()
    nout = int(total.value)
    oi, oj, ox = D._entries(nout, np.int32, np.int32, x.dtype)
    check(lib.mxd_coo_inject_na_fill(m, n, gi.ptr, gj.ptr, gx.ptr, D.value_dtype_of(x), nnz, gr.ptr, gr.n, gc.ptr, gc.n,
                                     gws.ptr, gmaps.ptr, oi.ptr, oj.ptr, ox.ptr, None))
    D._sync()
    D._untouched(gi, gj, gx, gr, gc)
    gws._download(), gmaps._download()
    return oi.result(nout), oj.result(nout), ox.result(nout)


def _triplets(rng, m, n, nnz, logical):
    i = rng.integers(0, m, size=nnz).astype(np.int32)
    j = rng.integers(0, n, size=nnz).astype(np.int32)
    if logical:
        x = rng.choice(np.array([0, 1, NM.NA_INT], dtype=np.int32), size=nnz).astype(np.int32)
    else:
        x = np.round(rng.normal(size=nnz), 3)
        x[::9] = NM.NA_REAL
        x[1::13] = OTHER_NAN
        x[2::17] = -0.0
    return i, j, x


def _pick(rng, n, k):
    return np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32)


# 12 293 triplets: three tiles of 4 096 and a ragged tail of 5; 200 x 130 with 7 NA rows and 9 NA columns, the
# reverse, each list alone, a whole axis, and the tie
@pytest.mark.parametrize("n_rna, n_cna", [(7, 9), (9, 7), (7, 0), (0, 9), (200, 3), (4, 130), (5, 5)])
@pytest.mark.parametrize("logical", [False, True])
def test_device_injection_matches_the_model_over_several_tiles(n_rna, n_cna, logical):
    rng = np.random.default_rng(1000 * n_rna + n_cna + logical)
    m, n, nnz = 200, 130, 12293
    i, j, x = _triplets(rng, m, n, nnz, logical)
    rna, cna = _pick(rng, m, n_rna), _pick(rng, n, n_cna)
    if 0 < n_rna < m:
        rna[0], rna[-1] = 0, m - 1
    want = NM.inject_coo(i, j, x, rna, cna, m, n)
    assert want[0].size > nnz // 2 + n_rna * n                            # most triplets stay, and the block is there
    _same_triplets(dev_inject(i, j, x, m, n, rna, cna), want)


def test_device_injection_without_triplets_and_with_one_line_matrices():
    none_i, none_x = np.zeros(0, dtype=np.int32), np.zeros(0)
    for m, n, rna, cna in ((5, 4, [1, 4], [0]), (1, 7, [0], [2, 6]), (6, 1, [0, 5], [0]), (3, 3, [], [1])):
        rna, cna = np.array(rna, dtype=np.int32), np.array(cna, dtype=np.int32)
        _same_triplets(dev_inject(none_i, none_i, none_x, m, n, rna, cna),
                       NM.inject_coo(none_i, none_i, none_x, rna, cna, m, n))


def test_a_total_above_int32_fails_in_the_count_pass():
    """50 000 x 50 000 with every row NA: 2.5e9 entries.  Only the workspace and the maps exist when the count refuses."""
    lib = _lib.load()
    m = n = 50000
    gi, gj = D.GuardedVec(np.int32, data=[0, 1, 2]), D.GuardedVec(np.int32, data=[2, 1, 0])
    gr, gc = D.GuardedVec(np.int32, data=np.arange(m, dtype=np.int32)), D.GuardedVec(np.int32, n=0)
    gws, gmaps, total = D._ws(lib.mxd_compact_workspace_bytes(3)), D.GuardedVec(np.int32, n=4 + 3 * m), C.c_int64(-1)
    rc = lib.mxd_coo_inject_na_count(m, n, gi.ptr, gj.ptr, 3, gr.ptr, gr.n, gc.ptr, 0, gws.ptr, gmaps.ptr,
                                     C.byref(total), None)
    assert rc != 0 and total.value == -1
    msg = lib.mx_last_error().decode()
    assert "2500000000 entries" in msg and "int32" in msg
    gws._download(), gmaps._download()
    D._untouched(gi, gj, gr)
    with pytest.raises(MxError, match="2500000000 entries"):
        G.inject_NAs_inplace_coo_numeric([0], [0], [1.0], np.arange(m, dtype=np.int32), [], m, n)


@pytest.mark.parametrize("rna, cna, word", [([3, 3], [], "rows"), ([4, 2], [], "rows"), ([0, 6], [], "rows"),
                                            ([-1, 2], [], "rows"), ([1], [2, 2], "columns"), ([1], [5], "columns"),
                                            ([0, 1, 2, 3, 4, 5, 6], [], "NA rows")])
def test_bad_lists_fail_with_a_message(rna, cna, word):
    i = np.array([0, 5, 2], dtype=np.int32)
    j = np.array([1, 4, 0], dtype=np.int32)
    with pytest.raises(MxError, match=word):
        G.inject_NAs_inplace_coo_numeric(i, j, [1.0, 2.0, 3.0], rna, cna, 6, 5)


def dev_csr_single(p, j, x, r, c):
    lib = _lib.load()
    A = D.GCsr(p, j, x)
    gws, k, value = D._ws(16), C.c_int64(-2), (C.c_uint8 * 8)()
    check(lib.mxd_csr_single(A.m, A.p.ptr, A.j.ptr, A.xptr, D.value_dtype_of(x), A.nnz, r, c, gws.ptr, C.byref(k), value,
                             None))
    D._sync()
    A.assert_untouched()
    gws._download()
    return int(k.value), bytes(value)


def test_device_csr_single_takes_the_first_hit_of_a_long_unsorted_row():
    """row 1 holds 300 entries (five steps of the wavefront) with column 17 at 70, 71 and 299; rows 0 and 2 hold it too"""
    rng = np.random.default_rng(5)
    row = rng.permutation(np.arange(100, 400)).astype(np.int32)
    row[[70, 71, 299]] = 17
    j = np.concatenate([[17, 3], row, [17]]).astype(np.int32)
    p = np.array([0, 2, 302, 302, 303], dtype=np.int32)
    x = np.arange(j.size, dtype=np.float64) + 0.5
    k, v = dev_csr_single(p, j, x, 1, 17)
    assert k == 72 and np.frombuffer(v, dtype=np.float64)[0] == 72.5
    assert dev_csr_single(p, j, x, 1, int(row[299 - 1]))[0] == 2 + 298
    assert dev_csr_single(p, j, x, 1, 99)[0] == -1                       # a miss
    assert dev_csr_single(p, j, x, 2, 17)[0] == -1                       # an empty row between two that hold it
    assert dev_csr_single(p, j, None, 3, 17)[0] == 302
    xl = np.full(j.size, NM.NA_INT, dtype=np.int32)
    k, v = dev_csr_single(p, j, xl, 0, 3)
    assert k == 1 and np.frombuffer(v[:4], dtype=np.int32)[0] == NM.NA_INT


def test_device_repeat_indices_and_dense_vector_between_guards():
    lib = _lib.load()
    ix, rem = np.array([1, 4, 5, 9], dtype=np.int32), np.array([1, 4], dtype=np.int32)
    want = NM.repeat_indices(ix, rem, 10, 1234565)                       # 123 456 full repeats and a remainder
    gix, grem, out = D.GuardedVec(np.int32, data=ix), D.GuardedVec(np.int32, data=rem), D.GuardedVec(np.int32, n=want.size)
    check(lib.mxd_repeat_indices(gix.ptr, 4, grem.ptr, 2, 10, 1234565, out.ptr, None))
    D._sync()
    D._untouched(gix, grem)
    assert np.array_equal(out.result(), want)

    rng = np.random.default_rng(9)
    length = 5001
    pos = rng.permutation(length)[:700].astype(np.int32)
    for vals, odt, dt in ((np.round(rng.normal(size=700), 3), _lib.MX_F64, np.float64),
                          (rng.choice(np.array([1, NM.NA_INT], dtype=np.int32), size=700), _lib.MX_LGL, np.int32),
                          (None, _lib.MX_F64, np.float64), (None, _lib.MX_LGL, np.int32)):
        want = np.zeros(length, dtype=dt)
        want[pos] = 1 if vals is None else vals
        gp, gv, out = D.GuardedVec(np.int32, data=pos), D._vec(vals), D.GuardedVec(dt, n=length)
        check(lib.mxd_entries_to_dense_vector(gp.ptr, D._ptr(gv), D.value_dtype_of(vals), 700, out.ptr, odt, length, None))
        D._sync()
        D._untouched(gp, gv)
        assert np.array_equal(_b(out.result()), _b(want))
        got = G.entries_to_dense_vector(pos, vals, length, logical=odt == _lib.MX_LGL)
        assert got.dtype == dt and np.array_equal(_b(got), _b(want))


# ---- the mirror end to end ------------------------------------------------------------------------------------------
import matrixextra_amd as mx  # noqa: E402
from matrixextra_amd import slice as S  # noqa: E402
from matrixextra_amd.assign import _assign_csr_internal  # noqa: E402
from matrixextra_amd.matrices import options  # noqa: E402

NA = mx.matrices.NA_INTEGER
M_ROWS, M_COLS = 37, 23
ROW_NAMES = [f"r{k}" for k in range(M_ROWS)]
COL_NAMES = [f"c{k}" for k in range(M_COLS)]


def _dense(kind, stored_na=True):
    """the 37 x 23 matrix of every mirror test, one value kind each: (dense float64 with nan for NA, triplets)"""
    rng = np.random.default_rng(77)
    mask = rng.random((M_ROWS, M_COLS)) < 0.3
    mask[5] = False
    mask[:, 7] = False
    i, j = np.nonzero(mask)
    o = rng.permutation(i.size)
    i, j = i[o].astype(np.int32), j[o].astype(np.int32)
    if kind == "d":
        x = np.round(rng.normal(size=i.size), 3) + 2.0
        x[::11] = NM.NA_REAL
    elif kind == "l":
        x = rng.choice(np.array([1, 1, NM.NA_INT if stored_na else 0], dtype=np.int32), size=i.size).astype(np.int32)
    else:
        x = None
    Dn = np.zeros((M_ROWS, M_COLS))
    Dn[i, j] = 1.0 if x is None else np.where(x == NM.NA_INT, np.nan, x) if kind == "l" else x
    return Dn, (i, j, x)


def _matrix(cls):
    """An lgRMatrix stores TRUE and FALSE only: a stored NA of an lgRMatrix comes back TRUE from the column-range
    route (copy_csr_rows_col_seq_logical hands its values on as doubles, src/slice.cpp:363), as in the reference, and
    that route is not the subject here.  The lgTMatrix stores NA too."""
    kind = cls.__name__[0]
    Dn, (i, j, x) = _dense(kind, stored_na=cls is not mx.lgRMatrix)
    T = {"d": mx.dgTMatrix, "l": mx.lgTMatrix, "n": mx.ngTMatrix}[kind](i, j, x, (M_ROWS, M_COLS), [ROW_NAMES, COL_NAMES])
    if issubclass(cls, mx.matrices.TsparseMatrix):
        return Dn, T
    R = mx.as_csr_matrix(T, logical=kind == "l", binary=kind == "n")
    assert type(R) is cls
    return Dn, R


def _mask(n, every):
    m = np.zeros(n, dtype=bool)
    m[::every] = True
    return m


# selector kinds: (i, j) as handed to subset_*, and the same as 1-based int arrays with NA_INT (None = all)
def _selectors():
    seq = np.array([3, 4, NA, 6, 7], np.int32)
    rev = np.array([9.0, 8.0, np.nan, 6.0])
    arb = np.array([12, 2, 12, NA, 30, NA, 2], np.int32)
    names = np.array(["c4", None, "c0", "c22"], dtype=object)
    names_int = np.array([5, NA, 1, 23], np.int32)
    mask_i = np.flatnonzero(_mask(M_ROWS, 5)) + 1
    yield "rows seq+NA, all columns", seq, None, seq, None
    yield "rows reversed+NA, columns by name+NA", rev, names, np.array([9, 8, NA, 6], np.int32), names_int
    yield "rows arbitrary with repeats+NA, columns seq", arb, np.arange(4, 15), arb, np.arange(4, 15)
    yield "all rows, columns arbitrary+NA", None, np.array([20, NA, 1, 20], np.int32), None, np.array([20, NA, 1, 20])
    yield "rows mask, columns NA first", _mask(M_ROWS, 5), [None, 3, 2], mask_i, np.array([NA, 3, 2], np.int32)
    yield "rows NA last, columns reversed full", np.array([1, 37, NA], np.int32), np.arange(M_COLS, 0, -1), \
        np.array([1, 37, NA], np.int32), np.arange(M_COLS, 0, -1)
    yield "both arbitrary+NA", np.array([NA, 5, 6, 36], np.int32), np.array([8, NA, NA, 2, 9], np.int32), \
        np.array([NA, 5, 6, 36], np.int32), np.array([8, NA, NA, 2, 9], np.int32)


SELECTORS = list(_selectors())
CLASSES = [mx.dgRMatrix, mx.lgRMatrix, mx.ngRMatrix, mx.dgTMatrix, mx.lgTMatrix, mx.ngTMatrix]


def _same_dense(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(want))


def _kept_duplicates_read_true(want, base, i_int, j_int):
    """A logical COO result with NA rows AND NA columns, read as a matrix.  The reference drops a triplet only when
    its row and its column are both NA (src/slice_coo.cpp:789-809), so a TRUE entry of an NA line outside the
    crossing stays beside the NA that the block stores for its cell, and `TRUE | NA` is TRUE.
    `base` is the NA-free slice."""
    rna = np.asarray(i_int) == NM.NA_INT if i_int is not None else np.zeros(want.shape[0], dtype=bool)
    cna = np.asarray(j_int) == NM.NA_INT if j_int is not None else np.zeros(want.shape[1], dtype=bool)
    if not (rna.any() and cna.any()):
        return want
    lines = (rna[:, None] | cna[None, :]) & ~(rna[:, None] & cna[None, :])
    return np.where(lines & (np.nan_to_num(base) != 0), 1.0, want)


def _expected_names(names, sel_int):
    if sel_int is None:
        return names
    return [None if k == NM.NA_INT else names[k - 1] for k in np.asarray(sel_int)]


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_mirror_slices_with_NA_selectors_match_the_dense_model(cls):
    Dn, X = _matrix(cls)
    sub = S.subset_csr if isinstance(X, mx.matrices.RsparseMatrix) else S.subset_coo
    for label, i, j, i_int, j_int in SELECTORS:
        out = sub(X, i, j, drop=False)
        want = NM.sliced_dense(Dn, i_int, j_int)
        kind = cls.__name__[0]
        lgl_out = kind != "d"
        assert type(out).__name__ == ("dg" if kind == "d" else "lg") + cls.__name__[2:], label
        got = out.toarray()
        if lgl_out:
            want = np.where(np.isnan(want), np.nan, (want != 0).astype(float))
            if isinstance(out, mx.matrices.TsparseMatrix):
                fill = [None if s is None else np.where(np.asarray(s) == NM.NA_INT, s[np.asarray(s) != NM.NA_INT][0], s)
                        for s in (i_int, j_int)]
                want = _kept_duplicates_read_true(want, NM.sliced_dense(Dn, *fill), i_int, j_int)
        try:
            _same_dense(got, want)
        except AssertionError:
            raise AssertionError(f"{cls.__name__}: {label}") from None
        assert out.Dimnames == [_expected_names(ROW_NAMES, i_int), _expected_names(COL_NAMES, j_int)], label


def test_csr_result_is_the_assignment_applied_by_hand():
    """x[i, j] with NAs = the NA-free slice with NA_real_ assigned to the NA rows, then to the NA columns"""
    _, X = _matrix(mx.dgRMatrix)
    i, j = np.array([12, 2, NA, 30, NA], np.int32), np.array([8, NA, 2, 9], np.int32)
    out = S.subset_csr(X, i, j)
    base = S.subset_csr(X, np.array([12, 2, 12, 30, 12]), np.array([8, 8, 2, 9]))
    cols, rows = np.arange(1, 5, dtype=np.int32), np.arange(1, 6, dtype=np.int32)
    by_hand = _assign_csr_internal(base, np.array([3, 5], np.int32), cols, NM.NA_REAL, None)
    by_hand = _assign_csr_internal(by_hand, rows, np.array([2], np.int32), NM.NA_REAL, None)
    assert np.array_equal(out.p, by_hand.p) and np.array_equal(out.j, by_hand.j)
    assert np.array_equal(NM.bits(out.x), NM.bits(by_hand.x))
    assert (NM.bits(out.x[out.p[2]:out.p[3]]) == NM.NA_REAL_BITS).all() and out.p[3] - out.p[2] == 4
    with pytest.raises(mx.matrices.MatrixExtraError, match="Indices contain NAs."):
        mx.assign_csr(X, i, None, 1.0)


def test_coo_result_keeps_the_cell_of_an_NA_row_twice():
    """both lists given: a triplet of an NA row outside the NA columns stays, and the NA block stores its cell again
    (the reference's rule); read as a matrix the cell is NA all the same"""
    T = mx.dgTMatrix([0, 1], [0, 1], [5.0, 6.0], (2, 2))
    out = S.subset_coo(T, np.array([NA, 1], np.int32), np.array([1, NA], np.int32))     # rows (1, 1), columns (1, 1)
    cells = list(zip(out.i.tolist(), out.j.tolist()))
    # kept: (0, 0) of the NA row and (1, 0), (1, 1); dropped: (0, 1), in both; the block: column 1, then (0, 0)
    assert cells == [(0, 0), (1, 0), (1, 1), (0, 1), (1, 1), (0, 0)]
    assert (NM.bits(out.x[3:]) == NM.NA_REAL_BITS).all() and list(out.x[:3]) == [5.0, 5.0, 5.0]
    dense = out.toarray()
    assert np.isnan(dense[[0, 0, 1], [0, 1, 1]]).all() and dense[1, 0] == 5.0        # 5 + NA is NA
    L = mx.lgTMatrix([0, 1], [0, 1], [1, 1], (2, 2))
    out = S.subset_coo(L, np.array([NA, 1], np.int32), np.array([1, NA], np.int32))
    assert list(out.x) == [1, 1, 1, NM.NA_INT, NM.NA_INT, NM.NA_INT]
    assert np.isnan(out.toarray()[0, 1]) and out.toarray()[0, 0] == 1.0                # TRUE | NA is TRUE


@pytest.fixture
def drop_route():
    options["mxgpu.slice_drop_route"] = True
    yield
    options.pop("mxgpu.slice_drop_route", None)
    options["MatrixExtra.drop_sparse"] = False


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_drop_route_vectors_and_scalars_match_the_model(cls, drop_route):
    Dn, X = _matrix(cls)
    kind = cls.__name__[0]
    is_csr = isinstance(X, mx.matrices.RsparseMatrix)
    sub = S.subset_csr if is_csr else S.subset_coo
    for i, j, i_int, j_int in ((np.array([4]), None, [4], None), (None, np.array([11]), None, [11]),
                               (np.array([9, NA, 6, 4], np.int32), [3], [9, NA, 6, 4], [3]),
                               ([6], np.array([3.0, np.nan, 1.0]), [6], [3, NA, 1])):
        want = NM.dropped(NM.sliced_dense(Dn, i_int, j_int))
        got = sub(X, i, j, drop=True)
        assert isinstance(got, np.ndarray) and got.ndim == 1
        if kind == "d":
            assert got.dtype == np.float64
            _same_dense(got, want)
        else:
            assert got.dtype == np.int32
            _same_dense(np.where(got == NM.NA_INT, np.nan, got), np.where(np.isnan(want), np.nan, want != 0))
        kept = sub(X, i, j, drop=False)
        assert not isinstance(kept, np.ndarray) and kept.Dim == NM.sliced_dense(Dn, i_int, j_int).shape
    wide = sub(X, np.array([4, 5]), None, drop=True)
    assert not isinstance(wide, np.ndarray) and wide.Dim == (2, M_COLS)
    # scalars: a stored cell, an empty cell, an NA index, the bounds message
    r, c = (int(v) for v in np.argwhere(~np.isnan(Dn) & (Dn != 0))[0])
    got = sub(X, r + 1, c + 1, drop=True)
    assert got == (Dn[r, c] if kind == "d" else True)
    assert sub(X, 6, 8, drop=True) == 0                                   # row 6 and column 8 are empty
    na = sub(X, np.nan, 2, drop=True)
    assert np.array([na]).view(np.uint64)[0] == NM.NA_REAL_BITS
    with pytest.raises(mx.matrices.MatrixExtraError, match="Subscript out of bounds."):
        sub(X, M_ROWS + 1, 1, drop=True)
    one = sub(X, r + 1, c + 1, drop=False)
    assert type(one) is cls and one.Dim == (1, 1) and one.toarray()[0, 0] == (Dn[r, c] if kind == "d" else 1.0)
    assert sub(X, 6, 8, drop=False).toarray()[0, 0] == 0 and type(X[r, c]) is cls
    options["MatrixExtra.drop_sparse"] = True
    v = sub(X, np.array([4]), None, drop=True)
    want = Dn[3]
    assert type(v).__name__ == kind + "sparseVector" and v.length == M_COLS
    assert np.all(np.diff(v.i) > 0) and (v.x is None) == (kind == "n")
    _same_dense(v.toarray(), want if kind == "d" else np.where(np.isnan(want), np.nan, (want != 0).astype(float)))
    assert isinstance(sub(X, r + 1, c + 1, drop=True), (float, bool, np.floating))      # 1 x 1 is never sparse


@pytest.mark.parametrize("cls", [mx.dgRMatrix, mx.lgTMatrix], ids=lambda c: c.__name__)
def test_with_the_option_off_no_earlier_result_changes(cls):
    assert "mxgpu.slice_drop_route" not in options
    Dn, X = _matrix(cls)
    sub = S.subset_csr if isinstance(X, mx.matrices.RsparseMatrix) else S.subset_coo
    out = sub(X, np.array([4]), None, drop=True)
    assert type(out) is cls and out.Dim == (1, M_COLS)
    out = sub(X, np.array([4, 9, 4]), np.array([11]), drop=True)
    assert type(out) is cls and out.Dim == (3, 1)
    if cls is mx.dgRMatrix:
        one = sub(X, 4, 11, drop=True)                                  # no scalar route for a CSR without the option
        assert type(one) is cls and one.Dim == (1, 1) and one.Dimnames == [["r3"], ["c10"]]
    assert sub(X, None, None, drop=True) is X


def test_sparse_vector_selectors_on_the_device():
    Dn, X = _matrix(mx.dgRMatrix)
    sel = mx.matrices.nsparseVector([5, 1, 3], None, 5)                  # recycled over 37 rows, unsorted as given
    want_rows = np.array([k for k in range(M_ROWS) if k % 5 in (0, 2, 4)])
    out = S.subset_csr(X, sel, None)
    _same_dense(out.toarray(), Dn[want_rows])
    lsel = mx.matrices.lsparseVector([2, 1], [NM.NA_INT, 1], M_COLS)
    out = S.subset_csr(X, None, lsel)
    want = NM.sliced_dense(Dn, None, np.array([1, NM.NA_INT]))
    _same_dense(out.toarray(), want)
    with pytest.raises(mx.matrices.MatrixExtraError, match="Dimension of indexing vector is larger"):
        S.subset_csr(X, mx.matrices.nsparseVector([1], None, M_ROWS + 1), None)
