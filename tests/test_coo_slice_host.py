"""COO slicing (subset_coo / TsparseMatrix.__getitem__) checks that need no GPU: with the exports replaced by
recorders, the route each selector takes (R/slice_coo.R), the flags handed to slice_coo_arbitrary_* (get_ij_properties,
R/slice.R:59-143), the scalar route's rules and the error messages; and the new C-ABI entries."""
import numpy as np
import pytest

import matrixextra_amd as mx
from matrixextra_amd import _lib, exports as G
from matrixextra_amd import slice as S


def _seq(a, rev=False):
    a = np.asarray(a, dtype=np.int64)
    if a.size < 2:
        return True
    return bool(np.all(np.diff(a) == (-1 if rev else 1)))


@pytest.fixture
def calls(monkeypatch):
    """Replaces the device-backed exports with recorders; returns the list of (name, args)."""
    log = []
    monkeypatch.setattr(G, "check_is_seq", lambda a: _seq(a))
    monkeypatch.setattr(G, "check_is_rev_seq", lambda a: _seq(a, rev=True))

    def arbitrary(name):
        def f(*args):
            log.append((name, args))
            return dict(ii=np.zeros(0, np.int32), jj=np.zeros(0, np.int32),
                        xx=None if name.endswith("binary") else np.zeros(0))
        return f

    def single(name, val):
        def f(*args):
            log.append((name, args))
            return val
        return f

    for k in ("numeric", "logical", "binary"):
        monkeypatch.setattr(G, "slice_coo_arbitrary_" + k, arbitrary("slice_coo_arbitrary_" + k))
    monkeypatch.setattr(G, "slice_coo_single_numeric", single("slice_coo_single_numeric", 2.5))
    monkeypatch.setattr(G, "slice_coo_single_logical", single("slice_coo_single_logical", True))
    monkeypatch.setattr(G, "slice_coo_single_binary", single("slice_coo_single_binary", False))
    return log


def _T(cls=mx.dgTMatrix, names=False):
    i = np.array([0, 3, 2, 4, 0], np.int32)
    j = np.array([1, 0, 2, 3, 1], np.int32)
    x = None if cls is mx.ngTMatrix else (np.array([1.0, 2.0, 3.0, 4.0, 5.0]) if cls is mx.dgTMatrix
                                          else np.array([1, 0, 1, 1, -2147483648], np.int32))
    dn = [["a", "b", "c", "d", "e"], ["w", "x", "y", "z"]] if names else None
    return cls(i, j, x, (5, 4), dn)


def _flags(args):
    # (ii, jj, [xx,] i, j, all_i, all_j, i_is_seq, j_is_seq, i_is_rev_seq, j_is_rev_seq, nrows, ncols)
    return tuple(bool(v) for v in args[-8:-2])


@pytest.mark.parametrize("i, j, want", [
    (None, [2, 3], (True, False, True, True, False, False)),                  # all x seq
    ([2, 3, 4], None, (False, True, True, False, False, False)),              # seq x all
    ([1, 2, 3, 4, 5], [2, 3], (True, False, True, True, False, False)),       # full-range i: all_i and i_is_seq
    ([2, 3], [1, 2, 3, 4], (False, True, True, False, False, False)),         # full-range j: all_j, j_is_seq FALSE
    ([4, 3, 2], [3, 2], (False, False, False, False, True, True)),            # partial rev x rev
    ([5, 4, 3, 2, 1], [4, 3, 2, 1], (False, False, False, False, True, True)),  # full reversal: the kernel too
    ([3, 1, 3], [2, 4], (False, False, False, False, False, False)),          # arbitrary
    ([2], [1, 3], (False, False, True, False, False, False)),                 # length-1 vector is seq (not scalar)
])
def test_branch_flags(calls, i, j, want):
    S.subset_coo(_T(), np.asarray(i) if i is not None else None, np.asarray(j) if j is not None else None)
    assert len(calls) == 1 and calls[0][0] == "slice_coo_arbitrary_numeric"
    assert _flags(calls[0][1]) == want
    assert calls[0][1][-2:] == (5, 4)


@pytest.mark.parametrize("cls, name", [(mx.dgTMatrix, "numeric"), (mx.lgTMatrix, "logical"), (mx.ngTMatrix, "binary")])
def test_kind_picks_the_export_and_the_result_class(calls, cls, name):
    out = S.subset_coo(_T(cls, names=True), np.array([3, 1]), np.array(["z", "w"]))
    assert calls[0][0] == "slice_coo_arbitrary_" + name
    args = calls[0][1]
    i_sel, j_sel = (args[3], args[4]) if name != "binary" else (args[2], args[3])
    assert list(i_sel) == [3, 1] and list(j_sel) == [4, 1]
    assert type(out) is cls and out.Dim == (2, 2) and out.Dimnames == [["c", "a"], ["z", "w"]]
    assert (out.x is None) == (cls is mx.ngTMatrix)


def test_early_exits_need_no_device(calls):
    T = _T(names=True)
    assert S.subset_coo(T) is T
    assert S.subset_coo(T, None, None) is T
    assert S.subset_coo(T, np.arange(1, 6), np.arange(1, 5)) is T
    e = S.subset_coo(T, np.zeros(0, np.int32), np.array([2, 1]))
    assert type(e) is mx.dgTMatrix and e.Dim == (0, 2) and e.i.size == 0 and e.Dimnames == [[], ["x", "w"]]          # row_names[integer(0)]
    e = S.subset_coo(T, [-1, -2, -3, -4, -5], None)
    assert e.Dim == (0, 4)
    E = mx.lgTMatrix(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), (5, 4))
    e = S.subset_coo(E, np.array([2, 2]), np.array([1]))
    assert type(e) is mx.lgTMatrix and e.Dim == (2, 1) and e.x.dtype == np.int32
    assert calls == []


def test_scalar_route(calls):
    T = _T(names=True)
    assert S.subset_coo(T, 2, 3) == 2.5
    assert calls[-1] == ("slice_coo_single_numeric", (T.i, T.j, T.x, 1, 2))
    assert S.subset_coo(T, 2.9, np.int64(1)) == 2.5                           # as.integer() truncates
    assert calls[-1][1][3:] == (1, 0)
    assert S.subset_coo(T, 0, 1) == 2.5 and calls[-1][1][3:] == (-1, 0)       # (sic) reaches the routine as a miss
    assert S.subset_coo(_T(mx.lgTMatrix), 1, 1) is True
    assert S.subset_coo(_T(mx.ngTMatrix), 1, 1) is False
    n = len(calls)
    S.subset_coo(T, True, 1)                                                  # a logical is not a scalar index
    S.subset_coo(T, "b", 1)                                                   # nor is a name
    S.subset_coo(T, [2], None)                                                # both must be given
    assert [c[0] for c in calls[n:]] == ["slice_coo_arbitrary_numeric"] * 3


def test_scalar_route_drop_false(calls):
    T = _T(names=True)
    out = S.subset_coo(T, 2, 3, drop=False)
    assert type(out) is mx.dgTMatrix and out.Dim == (1, 1) and out.Dimnames == [["b"], ["y"]]
    assert list(out.x) == [2.5]
    out = S.subset_coo(_T(mx.ngTMatrix), 1, 1, drop=False)                   # FALSE: no entry
    assert type(out) is mx.ngTMatrix and out.i.size == 0 and out.x is None


def test_scalar_out_of_bounds():
    T = _T()
    with pytest.raises(mx.MatrixExtraError, match="Subscript out of bounds."):
        S.subset_coo(T, 6, 1)
    with pytest.raises(mx.MatrixExtraError, match="Subscript out of bounds."):
        S.subset_coo(T, 1, 5)


def test_selector_errors(calls):
    T = _T(names=True)
    with pytest.raises(mx.MatrixExtraError, match="can't mix positive and negative subscripts"):
        S.subset_coo(T, [1, -2], None)
    with pytest.raises(mx.MatrixExtraError, match="not present in matrix"):
        S.subset_coo(T, [1, 9], None)
    with pytest.raises(mx.MatrixExtraError, match="not present in matrix"):
        S.subset_coo(T, np.array(["a", "zz"]), None)
    with pytest.raises(mx.MatrixExtraError, match="incorrect number of dimensions"):
        T[1, 2, 3]
    with pytest.raises(mx.MatrixExtraError, match="boolean index has wrong length"):
        T[np.array([True, False])]


def test_getitem_is_zero_based(calls):
    T = _T()
    T[[2, 0], 1:3]
    assert _flags(calls[-1][1]) == (False, False, False, True, False, False)
    assert list(calls[-1][1][3]) == [3, 1] and list(calls[-1][1][4]) == [2, 3]
    T[-1]
    assert list(calls[-1][1][3]) == [5] and _flags(calls[-1][1])[1]          # all columns
    assert T[1, 2] is not None and calls[-1][0] == "slice_coo_single_numeric"
    assert calls[-1][1][3:] == (1, 2)
    T[np.array([1]), np.array([2])]                                           # vectors stay vectors
    assert calls[-1][0] == "slice_coo_arbitrary_numeric"
    assert T[:, :] is T


def test_csr_getitem_unchanged(monkeypatch):
    seen = []
    monkeypatch.setattr(S, "subset_csr", lambda x, i, j: seen.append((i, j)))
    X = mx.dgRMatrix(np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([1.0, 2.0]), (2, 3))
    X[1, ::2]
    X[[True, False]]
    assert list(seen[0][0]) == [2] and list(seen[0][1]) == [1, 3]
    assert list(seen[1][0]) == [1] and seen[1][1] is None


def test_coo_slice_entry_points_declared_and_exported():
    names = set(_lib.declared_symbols())
    wanted = {"mx_slice_coo_arbitrary_begin", "mx_slice_coo_single", "mxd_coo_slice_workspace_bytes",
              "mxd_coo_slice_count", "mxd_coo_slice_fill", "mxd_coo_single_workspace_bytes", "mxd_coo_single"}
    assert wanted <= names
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in wanted)
    assert lib.mxd_coo_slice_workspace_bytes(1 << 20) >= 8 * (1 << 20)
    assert lib.mxd_coo_single_workspace_bytes() >= 16
    assert callable(mx.subset_coo) and hasattr(mx.TsparseMatrix, "__getitem__")
