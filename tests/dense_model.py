"""numpy model of the dense <-> compressed conversions (include/mxgpu_dense.h): the keep and value rules written out.
Kinds of a dense operand: "f64", "f32", "i32" (R integers), "lgl" (R logicals, int32); of the values: "d", "l", "n".
CSR is row-major order, CSC column-major; everything is compared bit for bit with `bits`."""
import numpy as np

NA = np.int32(-2**31)
NA_REAL = np.array([0x7FF00000000007A2], dtype=np.uint64).view(np.float64)[0]


def bits(a):
    """the array as unsigned integers of its element size (None stays None)"""
    return None if a is None else np.ascontiguousarray(a).view(f"u{np.asarray(a).dtype.itemsize}")


def dense_to_csr(D, kind, by_col, out):
    """(indptr, indices, values) of the cells with D != 0 (NaN and NA kept, -0.0 dropped), values of kind `out`"""
    A = D.T if by_col else D
    seg, idx = np.nonzero(A != 0)                       # row-major: segments ascending, indices ascending
    indptr = np.concatenate([[0], np.cumsum((A != 0).sum(axis=1))]).astype(np.int32)
    x = A[seg, idx]
    if out == "n":
        v = None
    elif out == "d":
        v = x.astype(np.float64) if kind in ("f64", "f32") else np.where(x == NA, NA_REAL, x.astype(np.float64))
    elif kind == "lgl":
        v = x.astype(np.int32)
    else:
        v = np.where(np.isnan(x) if kind in ("f64", "f32") else x == NA, NA, np.int32(1)).astype(np.int32)
    return indptr, idx.astype(np.int32), v


def csr_to_dense(p, j, x, nother, by_col, logical):
    """the dense matrix of strictly ascending, in-range arrays: float64, or int32 R logicals with `logical`"""
    nseg = p.size - 1
    seg = np.repeat(np.arange(nseg), np.diff(p))
    if x is None:
        v = 1
    elif logical:
        v = x if x.dtype == np.int32 else np.where(np.isnan(x), NA, (x != 0).astype(np.int32))
    else:
        v = x if x.dtype == np.float64 else np.where(x == NA, NA_REAL, x.astype(np.float64))
    out = np.zeros((nseg, nother), dtype=np.int32 if logical else np.float64)
    out[seg, j] = v
    return np.asfortranarray(out.T if by_col else out)
