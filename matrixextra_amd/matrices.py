"""Host-side stand-ins for the `Matrix` / `float` S4 classes that cross the hot path.

R is not available in this image, so the S4 objects the reference dispatches on
 are mirrored as small Python classes with the same slots:

    dgRMatrix / lgRMatrix / ngRMatrix   @p int32[nrow+1], @j int32[nnz] (0-based), @x, @Dim, @Dimnames
    dgCMatrix                           @p int32[ncol+1], @i int32[nnz], @x
    dgTMatrix / lgTMatrix / ngTMatrix   @i, @j int32[nnz] (0-based triplets, any order, duplicates allowed), @x
    d/i/l/nsparseVector                 @i int32[nnz] (1-based, as in Matrix), @x, @length
    float32                             @Data  (numpy float32, column-major)

R logicals are int32 {0, 1, NA_LOGICAL}.  The classes hold data only; all
arithmetic goes through matrixextra_amd.{matmul,operators,slice} and from there
through the C-ABI.  Operators are wired like the reference's setMethod calls
(R/matmul.R:469, R/operators.R:147-215,792-921, R/slice.R:589-745).
"""
from __future__ import annotations

import numpy as np

NA_INTEGER = np.int32(-2147483648)
NA_LOGICAL = NA_INTEGER
NA_REAL = np.frombuffer(np.uint64(0x7FF00000000007A2).tobytes(), dtype=np.float64)[0]

# R options() read by the hot path (R/zzz.R:140-171)
options = {
    "MatrixExtra.nthreads": 1,          # accepted and forwarded; the GPU path ignores it
    "MatrixExtra.inplace_sort": False,
    "MatrixExtra.drop_sparse": False,
    "MatrixExtra.fast_transpose": False,   # t(): False -> t_deep (a real transpose), True -> t_shallow (R/trans.R:58-72)
}


def stop(msg):
    """R's stop(): all argument errors surface as MatrixExtraError with the reference's message."""
    raise MatrixExtraError(msg)


class MatrixExtraError(ValueError):
    pass


class RsparseMatrix:
    """Compressed sparse row. Subclasses fix the value type."""
    value_dtype = None
    r_class = "RsparseMatrix"
    __array_ufunc__ = None            # numpy arrays on the left defer to __rmatmul__ etc.

    def __init__(self, p, j, x=None, Dim=None, Dimnames=None):
        self.p = np.ascontiguousarray(p, dtype=np.int32)
        self.j = np.ascontiguousarray(j, dtype=np.int32)
        if self.value_dtype is None:
            self.x = None
        else:
            self.x = np.ascontiguousarray(x if x is not None else np.zeros(0), dtype=self.value_dtype)
        if Dim is None:
            ncol = int(self.j.max()) + 1 if self.j.size else 0
            Dim = (self.p.size - 1, ncol)
        self.Dim = (int(Dim[0]), int(Dim[1]))
        self.Dimnames = list(Dimnames) if Dimnames is not None else [None, None]

    # ---- R-like accessors
    def nrow(self):
        return self.Dim[0]

    def ncol(self):
        return self.Dim[1]

    @property
    def shape(self):
        return self.Dim

    def rownames(self):
        return self.Dimnames[0]

    def colnames(self):
        return self.Dimnames[1]

    def has_x(self):
        return self.x is not None

    def toarray(self):
        """as.matrix(): dense float64 (NA_LOGICAL -> nan for logical matrices)."""
        if _dense_route_on():
            return np.asarray(as_matrix(self))
        out = np.zeros(self.Dim, dtype=np.float64)
        for r in range(self.Dim[0]):
            s, e = self.p[r], self.p[r + 1]
            if self.x is None:
                out[r, self.j[s:e]] = 1.0
            else:
                vals = self.x[s:e].astype(np.float64)
                if self.value_dtype == np.int32:
                    vals = np.where(self.x[s:e] == NA_LOGICAL, np.nan, vals)
                np.add.at(out[r], self.j[s:e], vals)
        return out

    def copy(self):
        return type(self)(self.p.copy(), self.j.copy(), None if self.x is None else self.x.copy(),
                          self.Dim, list(self.Dimnames))

    def t(self):                                      # R/trans.R:66-72 (t_masked_csr)
        return _t_masked(self)

    # ---- operator wiring (setMethod registrations of the reference)
    def __matmul__(self, other):                      # `%*%`  R/matmul.R:469, :755-767
        from . import matmul
        return matmul.matmul(self, other)

    def __rmatmul__(self, other):
        from . import matmul
        return matmul.matmul(other, self)

    def __add__(self, other):                         # R/operators.R:792
        from . import operators
        return operators.add_csr_matrices(self, other, False)

    def __sub__(self, other):                         # R/operators.R:841
        from . import operators
        return operators.add_csr_matrices(self, other, True)

    def __mul__(self, other):                         # R/operators.R:147 (CSR), :1217-1260 (vector)
        from . import operators
        if _is_structured(other):                     # a symmetric / triangular operand converts itself and comes back
            return NotImplemented
        if isinstance(other, TsparseMatrix):          # R/operators.R:81-135, :169-180
            return operators.multiply_csr_by_coo(self, other, logical=False)
        if isinstance(other, sparseVector):           # :1634
            return operators.multiply_csr_by_svec_elemwise(self, other)
        if not isinstance(other, (RsparseMatrix, dgCMatrix)):
            return operators.csr_op_vector(self, other, "*")
        return operators.multiply_csr_by_csr(self, other, logical=False)

    def __rmul__(self, other):                        # v * X  (multiplication commutes: R/operators.R:1155-1161)
        from . import operators
        if isinstance(other, sparseVector):           # :1638
            return operators.multiply_csr_by_svec_elemwise(other, self)
        return operators.csr_op_vector(self, other, "*")

    def __and__(self, other):                         # R/operators.R:183 (CSR), :1163-1169 (vector)
        from . import operators
        if _is_structured(other):
            return NotImplemented
        if isinstance(other, TsparseMatrix):          # :194-206
            return operators.multiply_csr_by_coo(self, other, logical=True)
        if not isinstance(other, RsparseMatrix):
            return operators.csr_op_vector(self, other, "&")
        return operators.multiply_csr_by_csr(self, other, logical=True)

    def __truediv__(self, other):                     # X / v
        from . import operators
        return operators.csr_op_vector(self, other, "/")

    def __rtruediv__(self, other):                    # v / X
        from . import operators
        return operators.csr_op_vector(self, other, "/", X_is_LHS=False)

    def __pow__(self, other):                         # X ^ v   R/operators.R:1171-1177
        from . import operators
        return operators.csr_op_vector(self, other, "^")

    def __rpow__(self, other):
        from . import operators
        return operators.csr_op_vector(self, other, "^", X_is_LHS=False)

    def __mod__(self, other):                         # X %% v
        from . import operators
        return operators.csr_op_vector(self, other, "%%")

    def __rmod__(self, other):
        from . import operators
        return operators.csr_op_vector(self, other, "%%", X_is_LHS=False)

    def __floordiv__(self, other):                    # X %/% v
        from . import operators
        return operators.csr_op_vector(self, other, "%/%")

    def __rfloordiv__(self, other):
        from . import operators
        return operators.csr_op_vector(self, other, "%/%", X_is_LHS=False)

    def __or__(self, other):                          # R/operators.R:889
        from . import operators
        return operators.logicalor_csr_matrices(self, other)

    def __xor__(self, other):                         # xor_csr_matrices, R/operators.R:786 (registration commented out upstream)
        from . import operators
        return operators.xor_csr_matrices(self, other)

    def __getitem__(self, key):                       # `[`  R/slice.R:589-745 (0-based here; subset_csr is 1-based)
        from . import slice as _slice
        return _slice.getitem_python(self, key)

    def __repr__(self):
        return f"<{self.r_class} {self.Dim[0]}x{self.Dim[1]}, {self.j.size} entries>"


class dgRMatrix(RsparseMatrix):
    value_dtype = np.float64
    r_class = "dgRMatrix"

    def __setitem__(self, key, value):                # `[<-`  R/assignment.R:521-553 (0-based here; assign_csr is 1-based)
        from . import assign, slice as _slice
        rows, cols = _slice.canonical_key(self, key)
        res = assign.assign_csr(self, rows, cols, value)
        if not isinstance(res, RsparseMatrix):
            stop("This assignment gives a dense matrix, which cannot replace a dgRMatrix in place: "
                 "use assign_csr(x, i, j, value) and keep what it returns.")
        self.p, self.j, self.x = res.p, res.j, res.x


class lgRMatrix(RsparseMatrix):
    value_dtype = np.int32
    r_class = "lgRMatrix"


class ngRMatrix(RsparseMatrix):
    value_dtype = None
    r_class = "ngRMatrix"


class TsparseMatrix:
    """COO (triplets), as Matrix's TsparseMatrix: @i / @j 0-based row / column ids in any order, duplicates allowed
    (they add up).  Subclasses fix the value type.  Operators follow the reference's registrations for
    TsparseMatrix (R/operators.R:81-135, 169-215, 790-930, 1385-1500)."""
    value_dtype = None
    r_class = "TsparseMatrix"
    __array_ufunc__ = None

    def __init__(self, i, j, x=None, Dim=None, Dimnames=None):
        self.i = np.ascontiguousarray(i, dtype=np.int32)
        self.j = np.ascontiguousarray(j, dtype=np.int32)
        if self.value_dtype is None:
            self.x = None
        else:
            self.x = np.ascontiguousarray(x if x is not None else np.zeros(0), dtype=self.value_dtype)
        if Dim is None:
            Dim = (int(self.i.max()) + 1 if self.i.size else 0, int(self.j.max()) + 1 if self.j.size else 0)
        self.Dim = (int(Dim[0]), int(Dim[1]))
        self.Dimnames = list(Dimnames) if Dimnames is not None else [None, None]

    def nrow(self):
        return self.Dim[0]

    def ncol(self):
        return self.Dim[1]

    @property
    def shape(self):
        return self.Dim

    def rownames(self):
        return self.Dimnames[0]

    def colnames(self):
        return self.Dimnames[1]

    def has_x(self):
        return self.x is not None

    def toarray(self):
        """as.matrix(): dense float64 with repeated triplets combined as Matrix does (numeric: summed; logical:
        R's `|`, NA -> nan; pattern: 1)."""
        if _dense_route_on():
            return np.asarray(as_matrix(self))
        out = np.zeros(self.Dim, dtype=np.float64)
        if self.x is None:
            out[self.i, self.j] = 1.0
        elif self.value_dtype == np.int32:
            true, na = np.zeros(self.Dim, dtype=bool), np.zeros(self.Dim, dtype=bool)
            np.logical_or.at(true, (self.i, self.j), (self.x != 0) & (self.x != NA_LOGICAL))
            np.logical_or.at(na, (self.i, self.j), self.x == NA_LOGICAL)
            out[na] = np.nan
            out[true] = 1.0
        else:
            np.add.at(out, (self.i, self.j), self.x)
        return out

    def copy(self):
        return type(self)(self.i.copy(), self.j.copy(), None if self.x is None else self.x.copy(), self.Dim,
                          list(self.Dimnames))

    def t(self):                                      # t_masked_coo -> t_shallow (R/trans.R:74-76)
        return t_shallow(self)

    def __getitem__(self, key):                       # `[`  R/slice_coo.R:200-232 (0-based here; subset_coo is 1-based)
        from . import slice as _slice
        return _slice.getitem_python(self, key)

    # ---- operator wiring
    def __add__(self, other):                         # sparseMatrix + RsparseMatrix, R/operators.R:808-811
        from . import operators
        if isinstance(other, RsparseMatrix):
            return operators.add_csr_matrices(other, self, False)
        if isinstance(other, dgCMatrix):              # TsparseMatrix + CsparseMatrix, :832-835
            return t_shallow(operators.add_csr_matrices(t_shallow(other), t_shallow(self), False))
        return NotImplemented

    def __sub__(self, other):                         # sparseMatrix - RsparseMatrix, :857-860
        from . import operators
        if isinstance(other, RsparseMatrix):
            return operators.add_csr_matrices(self, other, True)
        if isinstance(other, dgCMatrix):
            # (the reference's TsparseMatrix - CsparseMatrix method, :884-888, passes its operands swapped and so
            # returns e2 - e1; the difference here is e1 - e2 like every other `-`)
            return t_shallow(operators.add_csr_matrices(t_shallow(self), t_shallow(other), True))
        return NotImplemented

    def __mul__(self, other):                         # :169-180 (CSR), :1388-1402 (vector)
        from . import operators
        if isinstance(other, RsparseMatrix):
            return operators.multiply_csr_by_coo(other, self, logical=False)
        if isinstance(other, dgCMatrix):              # :189-192
            return t_shallow(operators.multiply_csr_by_coo(t_shallow(other), t_shallow(self), logical=False))
        if isinstance(other, TsparseMatrix) or _is_structured(other):
            return NotImplemented
        if _coo_dense_route(other):                   # :495-515
            return operators.multiply_coo_by_dense(self, other)
        return operators.csr_op_vector(self, other, "*")

    def __rmul__(self, other):
        from . import operators
        if _coo_dense_route(other):                   # :519-539
            return operators.multiply_coo_by_dense(self, other)
        return operators.csr_op_vector(self, other, "*")

    def __and__(self, other):                         # :194-215 (CSR), :1405-1430 (vector)
        from . import operators
        if isinstance(other, RsparseMatrix):
            return operators.multiply_csr_by_coo(other, self, logical=True)
        if isinstance(other, dgCMatrix):
            return t_shallow(operators.multiply_csr_by_coo(t_shallow(other), t_shallow(self), logical=True))
        if isinstance(other, TsparseMatrix) or _is_structured(other):
            return NotImplemented
        if _coo_dense_route(other):                   # :544-552
            return operators.logicaland_coo_by_dense(self, other)
        return operators.csr_op_vector(self, other, "&")

    def __rand__(self, other):
        from . import operators
        if _coo_dense_route(other):                   # :556-564
            return operators.logicaland_coo_by_dense(self, other)
        return operators.csr_op_vector(self, other, "&")

    def __or__(self, other):                          # sparseMatrix | RsparseMatrix, :903-906
        from . import operators
        if isinstance(other, RsparseMatrix):
            return operators.logicalor_csr_matrices(self, other)
        if isinstance(other, dgCMatrix):              # :913-924: the result would be an lgCMatrix
            stop("TsparseMatrix | CsparseMatrix would give an lgCMatrix, which this package does not provide.")
        return NotImplemented

    def __truediv__(self, other):
        from . import operators
        return operators.csr_op_vector(self, other, "/")

    def __rtruediv__(self, other):
        from . import operators
        return operators.csr_op_vector(self, other, "/", X_is_LHS=False)

    def __pow__(self, other):
        from . import operators
        return operators.csr_op_vector(self, other, "^")

    def __rpow__(self, other):
        from . import operators
        return operators.csr_op_vector(self, other, "^", X_is_LHS=False)

    def __mod__(self, other):
        from . import operators
        return operators.csr_op_vector(self, other, "%%")

    def __rmod__(self, other):
        from . import operators
        return operators.csr_op_vector(self, other, "%%", X_is_LHS=False)

    def __floordiv__(self, other):
        from . import operators
        return operators.csr_op_vector(self, other, "%/%")

    def __rfloordiv__(self, other):
        from . import operators
        return operators.csr_op_vector(self, other, "%/%", X_is_LHS=False)

    def __repr__(self):
        return f"<{self.r_class} {self.Dim[0]}x{self.Dim[1]}, {self.i.size} entries>"


class dgTMatrix(TsparseMatrix):
    value_dtype = np.float64
    r_class = "dgTMatrix"


class lgTMatrix(TsparseMatrix):
    value_dtype = np.int32
    r_class = "lgTMatrix"


class ngTMatrix(TsparseMatrix):
    value_dtype = None
    r_class = "ngTMatrix"


class dgCMatrix:
    """Compressed sparse column, numeric: `matrix %*% CsparseMatrix`, t(), +, -, * with an RsparseMatrix, and * with
    a dense matrix or float32 on either side."""
    r_class = "dgCMatrix"
    __array_ufunc__ = None

    def __init__(self, p, i, x, Dim, Dimnames=None):
        self.p = np.ascontiguousarray(p, dtype=np.int32)
        self.i = np.ascontiguousarray(i, dtype=np.int32)
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        self.Dim = (int(Dim[0]), int(Dim[1]))
        self.Dimnames = list(Dimnames) if Dimnames is not None else [None, None]

    def nrow(self):
        return self.Dim[0]

    def ncol(self):
        return self.Dim[1]

    def rownames(self):
        return self.Dimnames[0]

    def colnames(self):
        return self.Dimnames[1]

    def __matmul__(self, other):                      # CsparseMatrix %*% matrix / vector: the transposed product
        from . import matmul
        return matmul.matmul(self, other)

    def __rmatmul__(self, other):                     # matrix %*% CsparseMatrix, R/matmul.R:200
        from . import matmul
        return matmul.matmul(other, self)

    def t(self):                                      # R/trans.R:58-64 (t_masked_csc)
        return _t_masked(self)

    # sparseMatrix (op) RsparseMatrix, R/operators.R:147-179, :810-870: the CSC side goes through as.csr.matrix and
    # the result is a dgRMatrix
    # CsparseMatrix (op) TsparseMatrix goes through t_shallow, R/operators.R:183-186, :826-829, :877-880
    def __add__(self, other):
        from . import operators
        if isinstance(other, TsparseMatrix):
            return t_shallow(operators.add_csr_matrices(t_shallow(self), t_shallow(other), False))
        if not isinstance(other, RsparseMatrix):
            return NotImplemented
        return operators.add_csr_matrices(self, other, False)

    def __sub__(self, other):
        from . import operators
        if isinstance(other, TsparseMatrix):
            return t_shallow(operators.add_csr_matrices(t_shallow(self), t_shallow(other), True))
        if not isinstance(other, RsparseMatrix):
            return NotImplemented
        return operators.add_csr_matrices(self, other, True)

    def __mul__(self, other):
        from . import operators
        if isinstance(other, TsparseMatrix):
            return t_shallow(operators.multiply_csr_by_coo(t_shallow(self), t_shallow(other), logical=False))
        if isinstance(other, RsparseMatrix):
            return operators.multiply_csr_by_csr(self, other, logical=False)
        if _dense_operand(other):                     # CsparseMatrix * matrix / float32, R/operators.R:673-677
            return operators.multiply_csc_by_dense(self, other)
        return NotImplemented

    def __rmul__(self, other):                        # matrix * CsparseMatrix, float32 * CsparseMatrix (:681-689)
        from . import operators
        if _dense_operand(other):
            return operators.multiply_csc_by_dense(self, other)
        return NotImplemented

    def __and__(self, other):                         # :208-211
        from . import operators
        if isinstance(other, TsparseMatrix):
            return t_shallow(operators.multiply_csr_by_coo(t_shallow(self), t_shallow(other), logical=True))
        if _dense_operand(other):                     # :693-709: the result would be an lgCMatrix
            return operators.logicaland_csc_by_dense(self, other)
        return NotImplemented

    def __rand__(self, other):
        from . import operators
        if _dense_operand(other):
            return operators.logicaland_csc_by_dense(self, other)
        return NotImplemented


class sparseVector:
    """Matrix's sparseVector: @i 1-based positions (int32, any order until sorted), @x the values of the stored
    positions (none for an nsparseVector) and @length.  Subclasses fix the value type.  `X * v`, `v * X` and
    `X %*% v` with an RsparseMatrix are wired on the matrix side (R/operators.R:1634-1638, R/matmul.R:755-767)."""
    value_dtype = None
    r_class = "sparseVector"
    __array_ufunc__ = None

    def __init__(self, i, x=None, length=None):
        self.i = np.ascontiguousarray(i, dtype=np.int32).reshape(-1)
        if self.value_dtype is None:
            self.x = None
        else:
            self.x = np.ascontiguousarray(x if x is not None else np.zeros(0), dtype=self.value_dtype).reshape(-1)
        if length is None:
            length = int(self.i.max()) if self.i.size else 0
        self.length = int(length)

    def __len__(self):
        return self.length

    def has_x(self):
        return self.x is not None

    def copy(self):
        return type(self)(self.i.copy(), None if self.x is None else self.x.copy(), self.length)

    def toarray(self):
        """as.numeric(): dense float64 (NA_integer_ / NA -> nan; an nsparseVector gives 1)."""
        out = np.zeros(self.length, dtype=np.float64)
        if self.x is None:
            vals = 1.0
        elif self.value_dtype == np.int32:
            vals = np.where(self.x == NA_INTEGER, np.nan, self.x.astype(np.float64))
        else:
            vals = self.x
        out[self.i.astype(np.int64) - 1] = vals
        return out

    def __rmatmul__(self, other):                     # X %*% v when X defers
        from . import matmul
        return matmul.matmul(other, self)

    def __mul__(self, other):                         # sparseVector * matrix / float32, R/operators.R:1697, :1705
        from . import operators
        if isinstance(other, float32) or (isinstance(other, np.ndarray) and other.ndim == 2):
            return operators.multiply_elemwise_dense_by_svec(self, other)
        return NotImplemented

    def __rmul__(self, other):                        # matrix / float32 * sparseVector, :1693, :1701
        from . import operators
        if isinstance(other, float32) or (isinstance(other, np.ndarray) and other.ndim == 2):
            return operators.multiply_elemwise_dense_by_svec(other, self)
        return NotImplemented

    def __repr__(self):
        return f"<{self.r_class} of length {self.length}, {self.i.size} entries>"


class dsparseVector(sparseVector):
    value_dtype = np.float64
    r_class = "dsparseVector"


class isparseVector(sparseVector):
    value_dtype = np.int32
    r_class = "isparseVector"


class lsparseVector(sparseVector):
    value_dtype = np.int32
    r_class = "lsparseVector"


class nsparseVector(sparseVector):
    value_dtype = None
    r_class = "nsparseVector"


class float32:
    """The `float` package's float32: @Data holds binary32 values, column-major (R/matmul.R:260,276)."""
    r_class = "float32"
    __array_ufunc__ = None

    def __init__(self, Data, Dimnames=None):
        Data = np.asarray(Data, dtype=np.float32)
        self.is_vector = Data.ndim == 1
        self.Data = np.asfortranarray(Data) if Data.ndim == 2 else np.ascontiguousarray(Data)
        self.Dimnames = list(Dimnames) if Dimnames is not None else [None, None]

    @property
    def shape(self):
        return self.Data.shape

    def __rmatmul__(self, other):
        from . import matmul
        return matmul.matmul(other, self)

    def __matmul__(self, other):
        from . import matmul
        return matmul.matmul(self, other)


class DenseMatrix(np.ndarray):
    """Base-R `matrix` with dimnames: an ndarray (column-major) carrying `.Dimnames`."""

    def __new__(cls, data, Dimnames=None):
        obj = np.asfortranarray(data).view(cls)
        obj.Dimnames = list(Dimnames) if Dimnames is not None else [None, None]
        return obj

    def __array_finalize__(self, obj):
        self.Dimnames = getattr(obj, "Dimnames", [None, None])


def _coo_dense_route(x):
    """Whether `TsparseMatrix (op) x` takes multiply_coo_by_dense_internal (R/operators.R:400-483): only under
    options["mxgpu.coo_dense_route"] (off unless set), and only for a dense matrix or a float32."""
    return bool(options.get("mxgpu.coo_dense_route", False)) and (
        isinstance(x, float32) or (isinstance(x, np.ndarray) and x.ndim == 2))


def _dense_operand(x):
    """A dense (or scalar / vector) right operand of a dgCMatrix operator: ndarray, DenseMatrix, float32 or a number."""
    return isinstance(x, (np.ndarray, float32)) or np.isscalar(x)


def dimnames_of(x):
    return getattr(x, "Dimnames", [None, None]) or [None, None]


def _dense_route_on():
    """options["mxgpu.dense_route"] (off unless set): the dense <-> sparse conversions run on the device
    (include/mxgpu_dense.h) and no longer through scipy and the Python loops of toarray()."""
    return bool(options.get("mxgpu.dense_route", False))


def _dense_route(x):
    """Whether as_csr_matrix / as_csc_matrix / as_coo_matrix of `x` take the device route: only under the option, and
    only for a dense matrix (ndarray, DenseMatrix) or a float32 matrix."""
    return _dense_route_on() and ((isinstance(x, float32) and not x.is_vector)
                                  or (isinstance(x, np.ndarray) and x.ndim == 2))


def _dense_to_compressed(x, by_col=False, logical=False, binary=False):
    """dict(indptr, indices, values) of the dense matrix `x` through exports.dense_to_csr: float64 / float32 arrays are
    numeric, int32 arrays R integers (NA_integer_ -> NA_real_), bool arrays logicals; with `logical` a NaN / NA cell
    becomes NA, with `binary` there are no values."""
    from . import _lib, exports
    data = x.Data if isinstance(x, float32) else np.asarray(x)
    if data.dtype not in (np.float64, np.float32, np.int32, np.bool_):
        data = data.astype(np.float64)
    kind = _lib.MX_NONE if binary else _lib.MX_LGL if logical else _lib.MX_F64
    return exports.dense_to_csr(data, by_col, kind)


def as_matrix(x, logical=False):
    """as.matrix() on the device (exports.csr_to_dense): a DenseMatrix with x's Dimnames, float64 (NA -> NA_real_, a
    pattern entry -> 1.0), or int32 R logicals with `logical`.  A TsparseMatrix goes through the device COO sort first
    (repeated triplets merged), a symmetric or triangular operand is expanded on the device first."""
    from . import exports
    if _is_structured(x):
        from . import structured
        x = structured.as_general(x)
    names = list(dimnames_of(x))
    if isinstance(x, TsparseMatrix):
        check_valid_matrix(x)
        x = _coo_to_compressed(x)
    if isinstance(x, RsparseMatrix):
        out = exports.csr_to_dense(x.p, x.j, x.x, x.Dim[1], False, logical)
    elif isinstance(x, dgCMatrix):
        out = exports.csr_to_dense(x.p, x.i, x.x, x.Dim[0], True, logical)
    else:
        stop(f"as_matrix: unsupported class {type(x).__name__}.")
    return DenseMatrix(out, names)


def from_scipy(A, logical=False, binary=False):
    """as.csr.matrix() for a scipy sparse matrix (canonical general CSR; sums duplicates like R's coercion)."""
    import scipy.sparse as sp
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    if binary:
        return ngRMatrix(A.indptr, A.indices, None, A.shape)
    if logical:
        return lgRMatrix(A.indptr, A.indices, (A.data != 0).astype(np.int32), A.shape)
    return dgRMatrix(A.indptr, A.indices, A.data.astype(np.float64), A.shape)


def as_csr_matrix(x, logical=False, binary=False):
    """as.csr.matrix (R/conversions.R:180-295), reduced to the classes that exist here:
    dgRMatrix passes through; lgRMatrix/ngRMatrix are expanded to numeric (or kept/converted
    to logical when `logical=TRUE`); a dgCMatrix goes through the device transpose, a d/l/n TsparseMatrix through
    the device COO sort (repeated triplets merged before the value type changes); scipy matrices and dense
    arrays are converted.  A symmetric or triangular operand (structured.py) is expanded on the device in its own kind
    first, as as(x, "generalMatrix") does, and then follows the same rules."""
    if _is_structured(x):
        from . import structured
        return structured.as_csr(x, logical=logical, binary=binary)
    if isinstance(x, dgCMatrix):
        check_valid_matrix(x)
        x = _csc_to_csr(x, binary=binary)
    if isinstance(x, TsparseMatrix):
        # Matrix coerces T -> R first (merging repeated triplets in the triplets' own type), then the value type
        check_valid_matrix(x)
        x = _coo_to_compressed(x, binary=binary)
    if isinstance(x, RsparseMatrix):
        if binary:
            return x if isinstance(x, ngRMatrix) else ngRMatrix(x.p, x.j, None, x.Dim, x.Dimnames)
        if logical:
            if isinstance(x, lgRMatrix):
                return x
            if isinstance(x, ngRMatrix):
                return lgRMatrix(x.p, x.j, np.ones(x.j.size, dtype=np.int32), x.Dim, x.Dimnames)
            xv = np.where(np.isnan(x.x), NA_LOGICAL, (x.x != 0).astype(np.int32)).astype(np.int32)
            return lgRMatrix(x.p, x.j, xv, x.Dim, x.Dimnames)
        if isinstance(x, dgRMatrix):
            return x
        if isinstance(x, ngRMatrix):
            return dgRMatrix(x.p, x.j, np.ones(x.j.size), x.Dim, x.Dimnames)
        xv = np.where(x.x == NA_LOGICAL, NA_REAL, x.x.astype(np.float64))
        return dgRMatrix(x.p, x.j, xv, x.Dim, x.Dimnames)
    if _dense_route(x):
        res = _dense_to_compressed(x, logical=logical, binary=binary)
        cls = ngRMatrix if binary else lgRMatrix if logical else dgRMatrix
        return cls(res["indptr"], res["indices"], res["values"], x.shape, list(dimnames_of(x)))
    if isinstance(x, np.ndarray):
        import scipy.sparse as sp
        out = from_scipy(sp.csr_matrix(x), logical=logical, binary=binary)
        out.Dimnames = list(dimnames_of(x))
        return out
    return from_scipy(x, logical=logical, binary=binary)


def _is_structured(x):
    """a symmetric or triangular operand (structured.py, which imports this module)"""
    from .structured import StructuredMatrix
    return isinstance(x, StructuredMatrix)


def _csc_to_csr(x, binary=False):
    """CSR arrays of a dgCMatrix through the device transpose (its CSC arrays are the CSR of x^T)."""
    from . import exports
    res = exports.csr_transpose(x.p, x.i, None if binary else x.x, x.Dim[0])
    if binary:
        return ngRMatrix(res["indptr"], res["indices"], None, x.Dim, x.Dimnames)
    return dgRMatrix(res["indptr"], res["indices"], res["values"], x.Dim, x.Dimnames)


def _coo_to_compressed(x, binary=False, csc=False):
    """CSR (csc=True: the CSC arrays, returned as the CSR of x^T) of a TsparseMatrix through the device COO sort,
    in the triplets' own value type."""
    from . import exports
    vals = None if binary else x.x
    if csc:
        res = exports.coo_to_csr(x.j, x.i, vals, x.Dim[1], x.Dim[0])
        Dim, Dimnames = (x.Dim[1], x.Dim[0]), list(reversed(dimnames_of(x)))
    else:
        res = exports.coo_to_csr(x.i, x.j, vals, x.Dim[0], x.Dim[1])
        Dim, Dimnames = x.Dim, list(dimnames_of(x))
    if vals is None:
        return ngRMatrix(res["indptr"], res["indices"], None, Dim, Dimnames)
    cls = lgRMatrix if x.value_dtype == np.int32 else dgRMatrix
    return cls(res["indptr"], res["indices"], res["values"], Dim, Dimnames)


def as_coo_matrix(x, binary=False, logical=False):
    """as.coo.matrix (R/conversions.R:515-590): a TsparseMatrix of the requested kind passes through; another
    TsparseMatrix changes its value type entry by entry (no merging, as the reference relabels the slots); a CSR or
    CSC gains the expanded index vector from the device (storage order: row-major for a CSR, column-major for a
    CSC); dense and scipy inputs go through as_csr_matrix first."""
    from . import exports
    if binary and logical:
        stop("Can pass only one of 'binary' or 'logical'.")
    if _is_structured(x):                             # expanded in its own kind first, then the rules below
        from . import structured
        return structured.as_coo(x, binary=binary, logical=logical)
    if ((type(x) is dgTMatrix and not binary and not logical) or (type(x) is ngTMatrix and binary)
            or (type(x) is lgTMatrix and logical)):
        return x
    if isinstance(x, TsparseMatrix):
        i, j, xv, Dim, Dimnames = x.i, x.j, x.x, x.Dim, list(dimnames_of(x))
        kind = x.value_dtype
    else:
        if isinstance(x, dgCMatrix):
            check_valid_matrix(x)
            i, j, xv = x.i, exports.csr_to_coo(x.p), x.x
        else:
            if not isinstance(x, RsparseMatrix):
                x = as_csr_matrix(x)
            check_valid_matrix(x)
            i, j, xv = exports.csr_to_coo(x.p), x.j, x.x
        Dim, Dimnames = x.Dim, list(dimnames_of(x))
        kind = None if xv is None else xv.dtype.type
    if binary:
        return ngTMatrix(i, j, None, Dim, Dimnames)
    if logical:
        if xv is None:
            lv = np.ones(i.size, dtype=np.int32)
        elif kind == np.int32:
            lv = xv
        else:
            lv = np.where(np.isnan(xv), NA_LOGICAL, (xv != 0).astype(np.int32)).astype(np.int32)
        return lgTMatrix(i, j, lv, Dim, Dimnames)
    if xv is None:
        dv = np.ones(i.size)
    elif kind == np.int32:
        dv = np.where(xv == NA_LOGICAL, NA_REAL, xv.astype(np.float64))
    else:
        dv = xv
    return dgTMatrix(i, j, dv, Dim, Dimnames)


def as_csc_matrix(x):
    """as.csc.matrix (R/conversions.R) -> dgCMatrix.  Values become f64 by as_csr_matrix's rules (NA_LOGICAL ->
    NA_real_, pattern -> 1.0); the CSR -> CSC step is the device transpose, and a TsparseMatrix is sorted into
    CSC order on the device directly (repeated triplets merged before the value type changes)."""
    from . import exports
    if isinstance(x, dgCMatrix):
        return x
    if _is_structured(x):
        from . import structured
        return structured.as_csc(x)
    if isinstance(x, TsparseMatrix):
        check_valid_matrix(x)
        T = as_csr_matrix(_coo_to_compressed(x, csc=True))            # CSR of x^T in f64 = the CSC of x
        return dgCMatrix(T.p, T.j, T.x, x.Dim, list(dimnames_of(x)))
    if _dense_route(x):
        res = _dense_to_compressed(x, by_col=True)
        return dgCMatrix(res["indptr"], res["indices"], res["values"], x.shape, list(dimnames_of(x)))
    x = as_csr_matrix(x)
    check_valid_matrix(x)
    res = exports.csr_transpose(x.p, x.j, x.x, x.Dim[1])
    return dgCMatrix(res["indptr"], res["indices"], res["values"], x.Dim, x.Dimnames)


_SHALLOW = {"dgRMatrix": "dgCMatrix", "dgCMatrix": "dgRMatrix", "lgRMatrix": "lgCMatrix", "ngRMatrix": "ngCMatrix"}


def t_shallow(x):
    """t_shallow (R/trans.R:1-30, :128-150): relabels CSR as the CSC of the transpose (and back) without copying:
    the result shares x's `p` and index arrays; Dim and Dimnames are swapped.  Only dgRMatrix <-> dgCMatrix exist
    here.  A TsparseMatrix stays one, with its `i` and `j` arrays swapped."""
    if _is_structured(x):                             # R <-> C with uplo flipped (R/trans.R:1-44)
        from . import structured
        return structured.t_shallow(x)
    Dim = (x.Dim[1], x.Dim[0])
    Dimnames = list(reversed(dimnames_of(x)))
    if isinstance(x, TsparseMatrix):                  # t_coo_to_coo (R/trans.R:74-76): i and j swap roles
        out = type(x).__new__(type(x))
        out.i, out.j, out.x = x.j, x.i, x.x
    elif type(x) is dgRMatrix:
        out = dgCMatrix.__new__(dgCMatrix)
        out.p, out.i, out.x = x.p, x.j, x.x
    elif type(x) is dgCMatrix:
        out = dgRMatrix.__new__(dgRMatrix)
        out.p, out.j, out.x = x.p, x.i, x.x
    else:
        target = _SHALLOW.get(getattr(x, "r_class", None))
        if target is None:
            stop(f"t_shallow: unsupported class {type(x).__name__}.")
        stop(f"t_shallow: {x.r_class} would become a {target}, which this package does not provide.")
    out.Dim, out.Dimnames = Dim, Dimnames
    return out


def t_deep(x):
    """t_deep (R/trans.R:46-56, :153-162): a real transpose on the device that keeps the class: the CSR (or CSC)
    arrays of x^T, rows in ascending order, Dim and Dimnames swapped."""
    from . import exports
    if _is_structured(x):                             # the stored triangle transposed, uplo flipped
        from . import structured
        return structured.t_deep(x)
    if not isinstance(x, (RsparseMatrix, dgCMatrix)):
        stop(f"t_deep: unsupported class {type(x).__name__}.")
    check_valid_matrix(x)
    if isinstance(x, dgCMatrix):
        res = exports.csr_transpose(x.p, x.i, x.x, x.Dim[0])
        return dgCMatrix(res["indptr"], res["indices"], res["values"], (x.Dim[1], x.Dim[0]),
                         list(reversed(dimnames_of(x))))
    res = exports.csr_transpose(x.p, x.j, x.x, x.Dim[1])
    return type(x)(res["indptr"], res["indices"], res["values"], (x.Dim[1], x.Dim[0]),
                   list(reversed(dimnames_of(x))))


def _t_masked(x):
    """t_masked_csr / t_masked_csc (R/trans.R:58-72)."""
    return t_shallow(x) if options.get("MatrixExtra.fast_transpose", False) else t_deep(x)


def _svec_values_as(v, target):
    """@x of sparse vector `v` in the kind `target` ("d", "i", "l"), by R's as.double / as.integer / as.logical."""
    n = v.i.size
    if v.x is None:
        return np.ones(n, dtype=np.float64 if target == "d" else np.int32)
    if isinstance(v, dsparseVector):
        if target == "d":
            return v.x
        nan = np.isnan(v.x)
        if target == "l":
            return np.where(nan, NA_LOGICAL, (v.x != 0).astype(np.int32)).astype(np.int32)
        with np.errstate(invalid="ignore"):
            return np.where(nan | np.isinf(v.x), NA_INTEGER, np.trunc(np.where(nan, 0.0, v.x))).astype(np.int32)
    na = v.x == NA_INTEGER
    if target == "d":
        return np.where(na, NA_REAL, v.x.astype(np.float64))
    if target == "l" and isinstance(v, isparseVector):
        return np.where(na, NA_LOGICAL, (v.x != 0).astype(np.int32)).astype(np.int32)
    return v.x


def _cells_colmajor(i, j, nrow, ncol):
    """1-based column-major cell numbers of the entries (i, j) of an nrow x ncol matrix, and the order that sorts
    them, as as(x, "sparseVector") numbers the cells of a sparse matrix."""
    if nrow * ncol > 2147483647:
        stop("Matrix has too many cells for the int32 positions of a sparse vector.")
    cell = i.astype(np.int64) + j.astype(np.int64) * nrow + 1
    order = np.argsort(cell, kind="stable")
    return cell[order].astype(np.int32), order


def as_sparse_vector(x, binary=False, logical=False, integer=False):
    """as.sparse.vector (R/conversions.R:593-619): a dsparseVector by default, else the kind asked for.  Dense input
    (a vector, or a matrix / float32 read column-major) stores its non-zero cells, NA included; a sparse vector
    changes kind (NA_integer_ / NA become NA_real_ on the way to a dsparseVector); a CSR, COO or CSC object gives its
    stored cells in column-major order, with the kind of its values."""
    if (binary and logical) or (logical and integer) or (binary and integer):
        stop("Can pass at most one of 'binary', 'logical', 'integer'.")
    if isinstance(x, float32):
        x = x.Data.astype(np.float64)                                 # float::dbl(x)
    if isinstance(x, TsparseMatrix):
        check_valid_matrix(x)
        x = _coo_to_compressed(x)                                     # repeated triplets merge first, as Matrix does
    if isinstance(x, (RsparseMatrix, dgCMatrix)):
        check_valid_matrix(x)
        if isinstance(x, dgCMatrix):
            rows, cols = x.i, np.repeat(np.arange(x.Dim[1], dtype=np.int64), np.diff(x.p))
        else:
            rows, cols = np.repeat(np.arange(x.Dim[0], dtype=np.int64), np.diff(x.p)), x.j
        cell, order = _cells_colmajor(rows, cols, x.Dim[0], x.Dim[1])
        n = x.Dim[0] * x.Dim[1]
        xv = getattr(x, "x", None)
        if xv is None:
            v = nsparseVector(cell, None, n)
        elif xv.dtype == np.int32:
            v = lsparseVector(cell, xv[order], n)
        else:
            v = dsparseVector(cell, xv[order], n)
    elif isinstance(x, sparseVector):
        v = x
    else:
        a = np.asarray(x)
        is_lgl = bool(getattr(x, "r_logical", False)) or a.dtype == np.bool_
        if a.ndim > 2:
            stop("Cannot convert an array of more than two dimensions to a sparse vector.")
        a = a.reshape(-1, order="F")
        if a.dtype == np.bool_:
            a = a.astype(np.int32)
        elif a.dtype != np.int32:
            a = a.astype(np.float64)
        keep = np.flatnonzero(a != 0)                                 # NaN != 0 and NA_integer_ != 0: NA cells stay
        cls = lsparseVector if is_lgl else isparseVector if a.dtype == np.int32 else dsparseVector
        v = cls(keep + 1, a[keep], a.size)
    if binary:
        return v if isinstance(v, nsparseVector) else nsparseVector(v.i, None, v.length)
    cls, target = ((isparseVector, "i") if integer else (lsparseVector, "l") if logical else (dsparseVector, "d"))
    if type(v) is cls:
        return v
    return cls(v.i, _svec_values_as(v, target), v.length)


def _check_valid_svec(X):
    """R/utils.R:456-468."""
    from . import exports
    if X.length is None:
        stop("Vector has invalid length.")
    if X.length < 0:
        stop("Vector has negative length.")
    if not isinstance(X, nsparseVector) and X.i.size != X.x.size:
        stop("Vector indices and values have different length.")
    res = exports.check_valid_svec(X.i, X.length)
    if res:
        stop(res["err"])


def check_valid_matrix(X):
    """R/utils.R:349-410, TsparseMatrix / RsparseMatrix / CsparseMatrix branches, and :456-468 for a sparseVector."""
    if isinstance(X, sparseVector):
        return _check_valid_svec(X)
    nrows, ncols = X.Dim
    if nrows < 0:
        stop("Matrix has invalid number of rows.")
    if ncols < 0:
        stop("Matrix has invalid number of columns.")
    dn = dimnames_of(X)
    if dn[0] is not None and len(dn[0]) and len(dn[0]) != nrows:
        stop("Row names of matrix do not match with number of rows.")
    if dn[1] is not None and len(dn[1]) and len(dn[1]) != ncols:
        stop("Column names of matrix do not match with number of columns.")
    if _is_structured(X):                             # :367-373, then the compressed-layout checks
        from . import structured
        return structured.check_valid_structured(X)
    if isinstance(X, TsparseMatrix):
        if X.i.size != X.j.size:
            stop("Matrix is invalid (row and column indices have different length).")
        if X.x is not None and X.x.size != X.i.size:
            stop("Matrix is invalid (values and indices have different number of entries).")
        return
    if isinstance(X, RsparseMatrix):
        idx, dim = X.j, nrows
    elif isinstance(X, dgCMatrix):
        idx, dim = X.i, ncols
    else:
        stop("Unexpected error. Please open an issue in GitHub explaining what you were doing.")
    if X.p.size and X.p[-1] == NA_INTEGER:
        stop("Matrix is invalid (missing last index pointer, might indicate integer overflow).")
    if getattr(X, "x", None) is not None and idx.size != X.x.size:
        stop("Matrix is invalid (lengths of indices and values differ).")
    if X.p.size - 1 != dim:
        stop("Matrix is invalid ('p' doesn't match with dimension).")
    if X.p[0] != 0 or X.p[dim] != idx.size:
        stop("Matrix is invalid ('p' has bad start/end.)")


def sort_sparse_indices(X, copy=False, byrow=True):
    """sort_sparse_indices (R/utils.R:22-161) for RsparseMatrix: per-row index sort on the
    device (src/misc.cpp:261-298).  copy=TRUE sorts deep copies of @j/@x and returns a new object.
    A sparseVector (:126-155) is sorted by @i, @x carried, by the device radix sort (src/misc.cpp:460-527).
    A TsparseMatrix (:85-124) has its triplets sorted by (i, j), or by (j, i) with byrow=False (the reference sorts
    the t_shallow of X and turns it back), by the device COO sort (src/misc.cpp:387-457): in place
    and returning X itself, or with copy=TRUE in deep copies of @i / @j / @x held by a new object.  Entries of one
    cell keep their input order.  `byrow` matters to a TsparseMatrix only."""
    from . import exports
    if isinstance(X, TsparseMatrix):
        check_valid_matrix(X)
        kind = {dgTMatrix: "numeric", lgTMatrix: "logical", ngTMatrix: "binary"}.get(type(X))
        if kind is None:
            stop("Method is only applicable to sparse matrices in CSR, CSC, and COO formats, and to sparse vectors.")
        if copy:
            X = X.copy()
        first, second = (X.i, X.j) if byrow else (X.j, X.i)
        if kind == "binary":
            exports.sort_coo_indices_binary(first, second)
        else:
            getattr(exports, "sort_coo_indices_" + kind)(first, second, X.x)
        return X
    if isinstance(X, sparseVector):
        if copy:
            X = X.copy()
        kind = {dsparseVector: "numeric", isparseVector: "integer", lsparseVector: "logical",
                nsparseVector: "binary"}.get(type(X))
        if kind is None:
            stop("Method is only applicable to sparse matrices in CSR, CSC, and COO formats, and to sparse vectors.")
        if kind == "binary":
            exports.sort_vector_indices_binary(X.i)
        else:
            getattr(exports, "sort_vector_indices_" + kind)(X.i, X.x)
        return X
    check_valid_matrix(X)
    if copy:
        X = type(X)(X.p, X.j.copy(), None if X.x is None else X.x.copy(), X.Dim, list(X.Dimnames))
    exports.sort_sparse_indices_inplace(X.p, X.j, X.x)
    return X
