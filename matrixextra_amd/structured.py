"""Stand-ins for Matrix's symmetric and triangular compressed classes, and their way onto the device path.

    dsRMatrix / lsRMatrix / nsRMatrix   @p, @j, @x, @Dim, @Dimnames, @uplo          one triangle of a symmetric matrix
    dtRMatrix / ltRMatrix / ntRMatrix   ... and @diag ("N", or "U": a unit diagonal that is not stored)
    dsCMatrix / dtCMatrix               @p, @i, @x: the numeric column-compressed twins (only the numeric C class
                                        exists here)

None of them is an RsparseMatrix or a dgCMatrix: they share one base, StructuredMatrix, so that code which has not
been taught about them fails loudly and never reads a triangle as the whole matrix.  The reference starts almost every
entry point with as.csr.matrix(x) (R/conversions.R:180-295), which leaves the expansion to Matrix's
as(x, "generalMatrix"); here the expansion runs on the device (include/mxgpu_sym.h):

    symmetric, row-compressed      exports.csr_symmetric_to_general
    symmetric, column-compressed   the same call on (p, i, x) with uplo flipped: the CSC arrays of a symmetric matrix
                                   are the CSR arrays of the same matrix, so there is no transpose
    triangular, diag = "N"         a relabel that shares the arrays
    triangular, diag = "U"         exports.csr_unit_triangular_to_general
    dtCMatrix                      t_shallow, the above, then as the CSC of x (as_csr_matrix goes on through the device
                                   transpose)

The operators convert with as_csr_matrix / as_csc_matrix and delegate, as each reference method does."""
from __future__ import annotations

import operator

import numpy as np

from . import exports, matrices as M
from .matrices import dgCMatrix, dgRMatrix, dimnames_of, lgRMatrix, ngRMatrix, stop

_FLIP = {"U": "L", "L": "U"}


class StructuredMatrix:
    """Common base of the symmetric and triangular classes.  `layout` is "R" (slots p, j) or "C" (slots p, i)."""
    value_dtype = None
    r_class = "sparseMatrix"
    layout = "R"
    symmetric = False
    general = None                        # the class of as(x, "generalMatrix")
    __array_ufunc__ = None

    def __init__(self, p, idx, x=None, Dim=None, Dimnames=None, uplo="U", diag="N"):
        self.p = np.ascontiguousarray(p, dtype=np.int32)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if self.layout == "R":
            self.j = idx
        else:
            self.i = idx
        if self.value_dtype is None:
            self.x = None
        else:
            self.x = np.ascontiguousarray(x if x is not None else np.zeros(0), dtype=self.value_dtype)
        n = self.p.size - 1
        self.Dim = (int(Dim[0]), int(Dim[1])) if Dim is not None else (n, n)
        self.Dimnames = list(Dimnames) if Dimnames is not None else [None, None]
        self.uplo = uplo
        if not self.symmetric:
            self.diag = diag

    @property
    def idx(self):
        return self.j if self.layout == "R" else self.i

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

    def copy(self):
        out = relabel(self, type(self), self.uplo)
        out.p, out.x = self.p.copy(), None if self.x is None else self.x.copy()
        setattr(out, "j" if self.layout == "R" else "i", self.idx.copy())
        return out

    def toarray(self):
        """as.matrix(): dense float64, through the device expansion"""
        return as_csr(self).toarray()

    def t(self):                                      # R/trans.R:58-72
        return M._t_masked(self)

    # ---- operator wiring: as.csr.matrix / as.csc.matrix of the operand, then the general classes' methods
    def _binary(self, other, op, reflected=False):
        a = as_general(self)
        b = as_general(other) if isinstance(other, StructuredMatrix) else other
        return op(b, a) if reflected else op(a, b)

    def __matmul__(self, other):
        return self._binary(other, operator.matmul)

    def __rmatmul__(self, other):
        return self._binary(other, operator.matmul, True)

    def __add__(self, other):
        return self._binary(other, operator.add)

    def __radd__(self, other):
        return self._binary(other, operator.add, True)

    def __sub__(self, other):
        return self._binary(other, operator.sub)

    def __rsub__(self, other):
        return self._binary(other, operator.sub, True)

    def __mul__(self, other):
        return self._binary(other, operator.mul)

    def __rmul__(self, other):
        return self._binary(other, operator.mul, True)

    def __and__(self, other):
        return self._binary(other, operator.and_)

    def __rand__(self, other):
        return self._binary(other, operator.and_, True)

    def __or__(self, other):
        return self._binary(other, operator.or_)

    def __ror__(self, other):
        return self._binary(other, operator.or_, True)

    def __truediv__(self, other):
        return self._binary(other, operator.truediv)

    def __rtruediv__(self, other):
        return self._binary(other, operator.truediv, True)

    def __pow__(self, other):
        return self._binary(other, operator.pow)

    def __rpow__(self, other):
        return self._binary(other, operator.pow, True)

    def __mod__(self, other):
        return self._binary(other, operator.mod)

    def __rmod__(self, other):
        return self._binary(other, operator.mod, True)

    def __floordiv__(self, other):
        return self._binary(other, operator.floordiv)

    def __rfloordiv__(self, other):
        return self._binary(other, operator.floordiv, True)

    def __getitem__(self, key):                       # `[`: R/slice.R:589-745 for the R classes; a C class converts first
        from . import slice as _slice
        return _slice.getitem_python(self if self.layout == "R" else M.as_csr_matrix(self), key)

    def __repr__(self):
        extra = f', uplo "{self.uplo}"' + ("" if self.symmetric else f', diag "{self.diag}"')
        return f"<{self.r_class} {self.Dim[0]}x{self.Dim[1]}, {self.idx.size} stored entries{extra}>"


def _cls(name, layout, symmetric, value_dtype, general):
    return type(name, (StructuredMatrix,), dict(r_class=name, layout=layout, symmetric=symmetric,
                                                value_dtype=value_dtype, general=general,
                                                __doc__=f"Matrix's {name}."))


dsRMatrix = _cls("dsRMatrix", "R", True, np.float64, dgRMatrix)
lsRMatrix = _cls("lsRMatrix", "R", True, np.int32, lgRMatrix)
nsRMatrix = _cls("nsRMatrix", "R", True, None, ngRMatrix)
dtRMatrix = _cls("dtRMatrix", "R", False, np.float64, dgRMatrix)
ltRMatrix = _cls("ltRMatrix", "R", False, np.int32, lgRMatrix)
ntRMatrix = _cls("ntRMatrix", "R", False, None, ngRMatrix)
dsCMatrix = _cls("dsCMatrix", "C", True, np.float64, dgCMatrix)
dtCMatrix = _cls("dtCMatrix", "C", False, np.float64, dgCMatrix)
_TWIN = {dsRMatrix: dsCMatrix, dsCMatrix: dsRMatrix, dtRMatrix: dtCMatrix, dtCMatrix: dtRMatrix}


def relabel(x, cls, uplo, Dim=None, Dimnames=None):
    """an object of class `cls` that shares x's arrays"""
    out = cls.__new__(cls)
    out.p, out.x = x.p, x.x
    setattr(out, "j" if cls.layout == "R" else "i", x.idx)
    out.Dim = x.Dim if Dim is None else Dim
    out.Dimnames = list(dimnames_of(x)) if Dimnames is None else Dimnames
    out.uplo = uplo
    if not cls.symmetric:
        out.diag = getattr(x, "diag", "N")
    return out


def _symmetric_dimnames(x):
    """the Dimnames of as(x, "generalMatrix") for a symmetricMatrix: Matrix gives both dimensions the names that are
    there (the reference's `sy` carries column names only; its general form has them on the rows too)"""
    rn, cn = dimnames_of(x)
    return [rn if rn is not None else cn, cn if cn is not None else rn]


# ---- validation -----------------------------------------------------------------------------------------------------------
WRONG_TRIANGLE = "Matrix is invalid (%d entries lie outside the triangle that 'uplo' names)."
STORED_UNIT_DIAGONAL = "Matrix is invalid (%d entries lie on the diagonal or outside the triangle, but 'diag' is \"U\")."


def check_valid_structured(X):
    """The symmetric / triangular branch of check_valid_matrix (R/utils.R:367-373, its three messages), the
    compressed-layout checks of :383-403, and then two checks that are this build's own, with its own messages
    (Matrix's validity text is not pinned here): no entry outside the stored triangle, counted on the device, and no
    stored diagonal under diag = "U"."""
    nrows, ncols = X.Dim
    if nrows != ncols:
        stop("Matrix type implies square shape, but number of rows and columns differ.")
    if hasattr(X, "diag") and not (isinstance(X.diag, str) and X.diag in ("N", "U")):
        stop("Matrix has invalid diagonal type.")
    if not (isinstance(X.uplo, str) and X.uplo in ("L", "U")):
        stop("Matrix has invalid 'uplo' field.")
    idx = X.idx
    if X.p.size and X.p[-1] == M.NA_INTEGER:
        stop("Matrix is invalid (missing last index pointer, might indicate integer overflow).")
    if X.x is not None and idx.size != X.x.size:
        stop("Matrix is invalid (lengths of indices and values differ).")
    if X.p.size - 1 != nrows:
        stop("Matrix is invalid ('p' doesn't match with dimension).")
    if X.p[0] != 0 or X.p[nrows] != idx.size:
        stop("Matrix is invalid ('p' has bad start/end.)")
    unit = getattr(X, "diag", "N") == "U"
    uplo = X.uplo if X.layout == "R" else _FLIP[X.uplo]           # a CSC's slots are the CSR of the transpose
    outside = exports.csr_triangle_check(X.p, idx, uplo, strict=unit)
    if outside:
        stop((STORED_UNIT_DIAGONAL if unit else WRONG_TRIANGLE) % outside)


# ---- as(x, "generalMatrix") -----------------------------------------------------------------------------------------------
def _expand_rows(x, uplo):
    """(p, idx, x) of the general form of the row-compressed slots (p, x.idx, x.x) that store the triangle `uplo`"""
    if x.symmetric:
        res = exports.csr_symmetric_to_general(x.p, x.idx, x.x, uplo)
    elif x.diag == "U":
        res = exports.csr_unit_triangular_to_general(x.p, x.idx, x.x, uplo)
    else:
        return x.p, x.idx, x.x                                     # diag = "N": the stored triangle is the matrix
    return res["indptr"], res["indices"], res["values"]


def as_general(x):
    """as(x, "generalMatrix") in the operand's own kind and layout: a dgRMatrix / lgRMatrix / ngRMatrix for the R
    classes, a dgCMatrix for the C classes."""
    M.check_valid_matrix(x)
    names = _symmetric_dimnames(x) if x.symmetric else list(dimnames_of(x))
    if x.layout == "R":
        p, j, xv = _expand_rows(x, x.uplo)
        return x.general(p, j, xv, x.Dim, names)
    p, i, xv = _expand_rows(x, _FLIP[x.uplo])
    return dgCMatrix(p, i, xv, x.Dim, names)


def as_csr(x, logical=False, binary=False):
    """as.csr.matrix of a structured operand: expanded in its own kind first, then the existing rules."""
    g = as_general(x)
    if isinstance(g, dgCMatrix) and x.symmetric:                   # the CSC arrays of a symmetric matrix are its CSR
        g = dgRMatrix(g.p, g.i, g.x, g.Dim, g.Dimnames)
    return M.as_csr_matrix(g, logical=logical, binary=binary)


def as_csc(x):
    """as.csc.matrix of a structured operand."""
    if x.symmetric and x.layout == "R":                            # no transpose: general CSR = general CSC
        g = M.as_csr_matrix(as_general(x))
        return dgCMatrix(g.p, g.j, g.x, g.Dim, g.Dimnames)
    return M.as_csc_matrix(as_general(x))


def as_coo(x, binary=False, logical=False):
    return M.as_coo_matrix(as_general(x), binary=binary, logical=logical)


# ---- transposes -----------------------------------------------------------------------------------------------------------
def t_shallow(x):
    """t_shallow (R/trans.R:1-44): R <-> C relabel with uplo flipped, sharing the arrays."""
    twin = _TWIN.get(type(x))
    if twin is None:
        stop(f"t_shallow: {x.r_class} would become its column-compressed twin, which this package does not provide.")
    return relabel(x, twin, _FLIP[x.uplo], (x.Dim[1], x.Dim[0]), list(reversed(dimnames_of(x))))


def t_deep(x):
    """t_deep keeps the class: the device transpose of the stored triangle, uplo flipped."""
    M.check_valid_matrix(x)
    res = exports.csr_transpose(x.p, x.idx, x.x, x.Dim[0])
    out = relabel(x, type(x), _FLIP[x.uplo], (x.Dim[1], x.Dim[0]), list(reversed(dimnames_of(x))))
    out.p, out.x = res["indptr"], res["values"]
    setattr(out, "j" if x.layout == "R" else "i", res["indices"])
    return out


# ---- x[i, j] with two scalars (R/slice.R:316-333) -------------------------------------------------------------------------
def _in_lower(i, j):
    return i > j


def scalar_route(x, i, j):
    """What R/slice.R:316-333 decides before extract_single_val_csr_*, for 1-based in-range (i, j): ("value", v) when
    the answer is known from the class alone (0 outside a triangular's triangle, 1 on a unit diagonal), else
    ("lookup", i, j) with (i, j) swapped into the stored triangle of a symmetric."""
    outside = (x.uplo == "U" and _in_lower(i, j)) or (x.uplo == "L" and _in_lower(j, i))
    if not x.symmetric and outside:
        return ("value", 0.0)
    if getattr(x, "diag", "N") == "U" and i == j:
        return ("value", 1.0)
    if x.symmetric and outside:
        i, j = j, i
    return ("lookup", i, j)


def stored_as_general(x):
    """the stored entries under the general class of x's kind, sharing the arrays (what extract_single_val_csr_* reads)"""
    return x.general(x.p, x.j, x.x, x.Dim, list(dimnames_of(x)))


__all__ = ["StructuredMatrix", "dsRMatrix", "lsRMatrix", "nsRMatrix", "dtRMatrix", "ltRMatrix", "ntRMatrix",
           "dsCMatrix", "dtCMatrix"]
