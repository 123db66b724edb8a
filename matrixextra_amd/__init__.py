"""matrixextra_amd — MI355X (gfx950) backend for MatrixExtra's CSR hot path.

Layers (SURVEY.md §1 / DESIGN.md):
  csrc/*.hip + include/mxgpu.h   hand-written HIP kernels behind a C-ABI (libmxgpu.so)
  exports.py                     twins of R/RcppExports.R wrappers (ctypes -> C-ABI)
  matrices.py                    dgRMatrix / lgRMatrix / ngRMatrix / dgCMatrix / d/l/ngTMatrix / d/i/l/nsparseVector / float32
                                 stand-ins
  structured.py                  dsR / lsR / nsR / dtR / ltR / ntR / dsC / dtC stand-ins and their device expansion
  matmul.py operators.py slice.py assign.py cleanup.py bind.py reduce.py   mirrors of the R glue (checks, messages, dimnames, classes)
  device.py                      device-resident CSR + mxd_* launches on torch tensors (bench, multi-GPU)
  distributed.py                 row-block sharding + RCCL all-gather of C

No CPU fallback anywhere: without libmxgpu.so and a GPU every compute call raises.
"""
from . import _lib  # noqa: F401
from .matrices import (DenseMatrix, MatrixExtraError, NA_INTEGER, NA_LOGICAL, NA_REAL, RsparseMatrix,  # noqa: F401
                       as_csr_matrix, check_valid_matrix, dgCMatrix, dgRMatrix, float32, from_scipy,
                       lgRMatrix, ngRMatrix, options, sort_sparse_indices)
from .matrices import as_csc_matrix, as_matrix, t_deep, t_shallow  # noqa: F401
from .matrices import TsparseMatrix, as_coo_matrix, dgTMatrix, lgTMatrix, ngTMatrix  # noqa: F401
from .matrices import (as_sparse_vector, dsparseVector, isparseVector, lsparseVector, nsparseVector,  # noqa: F401
                       sparseVector)
from .matmul import RLogical, crossprod, tcrossprod  # noqa: F401  (`%*%` is the @ operator)
from .operators import (add_csr_matrices, logicalor_csr_matrices, multiply_csr_by_coo,  # noqa: F401
                        multiply_csr_by_csr, multiply_csr_by_svec_elemwise, multiply_elemwise_dense_by_svec,
                        xor_csr_matrices)
from .slice import subset_coo, subset_csr  # noqa: F401
from .assign import assign_csr  # noqa: F401
from .cleanup import check_sparse_matrix, filterSparse, remove_sparse_zeros  # noqa: F401
from .bind import cbind, cbind2, rbind, rbind2, rbind_csr  # noqa: F401
from .structured import (StructuredMatrix, dsCMatrix, dsRMatrix, dtCMatrix, dtRMatrix, lsRMatrix, ltRMatrix,  # noqa: F401
                         nsRMatrix, ntRMatrix)
from .reduce import colMeans, colSums, diag, norm, rowMeans, rowSums  # noqa: F401

__version__ = "0.1.0"
