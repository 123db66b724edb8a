### mxgpu_overlay.R — route MatrixExtra's CSR hot path to the MI355X backend without rebuilding MatrixExtra.
###
### The S4 method registrations of the reference (R/matmul.R, R/operators.R, R/slice.R) and its R glue stay
### exactly as they are: `%*%`, `tcrossprod`, `+`, `-`, `*`, `&`, `|`, `[` on dgRMatrix objects dispatch
### unchanged, and so does `[<-` on a dgRMatrix.  The glue reaches native code only through the one-line wrappers of R/RcppExports.R
### (e.g. :148-150 `tcrossprod_csr_dense_numeric <- function(...) .Call(`_MatrixExtra_tcrossprod_csr_dense_numeric`, ...)`).
### This overlay rebinds those 19 wrappers inside the MatrixExtra namespace so that they `.Call` the routines of
### the same names registered by mxgpu_r.so (matrixextra_amd/csrc/r_shim.cpp), which forward to libmxgpu.so.
### Every other native routine (~140 of them) keeps pointing at MatrixExtra's own CPU code.
### It also rebinds t_deep_internal (R/trans.R:46-56) to the device transpose for general d/l/n R/C classes, and
### as.csr.matrix / as.csc.matrix to the device COO sort for general d/l/n TsparseMatrix inputs.
###
### Usage:
###   library(MatrixExtra)
###   source("mxgpu_overlay.R")
###   mxgpu_enable("/path/to/mxgpu_r.so")     # needs libmxgpu.so on the loader path and a visible MI355X
###   ... X %*% Y, X + Z, X[rows, ] ...       # now run on the GPU
###   mxgpu_disable()                         # restore the CPU wrappers
###
### NOT TESTED in the development image (no R there); see INTEGRATION.md.

.mxgpu_state <- new.env()

.mxgpu_hot_routines <- c(
    "matmul_dense_csc_numeric", "matmul_dense_csc_float32",
    "tcrossprod_dense_csr_numeric", "tcrossprod_dense_csr_float32",
    "tcrossprod_csr_dense_numeric", "tcrossprod_csr_dense_float32",
    "matmul_csr_dvec_numeric", "matmul_csr_dvec_integer", "matmul_csr_dvec_logical", "matmul_csr_dvec_float32",
    "multiply_csr_elemwise", "logicaland_csr_elemwise", "add_csr_elemwise", "logicalor_csr_elemwise",
    "copy_csr_rows_numeric", "copy_csr_rows_logical", "copy_csr_rows_binary",
    "check_is_seq", "check_is_rev_seq",
    ## SURVEY section 8(f) rank 2: column-filtering slices and reversals
    "copy_csr_rows_col_seq_numeric", "copy_csr_rows_col_seq_logical", "copy_csr_rows_col_seq_binary",
    "copy_csr_arbitrary_numeric", "copy_csr_arbitrary_logical", "copy_csr_arbitrary_binary",
    "reverse_rows_numeric", "reverse_rows_logical", "reverse_rows_binary",
    "reverse_columns_inplace_numeric", "reverse_columns_inplace_logical", "reverse_columns_inplace_binary",
    ## rank 4: values-only CSR (op) vector
    "multiply_csr_by_dvec_no_NAs_numeric", "logicaland_csr_by_dvec_internal",
    ## the NA-keeping route of CSR (op) vector (multiply_csr_by_dvec_elemwise_internal, R/operators.R:996-1129)
    "multiply_csr_by_dvec_with_NAs",
    ## COO (TsparseMatrix) operands
    "multiply_csr_by_coo_elemwise", "logicaland_csr_by_coo_elemwise",
    "multiply_coo_by_dense_ignore_NAs_numeric", "multiply_coo_by_dense_ignore_NAs_logical",
    ## COO slicing, X[i, j] of a TsparseMatrix (subset_coo, R/slice_coo.R)
    "slice_coo_single_numeric", "slice_coo_single_logical", "slice_coo_single_binary",
    "slice_coo_arbitrary_numeric", "slice_coo_arbitrary_logical", "slice_coo_arbitrary_binary",
    ## remove_sparse_zeros / filterSparse / check_sparse_matrix (R/utils.R): compaction and validation
    "remove_zero_valued_csr_numeric", "remove_zero_valued_csr_logical",
    "remove_zero_valued_coo_numeric", "remove_zero_valued_coo_logical",
    "remove_zero_valued_svec_numeric", "remove_zero_valued_svec_integer", "remove_zero_valued_svec_logical",
    "check_valid_csr_matrix", "check_valid_coo_matrix", "check_valid_svec", "rebuild_indptr_after_filter",
    ## CsparseMatrix * matrix (multiply_csc_by_dense, R/operators.R:568-710)
    "multiply_csc_by_dense_ignore_NAs_numeric", "multiply_csc_by_dense_ignore_NAs_float32",
    "multiply_csc_by_dense_ignore_NAs_integer", "multiply_csc_by_dense_ignore_NAs_logical",
    "logicaland_csc_by_dense_ignore_NAs",
    "multiply_csc_by_dense_keep_NAs_numeric", "multiply_csc_by_dense_keep_NAs_integer",
    "multiply_csc_by_dense_keep_NAs_logical", "multiply_csc_by_dense_keep_NAs_float32",
    ## RsparseMatrix * sparseVector (multiply_csr_by_svec_elemwise_internal, R/operators.R:1564-1622) and the
    ## sparse-vector branch of sort_sparse_indices (R/utils.R:126-155), which sorts its arguments in place
    "multiply_csr_by_svec_no_NAs", "multiply_csr_by_svec_keep_NAs",
    "sort_vector_indices_numeric", "sort_vector_indices_integer", "sort_vector_indices_logical",
    "sort_vector_indices_binary",
    ## the TsparseMatrix branch of sort_sparse_indices (R/utils.R:85-124), in place as well
    "sort_coo_indices_numeric", "sort_coo_indices_logical", "sort_coo_indices_binary",
    ## the outer products of a one-column RsparseMatrix (outerprod_csrsinglecol_by_dvec, R/matmul.R:659-751) and the
    ## float32 vector forms of `%*%` / tcrossprod / crossprod (R/matmul.R:220-262, 327-367, 405-427, 480-500)
    "matmul_colvec_by_scolvecascsr", "matmul_colvec_by_scolvecascsr_f32",
    "matmul_spcolvec_by_scolvecascsr_numeric", "matmul_spcolvec_by_scolvecascsr_integer",
    "matmul_spcolvec_by_scolvecascsr_logical", "matmul_spcolvec_by_scolvecascsr_binary",
    "matmul_rowvec_by_csc", "matmul_rowvec_by_cscbin",
    ## `[<-` of a dgRMatrix (assign_csr_internal, R/assignment.R:37-513): scalar values and whole-row replacement;
    ## the vector-valued routines (set_single_*_to_rowvec / _colvec / _svec) stay on the CPU
    "set_single_row_to_zero", "set_single_col_to_zero", "set_single_val_to_zero",
    "set_rowseq_to_zero", "set_colseq_to_zero", "set_arbitrary_rows_to_zero", "set_arbitrary_cols_to_zero",
    "set_arbitrary_rows_single_col_to_zero", "set_single_row_arbitrary_cols_to_zero",
    "set_arbitrary_rows_arbitrary_cols_to_zero",
    "set_single_row_to_const", "set_single_col_to_const", "set_single_val_to_const",
    "set_rowseq_to_const", "set_colseq_to_const", "set_arbitrary_rows_to_const", "set_arbitrary_cols_to_const",
    "set_arbitrary_rows_single_col_to_const", "set_single_row_arbitrary_cols_to_const",
    "set_arbitrary_rows_arbitrary_cols_to_const",
    "set_rowseq_to_smat", "set_arbitrary_rows_to_smat"
)

mxgpu_enable <- function(shim_path, min_nnz = 0L) {
    dll <- dyn.load(shim_path)
    ns <- asNamespace("MatrixExtra")
    .mxgpu_state$saved <- list()
    for (fn in .mxgpu_hot_routines) {
        cpu_fun <- get(fn, envir = ns)
        .mxgpu_state$saved[[fn]] <- cpu_fun
        native <- getNativeSymbolInfo(paste0("_MatrixExtra_", fn), dll)
        gpu_fun <- local({
            native <- native; cpu_fun <- cpu_fun; min_nnz <- min_nnz
            function(...) {
                ## tiny operands are cheaper on the host than a PCIe round trip: optional size gate on the
                ## length of the first index vector passed (0 = always use the GPU)
                args <- list(...)
                if (min_nnz > 0L) {
                    lens <- vapply(args, length, integer(1L))
                    if (max(lens) < min_nnz) return(do.call(cpu_fun, args))
                }
                do.call(.Call, c(list(native), args))
            }
        })
        formals_cpu <- formals(cpu_fun)
        unlockBinding(fn, ns)
        assign(fn, gpu_fun, envir = ns)
        lockBinding(fn, ns)
    }
    ## t_deep_internal (R/trans.R:46-56), which t(), t_deep() and the deep transposes behind it call: general
    ## d/l/n R/C classes go through the device transpose; any other class (symmetric, triangular, ...) keeps the
    ## saved CPU function.
    cpu_t <- get("t_deep_internal", envir = ns)
    .mxgpu_state$saved_t_deep <- cpu_t
    native_t <- getNativeSymbolInfo("mxgpu_csr_transpose", dll)
    gpu_t <- function(x) {
        cls <- class(x)[1L]
        if (!(cls %in% c("dgRMatrix", "lgRMatrix", "ngRMatrix", "dgCMatrix", "lgCMatrix", "ngCMatrix")))
            return(cpu_t(x))
        check_valid_matrix(x)
        csr <- inherits(x, "RsparseMatrix")
        vals <- if (startsWith(cls, "n")) NULL else x@x
        r <- .Call(native_t, x@p, if (csr) x@j else x@i, vals, if (csr) ncol(x) else nrow(x))
        out <- new(cls)
        out@Dim <- rev(x@Dim)
        out@Dimnames <- rev(x@Dimnames)
        out@p <- r$indptr
        if (csr) out@j <- r$indices else out@i <- r$indices
        if (!is.null(vals)) out@x <- r$values
        out
    }
    ## check_valid_matrix and the rest of MatrixExtra's internals resolve in its namespace
    environment(gpu_t) <- list2env(list(native_t = native_t, cpu_t = cpu_t), parent = ns)
    unlockBinding("t_deep_internal", ns)
    assign("t_deep_internal", gpu_t, envir = ns)
    lockBinding("t_deep_internal", ns)
    ## as.csr.matrix / as.csc.matrix (R/conversions.R): a general d/l/n TsparseMatrix is sorted into CSR / CSC
    ## order on the device (repeated triplets merged as Matrix merges them), then handed to the saved function,
    ## which applies the binary / logical flags and the value type to the CSR / CSC it receives.  Any other class
    ## goes to the saved CPU function unchanged.
    native_coo <- getNativeSymbolInfo("mxgpu_coo_to_csr", dll)
    .mxgpu_state$saved_conv <- list()
    for (conv in c("as.csr.matrix", "as.csc.matrix")) {
        cpu_conv <- get(conv, envir = ns)
        .mxgpu_state$saved_conv[[conv]] <- cpu_conv
        to_csr <- conv == "as.csr.matrix"
        gpu_conv <- function(x, ...) {
            cls <- class(x)[1L]
            if (!(cls %in% c("dgTMatrix", "lgTMatrix", "ngTMatrix")))
                return(cpu_conv(x, ...))
            check_valid_matrix(x)
            vals <- if (cls == "ngTMatrix") NULL else x@x
            r <- if (to_csr) .Call(native_coo, x@i, x@j, vals, nrow(x), ncol(x))
                 else .Call(native_coo, x@j, x@i, vals, ncol(x), nrow(x))
            out <- new(paste0(substr(cls, 1L, 2L), if (to_csr) "RMatrix" else "CMatrix"))
            out@Dim <- x@Dim
            out@Dimnames <- x@Dimnames
            out@p <- r$indptr
            if (to_csr) out@j <- r$indices else out@i <- r$indices
            if (!is.null(vals)) out@x <- r$values
            cpu_conv(out, ...)
        }
        environment(gpu_conv) <- list2env(list(native_coo = native_coo, cpu_conv = cpu_conv, to_csr = to_csr),
                                          parent = ns)
        unlockBinding(conv, ns)
        assign(conv, gpu_conv, envir = ns)
        lockBinding(conv, ns)
    }
    invisible(TRUE)
}

mxgpu_disable <- function() {
    ns <- asNamespace("MatrixExtra")
    if (!is.null(.mxgpu_state$saved_t_deep)) {
        unlockBinding("t_deep_internal", ns)
        assign("t_deep_internal", .mxgpu_state$saved_t_deep, envir = ns)
        lockBinding("t_deep_internal", ns)
        .mxgpu_state$saved_t_deep <- NULL
    }
    for (conv in names(.mxgpu_state$saved_conv)) {
        unlockBinding(conv, ns)
        assign(conv, .mxgpu_state$saved_conv[[conv]], envir = ns)
        lockBinding(conv, ns)
    }
    .mxgpu_state$saved_conv <- list()
    for (fn in names(.mxgpu_state$saved)) {
        unlockBinding(fn, ns)
        assign(fn, .mxgpu_state$saved[[fn]], envir = ns)
        lockBinding(fn, ns)
    }
    .mxgpu_state$saved <- list()
    invisible(TRUE)
}
