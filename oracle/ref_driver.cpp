/* C-ABI over the reference's own compiled translation units (oracle/Makefile target `ref`).
 *
 * Test infrastructure only.  The reference's functions are declared here with the signatures of its R-callable
 * entry points; arguments and results cross the boundary as handles to the stand-in's objects (refshim/Rcpp.h):
 * make a vector / matrix / list / S4 object from flat buffers, call a function by name, read type, length, data
 * and list items off the result, free.  A stop() or any other C++ exception comes back as status 1 + message. */
#include <cstdio>
#include <cstring>
#include <exception>
#include <map>
#include <string>
#include <utility>

#include "Rcpp.h"

typedef Rcpp::IntegerVector IV;
typedef Rcpp::NumericVector NV;
typedef Rcpp::LogicalVector LV;
typedef Rcpp::IntegerMatrix IM;
typedef Rcpp::NumericMatrix NM;
typedef Rcpp::LogicalMatrix LM;
typedef Rcpp::List RL;
typedef Rcpp::String RS;
typedef Rcpp::S4 S4;
typedef Rcpp::ListOf<Rcpp::S4> S4s;

/* ---- the reference's entry points (matmul, operators, slice, slice_coo, misc, cbind, rbind) ---- */
RL cbind_csr_numeric(IV, IV, NV, IV, IV, NV);
RL cbind_csr_logical(IV, IV, LV, IV, IV, LV);
RL cbind_csr_binary(IV, IV, IV, IV);
NM matmul_dense_csc_numeric(NM, IV, IV, NV, int);
IM matmul_dense_csc_float32(IM, IV, IV, NV, int);
NM tcrossprod_dense_csr_numeric(NM, IV, IV, NV, int, int);
IM tcrossprod_dense_csr_float32(IM, IV, IV, NV, int, int);
NM tcrossprod_csr_dense_numeric(IV, IV, NV, NM, int);
IM tcrossprod_csr_dense_float32(IV, IV, NV, IM, int);
NV matmul_csr_dvec_numeric(IV, IV, NV, NV, int);
NV matmul_csr_dvec_integer(IV, IV, NV, IV, int);
NV matmul_csr_dvec_logical(IV, IV, NV, LV, int);
IV matmul_csr_dvec_float32(IV, IV, NV, IV, int);
NV matmul_csr_svec_numeric(IV, IV, NV, IV, NV, int);
NV matmul_csr_svec_integer(IV, IV, NV, IV, IV, int);
NV matmul_csr_svec_logical(IV, IV, NV, IV, LV, int);
NV matmul_csr_svec_binary(IV, IV, NV, IV, int);
NV matmul_csr_svec_float32(IV, IV, NV, IV, IV, int);
IM matmul_rowvec_by_csc(IV, IV, IV, NV);
IM matmul_rowvec_by_cscbin(IV, IV, IV);
RL matmul_colvec_by_scolvecascsr_f32(IV, IV, IV, NV);
RL matmul_colvec_by_scolvecascsr(NV, IV, IV, NV);
RL matmul_spcolvec_by_scolvecascsr_numeric(IV, IV, NV, IV, NV, int);
RL matmul_spcolvec_by_scolvecascsr_integer(IV, IV, NV, IV, IV, int);
RL matmul_spcolvec_by_scolvecascsr_logical(IV, IV, NV, IV, LV, int);
RL matmul_spcolvec_by_scolvecascsr_binary(IV, IV, NV, IV, int);
bool contains_any_zero(NV);
bool contains_any_inf(NV);
bool contains_any_neg(NV);
int find_first_non_na(IV);
bool is_same_ngRMatrix(IV, IV, IV, IV);
bool check_is_sorted(IV);
bool check_indices_are_unsorted(IV, NV);
void sort_sparse_indices_numeric(IV, IV, NV);
void sort_sparse_indices_logical(IV, IV, LV);
void sort_sparse_indices_numeric_known_ncol(IV, IV, NV, int);
void sort_sparse_indices_logical_known_ncol(IV, IV, LV, int);
void sort_sparse_indices_binary(IV, IV);
void sort_coo_indices_numeric(IV, IV, NV);
void sort_coo_indices_logical(IV, IV, LV);
void sort_coo_indices_binary(IV, IV);
void sort_vector_indices_numeric(IV, NV);
void sort_vector_indices_integer(IV, IV);
void sort_vector_indices_logical(IV, LV);
void sort_vector_indices_binary(IV);
NV deepcopy_num(NV);
IV deepcopy_int(IV);
LV deepcopy_log(LV);
RS deepcopy_str(RS);
RL remove_zero_valued_csr_numeric(IV, IV, NV, bool);
RL remove_zero_valued_csr_logical(IV, IV, LV, bool);
RL remove_zero_valued_coo_numeric(IV, IV, NV, bool);
RL remove_zero_valued_coo_logical(IV, IV, LV, bool);
RL remove_zero_valued_svec_numeric(IV, NV, bool);
RL remove_zero_valued_svec_integer(IV, IV, bool);
RL remove_zero_valued_svec_logical(IV, LV, bool);
RL check_valid_csr_matrix(IV, IV, int, int);
RL check_valid_coo_matrix(IV, IV, int, int);
RL check_valid_svec(IV, int);
IV rebuild_indptr_after_filter(IV, LV);
RL multiply_csr_elemwise(IV, IV, IV, IV, NV, NV);
RL logicaland_csr_elemwise(IV, IV, IV, IV, LV, LV);
NV multiply_csr_by_dense_elemwise_double(IV, IV, NV, NV);
NV multiply_csr_by_dense_elemwise_float32(IV, IV, NV, IV);
NV multiply_csr_by_dense_elemwise_int(IV, IV, NV, IV);
NV multiply_csr_by_dense_elemwise_bool(IV, IV, NV, LV);
LV logicaland_csr_by_dense_cpp(IV, IV, LV, LV);
RL add_csr_elemwise(IV, IV, IV, IV, NV, NV, bool);
RL logicalor_csr_elemwise(IV, IV, IV, IV, LV, LV, bool);
RL multiply_csr_by_coo_elemwise(IV, IV, NV, IV, IV, NV, int, int);
RL logicaland_csr_by_coo_elemwise(IV, IV, LV, IV, IV, LV, int, int);
RL multiply_coo_by_dense_numeric(NM, IV, IV, NV);
RL multiply_coo_by_dense_integer(IM, IV, IV, NV);
RL multiply_coo_by_dense_logical(LM, IV, IV, NV);
RL multiply_coo_by_dense_float32(IM, IV, IV, NV);
RL logicaland_coo_by_dense_logical(LM, IV, IV, LV);
RL add_NAs_from_dense_after_elemenwise_mult_numeric(IV, IV, NM);
RL add_NAs_from_dense_after_elemenwise_mult_integer(IV, IV, IM);
RL add_NAs_from_dense_after_elemenwise_mult_float32(IV, IV, IM);
RL add_NAs_from_dense_after_elemenwise_mult_logical(IV, IV, LM);
NV multiply_csc_by_dense_ignore_NAs_numeric(IV, IV, NV, NM);
NV multiply_csc_by_dense_ignore_NAs_float32(IV, IV, NV, IM);
NV multiply_csc_by_dense_ignore_NAs_integer(IV, IV, NV, IM);
NV multiply_csc_by_dense_ignore_NAs_logical(IV, IV, NV, LM);
LV logicaland_csc_by_dense_ignore_NAs(IV, IV, LV, LM);
RL multiply_csc_by_dense_keep_NAs_numeric(IV, IV, NV, NM);
RL multiply_csc_by_dense_keep_NAs_integer(IV, IV, NV, IM);
RL multiply_csc_by_dense_keep_NAs_logical(IV, IV, NV, LM);
RL multiply_csc_by_dense_keep_NAs_float32(IV, IV, NV, IM);
RL logicaland_csc_by_dense_keep_NAs(IV, IV, LV, LM);
NV multiply_csr_by_dvec_no_NAs_numeric(IV, IV, NV, NV, int, bool, bool, bool, bool, bool, bool);
LV logicaland_csr_by_dvec_internal(IV, IV, LV, LV, int);
RL multiply_csr_by_dvec_with_NAs(IV, IV, NV, NV, int, bool, bool, bool, bool, bool, bool);
NV multiply_coo_by_dense_ignore_NAs_numeric(IV, IV, NV, NV, int, int, bool, bool, bool, bool, bool, bool);
LV multiply_coo_by_dense_ignore_NAs_logical(IV, IV, LV, LV, int, int);
RL multiply_csr_by_svec_no_NAs(IV, IV, NV, IV, NV, int);
RL multiply_csr_by_svec_keep_NAs(IV, IV, NV, IV, NV, int, int);
RL multiply_elemwise_dense_by_svec_numeric(NM, IV, NV, int, int);
RL multiply_elemwise_dense_by_svec_integer(IM, IV, NV, int, int);
RL multiply_elemwise_dense_by_svec_logical(LM, IV, NV, int, int);
RL multiply_elemwise_dense_by_svec_float32(IM, IV, NV, int, int);
IV concat_indptr2(IV, IV);
S4 concat_csr_batch(S4s, S4);
bool check_is_seq(IV);
bool check_is_rev_seq(IV);
RL reverse_rows_numeric(IV, IV, NV);
RL reverse_rows_logical(IV, IV, LV);
RL reverse_rows_binary(IV, IV);
void reverse_columns_inplace_numeric(IV, IV, NV, int);
void reverse_columns_inplace_logical(IV, IV, LV, int);
void reverse_columns_inplace_binary(IV, IV, NV, int);
RL copy_csr_rows_numeric(IV, IV, NV, IV);
RL copy_csr_rows_logical(IV, IV, LV, IV);
RL copy_csr_rows_binary(IV, IV, IV);
RL copy_csr_rows_col_seq_numeric(IV, IV, NV, IV, IV, bool);
RL copy_csr_rows_col_seq_logical(IV, IV, LV, IV, IV, bool);
RL copy_csr_rows_col_seq_binary(IV, IV, IV, IV, bool);
RL copy_csr_arbitrary_numeric(IV, IV, NV, IV, IV);
RL copy_csr_arbitrary_logical(IV, IV, LV, IV, IV);
RL copy_csr_arbitrary_binary(IV, IV, IV, IV);
IV repeat_indices_n_times(IV, IV, int, int);
double extract_single_val_csr_numeric(IV, IV, NV, int, int);
int extract_single_val_csr_logical(IV, IV, LV, int, int);
double extract_single_val_csr_binary(IV, IV, int, int);
double slice_coo_single_numeric(IV, IV, NV, int, int);
bool slice_coo_single_logical(IV, IV, LV, int, int);
bool slice_coo_single_binary(IV, IV, int, int);
RL slice_coo_arbitrary_numeric(IV, IV, NV, IV, IV, bool, bool, bool, bool, bool, bool, int, int);
RL slice_coo_arbitrary_logical(IV, IV, LV, IV, IV, bool, bool, bool, bool, bool, bool, int, int);
RL slice_coo_arbitrary_binary(IV, IV, IV, IV, bool, bool, bool, bool, bool, bool, int, int);
RL inject_NAs_inplace_coo_numeric(IV, IV, NV, IV, IV, int, int);
RL inject_NAs_inplace_coo_logical(IV, IV, LV, IV, IV, int, int);

namespace {

/* one letter per parameter / result type, so the Python side can cast its arguments without a second table */
template <class T> struct Kind;
template <> struct Kind<IV> { static const char c = 'I'; };
template <> struct Kind<NV> { static const char c = 'N'; };
template <> struct Kind<LV> { static const char c = 'L'; };
template <> struct Kind<IM> { static const char c = 'J'; };
template <> struct Kind<NM> { static const char c = 'M'; };
template <> struct Kind<LM> { static const char c = 'K'; };
template <> struct Kind<RL> { static const char c = 'R'; };
template <> struct Kind<RS> { static const char c = 'S'; };
template <> struct Kind<S4> { static const char c = '4'; };
template <> struct Kind<S4s> { static const char c = 'O'; };
template <> struct Kind<int> { static const char c = 'i'; };
template <> struct Kind<double> { static const char c = 'd'; };
template <> struct Kind<bool> { static const char c = 'b'; };
template <> struct Kind<void> { static const char c = 'v'; };

struct Entry {
    std::string signature;  /* result kind, then one kind per parameter */
    SEXP (*call)(void *fn, SEXP *args);
    void *fn;
};

template <class R, class... A> struct Invoke {
    template <size_t... I> static SEXP run(R (*f)(A...), SEXP *args, std::index_sequence<I...>)
    {
        return Rcpp::wrap(f(Rcpp::as<A>(args[I])...));
    }
    static SEXP call(void *fn, SEXP *args)
    {
        return run(reinterpret_cast<R (*)(A...)>(fn), args, std::index_sequence_for<A...>());
    }
};
template <class... A> struct Invoke<void, A...> {
    template <size_t... I> static SEXP run(void (*f)(A...), SEXP *args, std::index_sequence<I...>)
    {
        f(Rcpp::as<A>(args[I])...);
        return nullptr;
    }
    static SEXP call(void *fn, SEXP *args)
    {
        return run(reinterpret_cast<void (*)(A...)>(fn), args, std::index_sequence_for<A...>());
    }
};

template <class R, class... A> Entry entry(R (*f)(A...))
{
    const char sig[] = {Kind<R>::c, Kind<A>::c..., '\0'};
    return Entry{sig, &Invoke<R, A...>::call, reinterpret_cast<void *>(f)};
}

#define REG(name) {#name, entry(&name)}

const std::map<std::string, Entry> &table()
{
    static const std::map<std::string, Entry> t = {
    REG(cbind_csr_numeric),
    REG(cbind_csr_logical),
    REG(cbind_csr_binary),
    REG(matmul_dense_csc_numeric),
    REG(matmul_dense_csc_float32),
    REG(tcrossprod_dense_csr_numeric),
    REG(tcrossprod_dense_csr_float32),
    REG(tcrossprod_csr_dense_numeric),
    REG(tcrossprod_csr_dense_float32),
    REG(matmul_csr_dvec_numeric),
    REG(matmul_csr_dvec_integer),
    REG(matmul_csr_dvec_logical),
    REG(matmul_csr_dvec_float32),
    REG(matmul_csr_svec_numeric),
    REG(matmul_csr_svec_integer),
    REG(matmul_csr_svec_logical),
    REG(matmul_csr_svec_binary),
    REG(matmul_csr_svec_float32),
    REG(matmul_rowvec_by_csc),
    REG(matmul_rowvec_by_cscbin),
    REG(matmul_colvec_by_scolvecascsr_f32),
    REG(matmul_colvec_by_scolvecascsr),
    REG(matmul_spcolvec_by_scolvecascsr_numeric),
    REG(matmul_spcolvec_by_scolvecascsr_integer),
    REG(matmul_spcolvec_by_scolvecascsr_logical),
    REG(matmul_spcolvec_by_scolvecascsr_binary),
    REG(contains_any_zero),
    REG(contains_any_inf),
    REG(contains_any_neg),
    REG(find_first_non_na),
    REG(is_same_ngRMatrix),
    {"check_is_sorted", entry(static_cast<bool (*)(IV)>(&check_is_sorted))},
    REG(check_indices_are_unsorted),
    REG(sort_sparse_indices_numeric),
    REG(sort_sparse_indices_logical),
    REG(sort_sparse_indices_numeric_known_ncol),
    REG(sort_sparse_indices_logical_known_ncol),
    REG(sort_sparse_indices_binary),
    REG(sort_coo_indices_numeric),
    REG(sort_coo_indices_logical),
    REG(sort_coo_indices_binary),
    REG(sort_vector_indices_numeric),
    REG(sort_vector_indices_integer),
    REG(sort_vector_indices_logical),
    REG(sort_vector_indices_binary),
    REG(deepcopy_num),
    REG(deepcopy_int),
    REG(deepcopy_log),
    REG(deepcopy_str),
    REG(remove_zero_valued_csr_numeric),
    REG(remove_zero_valued_csr_logical),
    REG(remove_zero_valued_coo_numeric),
    REG(remove_zero_valued_coo_logical),
    REG(remove_zero_valued_svec_numeric),
    REG(remove_zero_valued_svec_integer),
    REG(remove_zero_valued_svec_logical),
    REG(check_valid_csr_matrix),
    REG(check_valid_coo_matrix),
    REG(check_valid_svec),
    REG(rebuild_indptr_after_filter),
    REG(multiply_csr_elemwise),
    REG(logicaland_csr_elemwise),
    REG(multiply_csr_by_dense_elemwise_double),
    REG(multiply_csr_by_dense_elemwise_float32),
    REG(multiply_csr_by_dense_elemwise_int),
    REG(multiply_csr_by_dense_elemwise_bool),
    REG(logicaland_csr_by_dense_cpp),
    REG(add_csr_elemwise),
    REG(logicalor_csr_elemwise),
    REG(multiply_csr_by_coo_elemwise),
    REG(logicaland_csr_by_coo_elemwise),
    REG(multiply_coo_by_dense_numeric),
    REG(multiply_coo_by_dense_integer),
    REG(multiply_coo_by_dense_logical),
    REG(multiply_coo_by_dense_float32),
    REG(logicaland_coo_by_dense_logical),
    REG(add_NAs_from_dense_after_elemenwise_mult_numeric),
    REG(add_NAs_from_dense_after_elemenwise_mult_integer),
    REG(add_NAs_from_dense_after_elemenwise_mult_float32),
    REG(add_NAs_from_dense_after_elemenwise_mult_logical),
    REG(multiply_csc_by_dense_ignore_NAs_numeric),
    REG(multiply_csc_by_dense_ignore_NAs_float32),
    REG(multiply_csc_by_dense_ignore_NAs_integer),
    REG(multiply_csc_by_dense_ignore_NAs_logical),
    REG(logicaland_csc_by_dense_ignore_NAs),
    REG(multiply_csc_by_dense_keep_NAs_numeric),
    REG(multiply_csc_by_dense_keep_NAs_integer),
    REG(multiply_csc_by_dense_keep_NAs_logical),
    REG(multiply_csc_by_dense_keep_NAs_float32),
    REG(logicaland_csc_by_dense_keep_NAs),
    REG(multiply_csr_by_dvec_no_NAs_numeric),
    REG(logicaland_csr_by_dvec_internal),
    REG(multiply_csr_by_dvec_with_NAs),
    REG(multiply_coo_by_dense_ignore_NAs_numeric),
    REG(multiply_coo_by_dense_ignore_NAs_logical),
    REG(multiply_csr_by_svec_no_NAs),
    REG(multiply_csr_by_svec_keep_NAs),
    REG(multiply_elemwise_dense_by_svec_numeric),
    REG(multiply_elemwise_dense_by_svec_integer),
    REG(multiply_elemwise_dense_by_svec_logical),
    REG(multiply_elemwise_dense_by_svec_float32),
    REG(concat_indptr2),
    REG(concat_csr_batch),
    REG(check_is_seq),
    REG(check_is_rev_seq),
    REG(reverse_rows_numeric),
    REG(reverse_rows_logical),
    REG(reverse_rows_binary),
    REG(reverse_columns_inplace_numeric),
    REG(reverse_columns_inplace_logical),
    REG(reverse_columns_inplace_binary),
    REG(copy_csr_rows_numeric),
    REG(copy_csr_rows_logical),
    REG(copy_csr_rows_binary),
    REG(copy_csr_rows_col_seq_numeric),
    REG(copy_csr_rows_col_seq_logical),
    REG(copy_csr_rows_col_seq_binary),
    REG(copy_csr_arbitrary_numeric),
    REG(copy_csr_arbitrary_logical),
    REG(copy_csr_arbitrary_binary),
    REG(repeat_indices_n_times),
    REG(extract_single_val_csr_numeric),
    REG(extract_single_val_csr_logical),
    REG(extract_single_val_csr_binary),
    REG(slice_coo_single_numeric),
    REG(slice_coo_single_logical),
    REG(slice_coo_single_binary),
    REG(slice_coo_arbitrary_numeric),
    REG(slice_coo_arbitrary_logical),
    REG(slice_coo_arbitrary_binary),
    REG(inject_NAs_inplace_coo_numeric),
    REG(inject_NAs_inplace_coo_logical),
    };
    return t;
}

void put_error(char *buf, int len, const char *msg)
{
    if (buf && len > 0) std::snprintf(buf, (size_t)len, "%s", msg);
}

}  // namespace

extern "C" {

/* objects handed to Python carry one reference of their own; mxref_free drops it */
static void *hand_out(SEXP s)
{
    mxref::retain(s);
    return s;
}

void *mxref_vector(int type, const void *data, long n)
{
    try {
        SEXP s = mxref::alloc(type, (R_xlen_t)n);
        if (n > 0) std::memcpy(s->data, data, (size_t)n * (type == REALSXP ? sizeof(double) : sizeof(int)));
        return hand_out(s);
    } catch (...) {
        return nullptr;
    }
}

void *mxref_matrix(int type, const void *data, int nrow, int ncol)
{
    void *h = mxref_vector(type, data, (long)nrow * (long)ncol);
    if (h) {
        ((SEXP)h)->nrow = nrow;
        ((SEXP)h)->ncol = ncol;
    }
    return h;
}

void *mxref_string(const char *c)
{
    SEXP s = mxref::alloc(STRSXP, 1);
    s->str = c;
    return hand_out(s);
}

/* a list (type VECSXP) or an S4 object (type S4SXP, classes separated by spaces, most derived first) */
void *mxref_container(int type, const char *classes)
{
    SEXP s = mxref::alloc(type, 0);
    if (classes) {
        std::string all(classes);
        size_t pos = 0;
        while (pos < all.size()) {
            size_t sp = all.find(' ', pos);
            if (sp == std::string::npos) sp = all.size();
            if (sp > pos) s->classes.push_back(all.substr(pos, sp - pos));
            pos = sp + 1;
        }
    }
    return hand_out(s);
}

void mxref_container_add(void *container, const char *name, void *item)
{
    SEXP s = (SEXP)container;
    mxref::retain((SEXP)item);
    s->names.push_back(name ? name : "");
    s->items.push_back((SEXP)item);
    s->length = (R_xlen_t)s->items.size();
}

int mxref_type(void *h) { return h ? ((SEXP)h)->type : NILSXP; }
long mxref_length(void *h) { return (long)Rf_xlength((SEXP)h); }
void *mxref_data(void *h) { return ((SEXP)h)->data; }
int mxref_nrow(void *h) { return ((SEXP)h)->nrow; }
int mxref_ncol(void *h) { return ((SEXP)h)->ncol; }
const char *mxref_chars(void *h) { return ((SEXP)h)->str.c_str(); }
const char *mxref_item_name(void *h, long i) { return ((SEXP)h)->names.at((size_t)i).c_str(); }
void *mxref_item(void *h, long i) { return hand_out(((SEXP)h)->items.at((size_t)i)); }

void mxref_free(void *h)
{
    mxref::release((SEXP)h);
    mxref::collect();
}

long mxref_live_objects(void) { return mxref::live_objects(); }

const char *mxref_signature(const char *name)
{
    auto it = table().find(name);
    return it == table().end() ? nullptr : it->second.signature.c_str();
}

long mxref_function_count(void) { return (long)table().size(); }
const char *mxref_function_name(long i)
{
    auto it = table().begin();
    std::advance(it, i);
    return it->first.c_str();
}

/* status 0: *result holds the value (NULL for a void function); 1: a C++ exception, message in errbuf;
 * 2: unknown function or wrong argument count */
int mxref_call(const char *name, void **args, int nargs, void **result, char *errbuf, int errlen)
{
    *result = nullptr;
    auto it = table().find(name);
    if (it == table().end() || (int)it->second.signature.size() - 1 != nargs) {
        put_error(errbuf, errlen, "unknown function or wrong number of arguments");
        return 2;
    }
    int status = 0;
    try {
        SEXP out = it->second.call(it->second.fn, reinterpret_cast<SEXP *>(args));
        if (out) *result = hand_out(out);
    } catch (const std::exception &e) {
        put_error(errbuf, errlen, e.what());
        status = 1;
    } catch (...) {
        put_error(errbuf, errlen, "unknown C++ exception");
        status = 1;
    }
    mxref::collect();
    return status;
}

}  /* extern "C" */
