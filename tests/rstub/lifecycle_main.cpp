// lifecycle_main.cpp: the .Call shim's handle lifecycle as a stand-alone host program, for a sanitizer build
// (`make -C matrixextra_amd/csrc rshim-sanitize`: -fsanitize=address,undefined).  Linked statically with
// r_shim.cpp, the R stand-in (rstub.cpp) and the generated fake of the C-ABI; it neither links nor loads libmxgpu or
// HIP and needs no GPU.  It drives add_csr_elemwise (finish_guarded), remove_zero_valued_svec_integer (integer values,
// a two-element list cut from the three) and copy_csr_arbitrary_binary (the re-wrapped two-element list) through the
// fake's three modes, plain and under the gctorture-like mode, then makes every allocation of the successful call fail
// in turn, and exits non-zero on any ledger or stand-in violation.
#include <R.h>
#include <Rinternals.h>
#include <R_ext/Rdynload.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
SEXP rstub_new(int type, long n);
void *rstub_data(SEXP s);
long rstub_len(SEXP s);
int rstub_type(SEXP s);
SEXP rstub_elt(SEXP s, long i);
const char *rstub_names(SEXP s, long i);
int rstub_call(void *fn, int nargs, SEXP *args, SEXP *out);
const char *rstub_error_message(void);
int rstub_protect_depth(void);
int rstub_precious_count(void);
int rstub_violations(char *buf, int n);
void rstub_torture(int on);
void rstub_fail_allocation(int nth);
int rstub_allocations(void);
void rstub_reset(void);
int rstub_registered(int i, const char **name, void **fn, int *nargs);
void R_init_mxgpu_r(DllInfo *dll);

void fake_set_mode(int mode);
void fake_set_canned(int64_t indptr_len, int64_t nnz, int64_t values_len, int values_dtype, int alias);
long fake_begun(void);
long fake_finished(void);
long fake_discarded(void);
long fake_double_released(void);
long fake_unknown_released(void);
long fake_open(void);
void fake_reset(void);
}

namespace {

int g_failures = 0;

void expect(bool ok, const char *what, const char *routine, int mode, int torture)
{
    if (ok) return;
    ++g_failures;
    fprintf(stderr, "FAIL %s (mode %d, torture %d): %s\n", routine, mode, torture, what);
}

SEXP ints(int type, std::vector<int> v)
{
    SEXP s = rstub_new(type, (long)v.size());
    if (!v.empty()) memcpy(rstub_data(s), v.data(), v.size() * sizeof(int));
    return s;
}
SEXP reals(std::vector<double> v)
{
    SEXP s = rstub_new(REALSXP, (long)v.size());
    if (!v.empty()) memcpy(rstub_data(s), v.data(), v.size() * sizeof(double));
    return s;
}

void *routine(const char *name)
{
    const char *nm;
    void *fn;
    int n;
    for (int i = 0; rstub_registered(i, &nm, &fn, &n); ++i)
        if (!strcmp(nm, name)) return fn;
    return nullptr;
}

// values_dtype of include/mxgpu.h: MX_F64 0, MX_I32 2, MX_NONE 4
struct Drive { const char *name; int values_dtype; int64_t first, nnz, nvalues; int nlist; };

// returns the number of allocations the call made
int drive(const Drive &d, int mode, int torture, int fail_allocation = 0)
{
    rstub_reset();
    fake_reset();
    fake_set_mode(mode);
    fake_set_canned(d.first, d.nnz, d.nvalues, d.values_dtype, 0);
    std::vector<SEXP> args;
    if (!strcmp(d.name, "_MatrixExtra_add_csr_elemwise"))
        args = {ints(INTSXP, {0, 1, 2}), ints(INTSXP, {0, 1, 2}), ints(INTSXP, {0, 1}), ints(INTSXP, {1, 0}),
                reals({1.0, 2.0}), reals({3.0, 4.0}), ints(LGLSXP, {0})};
    else if (!strcmp(d.name, "_MatrixExtra_remove_zero_valued_svec_integer"))
        args = {ints(INTSXP, {1, 4, 6}), ints(INTSXP, {5, 0, INT32_MIN}), ints(LGLSXP, {0})};
    else
        args = {ints(INTSXP, {0, 1, 2}), ints(INTSXP, {0, 1}), ints(INTSXP, {1, 0}), ints(INTSXP, {1})};
    void *fn = routine(d.name);
    expect(fn != nullptr, "registered", d.name, mode, torture);
    if (!fn) return 0;
    rstub_torture(torture);
    rstub_fail_allocation(fail_allocation);
    SEXP out = nullptr;
    const int status = rstub_call(fn, (int)args.size(), args.data(), &out);
    rstub_torture(0);
    char log[4096];
    const int nviol = rstub_violations(log, sizeof log);
    if (nviol) fprintf(stderr, "%s", log);
    expect(nviol == 0, "no stand-in violation", d.name, mode, torture);
    expect(rstub_protect_depth() == 0, "protect stack back at its depth", d.name, mode, torture);
    expect(rstub_precious_count() == 0, "precious list empty", d.name, mode, torture);
    expect(fake_open() == 0, "no handle left open", d.name, mode, torture);
    expect(fake_double_released() == 0, "no handle released twice", d.name, mode, torture);
    expect(fake_unknown_released() == 0, "no unknown handle released", d.name, mode, torture);
    if (fail_allocation) {
        expect(status == 1 && strstr(rstub_error_message(), "cannot allocate") != nullptr,
               "the call ends in R's allocation error", d.name, mode, torture);
    } else if (mode == 1) {
        expect(status == 0 && out, "the call succeeds", d.name, mode, torture);
        expect(fake_begun() == 1 && fake_finished() == 1, "one handle begun and finished", d.name, mode, torture);
        if (status == 0 && out) {
            expect(rstub_type(out) == VECSXP && rstub_len(out) == d.nlist, "list length", d.name, mode, torture);
            expect(rstub_names(out, 0) != nullptr, "names attribute", d.name, mode, torture);
            expect(rstub_len(rstub_elt(out, d.nlist - 1)) == (d.nlist == 2 && d.values_dtype == 4 ? d.nnz : d.nvalues),
                   "canned length of the last element", d.name, mode, torture);
        }
    } else {
        expect(status == 1, "the call ends in Rf_error", d.name, mode, torture);
        expect(strstr(rstub_error_message(), "fake libmxgpu") != nullptr, "the library's message", d.name, mode, torture);
        if (mode == 2)
            expect(fake_begun() == 1 && fake_finished() == 1 && fake_discarded() == 0,
                   "the handle finish consumed is not discarded again", d.name, mode, torture);
    }
    return rstub_allocations();
}

}  // namespace

int main()
{
    R_init_mxgpu_r(nullptr);
    const Drive drives[] = {
        {"_MatrixExtra_add_csr_elemwise", 0, 3, 2, 2, 3},
        {"_MatrixExtra_remove_zero_valued_svec_integer", 2, 0, 2, 2, 2},
        {"_MatrixExtra_copy_csr_arbitrary_binary", 4, 2, 3, 0, 2},
    };
    int runs = 0;
    for (const Drive &d : drives)
        for (int mode = 0; mode < 3; ++mode)
            for (int torture = 0; torture < 2; ++torture, ++runs) drive(d, mode, torture);
    for (const Drive &d : drives) {
        const int allocations = drive(d, 1, 0);
        for (int nth = 1; nth <= allocations; ++nth)
            for (int torture = 0; torture < 2; ++torture, ++runs) drive(d, 1, torture, nth);
    }
    rstub_reset();
    printf("rshim lifecycle: %d runs, %d failure(s)\n", runs, g_failures);
    return g_failures ? 1 : 0;
}
