/* Stand-in for <Rcpp.h>: only what the reference's hot files use, written from Rcpp's documented behaviour.
 * Test infrastructure only (oracle/Makefile target `ref`); never part of the product.
 *
 *  - SEXP points to a tagged, reference-counted object: logical / integer / real vector (optionally with a
 *    two-element dim), list with names, string, S4 object with class names and slots.
 *  - Vector<T> / Matrix<T> are handles: a copy shares the buffer, as in Rcpp.  Matrices are column-major.
 *  - An object whose count drops to zero is parked and freed by mxref::collect() at the end of a driver call, so
 *    a bare SEXP returned from a function stays valid until a handle picks it up (R's GC gives the same grace). */
#ifndef MXREF_SHIM_RCPP_H
#define MXREF_SHIM_RCPP_H

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <algorithm>
#include <iostream>
#include <iterator>
#include <limits>
#include <memory>
#include <mutex>
#include <numeric>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "R.h"
#include "Rinternals.h"
#include "R_ext/RS.h"
#include "R_ext/BLAS.h"

struct SEXPREC {
    int type = NILSXP;
    long refs = 0;
    bool parked = false;
    R_xlen_t length = 0;
    void *data = nullptr;            /* int[] or double[] for LGLSXP / INTSXP / REALSXP */
    int nrow = -1, ncol = -1;        /* dim attribute, -1 when absent */
    std::vector<SEXP> items;         /* list elements or S4 slots */
    std::vector<std::string> names;  /* their names */
    std::vector<std::string> classes;/* S4: class and its superclasses */
    std::string str;                 /* STRSXP of length one */
};

namespace mxref {

struct Heap {
    std::mutex lock;
    std::vector<SEXP> parked;
    long live = 0;
};
Heap &heap();

inline SEXP alloc(int type, R_xlen_t n)
{
    SEXP s = new SEXPREC;
    s->type = type;
    s->length = n;
    if (type == LGLSXP || type == INTSXP)
        s->data = std::calloc((size_t)(n > 0 ? n : 1), sizeof(int));
    else if (type == REALSXP)
        s->data = std::calloc((size_t)(n > 0 ? n : 1), sizeof(double));
    if ((type == LGLSXP || type == INTSXP || type == REALSXP) && !s->data) {
        delete s;
        throw std::bad_alloc();
    }
    Heap &h = heap();
    std::lock_guard<std::mutex> g(h.lock);
    h.live++;
    s->parked = true;                /* born unowned */
    h.parked.push_back(s);
    return s;
}

inline void retain(SEXP s)
{
    if (!s) return;
    std::lock_guard<std::mutex> g(heap().lock);
    s->refs++;
}

inline void release(SEXP s)
{
    if (!s) return;
    Heap &h = heap();
    std::lock_guard<std::mutex> g(h.lock);
    if (--s->refs <= 0 && !s->parked) {
        s->parked = true;
        h.parked.push_back(s);
    }
}

void collect();  /* frees every parked object that nobody holds */
long live_objects();

inline SEXP checked(SEXP s, int type, const char *what)
{
    if (!s || s->type != type) throw std::runtime_error(std::string("expected ") + what);
    return s;
}

}  // namespace mxref

namespace Rcpp {

class exception : public std::runtime_error {
public:
    explicit exception(const std::string &m) : std::runtime_error(m) {}
};

[[noreturn]] inline void stop(const std::string &msg) { throw exception(msg); }
[[noreturn]] inline void stop(const char *msg) { throw exception(msg); }
inline void checkUserInterrupt() {}

/* owning handle over a SEXP */
class RObject {
protected:
    SEXP s_ = nullptr;
    void set(SEXP x)
    {
        mxref::retain(x);
        mxref::release(s_);
        s_ = x;
    }
public:
    RObject() {}
    RObject(SEXP x) { set(x); }
    RObject(const RObject &o) { set(o.s_); }
    RObject &operator=(const RObject &o) { set(o.s_); return *this; }
    ~RObject() { mxref::release(s_); }
    operator SEXP() const { return s_; }
    SEXP get__() const { return s_; }
};

template <int RTYPE> struct storage { typedef int type; };
template <> struct storage<REALSXP> { typedef double type; };

template <int RTYPE>
class Vector : public RObject {
public:
    typedef typename storage<RTYPE>::type stored_type;
    typedef stored_type *iterator;
    typedef const stored_type *const_iterator;
    typedef stored_type value_type;

    Vector() { set(mxref::alloc(RTYPE, 0)); }
    Vector(SEXP x) { adopt(x); }
    Vector(const Vector &o) : RObject(o) {}
    Vector &operator=(const Vector &o) { set(o.s_); return *this; }
    Vector &operator=(SEXP x) { adopt(x); return *this; }

    template <class N, typename std::enable_if<std::is_arithmetic<N>::value, int>::type = 0>
    Vector(const N &n) { set(mxref::alloc(RTYPE, (R_xlen_t)n)); }

    template <class N, class U,
              typename std::enable_if<std::is_arithmetic<N>::value && std::is_arithmetic<U>::value, int>::type = 0>
    Vector(const N &n, const U &fill)
    {
        set(mxref::alloc(RTYPE, (R_xlen_t)n));
        for (R_xlen_t i = 0; i < (R_xlen_t)n; i++) begin()[i] = (stored_type)fill;
    }

    template <class It, typename std::enable_if<!std::is_arithmetic<It>::value, int>::type = 0>
    Vector(It first, It last)
    {
        R_xlen_t n = (R_xlen_t)(last - first);
        set(mxref::alloc(RTYPE, n));
        stored_type *p = begin();
        for (R_xlen_t i = 0; i < n; i++, ++first) p[i] = (stored_type)*first;
    }

    R_xlen_t size() const { return s_->length; }
    R_xlen_t length() const { return s_->length; }
    iterator begin() { return (stored_type *)s_->data; }
    iterator end() { return begin() + s_->length; }
    const_iterator begin() const { return (const stored_type *)s_->data; }
    const_iterator end() const { return begin() + s_->length; }
    template <class I> stored_type &operator[](I i) { return ((stored_type *)s_->data)[i]; }
    template <class I> const stored_type &operator[](I i) const { return ((const stored_type *)s_->data)[i]; }
    template <class I> stored_type &operator()(I i) { return ((stored_type *)s_->data)[i]; }
    void fill(stored_type v) { for (R_xlen_t i = 0; i < s_->length; i++) begin()[i] = v; }

protected:
    void adopt(SEXP x)
    {
        if (!x) throw std::runtime_error("NULL where a vector was expected");
        if (x->type == RTYPE) { set(x); return; }
        /* as(): logical <-> integer share a representation, integer -> real converts NA; each makes a copy */
        if ((RTYPE == LGLSXP && x->type == INTSXP) || (RTYPE == INTSXP && x->type == LGLSXP)) {
            SEXP c = mxref::alloc(RTYPE, x->length);
            std::memcpy(c->data, x->data, sizeof(int) * (size_t)x->length);
            c->nrow = x->nrow; c->ncol = x->ncol;
            set(c);
            return;
        }
        if (RTYPE == INTSXP && x->type == REALSXP) {        /* as.integer(): toward zero, NaN and overflow are NA */
            SEXP c = mxref::alloc(RTYPE, x->length);
            const double *from = (const double *)x->data;
            for (R_xlen_t i = 0; i < x->length; i++)
                ((int *)c->data)[i] = (from[i] != from[i] || from[i] >= 2147483648.0 || from[i] <= -2147483649.0)
                                          ? NA_INTEGER : (int)from[i];
            set(c);
            return;
        }
        if (RTYPE == REALSXP && (x->type == INTSXP || x->type == LGLSXP)) {
            SEXP c = mxref::alloc(RTYPE, x->length);
            const int *from = (const int *)x->data;
            for (R_xlen_t i = 0; i < x->length; i++)
                ((double *)c->data)[i] = (from[i] == NA_INTEGER) ? NA_REAL : (double)from[i];
            set(c);
            return;
        }
        throw std::runtime_error("vector of another type where Rcpp would coerce");
    }
};

typedef Vector<INTSXP> IntegerVector;
typedef Vector<REALSXP> NumericVector;
typedef Vector<LGLSXP> LogicalVector;

template <int RTYPE>
class Matrix : public Vector<RTYPE> {
    typedef Vector<RTYPE> V;
public:
    typedef typename V::stored_type stored_type;
    Matrix() : V() { this->s_->nrow = 0; this->s_->ncol = 0; }
    Matrix(SEXP x) : V(x)
    {
        if (this->s_->nrow < 0) throw std::runtime_error("not a matrix");
    }
    Matrix(const Matrix &o) : V(o) {}
    Matrix &operator=(const Matrix &o) { V::operator=(o); return *this; }
    template <class N, class M,
              typename std::enable_if<std::is_arithmetic<N>::value && std::is_arithmetic<M>::value, int>::type = 0>
    Matrix(const N &nrow, const M &ncol) : V((size_t)nrow * (size_t)ncol)
    {
        this->s_->nrow = (int)nrow;
        this->s_->ncol = (int)ncol;
    }
    int nrow() const { return this->s_->nrow; }
    int ncol() const { return this->s_->ncol; }
    int rows() const { return this->s_->nrow; }
    int cols() const { return this->s_->ncol; }
    template <class I, class J> stored_type &operator()(I i, J j)
    {
        return ((stored_type *)this->s_->data)[(size_t)i + (size_t)j * (size_t)this->s_->nrow];
    }
};

typedef Matrix<INTSXP> IntegerMatrix;
typedef Matrix<REALSXP> NumericMatrix;
typedef Matrix<LGLSXP> LogicalMatrix;

class String {
    std::string v_;
public:
    String() {}
    String(const char *c) : v_(c) {}
    String(const std::string &c) : v_(c) {}
    String(SEXP x) : v_(mxref::checked(x, STRSXP, "a string")->str) {}
    const char *get_cstring() const { return v_.c_str(); }
    operator std::string() const { return v_; }
    bool operator==(const String &o) const { return v_ == o.v_; }
};

/* wrap(): C++ value -> SEXP */
inline SEXP wrap(SEXP x) { return x; }
inline SEXP wrap(const RObject &x) { return x.get__(); }
inline SEXP wrap(const String &x)
{
    SEXP s = mxref::alloc(STRSXP, 1);
    s->str = x.get_cstring();
    return s;
}
inline SEXP wrap(const char *x) { return wrap(String(x)); }
inline SEXP wrap(const std::string &x) { return wrap(String(x)); }
inline SEXP wrap(bool x)
{
    SEXP s = mxref::alloc(LGLSXP, 1);
    ((int *)s->data)[0] = x ? 1 : 0;
    return s;
}
inline SEXP wrap(int x)
{
    SEXP s = mxref::alloc(INTSXP, 1);
    ((int *)s->data)[0] = x;
    return s;
}
inline SEXP wrap(double x)
{
    SEXP s = mxref::alloc(REALSXP, 1);
    ((double *)s->data)[0] = x;
    return s;
}
inline SEXP wrap(size_t x) { return wrap((double)x); }
inline SEXP wrap(const std::vector<int> &x) { return IntegerVector(x.begin(), x.end()).get__(); }
inline SEXP wrap(const std::vector<double> &x) { return NumericVector(x.begin(), x.end()).get__(); }

/* as<T>(): SEXP -> C++ value */
template <class T, class Enable = void> struct As {
    static T get(SEXP x) { return T(x); }
};
template <class T> struct As<T, typename std::enable_if<std::is_arithmetic<T>::value>::type> {
    static T get(SEXP x)
    {
        if (!x || x->length != 1) throw std::runtime_error("Expecting a single value");
        if (x->type == REALSXP) return (T)((double *)x->data)[0];
        if (x->type == INTSXP || x->type == LGLSXP) return (T)((int *)x->data)[0];
        throw std::runtime_error("Expecting a single numeric value");
    }
};
template <class T> T as(SEXP x) { return As<T>::get(x); }

struct NamedValue {
    std::string name;
    RObject value;
};
struct NamedPlaceholder {
    struct Name {
        std::string name;
        template <class T> NamedValue operator=(const T &v) const { return NamedValue{name, RObject(wrap(v))}; }
    };
    Name operator[](const char *n) const { return Name{n}; }
    Name operator[](const std::string &n) const { return Name{n}; }
};
static const NamedPlaceholder _ = NamedPlaceholder();

class List : public RObject {
public:
    List() { set(mxref::alloc(VECSXP, 0)); }
    List(SEXP x) { set(mxref::checked(x, VECSXP, "a list")); }
    List(const List &o) : RObject(o) {}
    List &operator=(const List &o) { set(o.s_); return *this; }

    class Proxy {
        SEXP list_;
        std::string name_;
        R_xlen_t index_;
        SEXP find() const
        {
            if (index_ >= 0) return list_->items.at((size_t)index_);
            for (size_t i = 0; i < list_->names.size(); i++)
                if (list_->names[i] == name_) return list_->items[i];
            throw std::runtime_error("no list element named '" + name_ + "'");
        }
        void put(SEXP v)
        {
            mxref::retain(v);
            if (index_ >= 0) {
                mxref::release(list_->items.at((size_t)index_));
                list_->items[(size_t)index_] = v;
                return;
            }
            for (size_t i = 0; i < list_->names.size(); i++)
                if (list_->names[i] == name_) {
                    mxref::release(list_->items[i]);
                    list_->items[i] = v;
                    return;
                }
            list_->names.push_back(name_);
            list_->items.push_back(v);
            list_->length = (R_xlen_t)list_->items.size();
        }
    public:
        Proxy(SEXP l, const std::string &n) : list_(l), name_(n), index_(-1) {}
        Proxy(SEXP l, R_xlen_t i) : list_(l), index_(i) {}
        template <class T> Proxy &operator=(const T &v) { put(wrap(v)); return *this; }
        Proxy &operator=(const Proxy &o) { put(o.find()); return *this; }
        operator SEXP() const { return find(); }
        template <int RTYPE> operator Vector<RTYPE>() const { return Vector<RTYPE>(find()); }
        template <int RTYPE> operator Matrix<RTYPE>() const { return Matrix<RTYPE>(find()); }
        operator int() const { return as<int>(find()); }
        operator double() const { return as<double>(find()); }
        operator bool() const { return as<bool>(find()); }
    };

    Proxy operator[](const char *n) { return Proxy(s_, std::string(n)); }
    Proxy operator[](const std::string &n) { return Proxy(s_, n); }
    Proxy operator[](int i) { return Proxy(s_, (R_xlen_t)i); }
    Proxy operator[](size_t i) { return Proxy(s_, (R_xlen_t)i); }
    R_xlen_t size() const { return (R_xlen_t)s_->items.size(); }
    R_xlen_t length() const { return size(); }
    bool containsElementNamed(const char *n) const
    {
        for (const std::string &k : s_->names)
            if (k == n) return true;
        return false;
    }

    static List create() { return List(); }
    template <class... Args> static List create(const Args &... args)
    {
        List out;
        int unused[] = {0, (out.append(args), 0)...};
        (void)unused;
        return out;
    }

private:
    void append(const NamedValue &nv) { (*this)[nv.name] = nv.value; }
    template <class T> void append(const T &v)
    {
        SEXP x = wrap(v);
        mxref::retain(x);
        s_->names.push_back(std::string());
        s_->items.push_back(x);
        s_->length = (R_xlen_t)s_->items.size();
    }
};

class S4 : public RObject {
public:
    S4() {}
    S4(SEXP x) { set(mxref::checked(x, S4SXP, "an S4 object")); }
    S4(const S4 &o) : RObject(o) {}
    S4 &operator=(const S4 &o) { set(o.s_); return *this; }
    bool inherits(const char *cls) const
    {
        for (const std::string &c : s_->classes)
            if (c == cls) return true;
        return false;
    }
    bool is(const char *cls) const { return inherits(cls); }
    bool hasSlot(const std::string &name) const
    {
        for (const std::string &k : s_->names)
            if (k == name) return true;
        return false;
    }
    SEXP slot(const std::string &name) const
    {
        for (size_t i = 0; i < s_->names.size(); i++)
            if (s_->names[i] == name) return s_->items[i];
        throw std::runtime_error("no slot of name \"" + name + "\"");
    }
};

template <class T>
class ListOf : public RObject {
public:
    ListOf() {}
    ListOf(SEXP x) { set(mxref::checked(x, VECSXP, "a list")); }
    R_xlen_t size() const { return (R_xlen_t)s_->items.size(); }
    template <class I> T operator[](I i) const { return T(s_->items.at((size_t)i)); }
};

inline SEXP unwindProtect(SEXP (*f)(void *), void *arg);

}  // namespace Rcpp

#endif
