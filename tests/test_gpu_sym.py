"""Device level of the structured-matrix family (include/mxgpu_sym.h) on guarded buffers (tests/devmem.py): every
operand and output lies between sentinels, outputs and the workspace start as poison, inputs are checked untouched.
Expectations come from tests/sym_model.py and are compared with `==` on bits (the routines only copy); every call is
made twice and must give the same bits.  The cases are the smallest at which count -> scan -> fill can go wrong."""
import ctypes as C

import numpy as np
import pytest

import sym_model as SM
from devmem import GCsr, GuardedVec, _sync, last_row_launch
from matrixextra_amd import _lib

pytestmark = pytest.mark.gpu

VD = {"d": _lib.MX_F64, "l": _lib.MX_LGL, "n": _lib.MX_NONE}
VT = {"d": np.float64, "l": np.int32}
UP = {"U": _lib.MX_UPLO_UPPER, "L": _lib.MX_UPLO_LOWER}
CASES = SM.triplet_cases()


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = SM.bits(a), SM.bits(b)
    return a.dtype == b.dtype and np.array_equal(a, b)


def dev_symmetric(n, p, j, x, kind, uplo):
    """count, then fill: (out_p, out_j, out_x, None), or (None, None, None, message) when the count refuses"""
    lib = _lib.load()
    A = GCsr(p, j, x)
    nnz = int(j.size)
    gp = GuardedVec(np.int32, n=n + 1)
    gws = GuardedVec(np.uint8, n=lib.mxd_csr_sym_workspace_bytes(n, nnz))
    nnz_out = C.c_int64(-1)
    rc = lib.mxd_csr_symmetric_to_general_count(n, A.p.ptr, A.j.ptr, nnz, UP[uplo], gp.ptr, gws.ptr, C.byref(nnz_out), None)
    if rc != 0:
        err = lib.mx_last_error().decode()
        _sync()
        A.assert_untouched()
        gp._download()                                   # whatever it wrote stayed between the guards
        gws._download()
        return None, None, None, err
    gj = GuardedVec(np.int32, n=nnz_out.value)
    gx = None if kind == "n" else GuardedVec(VT[kind], n=nnz_out.value)
    _lib.check(lib.mxd_csr_symmetric_to_general_fill(n, A.p.ptr, A.j.ptr, A.xptr, VD[kind], nnz, UP[uplo], gp.ptr,
                                                     nnz_out.value, gj.ptr, None if gx is None else gx.ptr, gws.ptr, None))
    launch = last_row_launch()
    _sync()
    A.assert_untouched()
    gws._download()
    return gp.result(), gj.result(), None if gx is None else gx.result(), launch


def dev_unit_triangular(n, p, j, x, kind, uplo):
    lib = _lib.load()
    A = GCsr(p, j, x)
    nnz = int(j.size)
    gp, gj = GuardedVec(np.int32, n=n + 1), GuardedVec(np.int32, n=nnz + n)
    gx = None if kind == "n" else GuardedVec(VT[kind], n=nnz + n)
    _lib.check(lib.mxd_csr_unit_triangular_to_general(n, A.p.ptr, A.j.ptr, A.xptr, VD[kind], nnz, UP[uplo], gp.ptr, gj.ptr,
                                                      None if gx is None else gx.ptr, None))
    _sync()
    A.assert_untouched()
    return gp.result(), gj.result(), None if gx is None else gx.result()


def dev_triangle_check(n, p, j, uplo, strict):
    lib = _lib.load()
    A = GCsr(p, j)
    gws = GuardedVec(np.uint8, n=16)
    outside = C.c_int64(-1)
    _lib.check(lib.mxd_csr_triangle_check(n, A.p.ptr, A.j.ptr, int(j.size), UP[uplo], int(strict), gws.ptr,
                                          C.byref(outside), None))
    _sync()
    A.assert_untouched()
    gws._download()
    return outside.value


@pytest.mark.parametrize("kind", SM.KINDS)
@pytest.mark.parametrize("uplo", SM.UPLOS)
@pytest.mark.parametrize("name", list(CASES))
def test_symmetric_to_general(gpu, name, uplo, kind):
    n, p, j, x = SM.case(name, uplo, kind, CASES)
    want_p, want_j, want_x = SM.symmetric_to_general(p, j, x, uplo)
    got_p, got_j, got_x, launch = dev_symmetric(n, p, j, x, kind, uplo)
    assert got_p is not None, launch
    assert np.array_equal(got_p, want_p) and np.array_equal(got_j, want_j) and same_bits(got_x, want_x)
    if name.startswith("lanes-"):
        G = int(name.split("-")[1])
        assert SM.pick_group(want_j.size / n) == G and launch == ("sym_fill", G)
    again = dev_symmetric(n, p, j, x, kind, uplo)
    assert np.array_equal(again[0], got_p) and np.array_equal(again[1], got_j) and same_bits(again[2], got_x)


def strict_part(p, j, x):
    """the case without its diagonal entries: what a unit-triangular operand stores"""
    r = SM.rows_of(p)
    keep = np.asarray(j) != r
    q = np.zeros(p.size, dtype=np.int32)
    if p.size > 1:
        q[1:] = np.cumsum(np.bincount(r[keep], minlength=p.size - 1))
    return q, SM.i32(j[keep]), None if x is None else x[keep]


@pytest.mark.parametrize("kind", SM.KINDS)
@pytest.mark.parametrize("uplo", SM.UPLOS)
@pytest.mark.parametrize("name", list(CASES))
def test_unit_triangular_to_general(gpu, name, uplo, kind):
    n, p, j, x = SM.case(name, uplo, kind, CASES)
    p, j, x = strict_part(p, j, x)
    want = SM.unit_triangular_to_general(p, j, x, kind, uplo)
    got = dev_unit_triangular(n, p, j, x, kind, uplo)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_bits(got[2], want[2])
    assert got[1].size == j.size + n
    again = dev_unit_triangular(n, p, j, x, kind, uplo)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]) and same_bits(again[2], got[2])


@pytest.mark.parametrize("uplo", SM.UPLOS)
@pytest.mark.parametrize("name", list(CASES))
def test_triangle_check(gpu, name, uplo):
    n, p, j, _ = SM.case(name, uplo, "n", CASES)
    other = "L" if uplo == "U" else "U"
    for stated in (uplo, other):
        for strict in (False, True):
            want = SM.triangle_check(p, j, stated, strict)
            assert dev_triangle_check(n, p, j, stated, strict) == want
            assert dev_triangle_check(n, p, j, stated, strict) == want
    assert SM.triangle_check(p, j, uplo) == 0


@pytest.mark.parametrize("kind", SM.KINDS)
@pytest.mark.parametrize("uplo", SM.UPLOS)
def test_a_wrong_triangle_entry_fails_the_count(gpu, uplo, kind):
    """one entry of the n = 300 case moved across the diagonal: the count refuses it before any fill"""
    n, p, j, x = SM.case("n300-crosses-the-tiles", uplo, kind, CASES)
    r = SM.rows_of(p)
    at = np.flatnonzero((j != r) & (r > 0) & (r < n - 1))[1234]
    jj = j.copy()
    jj[at] = r[at] - 1 if uplo == "U" else r[at] + 1
    assert SM.triangle_check(p, jj, uplo) == 1
    with pytest.raises(ValueError):
        SM.symmetric_to_general(p, jj, x, uplo)
    got_p, _, _, err = dev_symmetric(n, p, jj, x, kind, uplo)
    assert got_p is None and "1 entry lies outside the stored triangle" in err and f'uplo = "{uplo}"' in err
    assert dev_triangle_check(n, p, jj, uplo, False) == 1


@pytest.mark.parametrize("uplo", SM.UPLOS)
def test_a_stored_diagonal_counts_under_strict(gpu, uplo):
    n, p, j, _ = SM.case("n300-crosses-the-tiles", uplo, "n", CASES)
    on_diagonal = int(np.count_nonzero(j == SM.rows_of(p)))
    assert on_diagonal > 10
    assert dev_triangle_check(n, p, j, uplo, False) == 0
    assert dev_triangle_check(n, p, j, uplo, True) == on_diagonal


def test_export_level_matches_the_model(gpu):
    """mx_csr_symmetric_to_general_begin / _unit_triangular_ / mx_csr_triangle_check through exports.py"""
    from matrixextra_amd import exports as E
    for uplo in SM.UPLOS:
        for kind in SM.KINDS:
            n, p, j, x = SM.case("unsorted-with-repeats", uplo, kind, CASES)
            want = SM.symmetric_to_general(p, j, x, uplo)
            before = (p.copy(), j.copy(), None if x is None else x.copy())
            got = E.csr_symmetric_to_general(p, j, x, uplo)
            got = (got["indptr"], got["indices"], got["values"])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_bits(got[2], want[2])
            sp, sj, sx = strict_part(p, j, x)
            want = SM.unit_triangular_to_general(sp, sj, sx, kind, uplo)
            got = E.csr_unit_triangular_to_general(sp, sj, sx, uplo)
            got = (got["indptr"], got["indices"], got["values"])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_bits(got[2], want[2])
            assert E.csr_triangle_check(p, j, uplo, strict=True) == SM.triangle_check(p, j, uplo, True) > 0
            with pytest.raises(_lib.MxError, match="on the diagonal or outside the stored triangle"):
                E.csr_unit_triangular_to_general(p, j, x, uplo)
            assert np.array_equal(before[0], p) and np.array_equal(before[1], j) and same_bits(before[2], x)
