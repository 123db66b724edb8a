"""The device-level entry points of include/mxgpu_gram.h on a side stream behind pending work, with the harness of
tests/streams.py (gate, side_stream, run_ordered, run_reuse): mxd_csr_spgemm_tri_count synchronises once, for its two
totals, and mxd_csr_spgemm_tri_fill enqueues and returns.  One row per mask (upper with b_sorted, lower without), each
with two operand sets of one shape and rows in every bin under the mask: in the ordered tests the buffers hold the
second set until a copy behind the gate brings the first, so a launch on the wrong stream, or a total read too early,
gives the second set's answer; the reuse test issues the fill twice behind one gate on the same buffers.  Data is
integer-valued: the expected sums are exact in any order, and the model gives them in the defined one."""
import ctypes as C

import numpy as np
import pytest

import gram_model as GM
import streams as ST
from matrixextra_amd import _lib
from streams import B, Case, H, In, Out, Row, Step, Ws

F64 = _lib.MX_F64
U, L = _lib.MX_UPLO_UPPER, _lib.MX_UPLO_LOWER
i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)                  # noqa: E731
K_ = 24


def lib():
    return _lib.load()


def limits():
    g, l = C.c_int(0), C.c_int(0)
    _lib.check(lib().mxd_csr_spgemm_limits(1, 1, C.byref(g), C.byref(l), None))
    return g.value, l.value


GU, LU = limits()
N_ = LU + 40
M_ = N_                                                                 # square: both windows run from 1 to n


def operands(v, b_sorted):
    """(Ap, Aj, Ax, Bp, Bj, Bx) of variant v: B rows of 2 .. n entries (ascending for b_sorted), A rows of 0 .. 4 entries
    at 120 places spread over the rows, so that both windows leave rows for every bin"""
    rng = np.random.default_rng([82, v])
    lens = rng.permutation([2, 3, 5, 7, 8, 12, 16, 20, GU, GU + 1, 50, 90, LU // 2, LU, LU + 1, N_, N_] + [4] * 7)
    Brows = [rng.choice(N_, size=int(k), replace=False) for k in lens]
    if b_sorted:
        Brows = [np.sort(r) for r in Brows]
    Arows = [np.zeros(0, np.int64) for _ in range(M_)]
    middle = rng.choice(np.arange(20, M_ - 20), size=80, replace=False)
    for i in np.concatenate([np.arange(20), np.arange(M_ - 20, M_), middle]):
        Arows[i] = rng.choice(K_, size=int(rng.integers(0, 5)), replace=True)
    Bp, Ap = np.zeros(K_ + 1, np.int32), np.zeros(M_ + 1, np.int32)
    Bp[1:], Ap[1:] = np.cumsum([r.size for r in Brows]), np.cumsum([r.size for r in Arows])
    Aj, Bj = i32(np.concatenate(Arows)), i32(np.concatenate(Brows))
    Ax = rng.integers(-9, 10, size=Aj.size).astype(np.float64)
    Bx = rng.integers(-9, 10, size=Bj.size).astype(np.float64)
    return Ap, Aj, Ax, Bp, Bj, Bx


def product(uplo, b_sorted):
    def make(v):
        Ap, Aj, Ax, Bp, Bj, Bx = operands(v, b_sorted)
        p, j, x = GM.spgemm_tri(Ap, Aj, Ax, Bp, Bj, Bx, K_, N_, uplo)
        ub = GM.row_bounds(Ap, Aj, Bp, Bj, K_, N_, uplo, b_sorted)
        assert (ub == 0).any() and ((ub > 0) & (ub <= GU)).any() and ((ub > GU) & (ub <= LU)).any() and (ub > LU).any()
        bufs = dict(Ap=In(Ap), Aj=In(Aj), Ax=In(Ax), Bp=In(Bp), Bj=In(Bj), Bx=In(Bx), out_p=Out(np.int32, p),
                    out_j=Out(np.int32, j), out_x=Out(np.float64, x), ws=Ws(lib().mxd_csr_spgemm_workspace_bytes(M_, N_)))
        return Case(bufs, [
            Step("mxd_csr_spgemm_tri_count", [M_, K_, N_, B("Ap"), B("Aj"), Aj.size, B("Bp"), B("Bj"), Bj.size, uplo,
                                              b_sorted, B("out_p"), B("ws"), H("products"), H("nnz_out")],
                 late=("Ap", "Aj", "Bp", "Bj"), waits=True,
                 host=dict(products=GM.products(Ap, Aj, Bp, Bj, K_, uplo, b_sorted), nnz_out=int(p[-1]))),
            Step("mxd_csr_spgemm_tri_fill", [M_, K_, N_, B("Ap"), B("Aj"), B("Ax"), F64, B("Bp"), B("Bj"), B("Bx"), F64, uplo,
                                             b_sorted, B("out_p"), B("out_j"), B("out_x"), B("ws")],
                 late=("Ax", "Bx"))])
    return make


ROWS = [Row("tri_upper_sorted", product(U, 1)), Row("tri_lower_as_is", product(L, 0))]
STEPS = [(row, k) for row in ROWS for k, st in enumerate(row.cases()[0].steps) if not st.pre]
FREE = [(row, k) for row, k in STEPS if not row.cases()[0].steps[k].waits]
step_id = lambda rk: f"{rk[0].name}-{rk[0].cases()[0].steps[rk[1]].fn}"      # noqa: E731


def test_the_rows_cover_the_entry_points_and_their_sync_contract():
    for row in ROWS:
        fns = {st.fn: st.waits for st in row.cases()[0].steps}
        assert fns == {"mxd_csr_spgemm_tri_count": True, "mxd_csr_spgemm_tri_fill": False}
        a, b = row.cases()                                              # the two operand sets differ where it matters
        assert all(not np.array_equal(a.bufs[n].expect, b.bufs[n].expect) for n in ("out_p", "out_j", "out_x"))
        assert a.steps[0].host != b.steps[0].host
    declared = {n for n, (ret, _) in _lib.GRAM_HEADER.functions.items() if n.startswith("mxd_") and ret is C.c_int}
    assert declared == set(fns)
    with open(_lib.GRAM_HEADER_PATH) as f:
        text = f.read()
    for name in fns:
        at = text.index("int %s(" % name)
        comment = text[text.rindex("/*", 0, at):at]
        assert ("One synchronisation" in comment) == fns[name] and ("no synchronisation" in comment) == (not fns[name]), name


@pytest.mark.gpu
@pytest.mark.parametrize("rk", STEPS, ids=[step_id(rk) for rk in STEPS])
def test_ordered(gpu, rk):
    ST.run_ordered(*rk)


@pytest.mark.gpu
@pytest.mark.parametrize("rk", FREE, ids=[step_id(rk) for rk in FREE])
def test_reuse(gpu, rk):
    ST.run_reuse(*rk)
