"""The device-level entry points of include/mxgpu_spgemm.h on a side stream behind pending work, with the harness of
tests/streams.py (gate, side_stream, run_ordered, run_reuse): mxd_csr_spgemm_count synchronises once, for its two
totals, and mxd_csr_spgemm_fill enqueues and returns.  The row has two operand sets of one shape, with rows in every
bin: in the ordered tests the buffers hold the second one until a copy behind the gate brings the first, so a launch on
the wrong stream, or a total read too early, gives the second set's answer; the reuse test issues the fill twice behind
one gate on the same buffers, each time behind its own count's workspace.  Data is integer-valued: the expected sums are
exact in any order, and the model gives them in the defined one."""
import ctypes as C

import numpy as np
import pytest

import spgemm_model as SM
import streams as ST
from matrixextra_amd import _lib
from streams import B, Case, H, In, Out, Row, Step, Ws

F64 = _lib.MX_F64
i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)                  # noqa: E731
M_, K_ = 60, 24


def L():
    return _lib.load()


def limits():
    g, l = C.c_int(0), C.c_int(0)
    _lib.check(L().mxd_csr_spgemm_limits(M_, 1, C.byref(g), C.byref(l), None))
    return g.value, l.value


GU, LU = limits()
N_ = LU + 40


def operands(v):
    """(Ap, Aj, Ax, Bp, Bj, Bx) of variant v: B rows of 2 .. LU + 30 entries, A rows of 0 .. 4 entries"""
    rng = np.random.default_rng([81, v])
    lens = rng.permutation([2, 3, 5, 7, 8, 12, 16, 20, GU, GU + 1, 50, 90, LU // 4, LU // 2, LU, LU + 1, LU + 30] + [4] * 7)
    Brows = [rng.choice(N_, size=int(k), replace=False) for k in lens]
    Arows = [rng.choice(K_, size=int(c), replace=True) for c in rng.integers(0, 5, size=M_)]
    Bp, Ap = np.zeros(K_ + 1, np.int32), np.zeros(M_ + 1, np.int32)
    Bp[1:], Ap[1:] = np.cumsum([r.size for r in Brows]), np.cumsum([r.size for r in Arows])
    Aj, Bj = i32(np.concatenate(Arows)), i32(np.concatenate(Brows))
    Ax = rng.integers(-9, 10, size=Aj.size).astype(np.float64)
    Bx = rng.integers(-9, 10, size=Bj.size).astype(np.float64)
    return Ap, Aj, Ax, Bp, Bj, Bx


def product(v):
    Ap, Aj, Ax, Bp, Bj, Bx = operands(v)
    p, j, x = SM.spgemm(Ap, Aj, Ax, Bp, Bj, Bx, K_, N_)
    ub = SM.row_bounds(Ap, Aj, Bp, K_, N_)
    assert (ub == 0).any() and ((ub > 0) & (ub <= GU)).any() and ((ub > GU) & (ub <= LU)).any() and (ub > LU).any()
    bufs = dict(Ap=In(Ap), Aj=In(Aj), Ax=In(Ax), Bp=In(Bp), Bj=In(Bj), Bx=In(Bx), out_p=Out(np.int32, p),
                out_j=Out(np.int32, j), out_x=Out(np.float64, x), ws=Ws(L().mxd_csr_spgemm_workspace_bytes(M_, N_)))
    return Case(bufs, [
        Step("mxd_csr_spgemm_count", [M_, K_, N_, B("Ap"), B("Aj"), Aj.size, B("Bp"), B("Bj"), Bj.size, B("out_p"), B("ws"),
                                      H("products"), H("nnz_out")],
             late=("Ap", "Aj", "Bp", "Bj"), waits=True,
             host=dict(products=SM.products(Ap, Aj, Bp, K_), nnz_out=int(p[-1]))),
        Step("mxd_csr_spgemm_fill", [M_, K_, N_, B("Ap"), B("Aj"), B("Ax"), F64, B("Bp"), B("Bj"), B("Bx"), F64, B("out_p"),
                                     B("out_j"), B("out_x"), B("ws")],
             late=("Ax", "Bx"))])


ROWS = [Row("spgemm", product)]
STEPS = [(row, k) for row in ROWS for k, st in enumerate(row.cases()[0].steps) if not st.pre]
FREE = [(row, k) for row, k in STEPS if not row.cases()[0].steps[k].waits]
step_id = lambda rk: f"{rk[0].name}-{rk[0].cases()[0].steps[rk[1]].fn}"      # noqa: E731


def test_the_row_covers_the_entry_points_and_their_sync_contract():
    fns = {st.fn: st.waits for row in ROWS for st in row.cases()[0].steps}
    assert fns == {"mxd_csr_spgemm_count": True, "mxd_csr_spgemm_fill": False}
    declared = {n for n, (ret, _) in _lib.SPGEMM_HEADER.functions.items() if n.startswith("mxd_") and ret is C.c_int}
    assert declared == set(fns) | {"mxd_csr_spgemm_limits"}              # the limits are host arithmetic: no stream work
    with open(_lib.SPGEMM_HEADER_PATH) as f:
        text = f.read()
    for name in fns:
        at = text.index("int %s(" % name)
        comment = text[text.rindex("/*", 0, at):at]
        assert ("One synchronisation" in comment) == fns[name] and ("no synchronisation" in comment) == (not fns[name]), name
    a, b = ROWS[0].cases()                                               # the two operand sets differ where it matters
    assert all(not np.array_equal(a.bufs[n].expect, b.bufs[n].expect) for n in ("out_p", "out_j", "out_x"))
    assert a.steps[0].host != b.steps[0].host


@pytest.mark.gpu
@pytest.mark.parametrize("rk", STEPS, ids=[step_id(rk) for rk in STEPS])
def test_ordered(gpu, rk):
    ST.run_ordered(*rk)


@pytest.mark.gpu
@pytest.mark.parametrize("rk", FREE, ids=[step_id(rk) for rk in FREE])
def test_reuse(gpu, rk):
    ST.run_reuse(*rk)
