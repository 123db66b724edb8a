"""The device-level entry points of include/mxgpu_tprod.h on a side stream behind pending work, with the harness of
tests/streams.py (gate, side_stream, run_ordered, run_reuse): mxd_segment_dot and mxd_csr_transpose_by_order enqueue and
return.  Each row has two operand sets of one shape: in the ordered tests the buffers hold the second one until a copy
behind the gate brings the first, so a launch on the wrong stream gives the second set's answer; the reuse tests issue a
call twice behind one gate on the same buffers.  The last row is the chain a transposed product runs: the column order
(which synchronises once), the entry rows from it, the dot through both.  Data is integer-valued: the expected sums are
exact."""
import numpy as np
import pytest

import reduce_model as RM
import streams as ST
import tprod_model as TM
from conftest import rand_csr
from matrixextra_amd import _lib
from streams import B, Case, In, Out, Row, Step, Ws

F64, NONE = _lib.MX_F64, _lib.MX_NONE
i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)                  # noqa: E731
M_, N_ = 300, 70                                         # some 4200 entries: two tiles, columns across them


def L():
    return _lib.load()


def flipped(p, j):
    """the same matrix with its rows in reverse order: another valid CSR of the same shape and entry count"""
    m = p.size - 1
    order = np.concatenate([np.arange(p[r], p[r + 1]) for r in range(m - 1, -1, -1)] + [np.zeros(0, np.int64)]).astype(np.int64)
    q = np.zeros(m + 1, dtype=np.int32)
    q[1:] = np.cumsum(np.diff(p)[::-1])
    return q, i32(j[order])


def operand(v, seed):
    """(p, j, x, w, perm, colptr, rows in column order, X^T w) of variant v"""
    p, j, _ = rand_csr(M_, N_, 0.2, seed, sorted_cols=False)
    if v:
        p, j = flipped(p, j)
    rng = np.random.default_rng([seed, v])
    x = rng.integers(-9, 10, size=j.size).astype(np.float64)
    w = rng.integers(-9, 10, size=M_).astype(np.float64)
    perm, colptr = RM.column_order(j, N_)
    rows = TM.rows_of_entries(p)[perm]
    want = np.zeros(N_)
    np.add.at(want, j, x * w[TM.rows_of_entries(p)])
    assert j.size > RM.TILE
    return i32(p), i32(j), x, w, i32(perm), i32(colptr), i32(rows), want


def ws_dot(nnz):
    return Ws(4 * L().mxd_compact_workspace_bytes(nnz))


def segment_dot(v):
    p, j, x, w, perm, colptr, rows, want = operand(v, 71)
    nnz = j.size
    return Case(dict(x=In(x), perm=In(perm), key=In(rows), w=In(w), seg=In(colptr), out=Out(np.float64, want), ws=ws_dot(nnz)),
                [Step("mxd_segment_dot", [B("x"), F64, B("perm"), B("key"), B("w"), M_, nnz, B("seg"), N_, B("out"), B("ws")],
                      late=("x", "perm", "key", "w", "seg"))])


def segment_dot_rows(v):
    """the row form without values: X w of the pattern, perm = null and key = indices"""
    p, j, _, _, _, _, _, _ = operand(v, 72)
    w = np.random.default_rng([73, v]).integers(-9, 10, size=N_).astype(np.float64)
    want = np.zeros(M_)
    np.add.at(want, TM.rows_of_entries(p), w[j])
    return Case(dict(key=In(j), w=In(w), seg=In(p), out=Out(np.float64, want), ws=ws_dot(j.size)),
                [Step("mxd_segment_dot", [None, NONE, None, B("key"), B("w"), N_, j.size, B("seg"), M_, B("out"), B("ws")],
                      late=("key", "w", "seg"))])


def transpose_by_order(v):
    p, j, x, _, perm, _, rows, _ = operand(v, 74)
    return Case(dict(p=In(p), x=In(x), perm=In(perm), rows=Out(np.int32, rows), vals=Out(np.float64, x[perm])),
                [Step("mxd_csr_transpose_by_order", [M_, j.size, B("p"), B("x"), F64, B("perm"), B("rows"), B("vals")],
                      late=("p", "x", "perm"))])


def chain(v):
    """order -> rows -> dot: each step reads what the one before it wrote on the stream"""
    p, j, x, w, perm, colptr, rows, want = operand(v, 75)
    nnz = j.size
    bufs = dict(p=In(p), j=In(j), x=In(x), w=In(w), perm=Out(np.int32, perm), colptr=Out(np.int32, colptr),
                rows=Out(np.int32, rows), out=Out(np.float64, want), tws=Ws(L().mxd_csr_transpose_workspace_bytes(nnz)),
                ws=ws_dot(nnz))
    return Case(bufs, [
        Step("mxd_csr_column_order", [M_, N_, B("p"), B("j"), nnz, B("perm"), B("colptr"), B("tws")], late=("p", "j"),
             waits=True, pre=True),
        Step("mxd_csr_transpose_by_order", [M_, nnz, B("p"), None, NONE, B("perm"), B("rows"), None], late=("p",)),
        Step("mxd_segment_dot", [B("x"), F64, B("perm"), B("rows"), B("w"), M_, nnz, B("colptr"), N_, B("out"), B("ws")],
             late=("x", "w"))])


ROWS = [Row(name, make) for name, make in [
    ("segment_dot", segment_dot), ("segment_dot_rows", segment_dot_rows), ("transpose_by_order", transpose_by_order),
    ("chain", chain)]]
STEPS = [(row, k) for row in ROWS for k, st in enumerate(row.cases()[0].steps) if not st.pre]
FREE = [(row, k) for row, k in STEPS if not row.cases()[0].steps[k].waits]
step_id = lambda rk: f"{rk[0].name}-{rk[0].cases()[0].steps[rk[1]].fn}"      # noqa: E731


def test_the_rows_cover_the_entry_points_and_their_sync_contract():
    fns = {st.fn: st.waits for row in ROWS for st in row.cases()[0].steps}
    assert fns == {"mxd_segment_dot": False, "mxd_csr_transpose_by_order": False, "mxd_csr_column_order": True}
    declared = {n for n in _lib.TPROD_HEADER.functions if n.startswith("mxd_")}
    assert declared == set(fns) - {"mxd_csr_column_order"}               # the order is mxgpu_reduce.h's, tested there
    with open(_lib.TPROD_HEADER_PATH) as f:
        text = f.read()
    for name in declared:
        at = text.index("int %s(" % name)
        comment = text[text.rindex("/*", 0, at):at]
        assert ("One synchronisation" in comment) == fns[name] and ("no synchronisation" in comment) == (not fns[name]), name
    for row in ROWS:                                     # the two operand sets differ where it matters
        a, b = row.cases()
        assert any(not np.array_equal(a.bufs[n].expect, b.bufs[n].expect) for n in a.bufs if type(a.bufs[n]) is Out), row.name


@pytest.mark.gpu
@pytest.mark.parametrize("rk", STEPS, ids=[step_id(rk) for rk in STEPS])
def test_ordered(gpu, rk):
    ST.run_ordered(*rk)


@pytest.mark.gpu
@pytest.mark.parametrize("rk", FREE, ids=[step_id(rk) for rk in FREE])
def test_reuse(gpu, rk):
    ST.run_reuse(*rk)
