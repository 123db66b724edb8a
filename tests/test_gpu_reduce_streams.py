"""The device-level entry points of include/mxgpu_reduce.h on a side stream behind pending work, with the harness of
tests/streams.py (gate, side_stream, run_ordered, run_reuse): mxd_segment_reduce and mxd_csr_diag enqueue and return,
mxd_csr_column_order synchronises once (its error flag).  Each row has two operand sets of one shape: in the ordered
tests the buffers hold the second one until a copy behind the gate brings the first, so a launch, a memset or a copy
on the wrong stream, or a flag read too early, gives the second set's answer; the reuse tests issue a call twice
behind one gate on the same buffers.  Data is integer-valued: the expected sums are exact."""
import numpy as np
import pytest

import reduce_model as RM
import streams as ST
from conftest import rand_csr
from matrixextra_amd import _lib
from streams import B, Case, In, Out, Row, Step, Ws

F64 = _lib.MX_F64
i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)                  # noqa: E731


def L():
    return _lib.load()


def flipped(p, j):
    """the same matrix with its rows in reverse order: another valid CSR of the same shape and entry count"""
    m = p.size - 1
    order = np.concatenate([np.arange(p[r], p[r + 1]) for r in range(m - 1, -1, -1)] + [np.zeros(0, np.int64)]).astype(np.int64)
    q = np.zeros(m + 1, dtype=np.int32)
    q[1:] = np.cumsum(np.diff(p)[::-1])
    return q, i32(j[order])


def operand(v, seed, m, n, density):
    p, j, _ = rand_csr(m, n, density, seed, sorted_cols=False)
    if v:
        p, j = flipped(p, j)
    rng = np.random.default_rng([seed, v])
    x = rng.integers(-9, 10, size=j.size).astype(np.float64)
    x[rng.integers(0, j.size, size=5)] = np.nan
    return i32(p), i32(j), x


SR_M, SR_N = 45, 400                                     # 45 rows over some 9000 entries: three tiles, rows across them


def segment_reduce(v):
    p, j, x = operand(v, 61, SR_M, SR_N, 0.5)
    nnz = j.size
    assert nnz > 2 * RM.TILE
    perm = i32(np.random.default_rng([62, v]).permutation(nnz))
    want, skipped, _ = RM.segment_reduce(RM.SUM, x, p, perm, na_rm=True)
    assert skipped.sum() >= 1
    return Case(dict(x=In(x), perm=In(perm), seg=In(p), out=Out(np.float64, want), skip=Out(np.int32, skipped),
                     ws=Ws(4 * L().mxd_compact_workspace_bytes(nnz))),
                [Step("mxd_segment_reduce", [RM.SUM, B("x"), F64, B("perm"), nnz, B("seg"), SR_M, 1, B("out"), B("skip"),
                                             B("ws")], late=("x", "perm", "seg"))])


def segment_reduce_abs_max(v):
    """one segment over everything, NaN kept: what norm() ends with"""
    _, j, x = operand(v, 63, SR_M, SR_N, 0.5)
    x = np.where(np.isnan(x), 3.0, x) * (v + 1.0)
    nnz = j.size
    seg = i32([0, nnz])
    want = RM.segment_reduce(RM.ABS_MAX, x, seg)[0]
    assert want[0] == 9.0 * (v + 1.0)
    return Case(dict(x=In(x), seg=In(seg), out=Out(np.float64, want), ws=Ws(4 * L().mxd_compact_workspace_bytes(nnz))),
                [Step("mxd_segment_reduce", [RM.ABS_MAX, B("x"), F64, None, nnz, B("seg"), 1, 0, B("out"), None, B("ws")],
                      late=("x",))])


CO_M, CO_N = 300, 70


def column_order_case(v):
    """operands, buffers and the order step shared by the two rows below; both variants have the same entry count"""
    p, j, x = operand(v, 64, CO_M, CO_N, 0.2)
    nnz = j.size
    assert nnz > RM.TILE
    perm, colptr = RM.column_order(j, CO_N)
    bufs = dict(p=In(p), j=In(j), perm=Out(np.int32, perm), colptr=Out(np.int32, colptr),
                ws=Ws(L().mxd_csr_transpose_workspace_bytes(nnz)))
    step = Step("mxd_csr_column_order", [CO_M, CO_N, B("p"), B("j"), nnz, B("perm"), B("colptr"), B("ws")],
                late=("p", "j"), waits=True)
    return p, j, x, nnz, perm, colptr, bufs, step


def column_order(v):
    *_, bufs, step = column_order_case(v)
    return Case(bufs, [step])


def column_sums(v):
    """the order, then the column sums through it: the reduction reads what the order's launches wrote"""
    p, j, x, nnz, perm, colptr, bufs, step = column_order_case(v)
    want, skipped, _ = RM.segment_reduce(RM.SUM, x, colptr, perm, na_rm=True)
    bufs.update(x=In(x), out=Out(np.float64, want), skip=Out(np.int32, skipped),
                rws=Ws(4 * L().mxd_compact_workspace_bytes(nnz)))
    step.pre = True
    return Case(bufs, [step, Step("mxd_segment_reduce", [RM.SUM, B("x"), F64, B("perm"), nnz, B("colptr"), CO_N, 1, B("out"),
                                                          B("skip"), B("rws")], late=("x",))])


def diag(sorted_rows):
    def make(v):
        p, j, _ = rand_csr(50, 80, 0.25, 65, sorted_cols=bool(sorted_rows))
        if v:
            p, j = flipped(p, j)
        x = np.random.default_rng([66, v]).integers(1, 10, size=j.size).astype(np.float64)
        want = RM.diag(p, j, x, "d", 50, 80)
        assert np.count_nonzero(want) >= 3
        return Case(dict(p=In(i32(p)), j=In(i32(j)), x=In(x), out=Out(np.float64, want)),
                    [Step("mxd_csr_diag", [50, 80, B("p"), B("j"), B("x"), F64, j.size, sorted_rows, B("out")],
                          late=("p", "j", "x"))])
    return make


ROWS = [Row(name, make) for name, make in [
    ("segment_reduce", segment_reduce), ("segment_reduce_abs_max", segment_reduce_abs_max),
    ("column_order", column_order), ("column_sums", column_sums), ("diag_scan", diag(0)), ("diag_search", diag(1))]]
STEPS = [(row, k) for row in ROWS for k, st in enumerate(row.cases()[0].steps) if not st.pre]
FREE = [(row, k) for row, k in STEPS if not row.cases()[0].steps[k].waits]
step_id = lambda rk: f"{rk[0].name}-{rk[0].cases()[0].steps[rk[1]].fn}"      # noqa: E731


def test_the_rows_cover_the_three_entry_points_and_their_sync_contract():
    fns = {st.fn: st.waits for row in ROWS for st in row.cases()[0].steps}
    assert fns == {"mxd_segment_reduce": False, "mxd_csr_diag": False, "mxd_csr_column_order": True}
    declared = {n for n in _lib.REDUCE_HEADER.functions if n.startswith("mxd_")}
    assert declared == set(fns)
    with open(_lib.REDUCE_HEADER_PATH) as f:
        text = f.read()
    for name, waits in fns.items():
        at = text.index("int %s(" % name)
        comment = text[text.rindex("/*", 0, at):at]
        assert ("One synchronisation" in comment) == waits and ("no synchronisation" in comment) == (not waits), name
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
