"""The device-level entry points of include/mxgpu_sym.h on a side stream behind pending work, with the harness of
tests/streams.py (gate, side_stream, run_ordered, run_reuse): mxd_csr_symmetric_to_general_fill and
mxd_csr_unit_triangular_to_general enqueue and return; mxd_csr_triangle_check synchronises once (its count) and
mxd_csr_symmetric_to_general_count twice (the column order's flag, then the wrong-triangle count with nnz_out).  Each row
has two operand sets of one shape: in the ordered tests the buffers hold the second one until a copy behind the gate
brings the first, so a launch, a memset or a copy on the wrong stream, or a value read too early, gives the second set's
answer; the reuse tests issue a call twice behind one gate on the same buffers.  Expectations are sym_model's."""
import numpy as np
import pytest

import streams as ST
import sym_model as SM
from matrixextra_amd import _lib
from streams import B, Case, H, In, Out, Row, Step, Ws

F64 = _lib.MX_F64
UP = {"U": _lib.MX_UPLO_UPPER, "L": _lib.MX_UPLO_LOWER}
N = 300


def L():
    return _lib.load()


def operand(v, uplo, diagonal=True):
    """n = 300, some 9000 stored entries (three tiles of the scan and the radix passes); variant 1 is the same
    triangle reflected in the anti-diagonal: another triangle of the same side with the same entry counts"""
    r, c = SM.random_upper(N, 30, 4, diagonal=diagonal)
    if v:
        r, c = N - 1 - c, N - 1 - r
    p, j = SM.csr_of(N, r, c, uplo)
    x = np.random.default_rng([7, v]).integers(1, 1000, j.size).astype(np.float64)
    return p, j, x


def triangle_check(v):
    """every third (v = 0) or fifth (v = 1) off-diagonal entry of an upper triangle moved below the diagonal"""
    p, j, _ = operand(0, "U")
    r = SM.rows_of(p)
    move = np.flatnonzero((j != r) & (r > 0))[::3 if v == 0 else 5]
    j = j.copy()
    j[move] = r[move] - 1
    want = SM.triangle_check(p, j, "U")
    assert want == move.size > 500
    return Case(dict(p=In(p), j=In(j), ws=Ws(16)),
                [Step("mxd_csr_triangle_check", [N, B("p"), B("j"), j.size, UP["U"], 0, B("ws"), H("outside")],
                      late=("j",), waits=True, host={"outside": want})])


def symmetric_case(v, uplo):
    p, j, x = operand(v, uplo)
    nnz = j.size
    assert nnz > 2 * 4096
    op, oj, ox = SM.symmetric_to_general(p, j, x, uplo)
    bufs = dict(p=In(p), j=In(j), x=In(x), op=Out(np.int32, op), oj=Out(np.int32, oj), ox=Out(np.float64, ox),
                ws=Ws(L().mxd_csr_sym_workspace_bytes(N, nnz)))
    count = Step("mxd_csr_symmetric_to_general_count", [N, B("p"), B("j"), nnz, UP[uplo], B("op"), B("ws"), H("nnz_out")],
                 late=("p", "j"), waits=True, host={"nnz_out": int(op[-1])})
    fill = Step("mxd_csr_symmetric_to_general_fill", [N, B("p"), B("j"), B("x"), F64, nnz, UP[uplo], B("op"), int(op[-1]),
                                                      B("oj"), B("ox"), B("ws")], late=("p", "j", "x"))
    return bufs, count, fill


def symmetric_count(uplo):
    def make(v):
        bufs, count, _ = symmetric_case(v, uplo)
        del bufs["x"], bufs["oj"], bufs["ox"]
        return Case(bufs, [count])
    return make


def symmetric_fill(uplo):
    def make(v):
        bufs, count, fill = symmetric_case(v, uplo)
        count.pre = True
        return Case(bufs, [count, fill])
    return make


def unit_triangular(uplo):
    def make(v):
        p, j, x = operand(v, uplo, diagonal=False)
        op, oj, ox = SM.unit_triangular_to_general(p, j, x, "d", uplo)
        return Case(dict(p=In(p), j=In(j), x=In(x), op=Out(np.int32, op), oj=Out(np.int32, oj), ox=Out(np.float64, ox)),
                    [Step("mxd_csr_unit_triangular_to_general", [N, B("p"), B("j"), B("x"), F64, j.size, UP[uplo], B("op"),
                                                                 B("oj"), B("ox")], late=("p", "j", "x"))])
    return make


ROWS = [Row(name, make) for name, make in [
    ("triangle_check", triangle_check), ("symmetric_count_U", symmetric_count("U")), ("symmetric_count_L", symmetric_count("L")),
    ("symmetric_fill_U", symmetric_fill("U")), ("symmetric_fill_L", symmetric_fill("L")),
    ("unit_triangular_U", unit_triangular("U")), ("unit_triangular_L", unit_triangular("L"))]]
STEPS = [(row, k) for row in ROWS for k, st in enumerate(row.cases()[0].steps) if not st.pre]
FREE = [(row, k) for row, k in STEPS if not row.cases()[0].steps[k].waits]
step_id = lambda rk: f"{rk[0].name}-{rk[0].cases()[0].steps[rk[1]].fn}"      # noqa: E731


def test_the_rows_cover_every_stream_taking_prototype_and_its_sync_contract():
    fns = {st.fn: st.waits for row in ROWS for st in row.cases()[0].steps}
    assert fns == {"mxd_csr_triangle_check": True, "mxd_csr_symmetric_to_general_count": True,
                   "mxd_csr_symmetric_to_general_fill": False, "mxd_csr_unit_triangular_to_general": False}
    with open(_lib.SYM_HEADER_PATH) as f:
        text = f.read()
    takes_stream = {n for n in _lib.SYM_HEADER.functions
                    if n.startswith("mxd_") and "void *stream)" in text[text.index(n + "("):].split(";")[0]}
    assert takes_stream == set(fns)
    for name, waits in fns.items():
        at = text.index("int %s(" % name)
        comment = text[text.rindex("/*", 0, at):at]
        assert (" synchronisation" in comment.replace("no synchronisation", "")) == waits, name
        assert ("no synchronisation" in comment) == (not waits), name
    for row in ROWS:                                     # the two operand sets differ where it matters
        a, b = row.cases()
        outs = [n for n in a.bufs if type(a.bufs[n]) is Out]
        assert any(not np.array_equal(a.bufs[n].expect, b.bufs[n].expect) for n in outs) or \
            any(sa.host != sb.host for sa, sb in zip(a.steps, b.steps)), row.name


@pytest.mark.gpu
@pytest.mark.parametrize("rk", STEPS, ids=[step_id(rk) for rk in STEPS])
def test_ordered(gpu, rk):
    ST.run_ordered(*rk)


@pytest.mark.gpu
@pytest.mark.parametrize("rk", FREE, ids=[step_id(rk) for rk in FREE])
def test_reuse(gpu, rk):
    ST.run_reuse(*rk)
