"""The device-level C-ABI on a non-default stream, behind pending work (harness: tests/streams.py).

ROWS is the table: one row per entry point, per count / fill pair or per short chain.  A row builds its call sequence
twice, from the real operands (variant 0) and from a second valid operand set of the same shapes (variant 1: the stale
content of the ordered tests, the second operands of the reuse tests), with the expectations of both from CPU oracles:
oracle/oracle.py where it has the routine, the numpy models of the suite (assign_model, assign_vec_model,
dvec_na_model, dense_svec_model, na_slice_model, coo_sort_model, the plan model) and a few lines of numpy written from
mxgpu.h for the rest.  Bars: structure, copied and single-operation values bit for bit with NaN as NaN-ness; SpMM /
SpMV / the float32 row vector within rtol 1e-12 (f64) and 1e-5 (f32) of the oracle, on operands whose sums are exact.

  test_ordered   P1 + P2 + P4 for every step of every row: the step's late operands hold stale content, the real
                 content arrives behind the gate, the gate is pending right before the call and, where WAITS says the
                 entry point does not synchronise, right after it; host results equal the oracle's before the fill is
                 issued; the fill follows without a host synchronisation and is read back on the side stream.
  test_reuse     P3 for every sync-free step: twice behind one gate on the same buffers with two operand sets.
What the table cannot show: at m=257, K=300, n=128 AUTO picks the row-wave kernel (B fits an XCD's L2), so the packed
copy of B is reached through algo PLANNED of mxd_spmm_csr_dense_ex and through mxd_spmm_plan_run; and
mxd_spmm_plan_copy_to_host and mxd_reversed_iota have no operand that could arrive late (nothing but
mxd_spmm_plan_create writes a plan, and it returns with the gate drained), so their rows show the values under a
pending gate and, for the iota, the reuse, but would not notice the null stream.  Issued on the null stream, every
other ordered test fails with the stale answer.
Without a GPU: the table names every `void *stream` prototype of mxgpu.h (test_every_stream_prototype_has_a_row), both
operand sets of every row are valid and every output is as long as the larger of the two needs
(test_fixtures_are_valid), and what WAITS says agrees with the header's comments (test_sync_contract_is_documented).
"""
import ctypes as C
import re

import numpy as np
import pytest

import assign_model as AM
import assign_vec_model as VM
import coo_sort_model as CM
import dense_svec_model as DM
import dvec_na_model as NM
import na_slice_model as SM
import rowgroup_cases as RC
import streams as ST
from conftest import rand_csr
from matrixextra_amd import _lib
from oracle import oracle as O
from streams import B, H, IO, PLAN_IN, PLAN_OUT, S, STREAM, Case, In, Out, Row, Step, Ws
from test_gpu_plan_build import plan_model

F64, F32 = _lib.MX_F64, _lib.MX_F32
NA_REAL = RC.NA_REAL
i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)                  # noqa: E731
f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)                # noqa: E731


def L():
    return _lib.load()


class Idx(np.ndarray):
    """int32 indices that carry the range they have to stay in, [0, bound), and whether they must be strictly
    ascending, for test_fixtures_are_valid"""
    bound, ascending = None, False

    def __array_finalize__(self, obj):
        self.bound, self.ascending = getattr(obj, "bound", None), False


def idx(a, bound, ascending=False):
    out = i32(a).view(Idx)
    out.bound, out.ascending = int(bound), ascending
    return out


# ---- operands ----------------------------------------------------------------------------------------------------------
def ivals(rng, n):
    """non-zero small integers: sums and products of them are exact whatever the order"""
    return (rng.integers(1, 9, size=n) * rng.choice([-1, 1], size=n)).astype(np.float64)


def rows_of(p):
    return np.repeat(np.arange(p.size - 1), np.diff(p)).astype(np.int64)


def flip(p, j, x=None):
    """the same matrix with its rows in reverse order: another valid CSR of the same shape and entry count"""
    m = p.size - 1
    idx = np.concatenate([np.arange(p[r], p[r + 1]) for r in range(m - 1, -1, -1)] + [np.zeros(0, np.int64)]).astype(np.int64)
    q = np.zeros(m + 1, dtype=np.int32)
    q[1:] = np.cumsum(np.diff(p)[::-1])
    return q, j[idx].copy(), None if x is None else x[idx].copy()


def csr(v, seed, m, K, density=0.15):
    """sorted CSR with exact values; variant 1 is variant 0 with the rows reversed and other values"""
    p, j, _ = rand_csr(m, K, density, seed)
    if v:
        p, j, _ = flip(p, j)
    return p, idx(j, K), ivals(np.random.default_rng([seed, v, 7]), j.size)


def dense_of(p, j, x, K):
    D = np.zeros((p.size - 1, K))
    np.add.at(D, (rows_of(p), j), x)
    return D


def rgc(v):
    """the row-group case: 8 lanes per row, three blocks and one row"""
    c = RC.make_case(8, 97, seed=v)
    c.j, c.j2, c.rows_take, c.cols_sorted = idx(c.j, c.K), idx(c.j2, c.K), idx(c.rows_take, c.m), idx(c.cols_sorted, c.K)
    return c


def coo(v, seed, m, n, nnz, unique=False):
    rng = np.random.default_rng([seed, v])
    if unique:
        cells = rng.permutation(m * n)[:nnz]
        return idx(cells // n, m), idx(cells % n, n), ivals(rng, nnz)
    return idx(rng.integers(0, m, nnz), m), idx(rng.integers(0, n, nnz), n), ivals(rng, nnz)


def merged_csr(rows, cols, vals, m):
    """canonical CSR of triplets: rows, then columns ascending, repeated cells summed in input order"""
    order = np.lexsort((cols, rows))
    r, c, x = rows[order], cols[order], vals[order]
    first = np.ones(r.size, dtype=bool)
    first[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    grp = np.cumsum(first) - 1
    out_x = np.zeros(int(first.sum()))
    np.add.at(out_x, grp, x)
    p = np.zeros(m + 1, dtype=np.int32)
    p[1:] = np.cumsum(np.bincount(r[first], minlength=m))
    return p, i32(c[first]), out_x


def colmap(take, nmap):
    """mxd_colmap_build: start[nmap + 1], pos = the positions of every value of `take`, ascending"""
    start = np.zeros(nmap + 1, dtype=np.int32)
    start[1:] = np.cumsum(np.bincount(take, minlength=nmap))
    return start, i32(np.argsort(take, kind="stable"))


def single(fn, args, bufs, late=None, **kw):
    """a row of one call; by default every input arrives late (a whole, consistent operand set)"""
    if late is None:
        late = tuple(n for n, s in bufs.items() if isinstance(s, (In, IO)))
    return Case(bufs, [Step(fn, args, late=late, **kw)])


# ---- SpMM ----------------------------------------------------------------------------------------------------------------
SPMM_M, SPMM_K, SPMM_N = 257, 300, 128


def spmm_operands(v, dtype):
    p, j, x = csr(v, 11, SPMM_M, SPMM_K, 0.04)
    Bm = (np.random.default_rng([12, v]).integers(-16, 17, size=(SPMM_K, SPMM_N)) / 16.0).astype(dtype)
    Cm = (dense_of(p, j, x, SPMM_K) @ Bm.astype(np.float64)).astype(dtype)
    return p, j, x, Bm, Cm


def spmm_bufs(v, dtype, colmajor):
    p, j, x, Bm, Cm = spmm_operands(v, dtype)
    return dict(p=In(p), j=In(j), x=In(x), B=In(Bm),
                C=Out(dtype, Cm.T if colmajor else Cm, rtol=1e-12 if dtype == np.float64 else 1e-5))


def spmm_ex(algo, dtype=np.float64, colmajor=0):
    def make(v):
        m, K, n = SPMM_M, SPMM_K, SPMM_N
        return single("mxd_spmm_csr_dense_ex",
                      [m, n, K, B("p"), B("j"), B("x"), B("B"), n, B("C"), m if colmajor else n,
                       F64 if dtype == np.float64 else F32, colmajor, algo, 1, 0, 0],
                      spmm_bufs(v, dtype, colmajor), waits=algo == _lib.MX_SPMM_PLANNED)
    return make


def spmm_plain(v):
    m, n = SPMM_M, SPMM_N
    return single("mxd_spmm_csr_dense", [m, n, B("p"), B("j"), B("x"), B("B"), n, B("C"), m, F32, 1],
                  spmm_bufs(v, np.float32, 1))


def plan_create_step(pre=False):
    return Step("mxd_spmm_plan_create", [SPMM_M, SPMM_K, B("p"), B("j"), B("x"), 3, STREAM, PLAN_OUT],
                late=("p", "j", "x"), waits=True, pre=pre)


def spmm_plan(v):
    n = SPMM_N
    return Case(spmm_bufs(v, np.float64, 0),
                [plan_create_step(),
                 Step("mxd_spmm_plan_run", [PLAN_IN, n, B("B"), n, B("C"), n, F64, 0, 0, -1], late=("B",))])


def spmm_plan_copy(v):
    p, j, x, _, _ = spmm_operands(v, np.float64)
    step_off, pcol, pval, _ = plan_model(p, j, x, SPMM_K, 3)
    host = dict(step_off=step_off.tobytes(), pcol=pcol.tobytes(), pval=pval.tobytes())
    return Case(dict(p=In(p), j=In(j), x=In(x)),
                [plan_create_step(pre=True),
                 Step("mxd_spmm_plan_copy_to_host", [PLAN_IN] + [H(k, nbytes=len(b) + 64) for k, b in host.items()],
                      waits=True, host=host)])


# ---- the row-group families: one case, 8 lanes per row ---------------------------------------------------------------------
def rg_values(c, v, which=0):
    n = c.nnz if which == 0 else c.nnz2
    return ivals(np.random.default_rng([21, v, which]), n)


def spmv_dvec(v):
    c = rgc(v)
    x = rg_values(c, v)
    vec = np.random.default_rng([22, v]).integers(-8, 9, size=c.K) / 8.0
    y = O.matmul_csr_dvec_numeric(c.p, c.j, x, vec)
    return single("mxd_spmv_csr_dvec", [c.m, c.nnz, B("p"), B("j"), B("x"), B("v"), F64, B("y")],
                  dict(p=In(c.p), j=In(c.j), x=In(x), v=In(vec), y=Out(np.float64, y, rtol=1e-12)))


def merge(v):
    c = rgc(v)
    x1, x2 = rg_values(c, v), rg_values(c, v, 1)
    want = O.add_csr_elemwise(c.p, c.p2, c.j, c.j2, x1, x2, False)
    nout, op, m = int(want["indices"].size), _lib.MX_OP_ADD, c.m
    bufs = dict(p1=In(c.p), j1=In(c.j), x1=In(x1), p2=In(c.p2), j2=In(c.j2), x2=In(x2),
                ws=Ws(L().mxd_merge_workspace_bytes(m)), op=Out(np.int32, want["indptr"]),
                oj=Out(np.int32, want["indices"]), ox=Out(np.float64, want["values"]))
    return Case(bufs, [
        Step("mxd_csr_merge_count", [op, m, B("p1"), B("j1"), c.nnz, B("p2"), B("j2"), c.nnz2, B("op"), B("ws"), H("nnz")],
             late=("p1", "j1", "p2", "j2"), waits=True, host=dict(nnz=nout)),
        Step("mxd_csr_merge_fill", [op, m, B("p1"), B("j1"), B("x1"), c.nnz, B("p2"), B("j2"), B("x2"), c.nnz2, B("op"),
                                    B("oj"), B("ox")], late=("x1", "x2"))])


def values_elemwise(v):
    rng = np.random.default_rng([23, v])
    a, b = ivals(rng, 3001), ivals(rng, 3001)
    return single("mxd_values_elemwise", [_lib.MX_OP_MUL, 3001, B("a"), B("b"), B("out")],
                  dict(a=In(a), b=In(b), out=Out(np.float64, a * b)))


def count_fill(c, v, want, count, fill, extra, late_count, ws_rows):
    """the shape shared by the gather and the column slices: count -> scan -> fill over rows_take"""
    bufs = dict(p=In(c.p), j=In(c.j), x=In(rg_values(c, v)), rows=In(c.rows_take), **extra,
                ws=Ws(L().mxd_gather_workspace_bytes(ws_rows)), np_=Out(np.int32, want["indptr"]),
                nj=Out(np.int32, want["indices"]), nx=Out(np.float64, want["values"]))
    return Case(bufs, [Step(count[0], count[1], late=late_count, waits=True, host=dict(nnz=int(want["indices"].size))),
                       Step(fill[0], fill[1], late=("x",))])


def gather(v):
    c = rgc(v)
    r, want = int(c.rows_take.size), O.copy_csr_rows_numeric(c.p, c.j, rg_values(c, v), c.rows_take)
    return count_fill(c, v, want,
                      ("mxd_csr_gather_count", [r, B("p"), B("rows"), B("np_"), B("ws"), H("nnz")]),
                      ("mxd_csr_gather_fill", [r, B("p"), B("j"), B("x"), B("rows"), B("np_"), B("nj"), B("nx"), F64,
                                               int(want["indices"].size)]), {}, ("p", "rows"), r)


def colrange(v):
    c = rgc(v)
    r, lo, hi, avg = int(c.rows_take.size), 100, 400, c.nnz / c.m
    want = O.copy_csr_rows_col_seq_numeric(c.p, c.j, rg_values(c, v), c.rows_take, i32([lo, hi]), False)
    return count_fill(c, v, want,
                      ("mxd_csr_colrange_count", [r, B("p"), B("j"), B("rows"), lo, hi, avg, B("np_"), B("ws"), H("nnz")]),
                      ("mxd_csr_colrange_fill", [r, B("p"), B("j"), B("x"), F64, B("rows"), lo, hi, avg, B("np_"), B("nj"),
                                                 B("nx")]), {}, ("p", "j", "rows"), r)


def colmap_rows(v):
    c = rgc(v)
    cols = idx(c.cols_sorted, c.K)
    cols[-1] = c.K - 1                                  # both variants map K columns
    r, nmap, avg = int(c.rows_take.size), c.K, c.nnz / c.m
    start, pos = colmap(cols, nmap)
    want = O.copy_csr_arbitrary_numeric(c.p, c.j, rg_values(c, v), c.rows_take, cols)
    case = count_fill(c, v, want,
                      ("mxd_csr_colmap_count", [r, B("p"), B("j"), B("rows"), nmap, B("start"), avg, B("np_"), B("ws"),
                                                H("nnz")]),
                      ("mxd_csr_colmap_fill", [r, B("p"), B("j"), B("x"), F64, B("rows"), nmap, B("start"), B("pos"), avg,
                                               B("np_"), B("nj"), B("nx")]),
                      dict(cols=In(cols), start=Out(np.int32, start), pos=Out(np.int32, pos),
                           mws=Ws(L().mxd_colmap_workspace_bytes(nmap))), ("p", "j", "rows"), r)
    build = Step("mxd_colmap_build", [B("cols"), cols.size, nmap, B("start"), B("pos"), B("mws")], late=("cols",))
    return Case(case.bufs, [build] + case.steps)


def reverse_columns(v):
    c = rgc(v)
    x = rg_values(c, v)
    j2, x2 = c.j.copy(), x.copy()
    O.reverse_columns_inplace(c.p, j2, x2, c.K)
    return single("mxd_csr_reverse_columns", [c.m, c.nnz, B("p"), B("j"), B("x"), F64, c.K],
                  dict(p=In(c.p), j=IO(c.j, j2), x=IO(x, x2)))


def reversed_iota(v):
    n = (1000, 777)[v]
    return single("mxd_reversed_iota", [n, B("out")], dict(out=Out(np.int32, np.arange(n - 1, -1, -1))))


def cbind(shift):
    def make(v):
        c = rgc(v)
        x1, x2 = rg_values(c, v), rg_values(c, v, 1)
        want = O.cbind_csr_numeric(c.p, c.j, x1, c.p2, i32(c.j2 + c.K), x2)
        bufs = dict(Xp=In(c.p), Xj=In(c.j), Xx=In(x1), Yp=In(c.p2), Yj=In(c.j2 if shift else idx(c.j2 + c.K, 2 * c.K)), Yx=In(x2),
                    op=Out(np.int32, want["indptr"]), oj=Out(np.int32, want["indices"]), ox=Out(np.float64, want["values"]))
        tail = [B("Xp"), B("Xj"), B("Xx"), B("Yp"), B("Yj"), B("Yx"), F64, c.nnz + c.nnz2, B("op"), B("oj"), B("ox")]
        if shift:
            return single("mxd_csr_cbind_shift", [c.m, c.m, c.K] + tail, bufs)
        return single("mxd_csr_cbind", [c.m, c.m] + tail, bufs)
    return make


def svec_of(v, seed, length, n, sorted_=True):
    """n positions (1-based) of a sparse vector of `length` and exact values"""
    rng = np.random.default_rng([seed, v])
    at = rng.permutation(length)[:n]
    return idx((np.sort(at) if sorted_ else at) + 1, length + 1, ascending=sorted_), ivals(rng, n)


def rbind_parts(v):
    p, j, x = csr(v, 31, 40, 50)
    vi, vx = svec_of(v, 32, 50, 9)
    want = O.concat_csr_batch([(0, p, j, x, 40), (3, None, vi, vx, 1)], 0)
    return p, j, x, vi, vx, want


def rbind_append(v):
    p, j, x, vi, vx, want = rbind_parts(v)
    bufs = dict(p=In(p), j=In(j), x=In(x), vi=In(vi), vx=In(vx), op=Out(np.int32, want["indptr"], after=1),
                oj=Out(np.int32, want["indices"], after=1), ox=Out(np.float64, want["values"], after=1))
    out = [B("op"), B("oj"), B("ox")]
    return Case(bufs, [
        Step("mxd_csr_rbind_append", [0, B("p"), B("j"), B("x"), 40, j.size, 0, 0, 0] + out, late=("p", "j", "x")),
        Step("mxd_csr_rbind_append", [3, None, B("vi"), B("vx"), 1, vi.size, 0, 40, j.size] + out, late=("vi", "vx"))])


def rbind_batch(v):
    p, j, x, vi, vx, want = rbind_parts(v)

    def table(P):
        items = (_lib.RbindItem * 2)()
        items[0] = _lib.RbindItem(0, 40, P("p"), P("j"), P("x"), j.size, 0, 0)
        items[1] = _lib.RbindItem(3, 1, None, P("vi"), P("vx"), vi.size, j.size, 40)
        return np.frombuffer(bytes(items), dtype=np.uint8).copy()
    bufs = dict(p=In(p), j=In(j), x=In(x), vi=In(vi), vx=In(vx), items=In(table, nbytes=2 * C.sizeof(_lib.RbindItem)),
                op=Out(np.int32, want["indptr"]), oj=Out(np.int32, want["indices"]), ox=Out(np.float64, want["values"]))
    return single("mxd_csr_rbind_batch", [B("items"), 2, 0, 41, j.size + vi.size, B("op"), B("oj"), B("ox")], bufs,
                  late=("p", "j", "x", "vi", "vx"))


def coo_rbind_append(v):
    i, j, x = coo(v, 33, 40, 50, 300)
    vi, vx = svec_of(v, 34, 50, 9)
    bufs = dict(i=In(i), j=In(j), x=In(x), vi=In(vi), vx=In(vx),
                oi=Out(np.int32, np.concatenate([i, np.full(9, 40)]), after=1),
                oj=Out(np.int32, np.concatenate([j, vi - 1]), after=1), ox=Out(np.float64, np.concatenate([x, vx]), after=1))
    out = [B("oi"), B("oj"), B("ox")]
    return Case(bufs, [
        Step("mxd_coo_rbind_append", [0, B("i"), B("j"), B("x"), 300, 0, 0, 0] + out, late=("i", "j", "x")),
        Step("mxd_coo_rbind_append", [3, None, B("vi"), B("vx"), 9, 0, 40, 300] + out, late=("vi", "vx"))])


def cbind_svec(v):
    p, j, x = csr(v, 35, 40, 50)
    vi, vx = svec_of(v, 36, 40, 11)
    has = np.zeros(40, dtype=bool)
    has[vi - 1] = True
    val = np.zeros(40)
    val[vi - 1] = vx
    oj, ox, op = [], [], [0]
    for r in range(40):
        oj += list(j[p[r]:p[r + 1]]) + ([50] if has[r] else [])
        ox += list(x[p[r]:p[r + 1]]) + ([val[r]] if has[r] else [])
        op.append(len(oj))
    return single("mxd_csr_cbind_svec", [40, 50, B("p"), B("j"), B("x"), 0, B("vi"), B("vx"), 3, 11, 40, 0, 0, B("op"),
                                         B("oj"), B("ox")],
                  dict(p=In(p), j=In(j), x=In(x), vi=In(vi), vx=In(vx), op=Out(np.int32, op), oj=Out(np.int32, oj),
                       ox=Out(np.float64, ox)))


def spmv_svec(v):
    c = rgc(v)
    x = rg_values(c, v)
    yi, yv = svec_of(v, 37, c.K, 200)
    out = O.matmul_csr_svec_numeric(c.p, c.j, x, yi, yv)
    return single("mxd_spmv_csr_svec", [c.m, c.nnz, B("p"), B("j"), B("x"), B("yi"), 200, B("yv"), 0, B("out")],
                  dict(p=In(c.p), j=In(c.j), x=In(x), yi=In(yi), yv=In(yv), out=Out(np.float64, out, rtol=1e-12)))


def csr_by_dense(v):
    c = rgc(v)
    x = rg_values(c, v)
    D = np.asfortranarray(np.random.default_rng([38, v]).integers(-8, 9, size=(c.m, c.K)) / 8.0)
    out = O.multiply_csr_by_dense_elemwise_double(c.p, c.j, x, D)
    return single("mxd_csr_by_dense_elemwise", [c.m, c.nnz, B("p"), B("j"), B("x"), B("D"), 0, B("out")],
                  dict(p=In(c.p), j=In(c.j), x=In(x), D=In(D.reshape(-1, order="F")), out=Out(np.float64, out)))


def csr_by_dvec(v):
    c = rgc(v)
    x = rg_values(c, v)
    d = np.random.default_rng([39, v]).integers(1, 9, size=c.m) / 8.0
    out = O.multiply_csr_by_dvec_no_NAs_numeric(c.p, c.j, x, d, c.K, True, False, False, False, False, True)
    return single("mxd_csr_by_dvec", [c.m, c.K, c.nnz, B("p"), B("j"), B("x"), B("d"), c.m, _lib.MX_DV_MULTIPLY, 1, B("out")],
                  dict(p=In(c.p), j=In(c.j), x=In(x), d=In(d), out=Out(np.float64, out)))


def sort_rows(v):
    c = rgc(v)
    x = rg_values(c, v)
    js, perm = RC.shuffled_rows(c, seed=1 + v)
    return single("mxd_csr_sort_rows", [c.m, c.nnz, B("p"), B("j"), B("x"), F64, B("tj"), B("tx")],
                  dict(p=In(c.p), j=IO(idx(js, c.K), c.j), x=IO(x[perm], x), tj=Ws(4 * c.nnz), tx=Ws(8 * c.nnz)))


def csr_by_svec(v):
    c = rgc(v)
    x = rg_values(c, v)
    vi, vx = svec_of(v, 40, c.m, 30)
    scale = np.zeros(c.m)
    scale[vi - 1] = vx
    keep = np.zeros(c.m, dtype=bool)
    keep[vi - 1] = True
    lens = np.where(keep, np.diff(c.p), 0)
    op = np.zeros(c.m + 1, dtype=np.int32)
    op[1:] = np.cumsum(lens)
    sel = keep[rows_of(c.p)]
    oj, ox = c.j[sel], (x * scale[rows_of(c.p)])[sel]
    head = [c.m, c.K, c.nnz, B("p")]
    vec = [B("vi"), 30, B("vx"), c.m, 0, B("ws"), B("op")]
    bufs = dict(p=In(c.p), j=In(c.j), x=In(x), vi=In(vi), vx=In(vx), ws=Ws(L().mxd_csr_by_svec_workspace_bytes(c.m)),
                op=Out(np.int32, op), oj=Out(np.int32, oj), ox=Out(np.float64, ox))
    return Case(bufs, [
        Step("mxd_csr_by_svec_count", head + [B("x")] + vec + [H("nnz"), H("x_na")], late=("p", "vi"), waits=True,
             host=dict(nnz=int(oj.size), x_na=0)),
        Step("mxd_csr_by_svec_fill", head + [B("j"), B("x")] + vec + [B("oj"), B("ox")], late=("x", "vx"))])


# ---- scans, checks, conversions ------------------------------------------------------------------------------------------------
def scan(v):
    counts = i32(np.random.default_rng([41, v]).integers(0, 6, size=20001))
    out = np.zeros(counts.size + 1, dtype=np.int64)
    out[1:] = np.cumsum(counts)
    return single("mxd_exclusive_scan_i32", [B("c"), counts.size, B("out"), B("total"), B("ws")],
                  dict(c=In(counts), out=Out(np.int32, out), total=Out(np.int64, out[-1:]),
                       ws=Ws(L().mxd_scan_workspace_bytes(counts.size))))


def check_is_seq(v):
    seq = i32(np.arange(5, 3005))
    if v:
        seq[1777] += 1
    flag = int(O.check_is_seq(seq))
    assert flag == 1 - v
    return single("mxd_check_is_seq", [B("idx"), seq.size, 0, B("ws"), H("flag", C.c_int)],
                  dict(idx=In(seq), ws=Ws(4)), waits=True, host=dict(flag=flag))


def rows_sorted(v):
    c = rgc(0)
    j = idx(RC.shuffled_rows(c)[0], c.K) if v else c.j
    flag = int(O.check_indices_are_sorted(c.p, j))
    assert flag == 1 - v
    return single("mxd_csr_rows_sorted", [c.m, B("p"), B("j"), B("ws"), H("flag", C.c_int)],
                  dict(p=In(c.p), j=In(j), ws=Ws(4)), waits=True, host=dict(flag=flag))


def validate_indices(v):
    p, j, _ = csr(0, 42, 40, 50)
    j = i32(j).copy()
    want = 0
    if not v:                                            # the real operand is the bad one: validation only reads
        j[3], j[17] = -4, 50
        want = _lib.MX_BAD_NEGATIVE | _lib.MX_BAD_BOUND
    return single("mxd_validate_indices", [B("j"), j.size, 50, B("p"), 41, 40, B("ws"), H("flags", C.c_int)],
                  dict(p=In(p), j=In(j), ws=Ws(4)), waits=True, host=dict(flags=want))


T_M, T_N, T_NNZ = 60, 50, 4000          # 3000 cells for 4000 entries: repeated cells, and more than one radix tile


def transpose(v):
    i, j, x = coo(v, 43, T_M, T_N, T_NNZ)
    order = np.argsort(i, kind="stable")
    i, j, x = i[order], j[order], x[order]
    p = np.zeros(T_M + 1, dtype=np.int32)
    p[1:] = np.cumsum(np.bincount(i, minlength=T_M))
    tp, tj, tx = merged_csr(j, i, x, T_N)
    return single("mxd_csr_transpose", [T_M, T_N, B("p"), B("j"), B("x"), F64, T_NNZ, B("op"), B("oj"), B("ox"), B("ws"),
                                        H("nnz")],
                  dict(p=In(p), j=In(j), x=In(x), ws=Ws(L().mxd_csr_transpose_workspace_bytes(T_NNZ)),
                       op=Out(np.int32, tp), oj=Out(np.int32, tj, tail="any", alloc=T_NNZ),
                       ox=Out(np.float64, tx, tail="any", alloc=T_NNZ)), waits=True, host=dict(nnz=int(tj.size)))


def coo_to_csr(v):
    i, j, x = coo(v, 44, T_M, T_N, T_NNZ)
    tp, tj, tx = merged_csr(i, j, x, T_M)
    return single("mxd_coo_to_csr", [T_M, T_N, B("i"), B("j"), B("x"), F64, T_NNZ, B("op"), B("oj"), B("ox"), B("ws"),
                                     H("nnz")],
                  dict(i=In(i), j=In(j), x=In(x), ws=Ws(L().mxd_coo_to_csr_workspace_bytes(T_NNZ, T_N)),
                       op=Out(np.int32, tp), oj=Out(np.int32, tj, tail="any", alloc=T_NNZ),
                       ox=Out(np.float64, tx, tail="any", alloc=T_NNZ)), waits=True, host=dict(nnz=int(tj.size)))


def csr_to_coo(v):
    c = rgc(v)
    return single("mxd_csr_to_coo", [c.m, c.nnz, B("p"), B("rows")], dict(p=In(c.p), rows=Out(np.int32, rows_of(c.p))))


def coo_sort(v):
    i, j, x = coo(v, 45, T_M, T_N, T_NNZ)
    si, sj, sx = CM.model(i, j, x)
    return single("mxd_coo_sort", [B("i"), B("j"), B("x"), T_NNZ, F64, B("ws"), H("was_sorted", C.c_int)],
                  dict(i=IO(i, si), j=IO(j, sj), x=IO(x, sx), ws=Ws(L().mxd_coo_sort_workspace_bytes(T_NNZ))),
                  waits=True, host=dict(was_sorted=0))


def sort_vector(v):
    rng = np.random.default_rng([46, v])
    ii, xx = i32(rng.integers(0, 3000, size=T_NNZ)), ivals(rng, T_NNZ)
    order = np.argsort(ii, kind="stable")
    return single("mxd_sort_vector_indices", [B("i"), B("x"), T_NNZ, F64, B("ws"), H("was_sorted_host", C.c_int)],
                  dict(i=IO(ii, ii[order]), x=IO(xx, xx[order]), ws=Ws(L().mxd_sort_vector_indices_workspace_bytes(T_NNZ))),
                  waits=True, host=dict(was_sorted_host=0))


# ---- CSC / dense / COO products ---------------------------------------------------------------------------------------------------
def csc_by_dense(v):
    p, i, x = csr(v, 47, 30, 41)                          # the CSR arrays of the transpose: 30 columns, 41 rows
    D = np.asfortranarray(np.random.default_rng([48, v]).integers(-8, 9, size=(41, 30)) / 8.0)
    out = x * D[i, rows_of(p)]
    return single("mxd_csc_by_dense_elemwise", [30, 41, i.size, B("p"), B("i"), B("x"), B("D"), 0, B("out")],
                  dict(p=In(p), i=In(i), x=In(x), D=In(D.reshape(-1, order="F")), out=Out(np.float64, out)))


def csc_dense_na(v):
    nrows, ncols = 41, 30
    p, i, x = csr(v, 49, ncols, nrows)
    rng = np.random.default_rng([50, v])
    D = np.asfortranarray(rng.integers(-8, 9, size=(nrows, ncols)) / 8.0)
    D[rng.random(D.shape) < 0.1] = NA_REAL
    stored = np.zeros((nrows, ncols), dtype=bool)
    stored[i, rows_of(p)] = True
    val = np.zeros((nrows, ncols))
    val[i, rows_of(p)] = x
    na = np.isnan(D)
    take = stored | na
    with np.errstate(invalid="ignore"):
        out = np.where(stored, val * D, NA_REAL)
    oc, orow = np.nonzero(take.T)                         # by column, rows ascending
    op = np.zeros(ncols + 1, dtype=np.int32)
    op[1:] = np.cumsum(take.sum(axis=0))
    head = [nrows, ncols, i.size, B("p"), B("i")]
    bufs = dict(p=In(p), i=In(i), x=In(x), D=In(D.reshape(-1, order="F")),
                ws=Ws(L().mxd_csc_dense_na_workspace_bytes(nrows, ncols)), op=Out(np.int32, op),
                oi=Out(np.int32, orow), ox=Out(np.float64, out[orow, oc]))
    return Case(bufs, [
        Step("mxd_csc_dense_na_count", head + [B("D"), 0, B("ws"), H("nnz"), H("outside")], late=("p", "i", "D"),
             waits=True, host=dict(nnz=int(orow.size), outside=int((na & ~stored).any()))),
        Step("mxd_csc_dense_na_fill", head + [B("x"), B("D"), 0, B("ws"), B("op"), B("oi"), B("ox")], late=("x",))])


def dense_by_svec_dense(v):
    nrows, ncols, length = 13, 5, 7                       # the length neither covers nor divides: the flat dense route
    X = np.asfortranarray(np.random.default_rng([51, v]).integers(-8, 9, size=(nrows, ncols)) / 8.0)
    vi, vx = svec_of(v, 52, length, 4, sorted_=False)
    assert DM.route(nrows, ncols, length) == "D"
    want = DM.model("numeric", X, vi, vx, length, 0)[0]["X_dense"]
    return single("mxd_dense_by_svec_dense", [nrows, ncols, B("X"), 0, B("vi"), 4, B("vx"), length, 0, B("ws"), B("out")],
                  dict(X=In(X.reshape(-1, order="F")), vi=In(vi), vx=In(vx),
                       ws=Ws(L().mxd_dense_by_svec_workspace_bytes(0, length)),
                       out=Out(np.float64, want.reshape(-1, order="F"))))


def dense_by_svec_csr(v):
    nrows, ncols = 26, 5                                   # length == nrows: a CSR result
    X = np.asfortranarray(np.random.default_rng([53, v]).integers(-8, 9, size=(nrows, ncols)) / 8.0)
    vi, vx = svec_of(v, 54, nrows, 9, sorted_=False)
    want = DM.model("numeric", X, vi, vx, nrows, 0)[0]
    bufs = dict(X=In(X.reshape(-1, order="F")), vi=In(vi), vx=In(vx),
                ws=Ws(L().mxd_dense_by_svec_workspace_bytes(nrows, nrows)), op=Out(np.int32, want["indptr"]),
                oj=Out(np.int32, want["indices"]), ox=Out(np.float64, want["values"]))
    return Case(bufs, [
        Step("mxd_dense_by_svec_count", [nrows, ncols, B("X"), 0, B("vi"), 9, nrows, 0, B("ws"), B("op"), H("nnz")],
             late=("vi",), waits=True, host=dict(nnz=int(want["indices"].size))),
        Step("mxd_dense_by_svec_fill", [nrows, ncols, B("X"), 0, B("vx"), nrows, 0, B("ws"), B("op"), B("oj"), B("ox")],
             late=("X", "vx"))])


def coo_by_dense(v):
    i, j, x = coo(v, 55, 41, 30, 500)
    D = np.asfortranarray(np.random.default_rng([56, v]).integers(-8, 9, size=(41, 30)) / 8.0)
    return single("mxd_coo_by_dense", [500, B("i"), B("j"), B("x"), B("D"), 41, 30, 0, B("out")],
                  dict(i=In(i), j=In(j), x=In(x), D=In(D.reshape(-1, order="F")), out=Out(np.float64, x * D[i, j])))


def coo_by_dvec(v):
    i, j, x = coo(v, 57, 41, 30, 500)
    d = np.random.default_rng([58, v]).integers(1, 9, size=41) / 8.0
    out = x * d[(i.astype(np.int64) + j.astype(np.int64) * 41) % 41]
    return single("mxd_coo_by_dvec", [41, 30, 500, B("i"), B("j"), B("x"), B("d"), 41, _lib.MX_DV_MULTIPLY, 1, B("out")],
                  dict(i=In(i), j=In(j), x=In(x), d=In(d), out=Out(np.float64, out)))


def csr_by_coo(v):
    p, j, x = csr(v, 59, 40, 50, 0.3)
    yi, yj, yx = coo(v, 60, 40, 50, 600)
    yx = yx.copy()
    yx[::7] = 0.0
    X = dense_of(p, j, x, 50)
    keep = (yx != 0) & (X[yi, yj] != 0)
    head = [0, 40, 50, B("p"), B("j"), B("x"), B("yi"), B("yj"), B("yx"), 600, B("ws")]
    ins = ("p", "j", "x", "yi", "yj", "yx")
    bufs = dict(p=In(p), j=In(j), x=In(x), yi=In(yi), yj=In(yj), yx=In(yx), ws=Ws(L().mxd_csr_by_coo_workspace_bytes(600)),
                oi=Out(np.int32, yi[keep]), oj=Out(np.int32, yj[keep]), ox=Out(np.float64, (X[yi, yj] * yx)[keep]))
    return Case(bufs, [
        Step("mxd_csr_by_coo_count", head + [H("nnz")], late=ins, waits=True, host=dict(nnz=int(keep.sum()))),
        Step("mxd_csr_by_coo_fill", head + [B("oi"), B("oj"), B("ox")], late=("x", "yx"))])


# ---- outer products -------------------------------------------------------------------------------------------------------------------
def one_column(v, seed, m):
    """the CSR triple of a one-column matrix: rows with no entry or one"""
    rng = np.random.default_rng([seed, v])
    has = rng.random(m) < 0.6
    p = np.zeros(m + 1, dtype=np.int32)
    p[1:] = np.cumsum(has)
    return p, has, ivals(rng, int(has.sum()))


def outer_dense(v):
    m, dim = 45, 17
    p, has, x = one_column(v, 61, m)
    vec = np.random.default_rng([62, v]).integers(-8, 9, size=dim) / 8.0
    op = np.zeros(m + 1, dtype=np.int32)
    op[1:] = np.cumsum(has * dim)
    oj = np.tile(np.arange(dim), x.size)
    ox = 0.0 + np.outer(x, vec).reshape(-1)
    bufs = dict(p=In(p), x=In(x), vec=In(vec), ws=Ws(L().mxd_csr_outer_dense_workspace_bytes(m)), op=Out(np.int32, op),
                oj=Out(np.int32, oj), ox=Out(np.float64, ox))
    return Case(bufs, [
        Step("mxd_csr_outer_dense_count", [m, dim, B("p"), B("ws"), B("op"), H("nnz")], late=("p",), waits=True,
             host=dict(nnz=int(oj.size))),
        Step("mxd_csr_outer_dense_fill", [m, dim, x.size, B("p"), B("x"), B("vec"), F64, B("op"), B("oj"), B("ox")],
             late=("x", "vec"))])


def outer_svec(v):
    m, ylen, ny = 45, 23, 6
    p, has, x = one_column(v, 63, m)
    yi, yv = svec_of(v, 64, ylen, ny)
    rows = np.flatnonzero(has)
    per_col = np.zeros(ylen, dtype=np.int64)
    per_col[yi - 1] = rows.size
    op = np.zeros(ylen + 1, dtype=np.int32)
    op[1:] = np.cumsum(per_col)
    bufs = dict(p=In(p), x=In(x), yi=In(yi), yv=In(yv), ws=Ws(L().mxd_csr_outer_svec_workspace_bytes(m, ylen)),
                op=Out(np.int32, op), oi=Out(np.int32, np.tile(rows, ny)), ox=Out(np.float64, np.outer(yv, x).reshape(-1)))
    return Case(bufs, [
        Step("mxd_csr_outer_svec_count", [m, x.size, B("p"), B("x"), B("yi"), ny, ylen, B("ws"), B("op"), H("nonempty"),
                                          H("nnz")], late=("p", "x", "yi"), waits=True,
             host=dict(nonempty=int(rows.size), nnz=int(rows.size * ny))),
        Step("mxd_csr_outer_svec_fill", [m, B("yi"), ny, B("yv"), F64, ylen, int(rows.size), B("ws"), B("op"), B("oi"),
                                         B("ox")], late=("yv",))])


def rowvec_by_csc(v):
    p, i, x = csr(v, 65, 30, 41)                          # 30 columns of 41 rows
    vec = (np.random.default_rng([66, v]).integers(-8, 9, size=41) / 8.0).astype(np.float32)
    out = np.zeros(30)
    np.add.at(out, rows_of(p), x * vec[i].astype(np.float64))
    return single("mxd_rowvec_by_csc", [30, i.size, B("p"), B("i"), B("x"), B("vec"), B("out")],
                  dict(p=In(p), i=In(i), x=In(x), vec=In(vec), out=Out(np.float32, out.astype(np.float32), rtol=1e-5)))


# ---- the NA-keeping CSR (op) dense vector -----------------------------------------------------------------------------------------
def dvec_na_rows(v):
    m, ncols, Lv = 40, 33, 20
    p, j, x = NM.make_csr(m, ncols, 0.3, 70 + v)
    j = idx(j, ncols)
    d = NM.make_vector(Lv, "*", 72 + v, at=(0, Lv - 1), share=0.1)
    want = NM.model(p, j, x, d, ncols, "*")
    op = _lib.MX_DV_MULTIPLY
    bufs = dict(p=In(p), j=In(j), x=In(x), d=In(d), ws=Ws(L().mxd_csr_by_dvec_na_rows_workspace_bytes(m)),
                op=Out(np.int32, want["indptr"]), oj=Out(np.int32, want["indices"]), ox=Out(np.float64, want["values"]))
    return Case(bufs, [
        Step("mxd_csr_by_dvec_na_rows_count", [m, ncols, j.size, B("p"), B("d"), Lv, op, B("ws"), B("op"), H("nnz")],
             late=("p", "d"), waits=True, host=dict(nnz=int(want["indices"].size))),
        Step("mxd_csr_by_dvec_na_rows_fill", [m, ncols, j.size, B("p"), B("j"), B("x"), B("d"), Lv, op, B("op"), B("oj"),
                                              B("ox")], late=("j", "x", "d"))])


def dvec_na_flat(v):
    m, ncols, Lv = 40, 33, 41
    p, j, x = NM.make_csr(m, ncols, 0.3, 74 + v, positive=True)
    j = idx(j, ncols)
    d = NM.make_vector(Lv, "^", 76 + v, at=(0, Lv - 1), share=0.15)      # ^: the fill is 1, +Inf or NA by d
    want = NM.model(p, j, x, d, ncols, "^")
    nsp, cand, new, op = int(NM.special("^", d).sum()), int(want["candidates"]), int(want["new"]), _lib.MX_DV_POWERTO
    assert new > 0
    fill = want["fill"]
    cells = np.stack([rows_of(want["indptr"])[fill], want["indices"][fill].astype(np.int64)])
    vals = want["values"][fill]

    def same_cells(raw):
        r, c = raw["orow"][:4 * new].view(np.int32), raw["ocol"][:4 * new].view(np.int32)
        x_ = raw["oval"][:8 * new].view(np.float64)
        order = np.lexsort((c, r))
        assert np.array_equal(np.stack([r[order], c[order]]), cells), "the new cells are not the oracle's"
        assert ST.same(x_[order], vals), "the new cells' values are not the oracle's"
    bufs = dict(p=In(p), j=In(j), d=In(d), sws=Ws(L().mxd_dvec_na_special_workspace_bytes(Lv)),
                cws=Ws(L().mxd_dvec_na_cells_workspace_bytes(cand)), orow=Out(np.int32, [], tail="any", alloc=new),
                ocol=Out(np.int32, [], tail="any", alloc=new), oval=Out(np.float64, [], tail="any", alloc=new))
    return Case(bufs, [
        Step("mxd_dvec_na_special", [m, ncols, B("d"), Lv, op, B("sws"), H("nspecial"), H("candidates")], late=("d",),
             waits=True, host=dict(nspecial=nsp, candidates=cand)),
        Step("mxd_dvec_na_cells_count", [m, ncols, j.size, B("p"), B("j"), Lv, B("sws"), nsp, cand, B("cws"), H("new")],
             late=("p", "j"), waits=True, host=dict(new=new)),
        Step("mxd_dvec_na_cells_fill", [m, ncols, B("d"), Lv, op, B("sws"), nsp, cand, B("cws"), B("orow"), B("ocol"),
                                        B("oval")], late=("d",))],
        checks=[(("orow", "ocol", "oval"), same_cells)])


def join_disjoint(v):
    p1, j1, x1 = csr(v, 78, 40, 25)
    p2, j2, x2 = csr(v, 79, 40, 25)
    j1, j2 = idx(2 * j1, 50), idx(2 * j2 + 1, 50)                # even and odd columns: disjoint patterns, sorted rows
    r = np.concatenate([rows_of(p1), rows_of(p2)])
    c, x = np.concatenate([j1, j2]), np.concatenate([x1, x2])
    order = np.lexsort((c, r))
    return single("mxd_csr_join_disjoint", [40, B("p1"), B("j1"), B("x1"), j1.size, B("p2"), B("j2"), B("x2"), j2.size,
                                            B("op"), B("oj"), B("ox")],
                  dict(p1=In(p1), j1=In(j1), x1=In(x1), p2=In(p2), j2=In(j2), x2=In(x2), op=Out(np.int32, p1 + p2),
                       oj=Out(np.int32, c[order]), ox=Out(np.float64, x[order])))


# ---- COO slices, single cells, NA injection ------------------------------------------------------------------------------------------
def coo_slice(v):
    nrow, ncol, nnz, lo, hi = 40, 50, 500, 10, 39
    i, j, x = coo(v, 80, nrow, ncol, nnz)
    take = idx(np.random.default_rng([81, v]).integers(1, nrow + 1, size=60), nrow + 1)       # 1-based, with repeats
    take[0] = nrow
    nmap = nrow + 1
    start, pos = colmap(take, nmap)
    oi, oj, ox = [], [], []
    for k in range(nnz):
        if lo <= j[k] <= hi:
            for a in pos[start[i[k] + 1]:start[i[k] + 2]]:
                oi.append(a); oj.append(j[k] - lo); ox.append(x[k])         # noqa: E702
    ai = S(lambda P: _lib.CooAxis(_lib.MX_AXIS_MAP, 0, 0, 0, nmap, P("start"), P("pos")), names=("start", "pos"))
    aj = S(lambda P: _lib.CooAxis(_lib.MX_AXIS_AFFINE, lo, hi, 0, 0, None, None))
    bufs = dict(i=In(i), j=In(j), x=In(x), take=In(take), start=Out(np.int32, start), pos=Out(np.int32, pos),
                mws=Ws(L().mxd_colmap_workspace_bytes(nmap)), ws=Ws(L().mxd_coo_slice_workspace_bytes(nnz)),
                oi=Out(np.int32, oi), oj=Out(np.int32, oj), ox=Out(np.float64, ox))
    return Case(bufs, [
        Step("mxd_colmap_build", [B("take"), take.size, nmap, B("start"), B("pos"), B("mws")], late=("take",), pre=True),
        Step("mxd_coo_slice_count", [nrow, ncol, B("i"), B("j"), nnz, ai, aj, B("ws"), H("nnz")], late=("i", "j"),
             waits=True, host=dict(nnz=len(oi))),
        Step("mxd_coo_slice_fill", [nrow, ncol, B("i"), B("j"), B("x"), F64, nnz, ai, aj, B("ws"), B("oi"), B("oj"),
                                    B("ox")], late=("x",))])


def coo_single(v):
    i, j, x = coo(v, 82, 40, 50, 500)
    r, c = 7, 9
    if v:
        i[(i == r) & (j == c)] = r + 1                   # the stale operand does not store the cell
        k, val = -1, b""
    else:
        i[[123, 321]], j[[123, 321]] = r, c
        k = int(np.flatnonzero((i == r) & (j == c))[0])
        val = x[k:k + 1].tobytes()
    return single("mxd_coo_single", [B("i"), B("j"), B("x"), F64, 500, r, c, B("ws"), H("k"), H("value", nbytes=8)],
                  dict(i=In(i), j=In(j), x=In(x), ws=Ws(L().mxd_coo_single_workspace_bytes())), waits=True,
                  host=dict(k=k, value=val))


def csr_single(v):
    p, j, x = csr(v, 83, 40, 50, 0.3)
    r, c = 11, int(csr(0, 83, 40, 50, 0.3)[1][csr(0, 83, 40, 50, 0.3)[0][11] + 2])      # a cell variant 0 stores
    found, val = SM.extract_single_val_csr(p, j, x, r, c)
    k = int(p[r] + np.flatnonzero(j[p[r]:p[r + 1]] == c)[0]) if found else -1
    assert found or v
    return single("mxd_csr_single", [40, B("p"), B("j"), B("x"), F64, j.size, r, c, B("ws"), H("k"), H("value", nbytes=8)],
                  dict(p=In(p), j=In(j), x=In(x), ws=Ws(16)), waits=True,
                  host=dict(k=k, value=np.float64(val).tobytes() if found else b""))


def inject_na(v):
    nrow, ncol, nnz = 40, 50, 500
    i, j, x = coo(v, 84, nrow, ncol, nnz)
    rng = np.random.default_rng([85, v])
    rna, cna = idx(np.sort(rng.permutation(nrow)[:4]), nrow, True), idx(np.sort(rng.permutation(ncol)[:3]), ncol, True)
    oi, oj, ox = SM.inject_coo(i, j, x, rna, cna, nrow, ncol)
    head = [nrow, ncol, B("i"), B("j")]
    sel = [B("rna"), 4, B("cna"), 3, B("ws"), B("maps")]
    bufs = dict(i=In(i), j=In(j), x=In(x), rna=In(rna), cna=In(cna), ws=Ws(L().mxd_compact_workspace_bytes(nnz)),
                maps=Ws(4 * (4 + nrow + ncol + max(nrow, ncol))), oi=Out(np.int32, oi), oj=Out(np.int32, oj),
                ox=Out(np.float64, ox))
    return Case(bufs, [
        Step("mxd_coo_inject_na_count", head + [nnz] + sel + [H("nnz")], late=("i", "j", "rna", "cna"), waits=True,
             host=dict(nnz=int(oi.size))),
        Step("mxd_coo_inject_na_fill", head + [B("x"), F64, nnz] + sel + [B("oi"), B("oj"), B("ox")], late=("x",))])


def repeat_indices(v):
    rng = np.random.default_rng([86, v])
    ix, rem = idx(np.sort(rng.permutation(37)[:12]), 37), idx(np.sort(rng.permutation(37)[:5]), 37)
    out = SM.repeat_indices(ix, rem, 37, 37 * 9 + 20)
    return single("mxd_repeat_indices", [B("idx"), 12, B("rem"), 5, 37, 37 * 9 + 20, B("out")],
                  dict(idx=In(ix), rem=In(rem), out=Out(np.int32, out)))


def entries_to_dense(v):
    rng = np.random.default_rng([87, v])
    pos, vals = idx(rng.permutation(700)[:90], 700), ivals(rng, 90)
    out = np.zeros(700)
    out[pos] = vals
    return single("mxd_entries_to_dense_vector", [B("pos"), B("vals"), F64, 90, B("out"), F64, 700],
                  dict(pos=In(pos), vals=In(vals), out=Out(np.float64, out)))


# ---- assignment ---------------------------------------------------------------------------------------------------------------------------
def affine(lo, hi):
    return S(lambda P: _lib.CooAxis(_lib.MX_AXIS_AFFINE, lo, hi, 0, 0, None, None))


def assign_scalar(v):
    m, K = 40, 50
    p, j, x = csr(v, 88, m, K, 0.3)
    rows, cols, value, avg = np.arange(5, 21), np.arange(10, 31), 2.5, j.size / m
    op, oj, ox = AM.assign_scalar(p, j, x, K, rows, cols, value)
    r = rows_of(p)
    hits = int(((r >= 5) & (r <= 20) & (j >= 10) & (j <= 30)).sum())
    ai, aj = affine(5, 20), affine(10, 30)
    bufs = dict(p=In(p), j=In(j), x=In(x), ws=Ws(L().mxd_gather_workspace_bytes(m)), op=Out(np.int32, op),
                oj=Out(np.int32, oj), ox=Out(np.float64, ox))
    return Case(bufs, [
        Step("mxd_csr_assign_count", [m, K, B("p"), B("j"), j.size, ai, aj, 16, 21, 1, avg, B("op"), B("ws"), H("nnz"),
                                      H("hits")], late=("p", "j"), waits=True, host=dict(nnz=int(oj.size), hits=hits)),
        Step("mxd_csr_assign_fill", [m, K, B("p"), B("j"), B("x"), ai, aj, None, 21, 1, value, avg, B("op"), B("oj"),
                                     B("ox")], late=("x",))])


def replace_rows(v):
    m, K = 40, 50
    p, j, x = csr(v, 89, m, K, 0.3)
    vp, vj, vx = csr(v, 90, 16, K, 0.2)
    op, oj, ox = AM.replace_rows(p, j, x, np.arange(5, 21), vp, vj, vx)
    ai = affine(5, 20)
    bufs = dict(p=In(p), j=In(j), x=In(x), vp=In(vp), vj=In(vj), vx=In(vx), ws=Ws(L().mxd_gather_workspace_bytes(m)),
                op=Out(np.int32, op), oj=Out(np.int32, oj), ox=Out(np.float64, ox))
    return Case(bufs, [
        Step("mxd_csr_replace_rows_count", [m, B("p"), ai, 16, B("vp"), B("op"), B("ws"), H("nnz")], late=("p", "vp"),
             waits=True, host=dict(nnz=int(oj.size))),
        Step("mxd_csr_replace_rows_fill", [m, B("p"), B("j"), B("x"), ai, 16, B("vp"), B("vj"), B("vx"), j.size / m, B("op"),
                                           B("oj"), B("ox")], late=("x", "vx"))])


def assign_col(v):
    m, K, col, length = 40, 50, 17, 20
    p, j, x = csr(v, 91, m, K, 0.3)
    rng = np.random.default_rng([92, v])
    ii, xx = idx(np.sort(rng.permutation(length)[:8]), length, True), ivals(rng, 8)
    op, oj, ox = VM.assign_col(p, j, x, col, ii, VM.bits(xx), length)
    changed, avg = int((np.diff(op) != np.diff(p)).sum()), j.size / m
    assert changed > 0
    bufs = dict(p=In(p), j=In(j), x=In(x), ii=In(ii), xx=In(xx), ws=Ws(L().mxd_gather_workspace_bytes(m)),
                op=Out(np.int32, op), oj=Out(np.int32, oj), ox=Out(np.float64, ox))
    return Case(bufs, [
        Step("mxd_csr_assign_col_count", [m, K, B("p"), B("j"), j.size, col, B("ii"), 8, length, avg, B("op"), B("ws"),
                                          H("nnz"), H("changed")], late=("p", "j", "ii"), waits=True,
             host=dict(nnz=int(oj.size), changed=changed)),
        Step("mxd_csr_assign_col_fill", [m, K, B("p"), B("j"), B("x"), col, B("ii"), B("xx"), 8, length, avg, B("op"),
                                         B("oj"), B("ox")], late=("x", "xx"))])


def expand_pattern(v):
    rng = np.random.default_rng([93, v])
    length, reps = 37, 9
    ii, xx = idx(np.sort(rng.permutation(length)[:12]), length, True), ivals(rng, 12)
    t = np.arange(12 * reps)
    return single("mxd_csr_expand_pattern_row", [B("ii"), B("xx"), 12, length, reps, B("rp"), B("rj"), B("rx")],
                  dict(ii=In(ii), xx=In(xx), rp=Out(np.int32, [0, 12 * reps]),
                       rj=Out(np.int32, ii[t % 12] + length * (t // 12)), rx=Out(np.float64, xx[t % 12])))


# ---- compaction ---------------------------------------------------------------------------------------------------------------------------
def compact(v):
    p, j, x = csr(v, 94, 100, 200, 0.25)                  # about 5000 entries: more than one tile
    x = x.copy()
    x[np.random.default_rng([95, v]).random(x.size) < 0.3] = 0.0
    n = x.size
    keep = x != 0
    before = np.concatenate([[0], np.cumsum(keep)])
    args = [n, B("x"), F64, _lib.MX_KEEP_NONZERO, None]
    bufs = dict(p=In(p), j=In(j), x=In(x), ws=Ws(L().mxd_compact_workspace_bytes(n)), oj=Out(np.int32, j[keep]),
                ox=Out(np.float64, x[keep]), op=Out(np.int32, before[p]))
    return Case(bufs, [
        Step("mxd_compact_count", args + [B("ws"), H("kept")], late=("x",), waits=True, host=dict(kept=int(keep.sum()))),
        Step("mxd_compact_fill", args + [B("j"), None, 100, B("p"), B("ws"), B("oj"), None, B("ox"), B("op")],
             late=("x", "j", "p"))])


def dense_to_svec(v):
    rng = np.random.default_rng([96, v])
    n = 5000
    d = ivals(rng, n)
    d[rng.random(n) < 0.6] = 0.0
    keep = d != 0
    bufs = dict(d=In(d), ws=Ws(L().mxd_compact_workspace_bytes(n)), oi=Out(np.int32, np.flatnonzero(keep) + 1),
                ox=Out(np.float64, d[keep]))
    return Case(bufs, [
        Step("mxd_dense_to_svec_count", [n, B("d"), F64, B("ws"), H("kept")], late=("d",), waits=True,
             host=dict(kept=int(keep.sum()))),
        Step("mxd_dense_to_svec_fill", [n, B("d"), F64, B("ws"), B("oi"), B("ox")], late=("d",))])


ROWS = [Row(name, make) for name, make in [
    ("spmm_rowwave", spmm_ex(_lib.MX_SPMM_ROWWAVE)), ("spmm_slab", spmm_ex(_lib.MX_SPMM_SLAB)),
    ("spmm_auto", spmm_ex(_lib.MX_SPMM_AUTO)), ("spmm_planned_packed", spmm_ex(_lib.MX_SPMM_PLANNED)),
    ("spmm_slab_f32", spmm_ex(_lib.MX_SPMM_SLAB, np.float32, 1)), ("spmm_plain_f32", spmm_plain),
    ("spmm_plan", spmm_plan), ("spmm_plan_copy", spmm_plan_copy),
    ("spmv_dvec", spmv_dvec), ("merge", merge), ("values_elemwise", values_elemwise), ("gather", gather),
    ("colrange", colrange), ("colmap", colmap_rows), ("reverse_columns", reverse_columns), ("reversed_iota", reversed_iota),
    ("cbind", cbind(False)), ("cbind_shift", cbind(True)), ("rbind_append", rbind_append), ("rbind_batch", rbind_batch),
    ("coo_rbind_append", coo_rbind_append), ("cbind_svec", cbind_svec), ("spmv_svec", spmv_svec),
    ("csr_by_dense", csr_by_dense), ("csr_by_dvec", csr_by_dvec), ("sort_rows", sort_rows), ("csr_by_svec", csr_by_svec),
    ("scan", scan), ("check_is_seq", check_is_seq), ("rows_sorted", rows_sorted), ("validate_indices", validate_indices),
    ("transpose", transpose), ("coo_to_csr", coo_to_csr), ("csr_to_coo", csr_to_coo), ("coo_sort", coo_sort),
    ("sort_vector", sort_vector), ("csc_by_dense", csc_by_dense), ("csc_dense_na", csc_dense_na),
    ("dense_by_svec_dense", dense_by_svec_dense), ("dense_by_svec_csr", dense_by_svec_csr), ("coo_by_dense", coo_by_dense),
    ("coo_by_dvec", coo_by_dvec), ("csr_by_coo", csr_by_coo), ("outer_dense", outer_dense), ("outer_svec", outer_svec),
    ("rowvec_by_csc", rowvec_by_csc), ("dvec_na_rows", dvec_na_rows), ("dvec_na_flat", dvec_na_flat),
    ("join_disjoint", join_disjoint), ("coo_slice", coo_slice), ("coo_single", coo_single), ("csr_single", csr_single),
    ("inject_na", inject_na), ("repeat_indices", repeat_indices), ("entries_to_dense", entries_to_dense),
    ("assign_scalar", assign_scalar), ("replace_rows", replace_rows), ("assign_col", assign_col),
    ("expand_pattern", expand_pattern), ("compact", compact), ("dense_to_svec", dense_to_svec)]]

# The stream-taking prototypes without a row, each with its reason.  At most 6.
EXCLUDED = {
    "mx_dev_memset": "what the harness itself is made of; checked directly by test_raw_helpers_are_ordered",
    "mx_memcpy_h2d": "what the harness itself is made of; checked directly by test_raw_helpers_are_ordered",
    "mx_memcpy_d2h": "what the harness itself is made of; checked directly by test_raw_helpers_are_ordered",
    "mx_stream_sync": "what the harness itself is made of; checked directly by test_raw_helpers_are_ordered",
}
MAX_EXCLUDED = 6


# ---- the sync contract (P4) ---------------------------------------------------------------------------------------------------------------
def header_text():
    with open(_lib.HEADER_PATH) as f:
        return f.read()


def stream_prototypes(text):
    """name -> parameter list of every prototype of mxgpu.h with a `void *stream` parameter, comments stripped"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    out = {}
    for _, name, params in re.findall(r"([A-Za-z_][\w\s*]*?)\b(mxd?_\w+)\s*\(([^()]*)\)\s*;", text):
        ps = [" ".join(p.split()) for p in params.split(",")]
        if any(re.fullmatch(r"void ?\* ?stream", p) for p in ps):
            out[name] = ps
    return out


def waits_table():
    """entry point -> the set of `waits` flags its steps carry (one flag, but for mxd_spmm_csr_dense_ex)"""
    table = {}
    for row in ROWS:
        for st in row.cases()[0].steps:
            table.setdefault(st.fn, set()).add(st.waits)
    return table


def comment_before(text, name):
    """the comment block that documents a prototype: the nearest one in front of it"""
    at = re.search(rf"\b{name}\s*\(", re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)).start()
    blocks = [m for m in re.finditer(r"^/\*.*?\*/", text, flags=re.S | re.M) if m.end() <= at]      # not the inline ones
    return blocks[-1].group(0)


SYNC_WORDS = r"synchroni[sz]|stream sync|read-back|read back|round trip"


def test_every_stream_prototype_has_a_row():
    protos = stream_prototypes(header_text())
    assert "mxd_spmm_plan_create" in protos and len(protos) == 83, sorted(protos)       # 82 end in the stream
    assert sum(ps[-1].endswith("stream") for ps in protos.values()) == 82
    named = set(fn for row in ROWS for fn in row.entry_points())
    assert len(EXCLUDED) <= MAX_EXCLUDED and all(EXCLUDED.values())
    assert not named & set(EXCLUDED)
    missing, unknown = set(protos) - named - set(EXCLUDED), (named | set(EXCLUDED)) - set(protos)
    assert not missing, f"stream-taking prototypes without a row in ROWS: {sorted(missing)}"
    assert not unknown, f"rows or exclusions that name no stream-taking prototype: {sorted(unknown)}"
    # every entry point is the step under test somewhere, not only a preparation
    tested = set(st.fn for row in ROWS for st in row.cases()[0].steps if not st.pre)
    assert tested == named


def test_sync_contract_is_documented():
    """P4 without a GPU: an entry point with a *_host parameter waits; one that waits says so in its header comment."""
    text, protos, table = header_text(), stream_prototypes(header_text()), waits_table()
    with_host = sorted(n for n, ps in protos.items() if any(re.search(r"\w_host$", p) for p in ps))
    assert len(with_host) == 28
    for name in with_host:
        assert table[name] == {True}, f"{name} has a *_host result: it has to wait for it"
    silent = []
    for name, flags in sorted(table.items()):
        if name == "mxd_spmm_csr_dense_ex":
            assert flags == {True, False}                 # PLANNED waits for the plan's size, the other kernels do not
        else:
            assert len(flags) == 1, f"{name}: the rows disagree on whether it waits"
        if True in flags and not re.search(SYNC_WORDS, comment_before(text, name)):
            silent.append(name)
    assert not silent, f"these wait for the stream, and their comments in mxgpu.h do not say so: {silent}"


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_fixtures_are_valid(row):
    """Both operand sets of a row are valid operands of one shape, and a wrong answer stays in bounds: every index
    vector is non-negative, every indptr-like vector (named p, p1, p2, Xp, Yp, vp) is monotone from 0 and ends inside
    the allocation of its index vector, outputs and workspaces are as long as the larger variant needs."""
    a, b = row.cases()
    pairs = {"p": ("j", "i"), "p1": ("j1",), "p2": ("j2",), "Xp": ("Xj",), "Yp": ("Yj",), "vp": ("vj",)}
    for case in (a, b):
        for name, spec in case.bufs.items():
            alloc = row.payload_bytes(name)
            assert alloc == max(16, -(-max(a.bufs[name].nbytes, b.bufs[name].nbytes) // 16) * 16) >= spec.nbytes
            if isinstance(spec, Out) and not isinstance(spec, IO):
                assert spec.nbytes == (max(spec.alloc, spec.expect.size) + ST.SLACK) * spec.dtype.itemsize
            if isinstance(spec, (In, IO)) and not callable(spec.data) and spec.data.dtype == np.int32:
                data = spec.data
                if row.name != "validate_indices":
                    assert data.size == 0 or data.min() >= 0, f"{row.name}: '{name}' holds a negative index"
                if spec.bound is not None:
                    assert data.size == 0 or data.max() < spec.bound, f"{row.name}: '{name}' leaves [0, {spec.bound})"
                if spec.ascending:
                    assert np.all(np.diff(data) > 0), f"{row.name}: '{name}' is not ascending"
        for pname, jnames in pairs.items():
            if pname in case.bufs and isinstance(case.bufs[pname], In) and case.bufs[pname].data.dtype == np.int32:
                p = case.bufs[pname].data
                assert p[0] == 0 and np.all(np.diff(p) >= 0), f"{row.name}: '{pname}' is not monotone from 0"
                for jn in jnames:
                    if jn in case.bufs and not isinstance(case.bufs[jn], (Ws,)):
                        assert p[-1] * 4 <= row.payload_bytes(jn), f"{row.name}: '{pname}' ends outside '{jn}'"
        for st in case.steps:                                # host totals are asserted before the fill: they are there
            if st.fn.endswith("_count") or st.fn == "mxd_dvec_na_special":
                assert st.waits and st.host, f"{row.name}: {st.fn} returns no total to assert"
    assert [s.fn for s in a.steps] == [s.fn for s in b.steps]


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------------
STEPS = [(row, k) for row in ROWS for k, st in enumerate(row.cases()[0].steps) if not st.pre]
FREE = [(row, k) for row, k in STEPS if not row.cases()[0].steps[k].waits]
step_id = lambda rk: f"{rk[0].name}-{rk[0].cases()[0].steps[rk[1]].fn}"      # noqa: E731


@pytest.mark.gpu
def test_harness_sees_the_wrong_stream(gpu):
    """Torch only.  With the gate pending and a late copy queued behind it, a copy of the operand issued on the null
    stream observes the stale content, the same copy issued on the side stream the real one: the side stream does not
    serialise with the null stream, and a wrong-stream operation shows."""
    import torch
    side = ST.side_stream()
    stale, real = torch.full((4096,), 1, dtype=torch.int32, device="cuda"), torch.full((4096,), 2, dtype=torch.int32, device="cuda")
    operand, on_null, on_side = stale.clone(), torch.zeros_like(stale), torch.zeros_like(stale)
    torch.cuda.synchronize()
    ev = ST.gate(side)
    with torch.cuda.stream(side):
        operand.copy_(real, non_blocking=True)
    on_null.copy_(operand)                                   # the null stream does not wait for the side stream
    torch.cuda.current_stream().synchronize()
    ST.pending(ev, "after the null-stream copy")
    with torch.cuda.stream(side):
        on_side.copy_(operand, non_blocking=True)
    ST.pending(ev, "after the side-stream copy was queued")
    side.synchronize()
    assert bool((on_null == 1).all()), "the null stream waited for the side stream: the harness cannot see a wrong stream"
    assert bool((on_side == 2).all()), "the side stream did not order its own copies"


@pytest.mark.gpu
@pytest.mark.parametrize("rk", STEPS, ids=[step_id(rk) for rk in STEPS])
def test_ordered(gpu, rk):
    ST.run_ordered(*rk)


@pytest.mark.gpu
@pytest.mark.parametrize("rk", FREE, ids=[step_id(rk) for rk in FREE])
def test_reuse(gpu, rk):
    ST.run_reuse(*rk)


@pytest.mark.gpu
def test_raw_helpers_are_ordered(gpu):
    """mx_dev_memset, mx_memcpy_d2h, mx_memcpy_h2d and mx_stream_sync on the side stream behind the gate: each takes
    effect after the work queued before it, none of the first three waits for it (the host buffers are pinned), and
    mx_stream_sync returns only once the gate has drained."""
    import torch
    lib, side = _lib.load(), ST.side_stream()
    st, n = ST.stream_handle(side), 1 << 16
    dev, ones = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.full((n,), 1, dtype=torch.uint8, device="cuda")
    dev2 = torch.zeros(n, dtype=torch.uint8, device="cuda")
    up, down = torch.full((n,), 7, dtype=torch.uint8).pin_memory(), torch.zeros(n, dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize()
    ev = ST.gate(side)
    with torch.cuda.stream(side):
        dev.copy_(ones, non_blocking=True)                   # behind the gate; the memset has to come after it
    _lib.check(lib.mx_dev_memset(C.c_void_p(dev.data_ptr()), 0x5A, n, st))
    ST.pending(ev, "after mx_dev_memset")
    _lib.check(lib.mx_memcpy_d2h(C.c_void_p(down.data_ptr()), C.c_void_p(dev.data_ptr()), n, st))
    ST.pending(ev, "after mx_memcpy_d2h")
    with torch.cuda.stream(side):
        dev2.copy_(ones, non_blocking=True)
    _lib.check(lib.mx_memcpy_h2d(C.c_void_p(dev2.data_ptr()), C.c_void_p(up.data_ptr()), n, st))
    ST.pending(ev, "after mx_memcpy_h2d")
    assert bool((down == 0).all()), "mx_memcpy_d2h wrote before the stream reached it"
    _lib.check(lib.mx_stream_sync(st))
    assert ev.query(), "mx_stream_sync returned with the gate still pending"
    assert bool((down == 0x5A).all()), "mx_memcpy_d2h did not follow mx_dev_memset on the stream"
    with torch.cuda.stream(side):
        got, got2 = dev.cpu(), dev2.cpu()
    assert bool((got == 0x5A).all()), "mx_dev_memset ran ahead of the copy queued before it"
    assert bool((got2 == 7).all()), "mx_memcpy_h2d ran ahead of the copy queued before it"
