"""`[<-` of a dgRMatrix on the device (csrc/assign.hip, csrc/api_assign.hip, matrixextra_amd/assign.py): every
record of what the reference's own compiled set_* routines returned, replayed bit for bit; the kernels at every lane
width between guards; row replacement in any selector order; the Python mirror end to end; and the INT_MAX refusal.

Everything is compared exactly (indices as int32, values as their 64 bits): an assignment moves and writes values, it
computes none, so there is no tolerance to choose."""

import numpy as np
import pytest

import assign_model as AM
import matrixextra_amd as mx
import rowgroup_cases as RC
from assign_dev import dev_assign_scalar, dev_replace_rows
from conftest import rand_csr
from devmem import GCsr
from matrixextra_amd import _lib
from matrixextra_amd import exports as G

pytestmark = pytest.mark.gpu

RECORDS, _META = AM.load()
NA = mx.NA_REAL


def same(got, want, what=""):
    p, j, x = got
    q, k, y = want
    assert np.array_equal(p, q), f"{what}: indptr"
    assert np.array_equal(j, k), f"{what}: indices"
    assert np.array_equal(AM.bits(x), AM.bits(y)), f"{what}: values"


# ---- 1. golden replay ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(AM.ORDER))
def test_golden_replay(name):
    """Every record through its exports.set_* function: the three vectors bit for bit, the same vectors returned as
    they came in, the inputs unchanged.  Records with unsorted rows are compared after sorting the rows of both
    results; their alias flags are not, since rows sorted on the device are new vectors."""
    n = 0
    for r in RECORDS:
        if r["name"] != name:
            continue
        p, j, x = r["p"].copy(), r["j"].copy(), r["x"].copy()
        args = AM.call_args(name, r["args"])
        kept = [a.copy() if isinstance(a, np.ndarray) else a for a in args]
        out = getattr(G, name)(p, j, x, *args)
        got = (out["indptr"], out["indices"], out["values"])
        want = (r["out_p"], r["out_j"], r["out_x"])
        if r["sorted"]:
            same(got, want, r["label"])
            alias = (int(got[0] is p), int(got[1] is j), int(got[2] is x))
            assert alias == r["alias"], r["label"]
        else:
            same((got[0],) + AM.sort_rows(*got), (want[0],) + AM.sort_rows(*want), r["label"])
        assert np.array_equal(p, r["p"]) and np.array_equal(j, r["j"]) and np.array_equal(AM.bits(x), AM.bits(r["x"]))
        for a, b in zip(args, kept):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else AM.bits(a) == AM.bits(b), r["label"]
        n += 1
    assert n >= 5


# ---- 2. every lane width, between guards ---------------------------------------------------------------------------
M_ROWS = 203                                    # 4 blocks of 64 rows at G = 4, 51 blocks of 4 rows at G = 64


@pytest.fixture(scope="module")
def lane_cases():
    cases = {}
    for Gw in RC.LANE_GROUPS:
        c = RC.make_case(Gw, M_ROWS)
        want = {0, 1, Gw - 1, Gw, Gw + 1, 2 * Gw + 1, 65, RC.LONG_ROW}
        assert want <= set(c.lens.tolist()), (Gw, sorted(want - set(c.lens.tolist())))
        assert RC.pick_group(c.nnz / c.m) == Gw
        cases[Gw] = c
    return cases


def selectors_for(c):
    """Column selectors: a single stored column, a range over the first column, a range over the last column, and
    an arbitrary unsorted set with columns below and above every stored one.  Row selectors: all, a range, and an
    arbitrary unsorted set with an empty row and the last row."""
    stored = np.unique(c.j)
    assert stored.min() >= RC.EDGE and stored.max() < c.K - RC.EDGE
    rng = np.random.default_rng(c.G)
    some = rng.choice(stored, size=25, replace=False)
    arb_cols = np.concatenate([[c.K - 1, 2, int(stored[0])], some, [0, c.K - 3, int(stored[-1]), 17]]).astype(np.int32)
    arb_cols = arb_cols[np.sort(np.unique(arb_cols, return_index=True)[1])]
    cols = {"single": ("range", int(c.j[0]), int(c.j[0])), "first": ("range", 0, int(stored[len(stored) // 3])),
            "last": ("range", int(stored[2 * len(stored) // 3]), c.K - 1), "arbitrary": ("set", arb_cols)}
    empty = int(np.flatnonzero(c.lens == 0)[0])
    long_row = int(np.flatnonzero(c.lens == RC.LONG_ROW)[0])
    arb_rows = np.concatenate([[c.m - 1, empty, long_row], rng.choice(c.m - 1, size=40, replace=False)]).astype(np.int32)
    arb_rows = arb_rows[np.sort(np.unique(arb_rows, return_index=True)[1])]
    rows = {"all": None, "range": ("range", 5, c.m - 20), "arbitrary": ("set", arb_rows)}
    return rows, cols


def members(sel, n):
    return None if sel is None else np.arange(sel[1], sel[2] + 1) if sel[0] == "range" else sel[1]


@pytest.mark.parametrize("Gw", RC.LANE_GROUPS)
def test_kernels_at_every_lane_width(lane_cases, Gw):
    c = lane_cases[Gw]
    x = c.vals["gen"][0]
    A = GCsr(c.p, c.j, x)
    rows, cols = selectors_for(c)
    avg = c.nnz / c.m
    row_of = np.repeat(np.arange(c.m), c.lens)
    for value in (0.0, NA):
        for rname, rsel in rows.items():
            for cname, csel in cols.items():
                what = f"G{Gw} value {value} rows {rname} cols {cname}"
                p, j, v, total, hits, launches = dev_assign_scalar(A, c.K, rsel, csel, value, avg)
                want = AM.assign_scalar(c.p, c.j, x, c.K, members(rsel, c.m), members(csel, c.K), value)
                same((p, j, v), want, what)
                assert total == want[0][-1], what
                in_rows = np.ones(c.nnz, dtype=bool) if rsel is None else np.isin(row_of, members(rsel, c.m))
                assert hits == int((in_rows & np.isin(c.j, members(csel, c.K))).sum()), what
                assert launches == [("mxd_csr_assign_count", Gw), ("mxd_csr_assign_fill", Gw)], what
    # all columns: the count pass takes the hits from indptr alone
    for value in (0.0, 2.5):
        p, j, v, total, hits, _ = dev_assign_scalar(A, c.K, rows["arbitrary"], None, value, avg)
        same((p, j, v), AM.assign_scalar(c.p, c.j, x, c.K, rows["arbitrary"][1], None, value), f"G{Gw} all columns")
        assert hits == int(c.lens[rows["arbitrary"][1]].sum())


# ---- 3. row replacement --------------------------------------------------------------------------------------------
def value_rows(n_rows, K, seed, empty_rows):
    p, j, x = rand_csr(n_rows, K, 0.05, seed, empty_rows=empty_rows)
    return p, j, x


@pytest.mark.parametrize("Gw", (4, 32))
def test_row_replacement_device(lane_cases, Gw):
    c = lane_cases[Gw]
    x = c.vals["gen"][0]
    A = GCsr(c.p, c.j, x)
    m = c.m
    rng = np.random.default_rng(7)
    sels = {"seq": ("range", 3, 60), "rev-seq": ("range", 3, 60, 1),
            "arbitrary": ("set", rng.permutation(m)[:50].astype(np.int32)),
            "largest is nrows-2": ("set", np.array([m - 2, 0, 17], dtype=np.int32)),
            "every row": ("set", rng.permutation(m).astype(np.int32))}
    for what, sel in sels.items():
        order = (np.arange(sel[1], sel[2] + 1)[::-1] if len(sel) > 3 else np.arange(sel[1], sel[2] + 1)) \
            if sel[0] == "range" else sel[1]
        vp, vj, vx = value_rows(order.size, c.K, 11, empty_rows=(0, order.size - 1))
        V = GCsr(vp, vj, vx)
        avg = (c.nnz + vj.size) / m
        p, j, v, total, launch = dev_replace_rows(A, sel, V, avg)
        want = AM.replace_rows(c.p, c.j, x, order, vp, vj, vx)
        same((p, j, v), want, what)
        assert total == want[0][-1] and launch == ("mxd_csr_replace_rows_fill", RC.pick_group(avg)), what
        if what == "largest is nrows-2":                  # where the reference loses the last row
            assert p[-1] == total > 0 and np.array_equal(j[p[-2]:], c.j[c.p[-2]:])


def test_row_replacement_exports():
    p, j, x = rand_csr(40, 30, 0.3, 5, empty_rows=(3,))
    for rows in ([38, 2, 11], [39, 0], list(range(39, -1, -1))):
        vp, vj, vx = rand_csr(len(rows), 30, 0.2, 6, empty_rows=(1,))
        out = G.set_arbitrary_rows_to_smat(p, j, x, np.array(rows, dtype=np.int32), vp, vj, vx)
        same((out["indptr"], out["indices"], out["values"]), AM.replace_rows(p, j, x, rows, vp, vj, vx), str(rows))
    vp, vj, vx = rand_csr(4, 30, 0.2, 8)
    out = G.set_rowseq_to_smat(p, j, x, 36, 39, vp, vj, vx)
    same((out["indptr"], out["indices"], out["values"]), AM.replace_rows(p, j, x, [36, 37, 38, 39], vp, vj, vx), "seq")
    with pytest.raises(_lib.MxError, match="rows"):
        G.set_rowseq_to_smat(p, j, x, 0, 2, vp, vj, vx)


# ---- 4. the mirror, end to end -------------------------------------------------------------------------------------
NR, NC = 70, 90
# 18 selector shapes, 1-based as assign_csr takes them (None = missing)
SHAPES = [
    ([1], None), ([70], None), ([7, 8, 9, 10], None), ([40, 39, 38], None), ([70, 1, 33, 12], None),
    (None, [1]), (None, [90]), (None, [20, 21, 22]), (None, [90, 89, 88, 87]), (None, [90, 1, 45, 3, 60]),
    ([5], [9]), ([70], [90]), ([70, 2, 31], [44]), ([1, 2, 3], [90]), ([12], [90, 1, 50]),
    ([12], [4, 5, 6]), ([70, 1, 12, 13, 40], [90, 1, 30, 31]), ([10, 11, 12], [60, 59, 58]),
]


@pytest.fixture(scope="module")
def mirror_inputs():
    out = {}
    for tag, srt in (("sorted", True), ("shuffled", False)):
        p, j, x = rand_csr(NR, NC, 0.3, 21, sorted_cols=srt, empty_rows=(12, 69))
        dn = [[f"r{k}" for k in range(NR)], [f"c{k}" for k in range(NC)]]
        out[tag] = mx.dgRMatrix(p, j, x, (NR, NC), dn)
    return out


@pytest.mark.parametrize("tag", ("sorted", "shuffled"))
@pytest.mark.parametrize("value", (0, -0.0, 2.5, NA), ids=("0", "-0.0", "2.5", "NA"))
def test_mirror_end_to_end(mirror_inputs, tag, value):
    X = mirror_inputs[tag]
    before = (X.p.copy(), X.j.copy(), X.x.copy())
    sj, sx = AM.sort_rows(X.p, X.j, X.x)
    D = X.toarray()
    for i, j in SHAPES:
        what = f"{tag} value {value} i {i} j {j}"
        out = mx.assign_csr(X, i, j, value)
        assert (np.array_equal(X.p, before[0]) and np.array_equal(X.j, before[1])
                and np.array_equal(AM.bits(X.x), AM.bits(before[2]))), what
        assert out.Dim == X.Dim and out.Dimnames == X.Dimnames and isinstance(out, mx.dgRMatrix), what
        rows0 = None if i is None else np.array(i) - 1
        cols0 = None if j is None else np.array(j) - 1
        same((out.p, out.j, out.x), AM.assign_scalar(X.p, sj, sx, NC, rows0, cols0, float(value)), what)
        E = D.copy()
        E[np.ix_(np.arange(NR) if rows0 is None else rows0, np.arange(NC) if cols0 is None else cols0)] = value
        assert np.array_equal(out.toarray(), E, equal_nan=True), what
        Y = X.copy()
        Y[slice(None) if rows0 is None else rows0, slice(None) if cols0 is None else cols0] = value
        same((Y.p, Y.j, Y.x), (out.p, out.j, out.x), what + " (__setitem__)")


def test_mirror_row_replacement(mirror_inputs):
    X = mirror_inputs["sorted"]
    for i in ([3, 4, 5, 6], [6, 5, 4, 3], [70, 1, 33], list(np.random.default_rng(3).permutation(NR) + 1)):
        vp, vj, vx = rand_csr(len(i), NC, 0.2, 31, empty_rows=(1,))
        for V in (mx.dgRMatrix(vp, vj, vx, (len(i), NC)), mx.as_coo_matrix(mx.dgRMatrix(vp, vj, vx, (len(i), NC))),
                  mx.as_csc_matrix(mx.dgRMatrix(vp, vj, vx, (len(i), NC)))):
            out = mx.assign_csr(X, i, None, V)
            same((out.p, out.j, out.x), AM.replace_rows(X.p, X.j, X.x, np.array(i) - 1, vp, vj, vx), f"{i[:4]} {type(V)}")
            assert out.Dimnames == X.Dimnames


# ---- 5. overflow -----------------------------------------------------------------------------------------------------
def test_a_result_beyond_int_max_is_refused():
    nr, nc = 70000, 40000
    X = mx.dgRMatrix(np.zeros(nr + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), (nr, nc))
    with pytest.raises(_lib.MxError, match=r"^Error: resulting matrix would be larger than INT_MAX limit\.$"):
        mx.assign_csr(X, np.arange(1, nr), None, 1.0)
    with pytest.raises(_lib.MxError, match=r"^Error: resulting matrix would be larger than INT_MAX limit\.$"):
        X[0:nr - 1] = 1.0
    assert X.j.size == 0
    out = mx.assign_csr(X, [1, nr], None, 1.0)                    # and one that fits: 2 x 40 000 entries
    assert out.p[-1] == 2 * nc and np.array_equal(out.j[:nc], np.arange(nc)) and np.all(out.x == 1.0)
