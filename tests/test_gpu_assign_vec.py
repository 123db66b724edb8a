"""`X[r, ] <- vector` and `X[, c] <- vector` of a dgRMatrix on the device (csrc/assignvec.hip, csrc/api_assign.hip,
matrixextra_amd/assign.py): every record of what the reference's own compiled routines returned,
replayed bit for bit; the column kernels at every lane width between guards; the pattern expansion; rows that are not
sorted; the inputs on which the reference is defective; and the Python mirror end to end.

Everything is compared exactly (indices as int32, values as their 64 bits): an assignment moves and writes values, it
computes none, so there is no tolerance to choose."""

import numpy as np
import pytest

import assign_vec_model as VM
import matrixextra_amd as mx
import rowgroup_cases as RC
from assign_vec_dev import Pattern, dev_assign_col, dev_expand_pattern
from conftest import rand_csr
from devmem import GCsr
from matrixextra_amd import matrices
from matrixextra_amd import exports as G

pytestmark = pytest.mark.gpu

RECORDS, META = VM.load()
NA, NAN2 = VM.NA_REAL, VM.OTHER_NAN
OPTION = "mxgpu.assign_vec_route"
I32 = lambda *a: np.array(a, dtype=np.int32)        # noqa: E731
# what tests/golden/make_assign_vec_golden.py wrote: compared bit for bit / after sorting the rows of both sides
N_SORTED, N_SHUFFLED = 242, 57


def same(got, want, what=""):
    p, j, x = got
    q, k, y = want
    assert np.array_equal(p, q), f"{what}: indptr"
    assert np.array_equal(j, k), f"{what}: indices"
    assert np.array_equal(VM.bits(x), VM.bits(y)), f"{what}: values"


def sorted_rows(t):
    return (t[0],) + VM.sort_rows(*t)


def triple(out):
    return out["indptr"], out["indices"], out["values"]


# ---- 1. golden replay ----------------------------------------------------------------------------------------------
def replay(name):
    """(records compared bit for bit with their alias flags, records compared after sorting the rows)"""
    exact = loose = 0
    for r in RECORDS:
        if r["name"] != name:
            continue
        p, j, x = r["p"].copy(), r["j"].copy(), r["x"].copy()
        args = VM.call_args(name, r["args"])
        kept = [a.copy() if isinstance(a, np.ndarray) else a for a in args]
        out = getattr(G, name)(p, j, x, *args)
        got, want = triple(out), (r["out_p"], r["out_j"], r["out_x"])
        if r["sorted"]:
            same(got, want, r["label"])
            assert (int(got[0] is p), int(got[1] is j), int(got[2] is x)) == r["alias"], r["label"]
            exact += 1
        else:
            same(sorted_rows(got), sorted_rows(want), r["label"])
            loose += 1
        assert np.array_equal(p, r["p"]) and np.array_equal(j, r["j"]) and np.array_equal(VM.bits(x), VM.bits(r["x"]))
        for a, b in zip(args, kept):
            assert np.array_equal(VM.bits(a), VM.bits(b)) if isinstance(a, np.ndarray) else a == b, r["label"]
    return exact, loose


COUNTS = {}


@pytest.mark.parametrize("name", sorted(VM.ORDER))
def test_golden_replay(name):
    COUNTS[name] = replay(name)
    assert COUNTS[name][0] >= 20 and COUNTS[name][1] >= 5


def test_golden_replay_left_no_record_out():
    """Every record with sorted rows was compared bit for bit, and only the shuffled matrix's after sorting rows."""
    for name in VM.ORDER:
        if name not in COUNTS:
            COUNTS[name] = replay(name)
    assert sum(c[0] for c in COUNTS.values()) == N_SORTED == META["sorted_records"]
    assert sum(c[1] for c in COUNTS.values()) == N_SHUFFLED == META["shuffled_records"]
    assert N_SHUFFLED == sum(r["label"].startswith("shuffled:") for r in RECORDS)
    assert N_SORTED + N_SHUFFLED == len(RECORDS)


# ---- 2. the column kernels at every lane width, between guards -----------------------------------------------------
M_ROWS, K_COLS = 40, 200
BELOW, ABSENT, ABOVE = 0, 100, 199                  # no row stores these: below all, inside, above all of every row


def lane_matrix(Gw, every_row_stores=None):
    """40 x 200, rows of 0, 1, G - 1, G, G + 1 and 2G + 3 entries in turn; with `every_row_stores` that column is
    added to every row"""
    rng = np.random.default_rng(Gw)
    lens = [(0, 1, Gw - 1, Gw, Gw + 1, 2 * Gw + 3)[r % 6] for r in range(M_ROWS)]
    pool = np.setdiff1d(np.arange(5, 195), [ABSENT])
    rows = [np.sort(rng.choice(pool, size=n, replace=False)) for n in lens]
    if every_row_stores is not None:
        rows = [np.union1d(r, [every_row_stores]) for r in rows]
    p = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    j = np.concatenate(rows).astype(np.int32)
    x = np.round(rng.normal(size=j.size), 3)
    x[::5] = [0.0, -0.0, NA, NAN2][Gw % 4]
    return p, j, x


def patterns(rng):
    """dense and sparse patterns of length 40, 8 and 1, and a sparse one without entries"""
    out = {}
    for L in (40, 8, 1):
        v = np.round(rng.normal(size=L), 3)
        v[::3] = [0.0, NA, -0.0, NAN2][L % 4]
        out[f"dense{L}"] = (None, v, L)
        ii = np.sort(rng.choice(L, size=max(1, L // 2), replace=False)).astype(np.int32)
        out[f"sparse{L}"] = (ii, v[:ii.size].copy(), L)
    out["sparse8 without entries"] = (I32(), np.zeros(0), 8)
    return out


@pytest.mark.parametrize("Gw", RC.LANE_GROUPS)
def test_column_kernels_at_every_lane_width(Gw):
    p, j, x = lane_matrix(Gw)
    lens = np.diff(p)
    assert {0, 1, Gw - 1, Gw, Gw + 1, 2 * Gw + 3} <= set(lens.tolist())
    A = GCsr(p, j, x)
    long_row = int(np.flatnonzero(lens == 2 * Gw + 3)[0])
    own = j[p[long_row]:p[long_row + 1]]
    cols = {"first entry": int(own[0]), "last entry": int(own[-1]), "middle entry": int(own[own.size // 2]),
            "below all": BELOW, "above all": ABOVE, "absent": ABSENT}
    assert not np.isin([BELOW, ABOVE, ABSENT], j).any() and j.min() > BELOW and j.max() < ABOVE
    avg = float(Gw)
    assert RC.pick_group(avg) == Gw
    for pname, (ii, xx, L) in patterns(np.random.default_rng(100 + Gw)).items():
        pat = Pattern(ii, xx, L)
        mii = np.arange(L) if ii is None else ii.astype(np.int64)
        for cname, col in cols.items():
            what = f"G{Gw} {pname} col {cname}"
            q, k, v, total, changed, launches = dev_assign_col(A, K_COLS, col, pat, avg)
            want = VM.assign_col(p, j, x, col, mii, VM.bits(xx), L)
            same((q, k, v), want, what)
            assert total == want[0][-1], what
            assert changed == int((np.diff(want[0]) != lens).sum()), what
            assert launches == [("mxd_csr_assign_col_count", Gw), ("mxd_csr_assign_col_fill", Gw)], what


@pytest.mark.parametrize("Gw", RC.LANE_GROUPS)
def test_values_only_fill(Gw):
    """Every row stores the column and the vector is dense: no row changes structure, and the fill writes the values
    alone beside the input's own indptr."""
    p, j, x = lane_matrix(Gw, every_row_stores=ABSENT)
    A = GCsr(p, j, x)
    for L in (40, 8, 1):
        v = np.arange(1.0, L + 1.0)
        v[0] = NA
        pat = Pattern(None, v, L)
        q, k, vals, total, changed, launches = dev_assign_col(A, K_COLS, ABSENT, pat, float(Gw), values_only=True)
        want = VM.assign_col(p, j, x, ABSENT, np.arange(L), VM.bits(v), L)
        assert k is None and changed == 0 and total == j.size and np.array_equal(q, p) and np.array_equal(want[1], j)
        assert np.array_equal(VM.bits(vals), VM.bits(want[2])), (Gw, L)
        assert launches[1] == ("mxd_csr_assign_col_fill", Gw)


# ---- 3. pattern expansion ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Gw", (4, 64))
def test_pattern_expansion(Gw):
    rng = np.random.default_rng(Gw)
    for L in (1, Gw, 2 * Gw + 3):
        for reps in (1, 3):
            v = np.round(rng.normal(size=L), 3)
            v[0] = NA
            ii = rng.permutation(L)[:max(1, L // 2)].astype(np.int32)          # as stored: any order
            for what, pi, px in (("dense", None, v), ("sparse", ii, v[:ii.size].copy())):
                pat = Pattern(pi, px, L)
                mi = np.arange(L) if pi is None else pi.astype(np.int64)
                wj, wx = VM.recycled(mi, VM.bits(px), L, L * reps)
                rp, rj, rx = dev_expand_pattern(pat, reps)
                assert rp.tolist() == [0, wj.size] and np.array_equal(rj, wj), (what, L, reps)
                assert np.array_equal(VM.bits(rx), wx), (what, L, reps)
                _, none, rx = dev_expand_pattern(pat, reps, values_only=True)
                assert none is None and np.array_equal(VM.bits(rx), wx), (what, L, reps)
    rp, rj, rx = dev_expand_pattern(Pattern(I32(), np.zeros(0), 5), 2)          # no entries: an empty row
    assert rp.tolist() == [0, 0] and rj.size == 0 and rx.size == 0


@pytest.mark.parametrize("ncols, density", ((20, 0.2), (60, 0.4)), ids=("G4", "G32"))
def test_long_sparse_pattern(ncols, density):
    """A sparse vector as long as the matrix has rows: the group's search of ii runs over several levels."""
    m = 3001
    p, j, x = rand_csr(m, ncols, density, 13, empty_rows=(0, 1500, m - 1))
    rng = np.random.default_rng(m)
    for n_ii in (1, 1499, m):
        ii = np.sort(rng.choice(m, size=n_ii, replace=False)).astype(np.int32)
        xx = np.arange(1.0, n_ii + 1.0)
        for col in (0, ncols // 2, ncols - 1):
            out = G.set_single_col_to_svec(p, j, x, ncols, col, ii, xx, m)
            same(triple(out), VM.assign_col(p, j, x, col, ii, VM.bits(xx), m), f"{n_ii} entries, col {col}")


# ---- 4. rows that are not sorted, through the exports --------------------------------------------------------------
def test_unsorted_rows():
    p, j, x = rand_csr(24, 30, 0.4, 9, sorted_cols=False, empty_rows=(5,))
    assert not G.rows_are_sorted(p, j)
    sj, sx = VM.sort_rows(p, j, x)
    every = int(j[0])                                   # a column that every row is made to store
    vec = np.arange(1.0, 9.0)
    for col in (0, 17, 29):
        out = G.set_single_col_to_colvec(p, j, x, 30, col, vec)
        same(triple(out), VM.assign_col(p, sj, sx, col, np.arange(8), VM.bits(vec), 8), f"colvec {col}")
        assert out["indptr"] is not p and out["indices"] is not j
        ii = I32(1, 2, 6)
        out = G.set_single_col_to_svec(p, j, x, 30, col, ii, vec[:3], 8)
        same(triple(out), VM.assign_col(p, sj, sx, col, ii, VM.bits(vec[:3]), 8), f"svec {col}")
    # every row stores the column: the same structure, but rows sorted on the device are new vectors
    rows = [np.concatenate([[every], np.setdiff1d(j[p[r]:p[r + 1]], [every])[::-1]]) for r in range(24)]
    p2 = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    j2 = np.concatenate(rows).astype(np.int32)
    x2 = np.arange(1.0, j2.size + 1.0)
    assert not G.rows_are_sorted(p2, j2)
    out = G.set_single_col_to_colvec(p2, j2, x2, 30, every, vec)
    s2 = VM.sort_rows(p2, j2, x2)
    same(triple(out), VM.assign_col(p2, s2[0], s2[1], every, np.arange(8), VM.bits(vec), 8), "every row stores it")
    assert out["indptr"] is not p2 and out["indices"] is not j2 and np.array_equal(out["indptr"], p2)
    # the row routes leave the other rows as stored; a full row that is not sorted gives three new vectors
    rows_j = [j[p[r]:p[r + 1]] for r in range(24)]
    rows_j[3] = np.random.default_rng(3).permutation(30).astype(np.int32)
    p3 = np.concatenate([[0], np.cumsum([r.size for r in rows_j])]).astype(np.int32)
    j3, x3 = np.concatenate(rows_j).astype(np.int32), np.arange(1.0, p3[-1] + 1.0)
    v30 = np.arange(30.0)
    out = G.set_single_row_to_rowvec(p3, j3, x3, 30, 3, v30)
    same(triple(out), VM.assign_row(p3, j3, x3, 30, 3, np.arange(30), VM.bits(v30), 30), "full unsorted row")
    assert out["indptr"] is not p3 and out["indices"] is not j3
    assert np.array_equal(out["indices"][p3[3]:p3[4]], np.arange(30)) and np.array_equal(out["indptr"], p3)


# ---- 5. the inputs on which the reference is defective -------------------------------------------------------------
def test_defect_cases_follow_the_model():
    cases = [
        # a shorter row "matched" by the recycled fast path: the reference overwrites row 1's value
        (I32(0, 1, 2), I32(1, 0), np.array([1.0, 2.0]), dict(ncols=6, row=0, ii=I32(1), xx=np.array([50.0]), length=3),
         (I32(0, 2, 3), I32(1, 4, 0), np.array([50.0, 50.0, 2.0]))),
        # n_repeats = 1 and a row twice as long as ii: the reference reads ii past its end
        (I32(0, 4), I32(0, 2, 3, 5), np.arange(1.0, 5.0), dict(ncols=6, row=0, ii=I32(0, 2), xx=np.array([7.0, 8.0]), length=6),
         (I32(0, 2), I32(0, 2), np.array([7.0, 8.0]))),
        # an empty ii (the reference divides by zero) empties the row
        (I32(0, 2, 3), I32(0, 4, 2), np.array([1.0, 2.0, 3.0]), dict(ncols=6, row=0, ii=I32(), xx=np.zeros(0), length=3),
         (I32(0, 0, 1), I32(2), np.array([3.0]))),
    ]
    for p, j, x, args, want in cases:
        same(VM.run("set_single_row_to_svec", p, j, x, args), want, "model")
        out = G.set_single_row_to_svec(p, j, x, *VM.call_args("set_single_row_to_svec", args))
        same(triple(out), want, str(args))
        assert out["indptr"] is not p and out["indices"] is not j and out["values"] is not x
        assert x.tolist() == [float(k) for k in range(1, x.size + 1)]
    # the fast path proper still is one: equal lengths, equal indices
    p, j, x = I32(0, 4, 5), I32(1, 2, 4, 5, 0), np.arange(1.0, 6.0)
    out = G.set_single_row_to_svec(p, j, x, 6, 0, I32(1, 2), np.array([7.0, NA]), 3)
    assert out["indptr"] is p and out["indices"] is j and out["values"] is not x
    assert np.array_equal(VM.bits(out["values"]), VM.bits(np.array([7.0, NA, 7.0, NA, 5.0])))
    # set_single_col_to_svec without entries drops the column everywhere; an explicit zero is written
    out = G.set_single_col_to_svec(p, j, x, 6, 0, I32(), np.zeros(0), 2)
    same(triple(out), (I32(0, 4, 4), j[:4], x[:4]), "empty ii")
    out = G.set_single_col_to_svec(I32(0, 1, 2), I32(1, 1), np.array([1.0, 2.0]), 3, 1, I32(0, 1), np.array([50.0, 0.0]), 2)
    same(triple(out), (I32(0, 1, 2), I32(1, 1), np.array([50.0, 0.0])), "explicit zero")


# ---- 6. the mirror, end to end -------------------------------------------------------------------------------------
NR, NC = 12, 10


@pytest.mark.parametrize("tag", ("sorted", "shuffled"))
def test_mirror_end_to_end(monkeypatch, tag):
    monkeypatch.setitem(matrices.options, OPTION, True)
    p, j, x = rand_csr(NR, NC, 0.4, 21, sorted_cols=tag == "sorted", empty_rows=(7,))
    dn = [[f"r{k}" for k in range(NR)], [f"c{k}" for k in range(NC)]]
    X = mx.dgRMatrix(p, j, x, (NR, NC), dn)
    before = (X.p.copy(), X.j.copy(), X.x.copy())
    D = X.toarray()

    def stored(out, r, c):
        """the value bits stored at (r, c), or None"""
        k = np.flatnonzero(out.j[out.p[r]:out.p[r + 1]] == c)
        assert k.size <= 1
        return int(VM.bits(out.x[out.p[r]:out.p[r + 1]])[k[0]]) if k.size else None

    def check(out, E, what):
        assert isinstance(out, mx.dgRMatrix) and out.Dim == X.Dim and out.Dimnames == X.Dimnames, what
        assert np.array_equal(out.toarray(), E, equal_nan=True), what
        assert (np.array_equal(X.p, before[0]) and np.array_equal(X.j, before[1])
                and np.array_equal(VM.bits(X.x), VM.bits(before[2]))), what

    na_bits, zero_bits = int(VM.bits(np.array([NA]))[0]), 0
    # X[2, ] <- v (1-based row 2), recycled twice, with an explicit zero and an NA
    v = np.array([1.5, 0.0, NA, -2.0, 4.0])
    out = mx.assign_csr(X, [2], None, v)
    E = D.copy()
    E[1, :] = np.tile(v, 2)
    check(out, E, "row <- dense")
    assert out.p[2] - out.p[1] == NC and stored(out, 1, 1) == zero_bits and stored(out, 1, 7) == na_bits
    # X[, 3] <- v, recycled three times
    v = np.array([0.0, NA, 3.0, 4.0])
    out = mx.assign_csr(X, None, [3], v)
    E = D.copy()
    E[:, 2] = np.tile(v, 3)
    check(out, E, "column <- dense")
    assert all(stored(out, r, 2) is not None for r in range(NR))
    assert stored(out, 4, 2) == zero_bits and stored(out, 9, 2) == na_bits and G.rows_are_sorted(out.p, out.j)
    # X[2, ] <- sparseVector, positions as stored (not sorted), an explicit zero among them
    sv = mx.dsparseVector([4, 1, 3], [NA, 0.0, 2.5], 5)
    out = mx.assign_csr(X, [2], None, sv)
    E = D.copy()
    E[1, :] = np.tile(sv.toarray(), 2)
    check(out, E, "row <- sparseVector")
    assert out.j[out.p[1]:out.p[2]].tolist() == [3, 0, 2, 8, 5, 7]
    assert stored(out, 1, 0) == zero_bits and stored(out, 1, 8) == na_bits and stored(out, 1, 1) is None
    # X[, 3] <- sparseVector: stored positions are written, the others lose the column
    sv = mx.dsparseVector([3, 1], [0.0, NA], 4)
    out = mx.assign_csr(X, None, [3], sv)
    E = D.copy()
    E[:, 2] = np.tile(sv.toarray(), 3)
    check(out, E, "column <- sparseVector")
    assert [stored(out, r, 2) for r in range(4)] == [na_bits, None, zero_bits, None] and sv.i.tolist() == [3, 1]
    # a one-column sparse matrix into a row is the vector it spells
    cm = mx.as_csc_matrix(mx.dgRMatrix([0, 0, 1, 1, 2, 2], [0, 0], [6.0, 7.0], (5, 1)))
    out = mx.assign_csr(X, [12], None, cm)
    E = D.copy()
    E[11, :] = np.tile([0.0, 6.0, 0.0, 7.0, 0.0], 2)
    check(out, E, "row <- one-column sparse matrix")
    assert out.j[out.p[11]:out.p[12]].tolist() == [1, 3, 6, 8]
