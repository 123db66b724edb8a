"""Pure-numpy case generator for the row-group kernels (one G-lane group per row, G in {4, 8, 16, 32, 64}): CSR
operands whose TRUE mean row length selects a chosen G, with the row lengths, wavefront windows and partner overlaps
at which such kernels go wrong.  No GPU, no library: tests/test_row_group_cases.py checks the generator itself.

A wavefront of 64 lanes holds 64 / G consecutive rows, a 256-thread block 256 / G.  A case is laid out as
  rows [0, W)        register windows: every row <= G entries in BOTH operands (W = a multiple of 64 / G, >= 8 rows),
                     lengths G, G, G, G, G - 1, 1, 0, G / 2 and partner overlaps identical, disjoint, first-only,
                     last-only, strictly below, strictly above, A empty, identical
  rows [W, W + 64/G) a window in which exactly one row (G + 1 entries) exceeds G
  then               rows of 0, 1, G - 1, G, G + 1, 2G - 1, 2G, 2G + 1, 3G + 5, 64, 65 and LONG_ROW entries, G - 1, G,
                     G + 1 and 0 next to each other
  then               padding rows whose lengths bring the mean into G's band.
A block is left out when the row count m, or the band, has no room for it (m = 1 is one row; at G = 64 the band
(32, 64] cannot hold a 230-entry row in 13 rows): `Case.blocks` says which are present, and the four-digit m holds
all of them for every G.
"""
from dataclasses import dataclass, field

import numpy as np

LANE_GROUPS = (4, 8, 16, 32, 64)
MERGE_GROUPS = (8, 16, 32, 64)
LONG_ROW = 230                      # the sort kernel is O(len^2) per row: keep it short
EDGE = 64                           # columns [0, EDGE) and [K - EDGE, K) are free of A: room for B below / above A
K_COLS = 2 * EDGE + 600
NA_INT = np.int32(-2147483648)
NA_REAL = np.frombuffer(np.uint64(0x7FF00000000007A2).tobytes(), dtype=np.float64)[0]


def pick_group(avg_len, lo=4):
    """mx_common.h: smallest power of two >= the mean row length, clamped to [lo, 64]."""
    g = lo
    while g < 64 and float(g) < avg_len:
        g <<= 1
    return g


def spmv_group(m, nnz):
    """spmv.hip, gather.hip (nnz_out, r), svec.hip, dvec.hip: a negative hint means 32."""
    return 32 if nnz < 0 else pick_group(nnz / (m if m > 0 else 1))


def merge_group(m, nnz1, nnz2):
    """merge.hip: from the longer operand's mean, at least 8 lanes."""
    if nnz1 < 0 or nnz2 < 0 or m <= 0:
        return 32
    return pick_group(max(nnz1, nnz2) / m, 8)


def half_group(m, nnz):
    """bind.hip (nnz of both operands) and reverse-columns in colslice.hip: half the mean."""
    return pick_group(0.5 * nnz / m)


def band(G, scale=1, lo_group=4):
    """(lo, hi]: the means for which pick_group(mean / scale, lo_group) == G."""
    lo = 0.0 if G == lo_group else scale * G / 2.0
    return lo, float(scale * G)


def row_counts(G):
    """the m of the issue: around one block of 256 / G rows, three blocks and one, and a four-digit m that is not a
    multiple of the 64 / G rows of a wavefront"""
    b = 256 // G
    return [1, b - 1, b, b + 1, 3 * b + 1, 1003]


REQUIRED = ("G-1", "G", "G+1", "0", "1", "2G-1", "2G", "2G+1", "3G+5", "64", "65", "long")
OVERLAPS = ("identical", "disjoint", "first", "last", "below", "above", "a_empty", "b_empty")


def required_length(name, G):
    return {"G-1": G - 1, "G": G, "G+1": G + 1, "0": 0, "1": 1, "2G-1": 2 * G - 1, "2G": 2 * G, "2G+1": 2 * G + 1,
            "3G+5": 3 * G + 5, "64": 64, "65": 65, "long": LONG_ROW}[name]


@dataclass
class Case:
    G: int
    m: int
    scale: int
    K: int
    p: np.ndarray
    j: np.ndarray
    p2: np.ndarray
    j2: np.ndarray
    overlap: list                               # per row: the partner's overlap pattern
    blocks: dict = field(default_factory=dict)  # block name -> (first row, rows)
    vals: dict = field(default_factory=dict)    # "int" / "gen" / "lgl" -> (values of A, values of B)
    rows_take: np.ndarray = None
    cols_sorted: np.ndarray = None
    cols_unsorted: np.ndarray = None

    @property
    def nnz(self):
        return int(self.j.size)

    @property
    def nnz2(self):
        return int(self.j2.size)

    @property
    def lens(self):
        return np.diff(self.p)

    @property
    def lens2(self):
        return np.diff(self.p2)

    def colranges(self):
        """(name, min_col, max_col): no column, one stored column, all columns"""
        one = int(self.j[0]) if self.nnz else 0
        return [("empty", self.K + 5, self.K + 9), ("single", one, one), ("all", 0, self.K - 1)]

    def id(self):
        return f"G{self.G}-m{self.m}" + (f"-x{self.scale}" if self.scale != 1 else "")


def _lengths(G, m, scale, rng):
    """row lengths of A and the first row of every block that found room"""
    lo, hi = band(G, scale)
    wave = 64 // G
    W = -(-max(wave, 8) // wave) * wave
    cyc = [G, G, G, G, G - 1, 1, 0, max(G // 2, 1)]
    candidates = [("register_windows", [cyc[r % 8] for r in range(W)]),
                  ("one_long_window", [G + 1 if r == wave // 2 else cyc[(r + 3) % 8] for r in range(wave)])]
    candidates += [(name, [required_length(name, G)]) for name in REQUIRED]
    fixed, blocks = [], {}
    for name, lens in candidates:
        n, s = len(fixed) + len(lens), sum(fixed) + sum(lens)
        aligned = name != "one_long_window" or "register_windows" in blocks     # windows start at a wavefront's row
        if n > m or s > hi * m or (n == m and not s > lo * m) or not aligned:
            continue
        blocks[name] = (len(fixed), len(lens))
        fixed += lens
    npad = m - len(fixed)
    lens = np.array(fixed, dtype=np.int64)
    if npad:
        first_ok = int(np.floor(lo * m)) + 1                # smallest total inside the band
        target = max(int(0.9 * hi * m), first_ok, int(lens.sum()))
        target = min(target, int(hi * m))
        pad = rng.multinomial(target - int(lens.sum()), np.full(npad, 1.0 / npad))
        lens = np.concatenate([lens, pad])
    return lens, blocks


def _row_columns(n, rng):
    return np.sort(rng.choice(np.arange(EDGE, K_COLS - EDGE), size=n, replace=False)).astype(np.int32)


def _partner(cols, kind, rng):
    n = cols.size
    free = np.setdiff1d(np.arange(EDGE, K_COLS - EDGE, dtype=np.int32), cols)
    if kind == "identical":
        return cols.copy()
    if kind == "disjoint":                                  # interleaved with A: same range, no common column
        return np.sort(rng.choice(free, size=min(n, free.size), replace=False)).astype(np.int32)
    if kind in ("first", "last"):
        keep = cols[:1] if kind == "first" else cols[-1:]
        other = rng.choice(free, size=min(n - 1, free.size), replace=False)
        return np.sort(np.concatenate([keep, other])).astype(np.int32)
    if kind == "below":
        return np.sort(rng.choice(EDGE, size=min(n, EDGE), replace=False)).astype(np.int32)
    if kind == "above":
        return np.sort(K_COLS - 1 - rng.choice(EDGE, size=min(n, EDGE), replace=False)).astype(np.int32)
    if kind == "a_empty":
        return np.sort(rng.choice(K_COLS, size=2, replace=False)).astype(np.int32)
    return np.zeros(0, dtype=np.int32)                      # b_empty


def _values(nnz, p, rng, special_rows):
    ints = rng.integers(-3, 4, size=nnz).astype(np.float64)
    gen = rng.normal(size=nnz) * 10.0 ** rng.integers(-3, 4, size=nnz)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, NA_REAL])
    for r in special_rows:
        s, e = int(p[r]), int(p[r + 1])
        if e > s:
            at = rng.integers(s, e, size=min(6, e - s))
            gen[at] = specials[rng.integers(0, specials.size, size=at.size)]
    lgl = rng.choice(np.array([0, 1, NA_INT], dtype=np.int32), size=nnz, p=[0.25, 0.5, 0.25])
    return dict(int=ints, gen=gen, lgl=lgl)


def make_case(G, m, scale=1, seed=0):
    """A (p, j) and its partner B (p2, j2), both m x K_COLS with sorted, unique columns.  nnz / m lies in the band of
    G times `scale` (scale 2: the kernels that pick their width from half the mean), and so does the mean of
    A[rows_take, ] at scale 1; B never has more entries than A, so the merge picks G from A too."""
    for attempt in range(64):
        rng = np.random.default_rng([G, m, scale, seed, attempt])
        lens, blocks = _lengths(G, m, scale, rng)
        p = np.zeros(m + 1, dtype=np.int32)
        p[1:] = np.cumsum(lens)
        rows = [_row_columns(int(n), rng) for n in lens]
        overlap, rows2 = [], []
        for r, cols in enumerate(rows):
            if cols.size == 0:
                kind = "a_empty" if r % 2 == 0 else "b_empty"
            elif r < sum(blocks.get("register_windows", (0, 0))):
                kind = OVERLAPS[r % 8] if OVERLAPS[r % 8] != "a_empty" else "identical"
            else:
                kind = ("identical", "disjoint", "b_empty", "below", "above", "first", "last")[int(rng.integers(0, 7))]
            overlap.append(kind)
            rows2.append(_partner(cols, kind, rng))
        p2 = np.zeros(m + 1, dtype=np.int32)
        p2[1:] = np.cumsum([c.size for c in rows2])
        cat = lambda a: np.concatenate(a).astype(np.int32) if a else np.zeros(0, np.int32)      # noqa: E731
        c = Case(G, m, scale, K_COLS, p, cat(rows), p2, cat(rows2), overlap, blocks)
        special = rng.integers(0, m, size=min(m, 5))
        va, vb = _values(c.nnz, p, rng, special), _values(c.nnz2, p2, rng, special)
        c.vals = {k: (va[k], vb[k]) for k in va}
        # repeats, the first row, the last row and a reversed range
        extra = rng.integers(0, m, size=max(2, m // 8))
        c.rows_take = np.concatenate([[0, m - 1], np.arange(m - 1, -1, -1), [m - 1, 0], extra]).astype(np.int32)
        picks = rng.integers(0, K_COLS, size=K_COLS // 2).astype(np.int32)                       # with repeats
        c.cols_unsorted, c.cols_sorted = picks, np.sort(picks)
        lo, hi = band(G, scale)
        taken = float(lens[c.rows_take].sum()) / c.rows_take.size
        if lo < c.nnz / m <= hi and (scale != 1 or lo < taken <= hi) and c.nnz2 <= c.nnz:
            return c
    raise AssertionError(f"no case for G={G} m={m} scale={scale}")


def all_cases(groups=LANE_GROUPS, scale=1):
    return [make_case(G, m, scale) for G in groups for m in row_counts(G)]


def shuffled_rows(c, seed=1):
    """A with the entries of every row in random order: (indices, permutation of the entries)"""
    rng = np.random.default_rng([c.G, c.m, seed])
    perm = np.arange(c.nnz)
    for r in range(c.m):
        s, e = int(c.p[r]), int(c.p[r + 1])
        perm[s:e] = s + rng.permutation(e - s)
    return c.j[perm].copy(), perm


def dense(p, j, x, K):
    """m x K array of the stored values (columns unique), and the mask of stored cells"""
    m = p.size - 1
    rows = np.repeat(np.arange(m), np.diff(p))
    D = np.zeros((m, K), dtype=np.asarray(x).dtype)
    S = np.zeros((m, K), dtype=bool)
    D[rows, j] = x
    S[rows, j] = True
    return D, S
