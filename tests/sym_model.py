"""CPU model of the structured-matrix family (include/mxgpu_sym.h), in numpy alone: the general CSR of a symmetric CSR
that stores one triangle, of a unit-triangular CSR, and the triangle check.  It is the specification written out
(lexsort, no scipy), not a transcription of the kernels: tests/test_sym_host.py checks it against dense arithmetic
(T + T.T - diag(T), T + I), and the GPU tests compare the library with it bit for bit.

Symmetric expansion of the stored triangle `uplo`:
  uplo U: output row r = the mirrored segment, then the stored row r in its storage order
  uplo L: output row r = the stored row r, then the mirrored segment
  mirrored segment of row r: every stored (c, r) with c != r, as (r, c), ascending c, repeats in storage order
Unit-triangular expansion: row r gains (r, r) = 1.0 / TRUE / pattern in front (U) or behind (L).

The cases the GPU tests run are built here too, so that the host test can check what each of them is meant to hit."""
import json
import os

import numpy as np

NA_LOGICAL = np.int32(-2147483648)
NA_REAL = np.uint64(0x7FF00000000007A2).view(np.float64)
UPLOS = ("U", "L")
KINDS = ("d", "l", "n")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sym_reference_cases.json")


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def rows_of(p):
    return np.repeat(np.arange(p.size - 1, dtype=np.int64), np.diff(p))


def triangle_check(p, j, uplo, strict=False):
    """how many entries lie outside the triangle (strict: or on the diagonal)"""
    r, c = rows_of(p), np.asarray(j, dtype=np.int64)
    outside = (c < r) if uplo == "U" else (c > r)
    if strict:
        outside = outside | (c == r)
    return int(np.count_nonzero(outside))


def symmetric_to_general(p, j, x, uplo):
    """(p, j, x) of the general CSR; x None for a pattern.  A wrong-triangle entry is a ValueError."""
    if triangle_check(p, j, uplo):
        raise ValueError("entry outside the stored triangle")
    n, nnz = p.size - 1, j.size
    r, c, q = rows_of(p), np.asarray(j, dtype=np.int64), np.arange(nnz, dtype=np.int64)
    mq = q[c != r]
    mq = mq[np.lexsort((mq, r[mq], c[mq]))]             # by output row, then ascending c (= stored row), then storage
    out_row = np.concatenate([r, c[mq]])
    out_col = np.concatenate([c, r[mq]])
    src = np.concatenate([q, mq])
    mirrored = np.concatenate([np.zeros(nnz, dtype=np.int64), np.ones(mq.size, dtype=np.int64)])
    segment = 1 - mirrored if uplo == "U" else mirrored  # which half comes first
    within = np.concatenate([q, np.arange(mq.size, dtype=np.int64)])
    order = np.lexsort((within, segment, out_row))
    op = np.zeros(n + 1, dtype=np.int32)
    op[1:] = np.cumsum(np.bincount(out_row, minlength=n)[:n]) if n else 0
    return op, i32(out_col[order]), None if x is None else np.ascontiguousarray(x)[src[order]]


def unit_triangular_to_general(p, j, x, kind, uplo):
    """(p, j, x): every row gains its unit diagonal in front (U) or behind (L).  The input must be strictly triangular."""
    if triangle_check(p, j, uplo, strict=True):
        raise ValueError("entry on the diagonal or outside the stored triangle")
    n, nnz = p.size - 1, j.size
    one = {"d": np.float64(1.0), "l": np.int32(1), "n": None}[kind]
    op = i32(np.asarray(p, dtype=np.int64) + np.arange(n + 1))
    oj = np.empty(nnz + n, dtype=np.int32)
    ox = None if kind == "n" else np.empty(nnz + n, dtype=np.asarray(x).dtype)
    for r in range(n):
        s, e, o = int(p[r]), int(p[r + 1]), int(op[r])
        d_at, s_at = (o, o + 1) if uplo == "U" else (o + e - s, o)
        oj[d_at] = r
        oj[s_at:s_at + e - s] = j[s:e]
        if ox is not None:
            ox[d_at] = one
            ox[s_at:s_at + e - s] = x[s:e]
    return op, oj, ox


def to_dense(p, j, x, n):
    """dense f64 image, repeated entries summed (a pattern's entries count 1)"""
    D = np.zeros((p.size - 1, n))
    np.add.at(D, (rows_of(p), np.asarray(j, dtype=np.int64)), 1.0 if x is None else np.asarray(x, dtype=np.float64))
    return D


def pick_group(avg, lo=4):
    g = lo
    while g < 64 and g < avg:
        g <<= 1
    return g


# ---- the cases ------------------------------------------------------------------------------------------------------------
def csr_of(n, r, c, uplo, keep_order=False):
    """CSR (p, j) of the triplets (r, c), given in the upper triangle (r <= c) and swapped for uplo L.  Rows are sorted
    by column unless keep_order, which keeps the triplets' order inside a row."""
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    assert np.all(r <= c) and (r.size == 0 or (r.min() >= 0 and c.max() < n))
    if uplo == "L":
        r, c = c, r
    order = np.argsort(r, kind="stable") if keep_order else np.lexsort((c, r))
    p = np.zeros(n + 1, dtype=np.int32)
    if n:
        p[1:] = np.cumsum(np.bincount(r, minlength=n))
    return p, i32(c[order])


def random_upper(n, per_row, seed, diagonal=True):
    """about per_row * n distinct entries of the upper triangle, the diagonal included or not"""
    rng = np.random.default_rng(seed)
    r, c = np.triu_indices(n, 0 if diagonal else 1)
    take = rng.random(r.size) < per_row * n / max(r.size, 1)
    return r[take], c[take]


# output average row length -> lanes per row the fill must choose; n = 200, stored entries off the diagonal only
GROUP_TARGETS = {4: 3.0, 8: 7.0, 16: 14.0, 32: 28.0, 64: 56.0}
GROUP_N = 200


def triplet_cases():
    """name -> (n, r, c, keep_order), triplets in the upper triangle"""
    with open(GOLDEN) as f:
        gold = json.load(f)
    out = {}
    e = np.zeros(0, dtype=np.int64)
    out["n0"] = (0, e, e, False)
    out["n1-diagonal"] = (1, [0], [0], False)
    out["n1-empty"] = (1, e, e, False)
    for name in ("sy", "tri"):
        g = gold[name]
        p = np.asarray(g["p"])
        out["reference-" + name] = (g["n"], rows_of(p), g["j"], False)
    out["all-diagonal"] = (70, np.arange(70), np.arange(70), False)
    out["no-diagonal"] = (70,) + random_upper(70, 4, 1, diagonal=False) + (False,)
    rng = np.random.default_rng(2)
    live = np.arange(10, 60, 3)                          # rows and columns 0-9, 60-89 and two of every three are empty
    a, b = live[rng.integers(0, live.size, 80)], live[rng.integers(0, live.size, 80)]
    rc = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)]), axis=1)
    out["empty-rows-and-columns"] = (90, rc[0], rc[1], False)
    r, c = random_upper(130, 1, 3, diagonal=False)
    keep = r > 0
    out["full-first-row"] = (130, np.concatenate([np.zeros(130, dtype=np.int64), r[keep]]),
                             np.concatenate([np.arange(130), c[keep]]), False)
    out["n300-crosses-the-tiles"] = (300,) + random_upper(300, 30, 4) + (False,)
    for G, avg in GROUP_TARGETS.items():
        out[f"lanes-{G}"] = (GROUP_N,) + random_upper(GROUP_N, avg / 2, 10 + G, diagonal=False) + (False,)
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 60, 700), rng.integers(0, 60, 700)
    r = np.concatenate([np.minimum(a, b), [7, 7, 7, 20, 20]])           # repeats anywhere, diagonal repeats for sure
    c = np.concatenate([np.maximum(a, b), [7, 7, 7, 20, 20]])
    shuffle = rng.permutation(r.size)
    out["unsorted-with-repeats"] = (60, r[shuffle], c[shuffle], True)
    return out


def special_values(kind, nnz, p, j, seed):
    """values of a case: distinct ordinary ones, with the special ones on the first entries (and an explicit zero on
    the first diagonal and the first off-diagonal entry when there are any)"""
    if kind == "n":
        return None
    rng = np.random.default_rng(seed)
    if kind == "l":
        x = rng.choice(np.array([0, 1, NA_LOGICAL], dtype=np.int32), size=nnz, p=[0.25, 0.5, 0.25])
        if nnz >= 3:
            x[:3] = [NA_LOGICAL, 0, 1]
        return x
    x = (np.arange(nnz, dtype=np.float64) + 1.0) * 0.25 * rng.choice([-1.0, 1.0], size=nnz)
    special = np.array([NA_REAL, np.nan, np.inf, -np.inf, -0.0, 0.0])
    if nnz >= 2 * special.size:
        x[nnz - special.size:] = special
    r = rows_of(p)
    for mask in (np.asarray(j) == r, np.asarray(j) != r):
        at = np.flatnonzero(mask)
        if at.size > 2:
            x[at[1]] = 0.0
    return x


def case(name, uplo, kind, cases=None):
    """(n, p, j, x) of a case"""
    n, r, c, keep = (cases or triplet_cases())[name]
    p, j = csr_of(n, r, c, uplo, keep_order=keep)
    return n, p, j, special_values(kind, j.size, p, j, seed=len(name))
