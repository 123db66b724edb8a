"""tests/gram_model.py against tests/spgemm_model.py: the masked fold is the triangle of the full product bit for bit
(each cell is folded on its own, in the same order), for any m x n; the window sizes, the two product counts and the
masked bounds against a loop over the rows; and what the Gram product's symmetry rests on: the full crossprod is
bitwise symmetric always, the full tcrossprod only when the rows of X are sorted."""
import numpy as np

import gram_model as GM
import spgemm_model as SM
from conftest import rand_csr


def general_csr(m, K, density, seed, sorted_cols=True):
    p, j, _ = rand_csr(m, K, density, seed, sorted_cols=sorted_cols)
    rng = np.random.default_rng(seed)
    return p, j, rng.normal(size=j.size) * 10.0 ** rng.integers(-3, 4, j.size)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a[:2], b[:2])) and np.array_equal(bits(a[2]), bits(b[2]))


def test_the_masked_fold_is_the_triangle_of_the_full_product():
    for seed, (m, K, n) in enumerate([(60, 37, 60), (37, 60, 37), (50, 20, 13), (13, 20, 50), (1, 1, 1), (9, 4, 0)]):
        Ap, Aj, Ax = general_csr(m, K, 0.15, 30 + seed, sorted_cols=False)
        Bp, Bj, Bx = general_csr(K, n, 0.15, 40 + seed, sorted_cols=False)
        full = SM.spgemm(Ap, Aj, Ax, Bp, Bj, Bx, K, n)
        for uplo in (GM.UPPER, GM.LOWER):
            tri = GM.spgemm_tri(Ap, Aj, Ax, Bp, Bj, Bx, K, n, uplo)
            assert same(tri, GM.triangle_of(*full, uplo))
            rows = np.repeat(np.arange(m), np.diff(tri[0]))
            assert np.all(tri[1] >= rows) if uplo == GM.UPPER else np.all(tri[1] <= rows)
            assert np.all(np.diff(tri[0]) <= GM.window(uplo, m, n))
        up, lo = GM.spgemm_tri(Ap, Aj, Ax, Bp, Bj, Bx, K, n, GM.UPPER), GM.spgemm_tri(Ap, Aj, Ax, Bp, Bj, Bx, K, n, GM.LOWER)
        on_diagonal = int((np.repeat(np.arange(m), np.diff(full[0])) == full[1]).sum())
        assert up[1].size + lo[1].size == full[1].size + on_diagonal     # the diagonal is kept by both masks


def test_the_window_and_the_bounds_against_a_loop():
    assert GM.window(GM.UPPER, 5, 3).tolist() == [3, 2, 1, 0, 0] and GM.window(GM.LOWER, 5, 3).tolist() == [1, 2, 3, 3, 3]
    assert GM.window(GM.UPPER, 2, 4).tolist() == [4, 3] and GM.window(GM.LOWER, 2, 4).tolist() == [1, 2]
    m, K, n = 25, 12, 17
    Ap, Aj, _ = general_csr(m, K, 0.3, 50, sorted_cols=False)
    Bp, Bj, _ = general_csr(K, n, 0.3, 51)
    Aj = Aj.copy()
    Aj[::7] = K + 3                                                      # an A column outside [0, K) gives no step
    for uplo in (GM.UPPER, GM.LOWER):
        for b_sorted in (0, 1):
            f = np.zeros(m, dtype=np.int64)
            used = np.zeros(m, dtype=np.int64)
            for i in range(m):
                for k in Aj[Ap[i]:Ap[i + 1]]:
                    if 0 <= k < K:
                        cols = Bj[Bp[k]:Bp[k + 1]]
                        f[i] += int((cols >= i).sum() if uplo == GM.UPPER else (cols <= i).sum()) if b_sorted else cols.size
                        used[i] += 1
            assert GM.products(Ap, Aj, Bp, Bj, K, uplo, b_sorted) == int(f.sum())
            assert np.array_equal(GM.row_bounds(Ap, Aj, Bp, Bj, K, n, uplo, b_sorted), np.minimum(f, GM.window(uplo, m, n)))
            mean = np.where(used > 0, -(-f // np.maximum(used, 1)), 0)
            assert np.array_equal(GM.mean_step(Ap, Aj, Bp, Bj, K, uplo, b_sorted), mean)
        assert GM.products(Ap, Aj, Bp, Bj, K, uplo, 0) == SM.products(Ap, Aj, Bp, K)
        # the trimmed bound is never above the untrimmed one, and never below the row's entries
        tri = GM.spgemm_tri(Ap, Aj, None, Bp, Bj, None, K, n, uplo)
        ub1, ub0 = (GM.row_bounds(Ap, Aj, Bp, Bj, K, n, uplo, s) for s in (1, 0))
        assert np.all(np.diff(tri[0]) <= ub1) and np.all(ub1 <= ub0)


def test_the_transpose_is_stable_and_the_gram_product_is_that_of_the_two_operands():
    p, j, x = general_csr(40, 25, 0.2, 60, sorted_cols=False)
    tp, tj, tx = GM.transpose(p, j, x, 25)
    assert all(np.all(np.diff(tj[tp[c]:tp[c + 1]]) > 0) for c in range(25))
    D = np.zeros((40, 25))
    D[np.repeat(np.arange(40), np.diff(p)), j] = x
    T = np.zeros((25, 40))
    T[np.repeat(np.arange(25), np.diff(tp)), tj] = tx
    assert np.array_equal(T, D.T)
    for trans in (0, 1):
        for uplo in (GM.UPPER, GM.LOWER):
            got = GM.gram(p, j, x, (40, 25), trans, uplo)
            full = SM.spgemm(tp, tj, tx, p, j, x, 40, 25) if trans else SM.spgemm(p, j, x, tp, tj, tx, 25, 40)
            assert same(got, GM.triangle_of(*full, uplo))


def test_which_full_gram_products_are_bitwise_symmetric():
    """crossprod always; tcrossprod when the rows of X are sorted, and not otherwise: the common columns of two rows then
    meet in different orders.  This is why the mirror sorts an unsorted operand first, for both forms."""
    def symmetric(full, n):
        D = np.zeros((n, n), dtype=np.uint64)
        S = np.zeros((n, n), dtype=bool)
        rows = np.repeat(np.arange(n), np.diff(full[0]))
        D[rows, full[1]], S[rows, full[1]] = bits(full[2]), True
        return np.array_equal(S, S.T) and np.array_equal(D, D.T)

    p, j, x = general_csr(60, 37, 0.3, 70, sorted_cols=False)
    tp, tj, tx = GM.transpose(p, j, x, 37)
    assert symmetric(SM.spgemm(tp, tj, tx, p, j, x, 60, 37), 37)                      # crossprod, rows unsorted
    assert not symmetric(SM.spgemm(p, j, x, tp, tj, tx, 37, 60), 60)                  # tcrossprod, rows unsorted
    sp, sj, sx = GM.sort_rows(p, j, x)
    assert all(np.all(np.diff(sj[sp[r]:sp[r + 1]]) > 0) for r in range(60))
    stp, stj, stx = GM.transpose(sp, sj, sx, 37)
    assert symmetric(SM.spgemm(sp, sj, sx, stp, stj, stx, 37, 60), 60)                # tcrossprod, rows sorted
    assert symmetric(SM.spgemm(stp, stj, stx, sp, sj, sx, 60, 37), 37)
