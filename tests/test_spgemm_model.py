"""tests/spgemm_model.py against what it models: dense numpy on integer data (every order gives the same f64), the
vignette's 3 x 3 matrix, and the two rules that a dense product does not show: a lone -0.0 stays -0.0, and a sum that
cancels stays as an explicit zero."""
import time

import numpy as np

import spgemm_model as SM
from conftest import csr_to_dense, rand_csr


def int_csr(m, K, density, seed, sorted_cols=True):
    p, j, _ = rand_csr(m, K, density, seed, sorted_cols=sorted_cols)
    x = np.random.default_rng(seed).integers(-9, 10, size=j.size).astype(np.float64)
    return p, j, x


def test_model_against_dense_numpy_on_integer_data():
    for seed, (m, K, n) in enumerate([(7, 5, 9), (1, 1, 1), (30, 40, 20), (12, 1, 12), (5, 8, 1)]):
        Ap, Aj, Ax = int_csr(m, K, 0.4, 10 + seed, sorted_cols=False)
        Bp, Bj, Bx = int_csr(K, n, 0.4, 20 + seed, sorted_cols=False)
        p, j, x = SM.spgemm(Ap, Aj, Ax, Bp, Bj, Bx, K, n)
        A, B = csr_to_dense(Ap, Aj, Ax, K), csr_to_dense(Bp, Bj, Bx, n)
        assert np.array_equal(SM.to_dense(p, j, x, n), A @ B)
        symbolic = ((A != 0).astype(float) @ (B != 0).astype(float)) != 0   # stored zeros are entries too
        stored = csr_to_dense(Ap, Aj, np.ones(Aj.size), K) @ csr_to_dense(Bp, Bj, np.ones(Bj.size), n) != 0
        assert np.array_equal(SM.to_dense(p, j, np.ones(j.size), n) != 0, stored) and (symbolic <= stored).all()
        for r in range(m):
            assert np.all(np.diff(j[p[r]:p[r + 1]]) > 0)                    # sorted, unique
        assert SM.products(Ap, Aj, Bp, K) == int((np.diff(Bp)[Aj]).sum())


def test_the_vignettes_matrix_times_itself():
    p, j, x = np.array([0, 2, 3, 4], np.int32), np.array([0, 2, 2, 1], np.int32), np.array([1.0, 2, 3, 4])
    op, oj, ox = SM.spgemm(p, j, x, p, j, x, 3, 3)
    assert op.tolist() == [0, 3, 4, 5] and oj.tolist() == [0, 1, 2, 1, 2] and ox.tolist() == [1.0, 8.0, 2.0, 12.0, 12.0]


def test_a_lone_negative_zero_stays_and_a_sum_starts_from_its_first_term():
    Ap, Aj = np.array([0, 1, 3], np.int32), np.array([0, 0, 1], np.int32)
    Ax = np.array([-1.0, -1.0, 1.0])
    Bp, Bj, Bx = np.array([0, 1, 2], np.int32), np.array([0, 0], np.int32), np.array([0.0, -0.0])
    _, j, x = SM.spgemm(Ap, Aj, Ax, Bp, Bj, Bx, 2, 1)
    assert j.tolist() == [0, 0]
    assert np.signbit(x[0]) and x[0] == 0.0                                # -1 * 0 = -0, nothing added to it
    assert np.signbit(x[1]) and x[1] == 0.0                                # (-1 * 0) + (1 * -0) = -0 + -0 = -0
    Ax2 = np.array([-1.0, -1.0, -1.0])                                      # (-1 * 0) + (-1 * -0) = -0 + +0 = +0
    _, _, x2 = SM.spgemm(Ap, Aj, Ax2, Bp, Bj, Bx, 2, 1)
    assert not np.signbit(x2[1]) and x2[1] == 0.0


def test_a_sum_that_cancels_is_kept_as_a_zero():
    Ap, Aj, Ax = np.array([0, 2], np.int32), np.array([0, 1], np.int32), np.array([2.0, -2.0])
    Bp, Bj, Bx = np.array([0, 2, 3], np.int32), np.array([0, 1, 1], np.int32), np.array([5.0, 3.0, 3.0])
    p, j, x = SM.spgemm(Ap, Aj, Ax, Bp, Bj, Bx, 2, 2)
    assert p.tolist() == [0, 2] and j.tolist() == [0, 1] and x.tolist() == [10.0, 0.0]


def test_repeated_a_columns_are_further_terms_and_bad_indices_are_skipped():
    Ap, Aj, Ax = np.array([0, 4], np.int32), np.array([1, 1, 7, -1], np.int32), np.array([1.0, 2.0, 9.0, 9.0])
    Bp, Bj, Bx = np.array([0, 0, 3], np.int32), np.array([2, 5, 0], np.int32), np.array([1.0, 1.0, 4.0])
    p, j, x = SM.spgemm(Ap, Aj, Ax, Bp, Bj, Bx, 2, 3)
    assert j.tolist() == [0, 2] and x.tolist() == [12.0, 3.0] and SM.products(Ap, Aj, Bp, 2) == 6
    assert SM.row_bounds(Ap, Aj, Bp, 2, 3).tolist() == [3]


def test_logical_and_pattern_kinds():
    NA = SM.NA_INT
    assert np.array_equal(SM.as_double(None, 3), np.ones(3))
    v = SM.as_double(np.array([1, 0, NA], np.int32), 3)
    assert v[:2].tolist() == [1.0, 0.0] and v[2:].view(np.uint64)[0] == 0x7FF00000000007A2


def test_two_million_products_are_folded_quickly():
    Ap, Aj, Ax = int_csr(2000, 500, 0.1, 1)
    Bp, Bj, Bx = int_csr(500, 400, 0.05, 2)
    assert SM.products(Ap, Aj, Bp, 500) > 1_900_000
    t0 = time.perf_counter()
    p, j, x = SM.spgemm(Ap, Aj, Ax, Bp, Bj, Bx, 500, 400)
    assert time.perf_counter() - t0 < 1.0                           # some 0.3 s: a Python loop per run would take minutes
    assert np.array_equal(SM.to_dense(p, j, x, 400), csr_to_dense(Ap, Aj, Ax, 500) @ csr_to_dense(Bp, Bj, Bx, 400))
