"""The batched row concat: exports.concat_csr_batch (one staging upload, the device table, two launches) and the
mxd_csr_rbind_batch call itself on guarded buffers, both against the CPU restatement of concat_csr_batch
(src/rbind.cpp:24-173).  Bit-exact on indptr / indices; values exact with NaN-ness compared.

What the kernels can get wrong, and the case that shows it: the search for the operand of a row / an entry when
several operands share one offset (zero-row matrices, zero-entry operands); the tile that lies inside one operand
(a straight copy) against the one that spans operands (offsets staged in LDS) against the one whose span is wider
than the staging area (the table is searched); boundaries one before, on and one after the tile size; the value
conversions of all seven input kinds into the three output kinds."""
import numpy as np
import pytest

from bind_cases import (STAGE, TILE, dev_rbind_batch, empty_rows, matrix, matrix_of_nnz, nnz_of, same_csr, vector)
from matrixextra_amd import exports as G
from oracle import oracle as O

pytestmark = pytest.mark.gpu
COUNTS = [0, 1, 2, 3, 65, 301]


def all_kinds(n, seed):
    """n operands cycling through the seven kinds, 10 x 3 matrices (test-rbind.R:8) and vectors of 0..3 entries"""
    rng = np.random.default_rng(seed)
    return [matrix(k % 7, 10, 3, rng) if k % 7 <= 2 else vector(k % 7, int(rng.integers(0, 4)), 3, rng)
            for k in range(n)]


def tiny_vectors(n, seed):
    """only vectors of 0..3 entries, with runs of empty ones: one tile spans them all"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 4, size=n)
    sizes[n // 3:n // 3 + 7] = 0
    sizes[:2] = 0
    return [vector(3 + k % 4, int(s), 3, rng) for k, s in enumerate(sizes)]


def at_tile_edges(seed):
    """operand boundaries at TILE - 1, TILE, TILE + 1 and again around 2 * TILE and 3 * TILE"""
    rng = np.random.default_rng(seed)
    return [matrix_of_nnz(0, TILE - 1, 35, rng), vector(3, 1, 35, rng), vector(4, 1, 35, rng),      # 1023, 1024, 1025
            matrix_of_nnz(1, TILE - 2, 35, rng), vector(6, 2, 35, rng), vector(5, 0, 35, rng),      # 2047, 2049
            matrix_of_nnz(2, TILE - 1, 35, rng), matrix_of_nnz(0, 1, 35, rng)]                      # 3072, 3073


def empties(where, seed):
    """a zero-row matrix and a zero-entry matrix with rows in first / middle / last place"""
    rng = np.random.default_rng(seed)
    body = [matrix(0, 10, 3, rng), vector(5, 2, 3, rng), matrix(1, 10, 3, rng), vector(4, 0, 3, rng)]
    gap = [empty_rows(0, 0), empty_rows(1, 4), empty_rows(2, 0)]
    at = {"first": 0, "middle": 2, "last": len(body)}[where]
    return body[:at] + gap + body[at:]


def large_between_small(seed):
    rng = np.random.default_rng(seed)
    return [vector(3, 2, 35, rng), matrix(1, 10, 3, rng), matrix_of_nnz(0, 4 * TILE + 137, 35, rng), vector(6, 3, 35, rng),
            matrix(2, 10, 3, rng)]


def beyond_the_staging_area(seed):
    """more operands inside one tile than its LDS staging holds: almost all of them empty"""
    rng = np.random.default_rng(seed)
    sizes = np.zeros(STAGE + 600, int)
    sizes[[0, 5, STAGE // 2, STAGE + 1, STAGE + 599]] = [2, 1, 3, 2, 1]
    return [vector(3 + k % 4, int(s), 3, rng) for k, s in enumerate(sizes)]


CASES = {f"kinds{n}": all_kinds(n, 100 + n) for n in COUNTS}
CASES.update({f"vectors{n}": tiny_vectors(n, 200 + n) for n in COUNTS[3:]})
CASES["tile_edges"] = at_tile_edges(301)
CASES.update({f"empties_{w}": empties(w, 302) for w in ("first", "middle", "last")})
CASES["only_empties"] = [empty_rows(0, 0), empty_rows(2, 3), vector(3, 0, 3, np.random.default_rng(0)), empty_rows(1, 0)]
CASES["large_between_small"] = large_between_small(303)
CASES["beyond_staging"] = beyond_the_staging_area(304)
WANT = {}


def want(name, out_kind):
    """the oracle's result, computed once and shared by both tests"""
    if (name, out_kind) not in WANT:
        WANT[name, out_kind] = O.concat_csr_batch(CASES[name], out_kind)
    return WANT[name, out_kind]


def test_the_cases_are_what_they_claim():
    assert [len(CASES[f"kinds{n}"]) for n in COUNTS] == COUNTS
    ends = np.cumsum([np.asarray(o[2]).size for o in CASES["tile_edges"]])
    assert {TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1, 3 * TILE}.issubset(set(ends.tolist()))
    assert 0 < nnz_of(CASES["vectors301"]) < TILE and 0 < nnz_of(CASES["beyond_staging"]) < TILE
    assert len(CASES["beyond_staging"]) > STAGE
    assert nnz_of(CASES["large_between_small"]) > 4 * TILE


@pytest.mark.parametrize("out_kind", [0, 1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_export_concat_csr_batch(gpu, name, out_kind):
    same_csr(G.concat_csr_batch(CASES[name], out_kind), want(name, out_kind))


@pytest.mark.parametrize("out_kind", [0, 1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_device_rbind_batch_on_guarded_buffers(gpu, name, out_kind):
    same_csr(dev_rbind_batch(CASES[name], out_kind), want(name, out_kind))


def test_export_batch_beyond_the_pipelined_transfer_size(gpu):
    """operands of more than 16 MiB together go up through the pinned transfer slots, gathered from the operands that
    cross each 8 MiB chunk: boundaries inside a chunk, on none of its ends, and small operands between large ones"""
    rng = np.random.default_rng(305)
    objs = []
    for k in range(36):
        objs += [matrix_of_nnz(0 if k % 3 else 1, 50_000 + 17 * k, 35, rng), vector(3 + k % 4, k % 4, 35, rng)]
    assert sum(a.nbytes for o in objs for a in o[1:4] if a is not None) > 18 << 20
    for out_kind in (0, 1):
        same_csr(G.concat_csr_batch(objs, out_kind), O.concat_csr_batch(objs, out_kind))


def test_batch_refuses_rows_without_operands(gpu):
    lib = gpu.load()
    assert lib.mxd_csr_rbind_batch(None, 0, 0, 3, 0, None, None, None, None) != 0
    assert "mxd_csr_rbind_batch" in lib.mx_last_error().decode()
