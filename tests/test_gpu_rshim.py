"""The .Call shim (matrixextra_amd/csrc/r_shim.cpp) on the device: every recorded call of the fixtures replayed
through `.Call` as R would make it, over the stand-in for R's C API (tests/rstub, tests/rcall.py) and the real
libmxgpu.so.  The Python mirror (exports.py) is pinned by the same records elsewhere; this pins the second
marshalling layer, the one the product ships.

No tolerance is introduced here.  Every bar is the one the same records already have: tests/refpin.py for
reference_golden.npz, bit for bit for assign_golden.npz (tests/test_gpu_assign.py), tests/coo_sort_model.py for
coo_sort_golden.npz, the yardsticks of tests/test_gpu_outer.py for the eight matmul_rowvec / colvec / spcolvec
routines, and the numpy models of tests/test_gpu_transpose.py / tests/test_gpu_coo.py for the shim's own two routines.

Each call runs plain and under the stand-in's gctorture-like mode; after each the protect stack is where it was, the
precious list and the violation log are empty and no argument is dead or changed beyond what the record says.
All in one process: the stand-in and the library are loaded once."""
import numpy as np
import pytest

import assign_model as AM
import coo_sort_model as CM
import rcall
import refpin
import rshim_cases as RC
import test_gpu_coo as TC
import test_gpu_outer as TO
import test_gpu_transpose as TT
from test_gpu_outer import csc_operand  # noqa: F401 - the fixture of the row-vector cases

pytestmark = pytest.mark.gpu

GOLDEN = [(n, r) for n, r in enumerate(RC.GOLDEN) if r.fn not in RC.NOT_IN_SHIM]


@pytest.fixture(scope="module")
def shim(gpu):
    s = rcall.load(fake=False)
    yield s
    s.torture(False)
    s.reset()


def settled(shim, what, changed=()):
    """after a call: the stand-in saw nothing wrong and the arguments are alive and, but for `changed`, as they were"""
    shim.assert_clean(what)
    last = shim.last
    after = shim.arguments_after()
    for k, (sx, a, b) in enumerate(zip(last["sexps"], last["before"], after)):
        assert sx == shim.nil or not shim.lib.rstub_dead(sx), f"{what}: argument {k} was collected"
        assert k in changed or a == b, f"{what}: argument {k} changed"


def both_modes(shim):
    for torture in (False, True):
        shim.reset()
        shim.torture(torture)
        yield torture
    shim.torture(False)


# ----------------------------------------------------------------------------- reference_golden.npz
@pytest.mark.parametrize("rec", [r for _, r in GOLDEN], ids=[f"{n:03d}-{r!r}" for n, r in GOLDEN])
def test_reference_records_through_the_shim(shim, rec):
    assert refpin.has(shim, rec.fn), f"the shim registers no {rec.fn}"
    for torture in both_modes(shim):
        got, live = refpin.replay(shim, rec)
        refpin.compare_device(rec, got, live)
        settled(shim, f"{rec!r} torture={torture}", changed=set(rec.post))


# ----------------------------------------------------------------------------- assign_golden.npz
@pytest.mark.parametrize("name", sorted(AM.ORDER))
def test_assign_records_through_the_shim(shim, name):
    """as tests/test_gpu_assign.py::test_golden_replay: the three vectors bit for bit, the same vectors returned as
    they came in (the alias flags), the inputs unchanged; unsorted inputs are compared after sorting both results"""
    n = 0
    for r in AM.load()[0]:
        if r["name"] != name:
            continue
        for torture in both_modes(shim):
            p, j, x = r["p"].copy(), r["j"].copy(), r["x"].copy()
            args = AM.call_args(name, r["args"])
            kept = [a.copy() if isinstance(a, np.ndarray) else a for a in args]
            out = getattr(shim, name)(p, j, x, *args)
            what = f"{r['label']} torture={torture}"
            assert list(out) == ["indptr", "indices", "values"], what
            got = (out["indptr"], out["indices"], out["values"])
            want = (r["out_p"], r["out_j"], r["out_x"])
            assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float64, what
            if r["sorted"]:
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
                assert np.array_equal(AM.bits(got[2]), AM.bits(want[2])), what
                assert (int(got[0] is p), int(got[1] is j), int(got[2] is x)) == r["alias"], what
            else:
                gs, ws = AM.sort_rows(*got), AM.sort_rows(*want)
                assert np.array_equal(got[0], want[0]) and np.array_equal(gs[0], ws[0]), what
                assert np.array_equal(AM.bits(gs[1]), AM.bits(ws[1])), what
            assert np.array_equal(p, r["p"]) and np.array_equal(j, r["j"]) and np.array_equal(AM.bits(x), AM.bits(r["x"]))
            for a, b in zip(args, kept):
                assert np.array_equal(a, b) if isinstance(a, np.ndarray) else AM.bits(a) == AM.bits(b), what
            settled(shim, what)
        n += 1
    assert n >= 5


# ----------------------------------------------------------------------------- coo_sort_golden.npz
COO_RECORDS = CM.load()[0]


@pytest.mark.parametrize("rec", COO_RECORDS, ids=lambda r: f"{r['kind']}-{r['label']}")
def test_coo_sort_records_through_the_shim(shim, rec):
    """as tests/test_gpu_coo_sort.py::test_exports_match_the_reference_fixture: in place, on the caller's vectors"""
    inp = (rec["i"], rec["j"], rec["x"])
    for torture in both_modes(shim):
        got = CM.run(shim, rec["kind"], *inp)
        what = f"{rec['kind']} {rec['label']} torture={torture}"
        CM.assert_matches_reference(got, (rec["ri"], rec["rj"], rec["rx"]), what)
        CM.assert_equals_model(got, inp, what)
        settled(shim, what, changed={0, 1, 2})


# ----------------------------------------------------------------------------- the eight routines of test_gpu_outer.py
# its generators, its grid of sizes and patterns and its yardsticks
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_dense_outer_through_the_shim(shim, f32):
    name = "matmul_colvec_by_scolvecascsr" + ("_f32" if f32 else "")
    for m in TO.MS:
        for dim in TO.DIMS:
            for n, pattern in enumerate(TO.PATTERNS):
                p, j, x = TO.one_column(m, pattern, 100 * m + n)
                v = TO.dense_vector(dim, 7 * dim + m)
                with np.errstate(invalid="ignore", over="ignore"):
                    v = v.astype(np.float32) if f32 else v
                for torture in both_modes(shim):
                    what = f"{name} m={m} dim={dim} {pattern} torture={torture}"
                    TO.same_triple(getattr(shim, name)(v, p, j, x), TO.model_dense(v, p, x, f32), what)
                    settled(shim, what)


@pytest.mark.parametrize("kind", TO.KINDS)
def test_sparse_outer_through_the_shim(shim, kind):
    for m in TO.MS:
        for n, pattern in enumerate(TO.PATTERNS):
            p, j, x = TO.one_column(m, pattern, 100 * m + n)
            for length in (1, 70, 257):
                rng = np.random.default_rng(length + m)
                inner = np.sort(rng.permutation(np.arange(2, length))[:length // 3]).astype(np.int32)
                ends = np.unique(np.array([1, length], dtype=np.int32))
                for label, yi in (("every", np.arange(1, length + 1, dtype=np.int32)),
                                  ("ends", np.unique(np.concatenate([ends, inner]))), ("nothing", np.zeros(0, np.int32))):
                    yv = TO.svec_values(kind, yi.size, length + 3 * m)
                    for torture in both_modes(shim):
                        what = f"{kind} m={m} {pattern} length={length} {label} torture={torture}"
                        TO.same_triple(TO.call_svec(shim, kind, p, j, x, yi, yv, length),
                                       TO.model_svec(p, x, yi, yv, length, kind), what)
                        settled(shim, what)


@pytest.mark.parametrize("with_values", [True, False], ids=["values", "binary"])
def test_rowvec_by_csc_through_the_shim(shim, csc_operand, with_values):  # noqa: F811
    lens, p, i, x, v = csc_operand
    want = TO.model_rowvec(v, p, i, x if with_values else None)
    terms = np.abs((x if with_values else 1.0) * v[i].astype(np.float64))
    for torture in both_modes(shim):
        got = shim.matmul_rowvec_by_csc(v, p, i, x) if with_values else shim.matmul_rowvec_by_cscbin(v, p, i)
        assert got.dtype == np.float32 and got.shape == (1, lens.size)
        for c, n in enumerate(lens):
            bound = 2.0 * n * 2.0 ** -24 * terms[p[c]:p[c + 1]].sum()          # test_gpu_outer.py's bound
            err = abs(float(got[0, c]) - float(want[0, c]))
            print(f"column {c} (len {n}): |got - ref| = {err:.3e}, bound {bound:.3e}")
            assert got[0, c] == want[0, c] if n <= 1 else err <= bound
        settled(shim, f"rowvec values={with_values} torture={torture}")


# ----------------------------------------------------------------------------- the shim's own two routines
def _values(kind, n, rng):
    if kind == "d":                 # repeated cells are summed: no NaN here, whose payload a sum need not keep
        x = np.round(rng.normal(size=n), 3)
        x[:min(n, 2)] = [-0.0, 1e300][:min(n, 2)]
        return x
    if kind == "l":
        return rng.choice(np.array([0, 1, TT.NA_LGL], dtype=np.int32), size=n, p=[0.3, 0.5, 0.2])
    return None


def _triple(out, want, what):
    p, j, v = want
    assert list(out) == ["indptr", "indices", "values"], what
    assert out["indptr"].dtype == np.int32 and np.array_equal(out["indptr"], p), what
    assert np.array_equal(out["indices"], j), what
    if v is None:
        assert out["values"].size == 0, what
    else:
        assert out["values"].dtype == v.dtype and np.array_equal(out["values"].view(np.uint8), v.view(np.uint8)), what


@pytest.mark.parametrize("kind", ["d", "l", "n"])
def test_csr_transpose_through_the_shim(shim, kind):
    """numpy model of tests/test_gpu_transpose.py: unsorted rows with repeated (row, col) pairs; 300 columns are two
    radix passes, and an empty matrix"""
    rng = np.random.default_rng(3)
    for m, ncol, per_row in ((40, 300, 9), (1, 7, 5), (5, 3, 0)):
        lens = rng.integers(0, per_row + 1, size=m)
        p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        j = rng.integers(0, ncol, size=int(p[-1])).astype(np.int32)          # with replacement: repeats inside a row
        x = _values(kind, j.size, rng)
        for torture in both_modes(shim):
            what = f"transpose {kind} {m}x{ncol} torture={torture}"
            _triple(shim.mxgpu_csr_transpose(p, j, x, ncol), TT.ref_transpose(p, j, x, ncol), what)
            settled(shim, what)


@pytest.mark.parametrize("kind", ["d", "l", "n"])
def test_coo_to_csr_through_the_shim(shim, kind):
    """numpy model of tests/test_gpu_coo.py: shuffled triplets, a fifth of them repeats; two radix passes per key"""
    for m, n, nnz in ((300, 280, 900), (3, 4, 0)):
        i, j, x = TC.rand_coo(m, n, nnz, 5, dup_share=0.2 if nnz else 0.0, kind=kind)
        for torture in both_modes(shim):
            what = f"coo_to_csr {kind} {m}x{n} torture={torture}"
            _triple(shim.mxgpu_coo_to_csr(i, j, x, m, n), TC.ref_coo_to_csr(i, j, x, m, n), what)
            settled(shim, what)
    with pytest.raises(rcall.RError, match="different length"):
        shim.mxgpu_coo_to_csr(np.zeros(2, np.int32), np.zeros(3, np.int32), None, 3, 3)
    settled(shim, "coo_to_csr refusal")


# ----------------------------------------------------------------------------- coercion, as R callers pass arguments
CASES = {n: c for n, c in RC.first_cases().items() if n not in RC.NOT_IN_SHIM}


def _same_result(got, want, what):
    """the retyped call against the plain call: the same code on equal values, so bit for bit (refpin.exact)"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), what
        for key in want:
            _same_result(got[key], want[key], f"{what}[{key}]")
    elif isinstance(want, np.ndarray):
        refpin.exact(got, want, what)
    else:
        assert type(got) is type(want) and (got == want or (got != got and want != want)), what


@pytest.mark.parametrize("name", sorted(set(CASES) - set(RC.NO_COERCION)))
def test_retyped_arguments_give_the_same_result(shim, name):
    """an integer vector given as double, a double scalar for an int (nthreads, ncol, ...), a logical given as
    integer: every value converts exactly, so the result is the plain call's and the caller's objects are untouched"""
    case = CASES[name]
    shim.reset()
    shim.torture(False)
    plain = shim.call(name, case.live())
    for torture in both_modes(shim):
        live = case.live()
        got = shim.call(name, live, retype=True)
        what = f"{name} retyped torture={torture}"
        sig = rcall.signature(name)["args"]
        assert any(t != shim.lib.rstub_type(sx) for t, sx in
                   zip([rcall.SXP_OF.get(s) for s in sig], shim.last["sexps"]) if t is not None and sx != shim.nil), \
            f"{what}: nothing was retyped"
        _same_result(got, plain, what)
        settled(shim, what)
        for a, b in zip(live, case.args):
            assert not isinstance(a, np.ndarray) or a.tobytes() == b.tobytes(), what


def _family(name):
    return name.rsplit("_", 1)[0]


@pytest.mark.parametrize("name", RC.NO_COERCION)
def test_in_place_routines_refuse_index_vectors_of_another_type(shim, name):
    """sort_vector_indices_*, sort_coo_indices_* and reverse_columns_inplace_* write the caller's vectors, so a
    vector of another type cannot be coerced (the copy would be sorted, not the caller's): index vectors given as
    double are refused with the family's message and nothing is written"""
    case = CASES[name]
    for torture in both_modes(shim):
        live = case.live()
        what = f"{name} torture={torture}"
        with pytest.raises(rcall.RError) as e:
            shim.call(name, live, retype=True)
        assert str(e.value) == RC.NO_COERCION_MESSAGE[_family(name)], what
        settled(shim, what)
        for a, b in zip(live, case.args):
            assert not isinstance(a, np.ndarray) or a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("name", [n for n in RC.NO_COERCION if not n.endswith("_binary")])
def test_in_place_routines_and_values_of_another_type(shim, name):
    """integer index vectors with the values vector of another R type (a double one as integer, an integer or logical
    one as double): the sort routines refuse it and write nothing; reverse_columns_inplace_* takes it as absent, so the
    indices are reversed as the record says and the values stay as they are"""
    case = CASES[name]
    family = _family(name)
    pos = 1 if family == "sort_vector_indices" else 2
    wrong = rcall.INTSXP if case.args[pos].dtype == np.float64 else rcall.REALSXP
    for torture in both_modes(shim):
        live = case.live()
        what = f"{name} torture={torture}"
        if family == "reverse_columns_inplace":
            rec = next(r for r in RC.GOLDEN if r.fn == name and r.err is None)
            assert shim.call(name, live, as_types={pos: wrong}) is None, what
            assert 1 in rec.post and live[1].tobytes() == rec.post[1].tobytes(), f"{what}: the indices"
            assert live[pos].tobytes() == case.args[pos].tobytes() and live[0].tobytes() == case.args[0].tobytes(), what
            settled(shim, what, changed={1})
        else:
            with pytest.raises(rcall.RError) as e:
                shim.call(name, live, as_types={pos: wrong})
            assert str(e.value) == RC.NO_COERCION_VALUES_MESSAGE[family], what
            settled(shim, what)
            for a, b in zip(live, case.args):
                assert not isinstance(a, np.ndarray) or a.tobytes() == b.tobytes(), what
