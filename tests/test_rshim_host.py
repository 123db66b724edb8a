"""The .Call shim (matrixextra_amd/csrc/r_shim.cpp) compiled and run on the CPU: against the stand-in for R's C API
(tests/rstub) and a generated fake of the C-ABI (tests/rstub/make_fake_mxgpu.py), both built by build() into
tests/_build/.  No GPU and no libmxgpu.so are involved.  A missing tests/_build is a failure, not a skip.

1. the stand-in sees what it claims to see (it is the instrument of everything below and of tests/test_gpu_rshim.py);
2. what R_init_mxgpu_r registers is the reference's CallEntries[] by name and arity, under the exported symbols, and
   is what the overlay rebinds; the recorded routines the shim lacks are exactly a named list;
3. every registered routine, called with the arguments of its first record, in the fake's three modes, plain and
   under the gctorture-like mode: handles released exactly once, PROTECT balance, precious list, result types,
   lengths, names and aliasing, inputs untouched.

Everything here is exact: counts, types, names and bit patterns.  There is no tolerance to choose."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import rcall
import rshim_cases as RC

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "rstub"))
import make_fake_mxgpu as FAKE  # noqa: E402

from matrixextra_amd import _lib  # noqa: E402

NA_INT = -2147483648
NA_REAL_BITS = 0x7FF00000000007A2
MODES = FAKE.MODES
CASES = {n: c for n, c in RC.first_cases().items() if n not in RC.NOT_IN_SHIM}     # see the registration tests


@pytest.fixture(scope="module")
def shim():
    s = rcall.load(fake=True)
    lib = s.lib
    lib.fake_set_mode.argtypes = (C.c_int,)
    lib.fake_set_canned.argtypes = (C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int)
    for fn in ("fake_begun", "fake_finished", "fake_discarded", "fake_double_released", "fake_unknown_released",
               "fake_open", "fake_calls"):
        getattr(lib, fn).restype = C.c_long
    lib.fake_last_call.restype = C.c_char_p
    lib.fake_call_name.restype, lib.fake_call_name.argtypes = C.c_char_p, (C.c_int,)
    lib.fake_call_arg_int.restype, lib.fake_call_arg_int.argtypes = C.c_int64, (C.c_int, C.c_int)
    lib.fake_call_arg_double.restype, lib.fake_call_arg_double.argtypes = C.c_double, (C.c_int, C.c_int)
    for fn, res, args in (("Rf_coerceVector", C.c_void_p, (C.c_void_p, C.c_uint)), ("Rf_asInteger", C.c_int, (C.c_void_p,)),
                          ("Rf_asLogical", C.c_int, (C.c_void_p,)), ("Rf_asReal", C.c_double, (C.c_void_p,)),
                          ("Rf_nrows", C.c_int, (C.c_void_p,)), ("Rf_ncols", C.c_int, (C.c_void_p,))):
        f = getattr(lib, fn)
        f.restype, f.argtypes = res, args
    return s


@pytest.fixture
def fresh(shim):
    shim.reset()
    shim.torture(False)
    shim.lib.fake_reset()
    shim.lib.fake_set_mode(MODES["succeed"])
    yield shim
    shim.torture(False)
    shim.reset()


def ledger(shim):
    lib = shim.lib
    return dict(begun=lib.fake_begun(), finished=lib.fake_finished(), discarded=lib.fake_discarded(),
                double=lib.fake_double_released(), unknown=lib.fake_unknown_released(), open=lib.fake_open())


# ============================================================================= 1. the stand-in checks itself
def selftest(shim, name, *sexps):
    status, out = shim.raw_call(shim.symbol("rstub_selftest_" + name), list(sexps))
    return status, out, shim.violations()


def test_na_constants_are_rs(fresh):
    assert C.c_double.in_dll(fresh.lib, "R_NaReal").value != C.c_double.in_dll(fresh.lib, "R_NaReal").value      # a NaN
    assert C.c_uint64.in_dll(fresh.lib, "R_NaReal").value == NA_REAL_BITS
    assert fresh.lib.Rf_asInteger(fresh.vector(rcall.LGLSXP, [NA_INT])) == NA_INT


def test_an_unbalanced_unprotect_is_logged(fresh):
    x = fresh.vector(rcall.INTSXP, [1])
    status, out, (n, log) = selftest(fresh, "unprotect_too_many", x)
    assert status == 0 and n == 1 and "UNPROTECT(1)" in log and "imbalance" in log
    fresh.lib.rstub_clear_violations()
    status, out, (n, log) = selftest(fresh, "leaves_protected", x)
    assert n == 1 and "protect stack at depth 1" in log
    assert fresh.lib.rstub_protect_depth() == 0                    # and is reset, as R resets it after a .Call


def test_torture_kills_what_nothing_protects(fresh):
    nil = fresh.nil
    # without torture nothing is collected
    status, out, (n, _) = selftest(fresh, "unprotected", nil)
    assert status == 0 and n == 0 and fresh.read_vector(out).tolist() == [1]
    fresh.torture(True)
    status, out, (n, log) = selftest(fresh, "unprotected", nil)
    assert n >= 1 and "dead (collected) integer vector of length 4" in log
    assert fresh.read_vector(out).view(np.uint32).tolist() == [0xDFDFDFDF]      # the poison was read
    fresh.lib.rstub_clear_violations()
    status, out, (n, log) = selftest(fresh, "protected", nil)
    assert status == 0 and n == 0, log
    assert fresh.read_vector(out).tolist() == [1]
    status, out, (n, log) = selftest(fresh, "returns_collected", nil)
    assert n == 1 and "returned a dead" in log


def test_arguments_and_their_attributes_survive_torture(fresh):
    x = fresh.vector(rcall.REALSXP, np.arange(6.0), dim=(2, 3))
    fresh.torture(True)
    status, out, (n, log) = selftest(fresh, "protected", x)
    assert n == 0 and not fresh.lib.rstub_dead(x)
    assert fresh.lib.Rf_nrows(x) == 2 and fresh.lib.Rf_ncols(x) == 3 and fresh.violations()[0] == 0


def test_a_requested_allocation_failure_is_rs_error(fresh):
    fresh.lib.rstub_fail_allocation(2)
    status, out, (n, _) = selftest(fresh, "protected", fresh.nil)
    assert status == 1 and "cannot allocate vector of length 1" in fresh.error_message() and n == 0
    assert fresh.lib.rstub_protect_depth() == 0 and fresh.lib.rstub_allocations() == 2
    status, out, (n, _) = selftest(fresh, "protected", fresh.nil)          # one call only
    assert status == 0 and n == 0


def test_an_error_runs_each_pending_cleanup_once(fresh):
    counter = fresh.vector(rcall.INTSXP, [0])
    status, out, (n, _) = selftest(fresh, "cleanup", fresh.vector(rcall.LGLSXP, [0]), counter)
    assert status == 0 and n == 0 and fresh.read_vector(counter).tolist() == [1]          # no error: once, at the end
    status, out, (n, log) = selftest(fresh, "cleanup", fresh.vector(rcall.LGLSXP, [1]), counter)
    assert status == 1 and out is None and fresh.error_message() == "boom 7"               # formatted
    assert fresh.read_vector(counter).tolist() == [2]                                      # exactly once more
    assert n == 0 and fresh.lib.rstub_protect_depth() == 0                                 # the stack is reset, silently


def test_precious_list_guard_band_and_accessor_types(fresh):
    x = fresh.vector(rcall.INTSXP, [1, 2, 3])
    selftest(fresh, "preserves", x)
    assert fresh.lib.rstub_precious_count() == 1
    status, out, (n, log) = selftest(fresh, "overrun", x)
    assert n == 1 and "write past the end of a integer vector of length 3" in log
    fresh.lib.rstub_clear_violations()
    status, out, (n, log) = selftest(fresh, "wrong_accessor", fresh.vector(rcall.REALSXP, [1.0]))
    assert n == 1 and "INTEGER() of a double vector" in log


def test_the_coercion_table_is_rs(fresh):
    lib = fresh.lib
    na_real = np.array([NA_REAL_BITS], dtype=np.uint64).view(np.float64)[0]
    reals = np.array([0.0, -0.0, 1.9, -1.9, 2147483647.0, 2147483648.0, -2147483648.0, -2147483649.0, np.nan, na_real,
                      np.inf, -np.inf, 1e-300])
    x = fresh.vector(rcall.REALSXP, reals)
    assert lib.Rf_coerceVector(x, rcall.REALSXP) == x                                      # same type: the object itself
    got = fresh.read_vector(lib.Rf_coerceVector(x, rcall.INTSXP))
    assert got.tolist() == [0, 0, 1, -1, 2147483647, NA_INT, NA_INT, NA_INT, NA_INT, NA_INT, NA_INT, NA_INT, 0]
    got = fresh.read_vector(lib.Rf_coerceVector(x, rcall.LGLSXP))
    assert got.tolist() == [0, 0, 1, 1, 1, 1, 1, 1, NA_INT, NA_INT, 1, 1, 1]
    ints = fresh.vector(rcall.INTSXP, [0, 5, -7, NA_INT, 2147483647])
    got = fresh.read_vector(lib.Rf_coerceVector(ints, rcall.REALSXP))
    assert got[:3].tolist() == [0.0, 5.0, -7.0] and got[4] == 2147483647.0 and got.view(np.uint64)[3] == NA_REAL_BITS
    assert fresh.read_vector(lib.Rf_coerceVector(ints, rcall.LGLSXP)).tolist() == [0, 1, 1, NA_INT, 1]
    lgl = fresh.vector(rcall.LGLSXP, [0, 1, NA_INT])
    assert fresh.read_vector(lib.Rf_coerceVector(lgl, rcall.INTSXP)).tolist() == [0, 1, NA_INT]
    assert fresh.read_vector(lib.Rf_coerceVector(lgl, rcall.REALSXP)).view(np.uint64)[2] == NA_REAL_BITS
    empty = lib.Rf_coerceVector(fresh.nil, rcall.INTSXP)                                   # as.integer(NULL)
    assert lib.rstub_type(empty) == rcall.INTSXP and lib.rstub_len(empty) == 0
    # the scalar readers: the first element, by the same rules; nothing to read is NA
    assert lib.Rf_asInteger(fresh.vector(rcall.REALSXP, [3.99, 7.0])) == 3
    assert lib.Rf_asInteger(fresh.vector(rcall.REALSXP, [-3.99])) == -3
    assert lib.Rf_asInteger(fresh.vector(rcall.REALSXP, [np.nan])) == NA_INT
    assert lib.Rf_asInteger(fresh.vector(rcall.REALSXP, [3e9])) == NA_INT
    assert lib.Rf_asInteger(fresh.vector(rcall.LGLSXP, [1])) == 1
    assert lib.Rf_asInteger(fresh.vector(rcall.INTSXP, [])) == NA_INT
    assert lib.Rf_asLogical(fresh.vector(rcall.INTSXP, [-4])) == 1
    assert lib.Rf_asLogical(fresh.vector(rcall.INTSXP, [NA_INT])) == NA_INT
    assert lib.Rf_asLogical(fresh.vector(rcall.REALSXP, [0.0])) == 0
    assert lib.Rf_asLogical(fresh.vector(rcall.REALSXP, [np.nan])) == NA_INT
    assert lib.Rf_asLogical(fresh.nil) == NA_INT
    assert lib.Rf_asReal(fresh.vector(rcall.INTSXP, [-2])) == -2.0
    assert np.float64(lib.Rf_asReal(fresh.vector(rcall.INTSXP, [NA_INT]))).view(np.uint64) == NA_REAL_BITS
    assert np.float64(lib.Rf_asReal(fresh.vector(rcall.LGLSXP, [NA_INT]))).view(np.uint64) == NA_REAL_BITS
    # dim: a plain vector has length rows and one column; a matrix keeps its dim through a coercion
    v = fresh.vector(rcall.INTSXP, np.arange(6))
    assert (lib.Rf_nrows(v), lib.Rf_ncols(v)) == (6, 1)
    m = fresh.vector(rcall.INTSXP, np.arange(6), dim=(2, 3))
    md = lib.Rf_coerceVector(m, rcall.REALSXP)
    assert (lib.Rf_nrows(m), lib.Rf_ncols(m)) == (2, 3) == (lib.Rf_nrows(md), lib.Rf_ncols(md))
    assert fresh.violations()[0] == 0


# ============================================================================= 2. registration
def test_registration_is_the_references_by_name_and_arity(shim):
    assert shim.lib.rstub_dynamic_symbols() == 0                                          # R_useDynamicSymbols(dll, FALSE)
    names = [nm for nm, _, _ in shim.registered]
    assert len(names) == len(set(names)), "a name is registered twice"
    ours = [nm for nm in names if nm.startswith(rcall.PREFIX)]
    assert sorted(set(names) - set(ours)) == sorted(RC.OWN)
    for nm, addr, arity in shim.registered:
        assert addr == shim.symbol(nm), f"{nm} is registered under another function's address"
        if nm.startswith(rcall.PREFIX):
            short = nm[len(rcall.PREFIX):]
            assert short in rcall.SIGNATURES, f"the reference has no routine {nm}"
            assert arity == rcall.SIGNATURES[short]["arity"], f"{nm}: registered with {arity} arguments"
        else:
            assert arity == rcall.OWN_SIGNATURES[nm]["arity"]
    defined = RC.defined_routines()
    assert sorted(defined) == sorted(nm[len(rcall.PREFIX):] for nm in ours), "defined and registered routines differ"
    for short, nparams in defined.items():
        assert nparams == shim.routines[short][1], f"{short}: {nparams} parameters, registered with {shim.routines[short][1]}"
    assert len(ours) == 103


def test_the_overlay_rebinds_exactly_the_registered_routines(shim):
    overlay = RC.overlay_routines()
    assert len(overlay) == len(set(overlay))
    assert sorted(overlay) == sorted(nm[len(rcall.PREFIX):] for nm, _, _ in shim.registered if nm.startswith(rcall.PREFIX))


def test_recorded_routines_outside_the_shim_are_the_named_ones(shim):
    recorded = {rec.fn for rec in RC.GOLDEN}
    assert sorted(recorded - set(shim.routines)) == RC.NOT_IN_SHIM
    assert len(RC.NOT_IN_SHIM) == 19
    assert sorted(set(shim.routines) ^ set(CASES)) == [], "a registered routine without any recorded call"


# ============================================================================= 3. lifecycle over the fake
def canned_for(name, out, alias=0):
    """(indptr_len, nnz, values_len, dtype, alias) the fake reports, shaped like the fixture's result for `name`"""
    assert isinstance(out, dict)
    values = out.get("values", out.get("val", out.get("xx")))
    if name == "remove_zero_valued_svec_integer":
        dtype = _lib.MX_I32
    elif values is None or values.size == 0 and name.endswith("_binary"):
        dtype = _lib.MX_NONE
    elif values.dtype == np.float64 or name == "remove_zero_valued_svec_numeric":
        dtype = _lib.MX_F64
    else:
        dtype = _lib.MX_LGL
    keys = list(out)
    first = 0 if keys[:1] == ["ii"] and len(keys) == 2 else 4 if keys[0] in ("row", "ii") else 5
    return first, 4, 0 if dtype == _lib.MX_NONE else 4, dtype, alias


def run(shim, case, torture):
    shim.reset()
    shim.torture(torture)
    live = case.live()
    try:
        got = shim.call(case.name, live)
    except rcall.RError as e:
        got = e
    return got, live


def inputs_untouched(shim, what):
    assert shim.arguments_after() == shim.last["before"], f"{what}: an argument changed"
    assert not any(shim.lib.rstub_dead(s) for s in shim.last["sexps"]), f"{what}: an argument was collected"


@pytest.mark.parametrize("name", sorted(CASES))
def test_fail_mode(fresh, name):
    """every C-ABI call fails: Rf_error with the library's message, nothing leaked, nothing written"""
    case = CASES[name]
    for torture in (False, True):
        fresh.lib.fake_reset()
        fresh.lib.fake_set_mode(MODES["fail"])
        got, live = run(fresh, case, torture)
        what = f"{name} torture={torture}"
        assert isinstance(got, rcall.RError) and str(got) == FAKE.FAIL_MESSAGE, f"{what}: {got!r}"
        assert fresh.lib.fake_calls() >= 1, what
        led = ledger(fresh)
        assert led["open"] == 0 and led["double"] == 0 and led["unknown"] == 0, f"{what}: {led}"
        fresh.assert_clean(what)
        inputs_untouched(fresh, what)
        for a, b in zip(live, case.args):
            assert not isinstance(a, np.ndarray) or a.tobytes() == b.tobytes(), what


ALIAS_INPUT = {"multiply_csr_elemwise": (0, 2), "logicaland_csr_elemwise": (0, 2), "add_csr_elemwise": (0, 2),
               "logicalor_csr_elemwise": (0, 2), "multiply_csr_by_dvec_with_NAs": (0, 1)}
ALIAS_INPUT.update({n: (0, 1) for n in RC.AM.ORDER})
ALIAS_ALL = {n: (0, 1, 2) for n in RC.AM.ORDER}
ALIAS_ALL.update({"remove_zero_valued_csr_numeric": (0, 1, 2), "remove_zero_valued_csr_logical": (0, 1, 2),
                  "remove_zero_valued_coo_numeric": (0, 1, 2), "remove_zero_valued_coo_logical": (0, 1, 2),
                  "remove_zero_valued_svec_numeric": (0, 1), "remove_zero_valued_svec_integer": (0, 1),
                  "remove_zero_valued_svec_logical": (0, 1)})


def check_succeeded(shim, case, got, live, canned, what):
    name, out = case.name, case.out
    assert not isinstance(got, Exception), f"{what}: {got!r}"
    want_types = RC.expected_types(name, out)
    types = shim.describe(shim.last["result"])
    n_first, nnz, nvalues, dtype, alias = canned
    if not isinstance(out, dict) or not out:
        # fixed-size results: the type the reference returns, the shape the arguments imply (the fixture's)
        if isinstance(out, dict):
            assert got == {} and types == {}, what
            return
        assert types == want_types, f"{what}: SEXP type {types}, the fixture implies {want_types}"
        if isinstance(out, np.ndarray):
            assert got.shape == out.shape and got.dtype == out.dtype, f"{what}: {got.dtype}{got.shape} for {out.dtype}{out.shape}"
        elif out is None:
            assert got is None, what
        else:
            assert type(got) is type(out), f"{what}: {type(got)} for {type(out)}"
        return
    assert list(got) == list(out), f"{what}: list names {list(got)}, the reference's are {list(out)}"
    assert types == want_types, f"{what}: SEXP types {types}, the fixture implies {want_types}"
    keys = list(out)
    structure, vkey = (keys[:-1], keys[-1]) if keys[-1] in ("values", "val", "xx") else (keys, None)
    if alias == _lib.MX_ALIAS_ALL:
        for key, k in zip(keys, ALIAS_ALL[name]):
            assert got[key] is live[k], f"{what}: {key} is not the argument {k} itself"
        return
    lens = [n_first, nnz] if len(structure) == 2 else [nnz]
    pats = [FAKE.PATTERN["indptr"], FAKE.PATTERN["indices"]] if len(structure) == 2 else [FAKE.PATTERN["indices"]]
    for pos, (key, n, pat) in enumerate(zip(structure, lens, pats)):
        if alias == 1:
            assert got[key] is live[ALIAS_INPUT[name][pos]], f"{what}: {key} is not the argument itself"
        else:
            assert not any(got[key] is a for a in live), what
            assert got[key].tolist() == list(range(pat, pat + n)), f"{what}: {key} = {got[key]}"
    if vkey is not None:
        v = got[vkey]
        assert not any(v is a for a in live), what
        if dtype == _lib.MX_NONE:
            assert v.size == 0, what
        elif dtype == _lib.MX_F64:
            assert v.tolist() == [FAKE.PATTERN["f64"] + k for k in range(nvalues)], f"{what}: {vkey} = {v}"
        else:
            assert v.tolist() == [FAKE.PATTERN["int"] + k for k in range(nvalues)], f"{what}: {vkey} = {v}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_succeed_mode(fresh, name):
    """canned sizes: the result has them, with the reference's names and the R types its fixture implies; the download
    landed in the R vectors; aliased structure is the argument objects; the ledger is balanced"""
    case = CASES[name]
    listy = isinstance(case.out, dict) and bool(case.out)
    aliases = [0] + ([1] if name in ALIAS_INPUT else []) + ([_lib.MX_ALIAS_ALL] if name in ALIAS_ALL else [])
    for alias in aliases if listy else [0]:
        for torture in (False, True):
            fresh.lib.fake_reset()
            fresh.lib.fake_set_mode(MODES["succeed"])
            canned = canned_for(name, case.out, alias) if listy else (3, 2, 2, _lib.MX_F64, 0)
            fresh.lib.fake_set_canned(*canned)
            got, live = run(fresh, case, torture)
            what = f"{name} alias={alias} torture={torture}"
            check_succeeded(fresh, case, got, live, canned, what)
            led = ledger(fresh)
            assert led["open"] == 0 and led["double"] == 0 and led["unknown"] == 0, f"{what}: {led}"
            assert led["begun"] == (1 if listy else 0), f"{what}: {led}"
            assert (led["discarded"] == 1) == (alias == _lib.MX_ALIAS_ALL), f"{what}: {led}"
            fresh.assert_clean(what)
            inputs_untouched(fresh, what)


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if isinstance(c.out, dict) and c.out))
def test_finish_fails_mode(fresh, name):
    """mx_result_finish releases the handle and fails, as the real one does after a failed download: the call ends in
    Rf_error with its message and the handle is released exactly once (finish_guarded's cleanup must not discard a
    handle that finish has consumed; every routine with a variable-size result is held to it, the three
    remove_zero_valued_svec_* among them)"""
    case = CASES[name]
    for alias in [0] + ([1] if name in ALIAS_INPUT else []):
        for torture in (False, True):
            fresh.lib.fake_reset()
            fresh.lib.fake_set_mode(MODES["finish_fails"])
            fresh.lib.fake_set_canned(*canned_for(name, case.out, alias))
            got, live = run(fresh, case, torture)
            what = f"{name} alias={alias} torture={torture}"
            assert isinstance(got, rcall.RError) and str(got) == FAKE.FINISH_MESSAGE, f"{what}: {got!r}"
            led = ledger(fresh)
            assert led["begun"] == 1 and led["finished"] == 1, f"{what}: {led}"
            assert led["double"] == 0 and led["discarded"] == 0 and led["unknown"] == 0 and led["open"] == 0, \
                f"{what}: a handle released twice or leaked: {led}"
            fresh.assert_clean(what)
            inputs_untouched(fresh, what)


@pytest.mark.parametrize("name", sorted(CASES))
def test_an_allocation_failure_leaks_no_handle(fresh, name):
    """R's allocVector long-jumps when memory is out.  Every allocation of a successful call is made to fail in turn:
    the call ends in R's error, and a handle that was begun is released exactly once all the same (what
    finish_guarded's cleanup is for), with nothing left protected or preserved"""
    case = CASES[name]
    listy = isinstance(case.out, dict) and bool(case.out)
    canned = canned_for(name, case.out) if listy else (3, 2, 2, _lib.MX_F64, 0)
    fresh.lib.fake_set_canned(*canned)
    got, _ = run(fresh, case, False)
    assert not isinstance(got, Exception), got
    total = fresh.lib.rstub_allocations()
    for nth in range(1, total + 1):
        for torture in (False, True):
            fresh.lib.fake_reset()
            fresh.lib.fake_set_mode(MODES["succeed"])
            fresh.lib.fake_set_canned(*canned)
            fresh.reset()
            fresh.torture(torture)
            fresh.lib.rstub_fail_allocation(nth)
            live = case.live()
            what = f"{name}: allocation {nth} of {total} fails, torture={torture}"
            with pytest.raises(rcall.RError, match="cannot allocate"):
                fresh.call(name, live)
            led = ledger(fresh)
            assert led["open"] == 0 and led["double"] == 0 and led["unknown"] == 0, f"{what}: {led}"
            fresh.assert_clean(what)
            inputs_untouched(fresh, what)


# ============================================================================= 4. the two marshalling layers agree
def recorded_calls(lib, owner_of):
    """every C-ABI call the fake saw since fake_reset(): (name, arguments), a scalar as its value (a double as its
    bits), a pointer as the index of the caller's argument it points into, "null", or "other" (an output, a copy)"""
    calls = []
    for c in range(lib.fake_recorded()):
        args = []
        for k in range(lib.fake_call_nargs(c)):
            kind = lib.fake_call_arg_kind(c, k)
            if kind == 0:
                args.append(int(lib.fake_call_arg_int(c, k)))
            elif kind == 1:
                args.append(("f64", int(np.float64(lib.fake_call_arg_double(c, k)).view(np.uint64))))
            else:
                addr = lib.fake_call_arg_int(c, k)
                args.append("null" if addr == 0 else ("arg", owner_of[addr]) if addr in owner_of else "other")
        calls.append((lib.fake_call_name(c).decode(), args))
    return calls


@pytest.mark.parametrize("name", sorted(CASES))
def test_shim_and_python_mirror_pass_the_same_arguments_to_the_c_abi(fresh, monkeypatch, name):
    """matrixextra_amd/exports.py is pinned to the reference on the device; r_shim.cpp is a second hand-written
    marshalling layer over the same mx_* calls.  For the same recorded call both must make the same C-ABI calls:
    the same function, every scalar (sizes, row and column counts, flags, selectors) equal, every input pointer
    pointing into the same caller argument.  Where the mirror passes a copy it made (a matrix it had to re-lay-out)
    the shim's pointer is only required not to be another argument."""
    from matrixextra_amd import exports as G
    import refpin
    case = CASES[name]
    lib = fresh.lib
    mirror = C.CDLL(rcall.PATHS[True])                       # the same loaded library: one fake, one recorder
    for fn, (restype, argtypes) in _lib.HEADER.functions.items():
        f = getattr(mirror, fn)
        f.restype, f.argtypes = restype, argtypes
    monkeypatch.setattr(_lib, "_lib", mirror)
    listy = isinstance(case.out, dict) and bool(case.out)
    canned = canned_for(name, case.out) if listy else (3, 2, 2, _lib.MX_F64, 0)

    lib.fake_reset()
    lib.fake_set_canned(*canned)
    live = case.live()
    fn = {"mxgpu_csr_transpose": "csr_transpose", "mxgpu_coo_to_csr": "coo_to_csr"}.get(name, name)
    refpin.call(G, fn, live)                                  # the mirror accepts the fake's canned result: any error is one
    owners = {a.ctypes.data: k for k, a in enumerate(live) if isinstance(a, np.ndarray) and a.size}
    want = recorded_calls(lib, owners)
    assert want, f"{name}: the mirror made no C-ABI call"

    lib.fake_reset()
    lib.fake_set_canned(*canned)
    got_result, live2 = run(fresh, case, False)
    sexps = fresh.last["sexps"]
    owners = {}
    for k, sx in enumerate(sexps):
        if sx != fresh.nil and lib.rstub_len(sx) and isinstance(live2[k] if k < len(live2) else None, np.ndarray):
            owners.setdefault(lib.rstub_data(sx), k)
    got = recorded_calls(lib, owners)
    assert [c[0] for c in got] == [c[0] for c in want], f"{name}: C-ABI calls {[c[0] for c in got]} != {[c[0] for c in want]}"
    for (fn_name, g), (_, w) in zip(got, want):
        assert len(g) == len(w)
        for k, (a, b) in enumerate(zip(g, w)):
            if a == b:
                continue
            if b == "other" and a != "null" and isinstance(a, tuple) and a[0] == "arg" and case.args[a[1]].ndim == 2:
                continue                                       # the mirror re-laid-out a matrix; the shim borrows R's
            raise AssertionError(f"{name}: {fn_name} argument {k}: the shim passes {a!r}, the mirror {b!r}")


def test_a_missing_build_is_an_error_not_a_skip(monkeypatch):
    monkeypatch.setitem(rcall.PATHS, True, os.path.join(rcall.BUILD, "no_such_library.so"))
    monkeypatch.setattr(rcall, "_loaded", {})
    with pytest.raises(RuntimeError, match="not found: build it"):
        rcall.load(fake=True)
