"""Test harness: the device-level C-ABI (mxd_*) on a side stream, behind device work that is still pending.

Every mxd_* entry point takes the stream to work on.  On the null stream everything is serialised, so a launch, a memset
or a copy that lands on the wrong stream, a host read-back taken too early, or a reset that runs ahead of the work it
should follow, cannot be seen there.  Here the calls run on a `torch.cuda.Stream()` whose handle reaches the library as
`device._stream()` passes it, behind a *gate*:

  gate       one `torch.cuda._sleep` on the side stream, sized from a calibration run to GATE_MS milliseconds, and an
             event recorded right behind it.  The proof in every test is the event: `event.query()` must be False at
             the moments the test names, else the test FAILS with "gate too short: ordering not shown".
  late       an operand buffer first holds *stale* content (a valid operand of the same shape, uploaded and
             synchronised); the real content waits in a second device buffer and a device-to-device copy behind the
             gate moves it in.  A kernel on the wrong stream, or a host value read too early, gives the stale answer.
  guards     every buffer lies between GUARD bytes of sentinel; outputs and workspaces start as poison and are as long
             as the larger of the two operand sets needs (+ SLACK poisoned elements), so a wrong answer stays in bounds.

A table row (tests/test_gpu_streams.py) builds two `Case`s of the same call sequence: variant 0, the real operands, and
variant 1, the stale operands of the ordered tests and the second operand set of the reuse tests.  The expectations of
both come from CPU oracles; nothing here computes an expected value.

Measured on an MI355X, per call after a warm-up pass (the ordered tests print each figure): the host needs 3 to 16
microseconds to issue a sync-free call; the slowest was mxd_colmap_build with 16.0 microseconds (a memset and four
launches), then mxd_dense_by_svec_dense with 12.7 and mxd_csr_join_disjoint with 11.3.  The gate is GATE_MS = 40
milliseconds, 2500 times the slowest call: the reuse tests put two calls and some fifty small device-to-device copies
behind one gate, and the machines are shared, so the margin is kept; at 40 ms the 140 GPU tests of the table take 9
seconds together.  Every ordered test asserts for its own call that the gate is at least ten times its issue time.
"""
import ctypes as C
import time

import numpy as np

from matrixextra_amd import _lib

GUARD = 4096
SLACK = 64
GATE_MS = 40.0
# host-side issue time of the slowest sync-free call (microseconds) and its name, as measured on the MI355X
MEASURED_ISSUE_US, SLOWEST_CALL = 16.0, "mxd_colmap_build"
assert GATE_MS * 1e3 >= 10.0 * MEASURED_ISSUE_US

GUARD_PATTERN = np.array([0xA5, 0x5A, 0xC3, 0x3C], dtype=np.uint8)
POISON_PATTERN = np.frombuffer(np.uint64(0x7FF8DEAD6B6B6B6B).tobytes(), dtype=np.uint8)
TOO_SHORT = "gate too short: ordering not shown"


# ---- the description of a call sequence --------------------------------------------------------------------------------
class In:
    """An input operand.  `data` is a numpy array, or a function of the pointer lookup P(name) -> address that returns
    one (a table of device pointers), then with `nbytes`."""

    bound, ascending = None, False

    def __init__(self, data, nbytes=None, bound=None, ascending=False):
        self.data = data if callable(data) else np.array(data, copy=True, subok=False, order="C")
        self.nbytes = int(self.data.nbytes if nbytes is None else nbytes)
        # indices: all in [0, bound); selectors: strictly ascending (both read from a tagged array when not given)
        self.bound = getattr(data, "bound", None) if bound is None else bound
        self.ascending = bool(ascending or getattr(data, "ascending", False))


class Out:
    """An output of len(expect) elements.  tail "poison": nothing behind them is written; "any": the call may write up
    to `alloc` elements (the sorts write every entry before repeated cells are merged).  rtol None: equal bit for bit,
    NaN as NaN-ness.  `after`: index of the step after which the expectation holds (default: the first that names it)."""

    def __init__(self, dtype, expect, tail="poison", alloc=None, rtol=None, after=None):
        self.dtype = np.dtype(dtype)
        self.expect = np.ascontiguousarray(expect, dtype=self.dtype).reshape(-1)
        self.tail, self.rtol, self.after = tail, rtol, after
        self.alloc = self.expect.size if alloc is None else int(alloc)
        assert self.alloc >= self.expect.size
        self.nbytes = (self.alloc + SLACK) * self.dtype.itemsize


class IO(Out):
    """An operand changed in place: `data` before, `expect` after."""
    bound, ascending = None, False

    def __init__(self, data, expect, rtol=None, after=None):
        self.bound, self.ascending = getattr(data, "bound", None), bool(getattr(data, "ascending", False))
        data = np.ascontiguousarray(data)
        super().__init__(data.dtype, expect, rtol=rtol, after=after)
        assert self.expect.size == data.size
        self.data = data.reshape(-1)
        self.nbytes = data.nbytes


class Ws:
    """A workspace of exactly `nbytes` (what mxd_*_workspace_bytes publishes), between guards."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)


class B:
    """argument: the device address of buffer `name` (+ `offset` bytes)"""

    def __init__(self, name, offset=0):
        self.name, self.offset = name, int(offset)


class H:
    """argument: a host result of `ctype`, or of `nbytes` raw bytes"""

    def __init__(self, name, ctype=C.c_int64, nbytes=None):
        self.name, self.ctype, self.nbytes = name, ctype, nbytes


class S:
    """argument: a struct passed by reference, built by `make(P)` once the buffers have addresses"""

    def __init__(self, make, names=()):
        self.make, self.names = make, tuple(names)


PLAN_OUT, PLAN_IN, STREAM = "<plan**>", "<plan*>", "<stream>"


class Step:
    """One call.  `late`: the operands that arrive behind the gate when this step is the one under test.  `waits`: the
    entry point synchronises the stream (it has a *_host result or says so in mxgpu.h).  `host`: expected host
    results by name.  `pre`: a step that only prepares a later one and is tested in a row of its own."""

    def __init__(self, fn, args, late=(), waits=False, host=None, pre=False):
        self.fn, self.args, self.late, self.waits = fn, list(args), tuple(late), bool(waits)
        self.host, self.pre = dict(host or {}), bool(pre)
        assert self.waits or not self.host, f"{fn}: host results without a synchronisation"

    def buffers(self):
        names = []
        for a in self.args:
            if isinstance(a, B):
                names.append(a.name)
            elif isinstance(a, S):
                names.extend(a.names)
        return names


class Case:
    """`checks`: (buffer names, function of {name: payload bytes}) for outputs whose order is not fixed; run once
    every named buffer has been produced."""

    def __init__(self, bufs, steps, checks=()):
        self.bufs, self.steps, self.checks = dict(bufs), list(steps), list(checks)
        for k, st in enumerate(self.steps):
            for name in st.buffers() + list(st.late):
                assert name in self.bufs, f"step {k} ({st.fn}): no buffer '{name}'"
            for name in st.late:
                assert isinstance(self.bufs[name], (In, IO)), f"step {k} ({st.fn}): late operand '{name}' is no input"


class Row:
    """A table row: `make(variant)` -> Case, variant 0 the real operands, variant 1 the stale / second ones."""

    def __init__(self, name, make):
        self.name, self.make, self._cases = name, make, None

    def cases(self):
        if self._cases is None:
            self._cases = [self.make(0), self.make(1)]
            a, b = self._cases
            assert list(a.bufs) == list(b.bufs), f"{self.name}: the variants name different buffers"
            assert [s.fn for s in a.steps] == [s.fn for s in b.steps], f"{self.name}: the variants call differently"
            for sa, sb in zip(a.steps, b.steps):
                assert (sa.late, sa.waits, sa.pre) == (sb.late, sb.waits, sb.pre)
        return self._cases

    def entry_points(self):
        return [s.fn for s in self.cases()[0].steps]

    def payload_bytes(self, name):
        """allocation of a buffer: the larger of the two variants, padded to 16 bytes"""
        n = max(c.bufs[name].nbytes for c in self.cases())
        return max(16, -(-n // 16) * 16)


def same(got, want, rtol=None):
    """equal bit for bit with NaN as NaN-ness, or within rtol of the oracle (no absolute slack)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    g, w = got[~nan], want[~nan]
    if rtol is None:
        return bool(np.array_equal(g, w) and np.array_equal(np.signbit(g), np.signbit(w)))
    return bool(np.all(np.abs(g.astype(np.float64) - w.astype(np.float64)) <= rtol * np.abs(w.astype(np.float64))))


def host_image(spec, payload, P=None):
    """guard | payload | guard as bytes: an input's data (zero-padded: still a valid operand), else poison"""
    img = np.tile(GUARD_PATTERN, (2 * GUARD + payload) // 4)
    body = img[GUARD:GUARD + payload]
    if isinstance(spec, (In, IO)):
        data = spec.data(P) if callable(spec.data) else spec.data
        raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        assert raw.size <= payload
        body[:] = 0
        body[:raw.size] = raw
    else:
        body[:] = np.tile(POISON_PATTERN, payload // 8 + 1)[:payload]
    return img


# ---- the GPU side ------------------------------------------------------------------------------------------------------
_STATE = {}


def torch_mod():
    import torch
    return torch


def side_stream():
    """the one side stream of the session; created by torch, so it does not serialise with the null stream"""
    if "side" not in _STATE:
        _STATE["side"] = torch_mod().cuda.Stream()
    return _STATE["side"]


def stream_handle(stream):
    """what matrixextra_amd.device._stream() hands to the library for torch's current stream"""
    return C.c_void_p(stream.cuda_stream)


def _cycles_per_ms():
    if "cpm" not in _STATE:
        torch = torch_mod()
        side = side_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        probe = 2_000_000
        with torch.cuda.stream(side):
            torch.cuda._sleep(probe)                        # first launch: loads the kernel
            e0.record()
            torch.cuda._sleep(probe)
            e1.record()
        side.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.0
        _STATE["cpm"] = probe / ms
    return _STATE["cpm"]


def gate(stream=None, ms=GATE_MS):
    """Keeps `stream` busy for about `ms` milliseconds with one bounded spin kernel; returns the event recorded behind
    it.  While event.query() is False, nothing enqueued on the stream after this call has started."""
    torch = torch_mod()
    stream = side_stream() if stream is None else stream
    cycles = int(_cycles_per_ms() * ms)
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        ev.record()
    return ev


def pending(ev, when):
    """the proof of every test: the gate has not drained yet"""
    if ev.query():
        raise AssertionError(f"{TOO_SHORT} ({when})")


ISSUE_US = {}       # entry point -> the longest host-side issue time seen (microseconds), sync-free calls only


class Runner:
    """The buffers of one row on the device, and the two variants' contents staged beside them."""

    def __init__(self, row):
        torch = torch_mod()
        self.row, self.cases, self.lib, self.side = row, row.cases(), _lib.load(), side_stream()
        self.names = list(self.cases[0].bufs)
        self.payload = {n: row.payload_bytes(n) for n in self.names}
        self.dev = {n: torch.empty(2 * GUARD + self.payload[n], dtype=torch.uint8, device="cuda") for n in self.names}
        self.himg = [{n: host_image(c.bufs[n], self.payload[n], self.P) for n in self.names} for c in self.cases]
        self.img = [{n: torch.from_numpy(h[n]).cuda() for n in self.names} for h in self.himg]
        self.plans = [C.c_void_p(), C.c_void_p()]
        self.keep = []
        torch.cuda.synchronize()
        self.load(0)
        for k in range(len(self.cases[0].steps)):           # warm-up: kernels loaded, grow-only scratch grown
            self.call(k, 0)
        torch.cuda.synchronize()

    def P(self, name):
        return self.dev[name].data_ptr() + GUARD

    def close(self):
        torch_mod().cuda.synchronize()
        for p in self.plans:
            if p.value:
                self.lib.mxd_spmm_plan_destroy(p)
                p.value = None

    def load(self, v, names=None):
        """variant v's content into the buffers (all, or `names`), synchronised"""
        for n in (self.names if names is None else names):
            self.dev[n].copy_(self.img[v][n])
        torch_mod().cuda.synchronize()

    def late(self, v, names):
        """variant v's content arrives on the side stream: device to device, asynchronous"""
        torch = torch_mod()
        with torch.cuda.stream(self.side):
            for n in names:
                self.dev[n].copy_(self.img[v][n], non_blocking=True)

    def call(self, k, v):
        """issues step k with variant v's arguments on the side stream: (host results, seconds the call took)"""
        st = self.cases[v].steps[k]
        hosts, args, has_stream = {}, [], False
        for a in st.args:
            if isinstance(a, B):
                args.append(C.c_void_p(self.P(a.name) + a.offset))
            elif isinstance(a, H):
                obj = (C.c_uint8 * a.nbytes)() if a.nbytes else a.ctype(-1)
                hosts[a.name] = obj
                args.append(C.byref(obj))
            elif isinstance(a, S):
                obj = a.make(self.P)
                self.keep.append(obj)
                args.append(C.byref(obj))
            elif a is PLAN_OUT:
                args.append(C.byref(self.plans[v]))
            elif a is PLAN_IN:
                args.append(self.plans[v])
            elif a is STREAM:
                args.append(stream_handle(self.side))
                has_stream = True
            else:
                args.append(a)
        if not has_stream:
            args.append(stream_handle(self.side))
        fn = getattr(self.lib, st.fn)
        t0 = time.perf_counter()
        rc = fn(*args)
        dt = time.perf_counter() - t0
        _lib.check(rc)
        return hosts, dt

    def check_hosts(self, k, v, hosts):
        st = self.cases[v].steps[k]
        assert set(st.host) == set(hosts), f"{st.fn}: the row expects {sorted(st.host)}, the call has {sorted(hosts)}"
        for name, want in st.host.items():
            obj = hosts[name]
            got = bytes(obj)[:len(want)] if isinstance(want, bytes) else obj.value
            assert got == want, f"{st.fn}: *{name} = {got!r}, the oracle has {want!r}"

    def read_back(self, tensors=None):
        """the buffers as numpy bytes, copied on the side stream"""
        torch = torch_mod()
        tensors = self.dev if tensors is None else tensors
        with torch.cuda.stream(self.side):
            host = {n: torch.empty(t.shape, dtype=torch.uint8, pin_memory=True) for n, t in tensors.items()}
            for n, t in tensors.items():
                host[n].copy_(t, non_blocking=True)
        self.side.synchronize()
        return {n: h.numpy().copy() for n, h in host.items()}

    def check_buffers(self, raw, v, done):
        """`raw` after the steps `done` of variant v: guards intact, inputs unchanged, outputs as the oracle has them,
        nothing written behind them"""
        case = self.cases[v]
        named = {}
        for k in done:
            for n in case.steps[k].buffers():
                named.setdefault(n, k)
        for n in self.names:
            spec, got, img, pay = case.bufs[n], raw[n], self.himg[v][n], self.payload[n]
            what = f"{self.row.name}, variant {v}, buffer '{n}'"
            for side_, sl in (("front", slice(0, GUARD)), ("back", slice(GUARD + pay, None))):
                bad = np.flatnonzero(got[sl] != img[sl])
                assert bad.size == 0, f"{what}: {bad.size} byte(s) of the {side_} guard changed, first at {int(bad[0])}"
            body, before = got[GUARD:GUARD + pay], img[GUARD:GUARD + pay]
            if type(spec) is In:
                assert np.array_equal(body, before), f"{what}: an input changed"
                continue
            if isinstance(spec, Ws):
                continue
            first = named.get(n)
            produced = first is not None and (spec.after is None or max(done) >= spec.after)
            if not produced:
                if first is None:
                    assert np.array_equal(body, before), f"{what}: written by a step that does not name it"
                continue
            isz, ne = spec.dtype.itemsize, spec.expect.size
            val = body[:ne * isz].view(spec.dtype)
            if not same(val, spec.expect, spec.rtol):
                bad = np.flatnonzero(~((val == spec.expect) | ((val != val) & (spec.expect != spec.expect))))
                at = int(bad[0]) if bad.size else 0
                raise AssertionError(f"{what}: differs from the oracle in {bad.size} of {ne} element(s), first at {at}: "
                                     f"{val[at]!r} != {spec.expect[at]!r}")
            if isinstance(spec, IO):
                assert np.array_equal(body[ne * isz:], before[ne * isz:]), f"{what}: padding changed"
            else:
                lo = (spec.alloc if spec.tail == "any" else ne) * isz
                assert np.array_equal(body[lo:], before[lo:]), f"{what}: written behind element {lo // isz}"
        for names, fn in case.checks:
            if all(n in named and (case.bufs[n].after is None or max(done) >= case.bufs[n].after) for n in names):
                fn({n: raw[n][GUARD:GUARD + self.payload[n]] for n in names})


def run_ordered(row, k):
    """P1, P2 and P4 for step k of a row.  The steps before it run with the real operands and are synchronised.  Then
    the late operands of step k hold stale content, the gate is enqueued, the real content is queued behind it, and
    the call is made: the gate must be pending right before it and, for a sync-free entry point, right after it.  Host
    results are compared with the oracle's before anything else is issued; the sync-free steps that follow (the fill
    of a count) are issued with no host synchronisation in between, and everything is read back on the side stream."""
    R = Runner(row)
    try:
        steps = R.cases[0].steps
        st = steps[k]
        R.load(0)
        for i in range(k):
            R.call(i, 0)
        R.side.synchronize()
        R.load(1, st.late)
        ev = gate(R.side)
        R.late(0, st.late)
        pending(ev, f"before {st.fn}")
        hosts, dt = R.call(k, 0)
        if not st.waits:
            pending(ev, f"after {st.fn} returned: the header calls it asynchronous")
            us = dt * 1e6
            ISSUE_US[st.fn] = max(ISSUE_US.get(st.fn, 0.0), us)
            print(f"issue time {st.fn}: {us:.1f} us (gate {GATE_MS * 1e3:.0f} us)")
            assert GATE_MS * 1e3 >= 10.0 * us, f"{st.fn} took {us:.0f} us to issue: the gate is not ten times that"
        R.check_hosts(k, 0, hosts)
        done = list(range(k + 1))
        for i in range(k + 1, len(steps)):
            if steps[i].waits:
                break
            R.call(i, 0)
            done.append(i)
        R.check_buffers(R.read_back(), 0, done)
    finally:
        R.close()


def run_reuse(row, k):
    """P3 for the sync-free step k: issued twice, back to back, behind one gate, on the same operand, workspace and
    output buffers; the second operand set (and what the earlier steps left for it) is copied in on the stream between
    the calls, the first result is copied aside on the stream.  Both results must be the oracle's."""
    torch = torch_mod()
    R = Runner(row)
    try:
        assert not R.cases[0].steps[k].waits
        snaps = []
        for v in (0, 1):
            R.load(v)
            for i in range(k):
                R.call(i, v)
            torch.cuda.synchronize()
            snaps.append({n: R.dev[n].clone() for n in R.names})
        aside = [{n: torch.empty_like(R.dev[n]) for n in R.names} for _ in (0, 1)]
        torch.cuda.synchronize()
        ev = gate(R.side)
        for v in (0, 1):
            with torch.cuda.stream(R.side):
                for n in R.names:
                    R.dev[n].copy_(snaps[v][n], non_blocking=True)
            R.call(k, v)
            with torch.cuda.stream(R.side):
                for n in R.names:
                    aside[v][n].copy_(R.dev[n], non_blocking=True)
        pending(ev, f"after both {R.cases[0].steps[k].fn} calls")
        R.side.synchronize()
        for v in (0, 1):
            R.check_buffers(R.read_back(aside[v]), v, list(range(k + 1)))
    finally:
        R.close()
