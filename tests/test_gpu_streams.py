"""The stream contract of include/modmfcc.h ("Contract": asynchronous on the caller's stream, no allocation, no
synchronisation, graph-capture safe; a plan that is only computed with may be shared by threads) for EVERY compute entry in
every form: the cases of tests/stream_cases.py.

Nothing here checks a value against a reference: the eager call on the default stream is what the other test files pin.
Every comparison is bit for bit against that eager result of the same call on the same data.  Before the checks every
case runs two eager calls on data set 1 (the first is the warm-up: module load, hipFuncSetAttribute, cached device tables);
if the two differ in a bit the entry is not reproducible run to run, the case must name a tolerance and the existing test
file it comes from (Case.tol), and fails otherwise.  No registered case does.

A. side stream (one that is seen to run beside the default stream): gate (torch.cuda._sleep), event, fill(1), call(),
   clones -- all enqueued behind the gate with no host wait.
   The event must still be pending when call() returns (the call waited for nothing, read no lengths back, made no blocking
   upload) and the clones must hold set 1's result (a launch on another stream would have run on set 0).
B. capture and replay: one call() captured on one stream in the default error mode, replayed on set 0, set 1, set 0 and
   set 1 again; for a ragged case that is with other lengths than the capture saw.  (Four replays, not two: the one defect
   this file has found, a captured memset that wrote stale words, showed from the second replay of a graph on.)
C. one plan, two threads, each with its own stream, buffers and workspace.

The gate is calibrated once per session (20 x the longest host duration of any case's warmed call, 50 ms at the least).
"""
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import stream_cases as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

GATE_FLOOR_MS = 50.0
GATE_FACTOR = 20.0


# ---- comparison -----------------------------------------------------------------------------------------------------------
def _bits(t):
    import torch
    t = t.contiguous()
    if t.is_complex():
        t = torch.view_as_real(t).contiguous()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.reshape(-1).view(torch.uint8)


def bit_equal(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def assert_same(case, got, want, what, exact=True):
    import torch
    assert len(got) == len(want), (case.name, what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if exact:
            if not bit_equal(g, w):
                bad = int((_bits(g) != _bits(w)).sum()) if g.shape == w.shape and g.dtype == w.dtype else -1
                raise AssertionError(f"{case.name}: {what}: output {i} differs from the eager call in {bad} bytes of "
                                     f"{_bits(w).numel()} (shape {tuple(w.shape)}, {w.dtype})")
        else:
            src, rtol = case.tol
            g64, w64 = (torch.view_as_real(t) if t.is_complex() else t for t in (g, w))
            err = (g64.double() - w64.double()).abs().max().item()
            assert err <= rtol * w64.double().abs().max().item(), (case.name, what, i, err, src)


def _poison_any(ts, but=()):
    """NaN / -1 into tensors of any layout (the outputs a wrapper allocated inside a capture), except those the case owns:
    Prepared.poison() has filled them, and columns the library leaves alone must hold the same bits as in the eager run."""
    import torch
    owned = {o.data_ptr() for o in but}
    for t in ts:
        if t.data_ptr() in owned:
            continue
        if t.is_floating_point() or t.is_complex():
            t.fill_(float("nan"))
        elif t.dtype == torch.bool:
            t.fill_(True)
        else:
            t.fill_(-1)


def _clones(ts):
    return [t.clone() for t in ts]


# ---- the session: every case prepared, warmed and run eagerly once; the gate ---------------------------------------------------
class Entry:
    """One prepared case: its eager results on both sets, whether two eager runs agreed bit for bit, the host duration of
    a warmed call."""

    def __init__(self, case, gpu):
        import torch
        self.case = case
        self.error = None
        try:
            p = self.p = case.prepare(gpu)
            p.fill(1)
            p.poison()
            first = _clones(p.call())                   # (the warm-up)
            torch.cuda.synchronize()
            p.poison()
            t0 = time.perf_counter()
            outs = p.call()
            self.host_ms = (time.perf_counter() - t0) * 1e3
            self.eager = {1: _clones(outs)}
            torch.cuda.synchronize()
            self.reproducible = len(first) == len(self.eager[1]) and all(bit_equal(a, b) for a, b in zip(first, self.eager[1]))
            p.fill(0)
            p.poison()
            self.eager[0] = _clones(p.call())
            torch.cuda.synchronize()
        except Exception as e:                          # the case's own tests report it; the others go on
            self.error = e

    def exact(self):
        """Bit for bit, unless the entry was SHOWN irreproducible and names its tolerance."""
        if self.reproducible:
            return True
        if self.case.tol is None:
            pytest.fail(f"{self.case.name}: two eager calls on the same data differ in a bit and the case names no tolerance")
        return False


class Session:
    def __init__(self, gpu, cases=None):
        import torch
        self.gpu = gpu
        self.entries = {c.name: Entry(c, gpu) for c in (S.CASES if cases is None else cases)}
        torch.cuda._sleep(1_000_000)                    # (the sleep kernel's own first launch)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cycles = 20_000_000
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        torch.cuda.synchronize()
        self.cycles_per_ms = cycles / e0.elapsed_time(e1)
        good = [e for e in self.entries.values() if e.error is None and e.case.host_sync is None]
        self.longest = max(good, key=lambda e: e.host_ms)
        self.gate_ms = max(GATE_FLOOR_MS, GATE_FACTOR * self.longest.host_ms)
        self.capture_stuck = None
        self.side = self.pick_side_stream()
        by_family = {}
        for e in good:
            by_family[e.case.family] = max(by_family.get(e.case.family, (0.0, "")), (e.host_ms, e.case.name))
        print(f"\nstream gate: {self.cycles_per_ms:.0f} sleep cycles per ms; longest warmed call {self.longest.host_ms:.3f} ms "
              f"({self.longest.case.name}); gate {self.gate_ms:.1f} ms")
        for fam, (ms, name) in sorted(by_family.items()):
            print(f"stream gate: family {fam:9s} longest host duration {ms:7.3f} ms ({name})")

    def stray_launch_shows(self, s):
        """Does work that strays to the DEFAULT stream while `s` is gated overtake the work queued on `s`?  (The stand-in
        of test_detector_sees_a_launch_on_another_stream, in small.)"""
        import torch
        x0, x1 = torch.zeros(1024, device=self.gpu), torch.ones(1024, device=self.gpu)
        x, out = x0.clone(), torch.full((1024,), 2.0, device=self.gpu)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(int(self.gate_ms * self.cycles_per_ms))
            x.copy_(x1)
            with torch.cuda.stream(torch.cuda.default_stream()):
                out.copy_(x)
        torch.cuda.synchronize()
        return torch.equal(out, x0)

    def pick_side_stream(self):
        """The side stream of all cases of test A.  Streams share a few hardware queues, and a queue runs its work in
        order: on a side stream that lies on the default stream's queue a launch that strayed to the default stream
        would still run behind the gate and behind fill(1), and the order check could not see it (measured: the same
        stand-in gave set 0 on one fresh stream and set 1 on another).  So streams are tried until one shows it."""
        import torch
        tried = []
        for _ in range(16):
            tried.append(torch.cuda.Stream())
            if self.stray_launch_shows(tried[-1]):
                return tried[-1]
        pytest.fail("inconclusive: none of 16 streams runs beside the default stream; the order check would be blind")

    def get(self, case):
        e = self.entries[case.name]
        if e.error is not None:
            raise e.error
        return e


_SESSION = []


@pytest.fixture(scope="module")
def session(gpu):
    if not _SESSION:
        _SESSION.append(Session(gpu))
    return _SESSION[0]


# ---- A. order and asynchrony on a side stream -----------------------------------------------------------------------------------
CLEAN, WAITED, INCONCLUSIVE = "clean", "waited", "inconclusive"


def run_behind_gate(p, sess):
    """Set 0 in the inputs, NaN in the outputs; on the session's side stream (Session.pick_side_stream; idle at this point):
    gate, event, fill(1), call(), clones.  -> (verdict,
    clones).  verdict: CLEAN -- the gate's event was still pending when call() returned; INCONCLUSIVE -- the host had
    already been held up for half the gate's duration BEFORE call() began (a loaded machine) and the event was complete
    afterwards: nothing can be said; WAITED -- the event was complete when call() returned although call() began in good
    time: the call did not return before the work ahead of it on its stream was done."""
    import torch
    p.fill(0)
    p.poison()
    torch.cuda.synchronize()
    s = sess.side
    ev = torch.cuda.Event()
    with torch.cuda.stream(s):
        t0 = time.perf_counter()
        torch.cuda._sleep(int(sess.gate_ms * sess.cycles_per_ms))
        ev.record(s)
        p.fill(1)
        before_ms = (time.perf_counter() - t0) * 1e3
        outs = p.call()
        done = ev.query()
        got = _clones(outs)
    s.synchronize()
    torch.cuda.synchronize()
    if not done:
        return CLEAN, got
    return (INCONCLUSIVE if before_ms >= 0.5 * sess.gate_ms else WAITED), got


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_side_stream_order_and_asynchrony(case, session):
    e = session.get(case)
    verdict, got = run_behind_gate(e.p, session)
    if case.host_sync is None:
        assert verdict != INCONCLUSIVE, f"{case.name}: inconclusive -- the gate ended before call() returned on a held-up host"
        assert verdict == CLEAN, f"{case.name}: call() waited for its stream or the device (the gate's event was complete)"
    else:       # a documented read-back: the detector must see it
        assert verdict == WAITED, f"{case.name}: documented to read back ({case.host_sync}) but did not wait: {verdict}"
    assert_same(case, got, e.eager[1], "behind the gate on a side stream", e.exact())


def _stand_in(name, call_of, gpu):
    def data():
        r = np.random.default_rng(5)
        return {"x": (r.standard_normal(4096).astype(np.float32), r.standard_normal(4096).astype(np.float32))}
    return S.Case(name, "stand-in", "self-check", data, call_of).prepare(gpu)


def test_detector_sees_a_call_that_waits(gpu, session):
    """Self-check: a call that ends in .sum().item() must trip the event assertion."""
    import torch

    def setup(env):
        out = env.out((4096,), torch.float32)

        def call():
            out.copy_(env.buf["x"] * 2)
            out.sum().item()
            return out
        return call
    verdict, got = run_behind_gate(_stand_in("self-check/item", setup, gpu), session)
    assert verdict == WAITED


def test_detector_sees_a_launch_on_another_stream(gpu, session):
    """Self-check: a call that copies its input on the DEFAULT stream while the side stream is current returns at once --
    and produces set 0's values, because fill(1) still waits behind the gate."""
    import torch

    def setup(env):
        out = env.out((4096,), torch.float32)

        def call():
            with torch.cuda.stream(torch.cuda.default_stream()):
                out.copy_(env.buf["x"])
            return out
        return call
    p = _stand_in("self-check/wrong-stream", setup, gpu)
    verdict, got = run_behind_gate(p, session)
    assert verdict == CLEAN
    assert bit_equal(got[0], p.staged[0]["x"]) and not bit_equal(got[0], p.staged[1]["x"])


# ---- B. capture and replay ---------------------------------------------------------------------------------------------------
GRAPH_CASES = [c for c in S.CASES if c.host_sync is None]


@pytest.mark.parametrize("case", GRAPH_CASES, ids=lambda c: c.name)
def test_capture_and_replay(case, session):
    import torch
    if session.capture_stuck:
        pytest.fail(session.capture_stuck)
    e = session.get(case)
    p = e.p
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                          # warm-up on the side stream
        p.fill(1)
        p.call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g, stream=s):             # (its __exit__ ends the capture, failed or not)
            outs = p.call()
    finally:
        with torch.cuda.stream(s):
            if torch.cuda.is_current_stream_capturing():
                session.capture_stuck = f"a stream was left capturing by the failed capture of {case.name}: no further graph case can run"
    for k in (0, 1, 0, 1):                              # (1: for a ragged case, other lengths than the capture saw)
        p.fill(k)
        p.poison()
        _poison_any(outs, but=p.outs)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_same(case, outs, e.eager[k], f"replay on data set {k}", e.exact())
    del g


# ---- C. one plan, two threads ---------------------------------------------------------------------------------------------------
THREAD_CASES = [c for c in S.CASES if c.threads]
CALLS_PER_THREAD = 20


def run_two_threads(prepared, calls, warm):
    """Two threads, one Prepared each (same plan or handle; own stream, buffers, workspace): after a barrier each makes
    `calls` calls, alternating the data sets -> per thread [(set, clones)].  warm=False: the threads' calls are the first."""
    import torch
    streams = [torch.cuda.Stream() for _ in prepared]
    if warm:
        for p in prepared:
            p.fill(1)
            p.call()
    torch.cuda.synchronize()
    barrier = threading.Barrier(len(prepared))
    results, errors = [[] for _ in prepared], []

    def work(i):
        try:
            p = prepared[i]
            torch.cuda.set_device(p.gpu)
            with torch.cuda.stream(streams[i]):
                barrier.wait(timeout=60)
                for j in range(calls):
                    k = (i + j) % 2
                    p.fill(k)
                    results[i].append((k, _clones(p.call())))
            streams[i].synchronize()
        except Exception as exc:            # noqa: BLE001  (reported by the caller)
            errors.append((i, exc))
            barrier.abort()
    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(len(prepared))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a thread did not finish"
    assert not errors, errors
    torch.cuda.synchronize()
    return results


@pytest.mark.parametrize("case", THREAD_CASES, ids=lambda c: c.name)
def test_one_plan_two_threads(case, session, gpu):
    """Two Python threads compute with the same mm_plan / mm_hilbert (for mm_pyin_f32: the same parameter and table
    structs), each on its own stream with its own buffers and workspace, 20 calls each, the data sets alternating; every
    result must equal the serial one.  ctypes releases the GIL, so the host parts of the calls overlap.

    This detector is NOT deterministic: it can miss a race, it cannot invent one."""
    e = session.get(case)
    shared = {}
    prepared = [case.prepare(gpu, shared) for _ in range(2)]
    assert "plan" not in shared or len({id(shared["plan"])}) == 1
    for i, res in enumerate(run_two_threads(prepared, CALLS_PER_THREAD, warm=True)):
        assert len(res) == CALLS_PER_THREAD
        for j, (k, got) in enumerate(res):
            assert_same(case, got, e.eager[k], f"thread {i}, call {j}, data set {k}", e.exact())


def test_first_calls_of_a_process_on_two_threads():
    """A fresh process whose two threads make the FIRST compute calls of the process at the same moment (the per-device
    hipFuncSetAttribute flags of csrc/mm_common.h): tests/_stream_worker.py compares both threads' results with the serial
    call made afterwards and exits non-zero on a difference.  Nothing is started after it."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_stream_worker.py")], cwd=ROOT, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "first calls ok" in r.stdout
