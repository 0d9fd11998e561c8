"""The delayed producer: a harness that tells a stream-ordered call from one that merely ran after the data was there.

Almost every GPU test drives the library on the legacy default stream, which serialises implicitly against every blocking
stream, so a launch on the wrong stream, a missing event towards one of the ctx's private non-blocking streams or a host
read after synchronising the wrong stream cannot show there.  `run_delayed` drives one case (tests/stream_order_cases.py)
on a ctx bound to a non-blocking user stream, with the producer of the operands still in flight when the library
enqueues:

  1. every operand buffer holds a finite DECOY (the operands of another member of the same exact family: a premature
     read gives a different, exactly representable result) and every pure output buffer a sentinel;
  2. the producer is enqueued on the ctx stream: a delay, the copy of the true operands from device staging buffers, an
     event `produced`;
  3. the entry point is called at once from the host;
  4. vacuity guard: an entry that returns without synchronising must return while `produced` is still pending (else
     the delay is raised, 20 -> 40 -> 80 -> 100 ms, and beyond that the run FAILS with "delay too short"); an entry that
     synchronises must return after `produced` and after at least half the delay of host wall time (sync=None, for the
     few entries whose header leaves it open: one or the other must hold);
  5. join check: straight after the return the pure operands are overwritten with the decoy on the same stream --
     legal for a stream-ordered library, fatal for work left on an unjoined private stream -- and the outputs are
     downloaded through the same stream.

The delay is torch.cuda._sleep(cycles) where the build has it, else a fixed chain of torch matmuls; both are bounded.
Each case first runs once without delay on the same ctx (tables, plans and workspace are then cached, and the delayed
call's host time is short)."""
from __future__ import annotations

import time

import numpy as np

SENTINEL = -7777.0
DELAY_LADDER_MS = (20.0, 40.0, 80.0, 100.0)          # start at 20 ms, never beyond 100 ms per call
MATMUL_N = 2048                                       # fallback delay: fp32 matmuls of this order


def _torch():
    import torch
    return torch


class Delay:
    """A bounded delay on one stream, calibrated once with two events."""

    def __init__(self, stream):
        torch = _torch()
        self.stream = stream
        self.kind = "sleep" if hasattr(torch.cuda, "_sleep") else "matmul"
        with torch.cuda.stream(stream):
            if self.kind == "matmul":
                self.a = torch.ones(MATMUL_N, MATMUL_N, dtype=torch.float32, device=stream.device) / MATMUL_N
                self.b = self.a.clone()
                self._emit(4)                         # library load, first-use costs
            units, ms = (1 << 20 if self.kind == "sleep" else 8), 0.0
            for _ in range(12):                       # grow the probe until it lasts a few ms: bounded, at most 12 probes
                ms = self._time(units)
                if ms >= 4.0:
                    break
                units *= 4
            assert ms > 0.0, "the delay could not be calibrated"
            self.units_per_ms = units / ms
        self.chosen_ms = DELAY_LADDER_MS[0]

    def _emit(self, units):
        torch = _torch()
        if self.kind == "sleep":
            torch.cuda._sleep(int(units))
        else:
            for _ in range(int(units)):
                self.b = torch.matmul(self.a, self.b)

    def _time(self, units):
        torch = _torch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        self._emit(units)
        e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def enqueue(self, ms):
        """`ms` milliseconds of work on the current stream (which must be self.stream)"""
        self._emit(max(1, round(ms * self.units_per_ms)))

    def describe(self):
        return f"{self.kind}: {self.units_per_ms:.1f} {'cycles' if self.kind == 'sleep' else 'matmuls'}/ms"


def run_delayed(be, stage, call, outputs, sync=False, delay=None, what=""):
    """stage: [(DTensor, true staging torch tensor, decoy staging torch tensor)], the operand buffers; call(): the entry
    point(s) on `be`, returning host results or None; outputs: [DTensor] -- a buffer that is also staged is an in/out
    operand and is not refilled in step 5.  Returns ([host copy of every output], call's return value, info) with
    info = {"delay_ms", "returned_before_produced", "wall_ms"}."""
    torch = _torch()
    s = be.torch_stream
    assert s.cuda_stream != 0, "run_delayed needs a ctx on a user stream"
    delay = Delay(s) if delay is None else delay
    staged = {id(t.buf) for t, _, _ in stage}
    written = {id(o.buf) for o in outputs}
    with torch.cuda.stream(s):
        def fill(which, skip=()):
            for t, true, decoy in stage:
                if id(t.buf) not in skip:
                    t.buf[:true.numel()].copy_(true if which == "true" else decoy, non_blocking=True)

        fill("true")
        call()                                                       # warm-up: tables, plans, workspace
        s.synchronize()
        ladder = [ms for ms in DELAY_LADDER_MS if ms >= delay.chosen_ms]
        for ms in ladder:
            fill("decoy")
            for o in outputs:
                if id(o.buf) not in staged:
                    o.buf.fill_(SENTINEL)
            s.synchronize()
            delay.enqueue(ms)
            fill("true")
            produced = torch.cuda.Event()
            produced.record(s)
            t0 = time.perf_counter()
            ret = call()
            wall = (time.perf_counter() - t0) * 1e3
            done = produced.query()
            fill("decoy", skip=written)
            host = [o.buf[:o.size].cpu().numpy().copy() for o in outputs]
            s.synchronize()
            info = {"delay_ms": ms, "returned_before_produced": not done, "wall_ms": wall}
            if sync is None and done:                                   # unspecified: it waited for the producer, or returned early
                sync = True
            if sync:
                assert done, f"{what}: the entry returned before the producer had finished -- it did not synchronise the ctx stream"
                assert wall >= 0.5 * ms, f"{what}: host wall time {wall:.2f} ms of a synchronising entry under a {ms:.0f} ms delay"
                return host, ret, info
            if not done:
                delay.chosen_ms = max(delay.chosen_ms, ms)
                return host, ret, info
        raise AssertionError(f"{what}: delay too short -- the producer had finished when the call returned, even at "
                             f"{ladder[-1]:.0f} ms (host time of the call {wall:.2f} ms)")


def run_plain(be, stage, call, outputs):
    """the same call on a default-stream ctx with the true operands in place: ([host copy of every output], return value)"""
    torch = _torch()
    for t, true, _ in stage:
        t.buf[:true.numel()].copy_(true)
    for o in outputs:
        if not any(o.buf is t.buf for t, _, _ in stage):
            o.buf.fill_(SENTINEL)
    torch.cuda.synchronize()
    ret = call()
    be.synchronize()
    host = [o.buf[:o.size].cpu().numpy().copy() for o in outputs]
    torch.cuda.synchronize()
    return host, ret


class Staged:
    """The device side of one case: operand and output buffers (shared by both ctxs) and the staging copies."""

    def __init__(self, be, case):
        torch = _torch()
        from mpskit_jl_amd.backend import DTensor
        dev = be.device
        self.case = case
        self.dev, self.stage = {}, []
        for name, (true, decoy) in case.operands.items():
            true, decoy = np.ascontiguousarray(true, dtype=np.float64).ravel(), np.ascontiguousarray(decoy, dtype=np.float64).ravel()
            assert true.shape == decoy.shape, name
            t = DTensor(torch.zeros(max(true.size, 1), dtype=torch.float64, device=dev), (true.size,))
            self.dev[name] = t
            self.stage.append((t, torch.from_numpy(true.copy()).to(dev), torch.from_numpy(decoy.copy()).to(dev)))
        self.out_names = list(case.outputs)
        for name, n in case.outputs.items():
            if name not in self.dev:
                self.dev[name] = DTensor(torch.zeros(max(int(n), 1), dtype=torch.float64, device=dev), (int(n),))
        self.outputs = [self.dev[n] for n in self.out_names]
        torch.cuda.synchronize()

    def _result(self, host, ret):
        got = dict(zip(self.out_names, host))
        for k, v in (ret or {}).items():
            got["ret:" + k] = np.asarray(v)
        return got

    def delayed(self, be, delay):
        torch = _torch()
        with torch.cuda.stream(be.torch_stream):
            ctxobj = self.case.setup(be) if self.case.setup else None
            be.synchronize()
        host, ret, info = run_delayed(be, self.stage, lambda: self.case.run(be, self.dev, ctxobj), self.outputs,
                                      sync=self.case.sync, delay=delay, what=self.case.name)
        return self._result(host, ret), info

    def plain(self, be):
        ctxobj = self.case.setup(be) if self.case.setup else None
        host, ret = run_plain(be, self.stage, lambda: self.case.run(be, self.dev, ctxobj), self.outputs)
        return self._result(host, ret)
