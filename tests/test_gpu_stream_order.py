"""Every ABI family on a non-blocking user stream, with the producer of its operands still in flight.

The `be` fixture of the suite binds the legacy default stream, which serialises implicitly against every blocking stream:
a launch on stream 0 instead of the ctx stream, a missing fork or join event towards the ctx's private non-blocking streams
(stream2 in mpsk_qrpos2 / mpsk_qrlq_pair / mpsk_tsplit / the side section, xstreams[1..3] in the chained Jacobi schedule), a
host scalar read after synchronising the wrong stream, or a split-K workspace keyed to another stream cannot show there.
Here each case of tests/stream_order_cases.py runs through the delayed producer of tests/stream_order.py on ONE extra ctx
bound to a fresh torch.cuda.Stream: decoy operands in place, the true ones arriving 20 ms later on the ctx stream, the entry
called at once, the operands overwritten again straight after it returns.  The result must be the exact reference (or lie
inside the bound of the input module the case borrows from) AND bit-identical to the same call on the default-stream ctx.
Each case prints a STREAM-ORDER line (delay, whether the entry returned before the producer had finished); the lines of one
run are kept in profiles/stream_order_bounds.log."""
import ctypes as C

import numpy as np
import pytest

import stream_order as so
import stream_order_cases as soc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be2():
    import torch
    import mpskit_jl_amd as mk
    s = torch.cuda.Stream(0)
    b2 = mk.Backend(0, stream=s)
    yield b2
    b2.synchronize()
    b2.close()


@pytest.fixture(scope="module")
def delay(be2):
    d = so.Delay(be2.torch_stream)
    print(f"STREAM-ORDER calibration: {d.describe()}; first delay {so.DELAY_LADDER_MS[0]:.0f} ms, ceiling {so.DELAY_LADDER_MS[-1]:.0f} ms")
    yield d
    print(f"STREAM-ORDER chosen delay: {d.chosen_ms:.0f} ms")


@pytest.mark.parametrize("case", soc.CASES, ids=lambda c: c.name)
def test_entry_is_ordered_on_the_user_stream(be, be2, delay, case):
    st = so.Staged(be2, case)
    got, info = st.delayed(be2, delay)
    print(f"STREAM-ORDER {case.family} {case.name}: delay {info['delay_ms']:.0f} ms, returned before produced: "
          f"{info['returned_before_produced']}, host time of the call {info['wall_ms']:.2f} ms"
          + (f", private: {case.private}" if case.private else ""))
    assert case.sync is None or info["returned_before_produced"] == (not case.sync)
    if case.check is not None:
        bad = case.check(got)
        assert not bad, bad
    else:
        ref = case.reference(case.true())
        for k, v in ref.items():
            assert np.array_equal(got[k], np.asarray(v)), f"{case.name}: {k} differs from the exact reference"
    plain = st.plain(be)
    assert set(plain) == set(got)
    for k in got:
        assert np.array_equal(got[k], plain[k]), f"{case.name}: {k} differs from the same call on the default-stream ctx"


def test_harness_detects_an_unordered_consumer(be2, delay):
    """A torch-only stand-in for the library runs its copy on a SECOND non-blocking stream.  Without the fork (no wait for
    an event of the ctx stream) it reads ahead of the producer and must come back with the decoy's result.  With the fork
    but without the join (the ctx stream never waits for the second one, whose copy is still behind a short delay when the
    call returns) the refill of step 5 and the download overtake it: the result is the sentinel or the decoy, never the true
    values.  With both it passes: the harness accepts an ordered consumer."""
    import torch
    from mpskit_jl_amd.backend import DTensor
    n = 1 << 16
    dev = be2.device
    true, decoy = torch.arange(n, dtype=torch.float64, device=dev), -torch.arange(n, dtype=torch.float64, device=dev) - 1.0
    x, y = DTensor(torch.zeros(n, dtype=torch.float64, device=dev), (n,)), DTensor(torch.zeros(n, dtype=torch.float64, device=dev), (n,))
    side = torch.cuda.Stream(0)
    torch.cuda.synchronize()

    def consumer(fork, join):
        def call():
            if fork:
                side.wait_stream(be2.torch_stream)
            with torch.cuda.stream(side):
                if not join:
                    delay.enqueue(5.0)                     # the private stream is still busy when the call returns
                y.buf.copy_(x.buf, non_blocking=True)
            if join:
                be2.torch_stream.wait_stream(side)
        return call

    t_host, d_host = true.cpu().numpy(), decoy.cpu().numpy()
    (got,), _, info = so.run_delayed(be2, [(x, true, decoy)], consumer(False, True), [y], delay=delay, what="stand-in without fork")
    side.synchronize()
    assert info["returned_before_produced"]
    assert np.array_equal(got, d_host) and not np.array_equal(got, t_host), \
        "the unordered consumer was not caught: the delay, the decoys or the guards cannot see the defect class"
    (got,), _, info = so.run_delayed(be2, [(x, true, decoy)], consumer(True, False), [y], delay=delay, what="stand-in without join")
    side.synchronize()
    assert info["returned_before_produced"]
    assert not np.array_equal(got, t_host) and (np.array_equal(got, d_host) or np.all(got == so.SENTINEL)), \
        "work left on an unjoined stream was not caught by the refill and the download on the ctx stream"
    (got,), _, info = so.run_delayed(be2, [(x, true, decoy)], consumer(True, True), [y], delay=delay, what="ordered stand-in")
    side.synchronize()
    assert info["returned_before_produced"] and np.array_equal(got, t_host)


# ---- ctx plumbing ------------------------------------------------------------------------------------------------------
def _producer(be2, delay, n=4096):
    """a delayed fill of a fresh buffer on the ctx stream: (buffer, expected host values, event `produced`)"""
    import torch
    from mpskit_jl_amd.backend import DTensor
    s = be2.torch_stream
    src = torch.arange(n, dtype=torch.float64, device=be2.device) % 7.0 - 3.0
    x = DTensor(torch.full((n,), 5.0, dtype=torch.float64, device=be2.device), (n,))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay.enqueue(delay.chosen_ms)
        x.buf.copy_(src, non_blocking=True)
        produced = torch.cuda.Event()
        produced.record(s)
    return x, src.cpu().numpy(), produced


def test_get_stream_returns_the_bound_handle(be, be2):
    h = C.c_void_p(1)
    assert be2.lib.mpsk_ctx_get_stream(be2.ctx, C.byref(h)) == 0
    assert (h.value or 0) == be2.torch_stream.cuda_stream != 0
    assert be.lib.mpsk_ctx_get_stream(be.ctx, C.byref(h)) == 0
    assert (h.value or 0) == be.torch_stream.cuda_stream


def test_synchronize_returns_only_after_the_producer(be2, delay):
    x, _, produced = _producer(be2, delay)
    assert not produced.query(), "delay too short"
    be2.synchronize()
    assert produced.query()


def test_set_stream_synchronises_the_old_stream_and_orders_on_the_new_one(be2, delay):
    import torch
    old = be2.torch_stream
    new = torch.cuda.Stream(0)
    x, want, produced = _producer(be2, delay)
    assert not produced.query(), "delay too short"
    try:
        be2.bind_stream(new)                                   # work is queued on the old stream
        assert produced.query(), "mpsk_ctx_set_stream returned with the old stream still busy"
        h = C.c_void_p()
        assert be2.lib.mpsk_ctx_get_stream(be2.ctx, C.byref(h)) == 0 and h.value == new.cuda_stream
        # the next call is ordered on the NEW stream: a second delayed producer there, the norm of its product read at once
        x2, want2, produced2 = _producer(be2, delay)
        assert not produced2.query(), "delay too short"
        got = be2.norm(x2)
        assert produced2.query() and got == np.sqrt(float(want2 @ want2))
        assert be2.norm(x) == np.sqrt(float(want @ want))
    finally:
        be2.bind_stream(old)


def test_set_stream_is_refused_inside_a_side_section_and_with_a_factorization_pending(be2):
    import torch
    import exact_factor_inputs as fi
    other = torch.cuda.Stream(0)
    cur = be2.torch_stream.cuda_stream
    lib = be2.lib

    def refused(text):
        rc = lib.mpsk_ctx_set_stream(be2.ctx, C.c_void_p(other.cuda_stream))
        msg = lib.mpsk_last_error().decode()
        return rc, msg, text in msg

    be2.side_mark()
    be2.side_begin()
    try:
        rc, msg, ok = refused("side-stream section")
    finally:
        be2.side_end()
    assert rc == 1 and ok, (rc, msg)                          # MPSK_ERR_INVALID
    m, n = 768, 256                                           # the CholeskyQR3 path of mpsk_qrpos2: the deferral stays pending
    A1, A2 = be2_upload(be2, fi.qr_matrix(m, n, 3)[0]), be2_upload(be2, fi.qr_matrix(m, n, 4)[0])
    with torch.cuda.stream(be2.torch_stream):
        be2.qr_defer()
        out = be2.qrpos2(A1, A2)
        try:
            rc, msg, ok = refused("deferred factorization is pending")
        finally:
            redone = be2.qr_commit()
    assert rc == 1 and ok, (rc, msg)
    assert redone == 0 and out is not None
    h = C.c_void_p()
    assert lib.mpsk_ctx_get_stream(be2.ctx, C.byref(h)) == 0 and h.value == cur      # both refusals left the binding alone
    assert lib.mpsk_ctx_set_stream(be2.ctx, C.c_void_p(cur)) == 0


def be2_upload(be2, a):
    import torch
    with torch.cuda.stream(be2.torch_stream):
        t = be2.upload(a)
    be2.synchronize()
    return t
