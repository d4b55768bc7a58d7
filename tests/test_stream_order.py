"""Every launch, memset and copy of an entry point goes to the stream the caller set (-m gpu).

nlk_ctx_set_stream is how bench.py, the tools and the PyTorch recipe of INTEGRATION.md drive the library, on a
non-blocking torch stream. A launch that went to another stream (the context's own one, its second stream without
the join event, the null stream, which does not order with a non-blocking stream) would read its inputs before the
caller's work on that stream has produced them. Here the caller's stream is held back by a long delay, behind which
the real inputs are copied over buffers full of NaN: a call that does not wait in line computes on the NaN."""
import numpy as np
import pytest

import ctx_ops
from ctx_ops import OPS, with_env

pytestmark = pytest.mark.gpu

DELAY_N, DELAY_MATMULS = 2048, 200   # the delay: a chain of DELAY_MATMULS fp32 products of DELAY_N x DELAY_N matrices
WINDOWS = 3   # caller's streams tried per op (see the test)
_delay_state = {}


@pytest.fixture(scope="module")
def torch_ready():
    """torch on the device, the delay's buffers and the BLAS kernels it runs: set up once, outside every window (the
    first product of a process loads the kernel library, which takes seconds)."""
    import torch
    dev = torch.device("cuda", 0)
    m = torch.eye(DELAY_N, device=dev) * 0.5
    _delay_state.update(m=m, a=m.clone(), b=m.clone())
    torch.mm(_delay_state["a"], m, out=_delay_state["b"])
    torch.cuda.synchronize()
    return torch


def _delay():
    """Enqueue the delay on the current stream: ordinary torch work, no host synchronisation, no allocation."""
    import torch
    m, a, b = _delay_state["m"], _delay_state["a"], _delay_state["b"]
    for _ in range(DELAY_MATMULS // 2):
        torch.mm(a, m, out=b)
        torch.mm(b, m, out=a)


@pytest.mark.parametrize("op", OPS, ids=[op.name for op in OPS])
def test_calls_follow_the_callers_stream(built, monkeypatch, torch_ready, op):
    """A fresh context, warmed up by one run of the op (on other input values) on its own stream (growth, table
    uploads and first-use allocations done), then on a torch stream s, with no host synchronisation in between: inputs allocated as 0xFF
    bytes (NaN), the delay, event e, the real inputs copied in, the op on the tensors' data_ptr(), the outputs cloned.
    After s.synchronize() the outputs must be the op's fresh-context result. Where the op is not listed as
    synchronising (ctx_ops: syncs), e must not have happened when the library call returns: the window was open (the
    test did not pass vacuously) and the call did not wait for the device.

    Streams share the device's few hardware queues (four by default), and two streams on one queue run in the order
    of submission whatever stream they are: a launch that went to the wrong stream is then ordered by accident. So
    the window is opened WINDOWS times, on streams torch hands out one after the other (they sit on different
    queues): the context's own streams can share a queue with one of them at most, and every window must hold.

    The delay has to be at least ten times the longest op, so that it also covers the host's time to enqueue the
    longest call on a loaded host. Every window measures both with torch events (b0 before the delay, e behind it,
    a1 behind the call: the delay is b0 -> e, the call with the copies of its inputs e -> a1) and prints them, so
        pytest -m gpu tests/test_stream_order.py -rA | grep "stream-order:"
    re-measures the margin when ops are added. That command gave, on an MI355X (ROCm 7.0.2, torch-rocm, at the commit
    that added this file): delay 23.7 - 24.2 ms; the longest call 1.91 ms (tvl1-131x97, which waits for the device by
    itself), the longest that does not wait 1.29 ms (flt1-temporal-p20c3-90x70). The delay is 12 times the longest
    call. (The host needs 0.01 - 0.17 ms to enqueue a call that does not wait: time.perf_counter around the call.)"""
    torch = torch_ready
    I, want = ctx_ops.fresh(built, monkeypatch, op)
    want = {k: v for k, v in want.items() if k != "records"}
    dev = torch.device("cuda", 0)
    c = ctx_ops.context(built)
    try:
        # (warmed up on OTHER values of the same shapes and parameters: what the warm-up leaves in the context's
        # scratch and in its accumulator is not the answer, so a kernel that runs early cannot find it there)
        with_env(op, monkeypatch, lambda: op.run(c, op.inputs(1)))
        host = {k: np.ascontiguousarray(a).view(np.uint8).reshape(-1) for k, a in I["in"].items()}
        staged = {k: torch.from_numpy(a.copy()).to(dev) for k, a in host.items()}
        sizes = {k: a.size for k, a in host.items()}
        for k, (shape, dtype) in I["out"].items():
            sizes.setdefault(k, int(np.prod(shape)) * np.dtype(dtype).itemsize)
        torch.cuda.synchronize()
        for n in range(WINDOWS):
            s = torch.cuda.Stream(device=dev)
            c.set_stream(s.cuda_stream)
            with torch.cuda.stream(s):
                bufs = {k: torch.full((max(n_, 1),), 0xFF, dtype=torch.uint8, device=dev) for k, n_ in sizes.items()}
                b0, e, a1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                b0.record(s)
                _delay()
                e.record(s)
                for k, t in staged.items():
                    bufs[k][:sizes[k]].copy_(t, non_blocking=True)
                d = {k: t.data_ptr() for k, t in bufs.items()}
                extra = with_env(op, monkeypatch, lambda: op.call(c, d, I)) or {}
                waited = e.query()
                a1.record(s)
                outs = {k: bufs[k].clone() for k in I["out"]}
            s.synchronize()
            print(f"stream-order: {op.name} window {n}: delay {b0.elapsed_time(e):.2f} ms, call {e.elapsed_time(a1):.3f} ms, "
                  f"waited {waited}")
            got = {k: outs[k][:sizes[k]].cpu().numpy().view(dtype).reshape(shape) for k, (shape, dtype) in I["out"].items()}
            got.update({k: np.asarray(v) for k, v in extra.items()})
            op.same(got, want, f"{op.name} on the caller's stream (window {n})", I)
            if not op.syncs:
                assert not waited, (f"{op.name}: the delay enqueued before the call had finished when the call returned: "
                                    "the call waited for the device (or the delay is too short for this host)")
    finally:
        c.L.nlk_ctx_use_own_stream(c.h)
        c.close()
