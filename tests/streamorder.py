"""Stream-ordering harness for the C-ABI's entry points (tests/test_gpu_streams.py).

include/adl_bloom.h promises that every entry point enqueues its work on the
caller's stream.  On torch's default stream (handle 0, the legacy null stream)
a breach cannot show: the null stream orders itself against every blocking
stream.  A `Case` therefore runs one entry point on a fresh non-blocking
stream `s` and arranges that work issued anywhere else computes something
visibly different:

* every tensor is allocated up front, then one torch.cuda.synchronize();
* inputs start as a *decoy* (another valid input of the same shape whose
  expected output differs), outputs as 0xA5 bytes, workspaces as 0x5A bytes;
* on `s`, with no host synchronisation in between: a delay, a producer that
  copies the true inputs over the decoys, the entry point with stream = s, a
  consumer that copies every output into pinned host memory, and at the very
  end one s.synchronize().

The delay is 16 fill_ passes over a 1 GiB tensor: 16 GiB of writes, at least
2 ms at the HBM's 8 TB/s peak, which no run can beat -- two orders of
magnitude above a launch latency, and derived, not measured.  Work that runs
off `s` starts at least those 2 ms before the producer and so computes from
the decoy, or it ends after the consumer and the host sees 0xA5.  Either way
the bytes differ from the CPU oracle's on the true inputs (`check`).  The
producer also writes 0xA5 over every output once more, so that an entry point
with no input to go stale (the key generators) or one that only initialises
its output (verify's memsets) is caught as well: what it wrote early is gone.

No spinning kernel, no kernel waiting on a host flag, no graph capture; only
data can go stale, nothing can fault.  A case keeps every tensor alive until
after its final synchronise.

`Case.returned_early` says whether the entry point came back while the delay
was still running (an event recorded right after the delay had not completed):
the *_device functions do not synchronise.
"""
import ctypes

import numpy as np
import torch

OUT_FILL = 0xA5
WS_FILL = 0x5A
DELAY_BYTES = 1 << 30
DELAY_PASSES = 16

_delay_buf = {}


class StreamOrderError(AssertionError):
    """count: differing bytes; untouched: how many of them still hold 0xA5 (the
    consumer ran before the writer); first: index of the first differing byte."""

    def __init__(self, name, count, untouched, first, size):
        self.count, self.untouched, self.first = count, untouched, first
        super().__init__(f"{name}: {count} of {size} byte(s) differ from the oracle's, the first at {first}; "
                         f"{untouched} of them still hold 0x{OUT_FILL:02X}")


def check(got, want, name="output"):
    """Byte-for-byte comparison of a result with the oracle's."""
    g = np.ascontiguousarray(got).reshape(-1).view(np.uint8)
    w = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    assert g.size == w.size, (name, g.size, w.size)
    bad = g != w
    count = int(bad.sum())
    if count:
        raise StreamOrderError(name, count, int((g[bad] == OUT_FILL).sum()), int(bad.argmax()), g.size)


def sptr(stream):
    """The hipStream_t of a torch stream (None: NULL) as a ctypes argument."""
    return None if stream is None else ctypes.c_void_p(stream.cuda_stream)


def delay(stream, device="cuda"):
    """Enqueue the delay on `stream` (a torch stream; the buffer is shared and
    lives until release_delay())."""
    buf = _delay_buf.get("buf")
    if buf is None:
        buf = _delay_buf["buf"] = torch.empty(DELAY_BYTES, dtype=torch.uint8, device=device)
    with torch.cuda.stream(stream):
        for i in range(DELAY_PASSES):
            buf.fill_(i)


def release_delay():
    torch.cuda.synchronize()
    _delay_buf.clear()


def _bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class Case:
    """One run of an entry point behind the delay on a fresh non-blocking stream."""

    def __init__(self, device="cuda"):
        self.device = device
        self.stream = torch.cuda.Stream(device=device)  # torch's pool streams are non-blocking
        self._inputs = []   # (device tensor holding the decoy, device tensor holding the truth)
        self._outputs = []  # (device tensor, pinned host tensor)
        self._keep = []
        self.returned_early = None

    def input(self, true, decoy, pad=0):
        """A device buffer of true.nbytes + pad bytes that starts as `decoy` and is
        overwritten with `true` by the producer (numpy arrays of equal size)."""
        t, d = _bytes(true), _bytes(decoy)
        assert t.size == d.size, "the decoy has the input's shape"
        assert t.size == 0 or not np.array_equal(t, d), "the decoy must differ from the input"
        dst = torch.zeros(max(t.size + pad, 1), dtype=torch.uint8, device=self.device)
        src = torch.zeros(max(t.size + pad, 1), dtype=torch.uint8, device=self.device)
        if t.size:
            dst[:t.size] = torch.from_numpy(d.copy()).to(self.device)
            src[:t.size] = torch.from_numpy(t.copy()).to(self.device)
        self._inputs.append((dst, src))
        return dst

    def const(self, array):
        """A device copy of an input that has no decoy (sizes, offsets)."""
        t = torch.from_numpy(_bytes(array).copy()).to(self.device)
        self._keep.append(t)
        return t

    def output(self, nbytes):
        """nbytes of 0xA5 on the device; the consumer copies them to pinned host memory."""
        dev = torch.full((max(int(nbytes), 1),), OUT_FILL, dtype=torch.uint8, device=self.device)
        host = torch.full((max(int(nbytes), 1),), OUT_FILL, dtype=torch.uint8).pin_memory()
        self._outputs.append((dev, host))
        return dev

    def workspace(self, nbytes):
        ws = torch.full((max(int(nbytes), 1),), WS_FILL, dtype=torch.uint8, device=self.device)
        self._keep.append(ws)
        return ws

    def run(self, entry):
        """entry(stream): calls the entry point(s) under test with stream = `stream`
        (a torch stream) and must not synchronise anything."""
        s = self.stream
        torch.cuda.synchronize()
        delay(s, self.device)
        after_delay = torch.cuda.Event()
        after_delay.record(s)
        with torch.cuda.stream(s):
            for dst, src in self._inputs:  # the producer
                dst.copy_(src)
            for dev, _ in self._outputs:
                dev.fill_(OUT_FILL)
        entry(s)
        self.returned_early = not after_delay.query()
        with torch.cuda.stream(s):
            for dev, host in self._outputs:  # the consumer
                host.copy_(dev, non_blocking=True)
        s.synchronize()
        return self

    def result(self, dev, nbytes=None):
        """The host copy of output `dev` (a tensor output() returned), as uint8."""
        for d, host in self._outputs:
            if d is dev:
                a = host.numpy()
                return a if nbytes is None else a[:int(nbytes)]
        raise KeyError("not an output of this case")
