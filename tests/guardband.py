"""Guard bands for buffers handed to the C-ABI (tests/test_gpu_buffer_contracts.py,
tests/test_gpu_key_lengths.py; self-test in tests/test_guardband_cpu.py).

An output or workspace of exactly the size include/adl_bloom.h promises sits
inside a larger tensor filled with a known byte; after the call the bands on
both sides must still hold that byte.  torch.empty would hide an overrun in the
caching allocator's round-up or in a neighbouring tensor.

Inputs get the opposite treatment (`Poisoned`): 0xFF before and after, so a
byte from outside a key that reaches its hash changes the result (a zero pad
does not show under a sign-extending hash of a tail word).

Neither helper places a buffer at the end of an allocation: reads outside a
buffer are not tested (they could only show as a GPU fault).
"""
import numpy as np
import torch


class GuardBandError(AssertionError):
    """band: "lead" or "tail"; count: damaged bytes in that band; first: offset of
    the first damaged byte, relative to the payload's start (lead band, negative)
    or to the payload's end (tail band, 0 = the byte right after the payload)."""

    def __init__(self, name, band, count, first):
        self.band, self.count, self.first = band, count, first
        where = f"payload start{first:+d}" if band == "lead" else f"payload end+{first}"
        super().__init__(f"{name}: {count} byte(s) of the {band} guard band written, the first at {where}")


def _place(base, lead, align, skew):
    """Offset of the first address >= base + lead that is a multiple of `align`
    but not of 2*align, plus `skew`."""
    p = -(-(base + lead) // align) * align
    if p % (2 * align) == 0:
        p += align
    return p + skew - base


class Guarded:
    """nbytes of payload at an address aligned to `align` and deliberately not to
    2*align (plus `skew` bytes), inside one uint8 tensor filled with `fill`:
    at least `lead` bytes of band before it and exactly `tail` after it."""

    def __init__(self, nbytes, align, lead=4096, tail=4096, fill=0xA5, pinned_host=False, device="cuda", skew=0,
                 name="buffer"):
        assert align >= 1 and align & (align - 1) == 0
        self.nbytes, self.fill, self.name = int(nbytes), fill, name
        if pinned_host:
            self.buf = torch.empty(lead + 2 * align + skew + self.nbytes + tail, dtype=torch.uint8, pin_memory=True)
        else:
            self.buf = torch.empty(lead + 2 * align + skew + self.nbytes + tail, dtype=torch.uint8, device=device)
        self.buf.fill_(fill)
        self.start = _place(self.buf.data_ptr(), lead, align, skew)
        self.end = self.start + self.nbytes
        self.buf = self.buf[:self.end + tail]
        self.ptr = self.buf.data_ptr() + self.start
        assert (self.ptr - skew) % align == 0 and (self.ptr - skew) % (2 * align) != 0

    @property
    def view(self):
        return self.buf[self.start:self.end]

    def numpy(self):
        """The payload, downloaded."""
        return self.view.cpu().numpy()

    def check(self):
        """Both bands still hold `fill` (compared where the buffer lives; only
        the count and the first offset come back)."""
        for band, part, origin in (("lead", self.buf[:self.start], self.start), ("tail", self.buf[self.end:], 0)):
            bad = part != self.fill
            count = int(bad.sum().item())
            if count:
                first = int(bad.to(torch.uint8).argmax().item())
                raise GuardBandError(self.name, band, count, first - origin)


def check_all(*guarded):
    for g in guarded:
        g.check()


class Poisoned:
    """A device copy of an input array with 0xFF bytes before it and at least 32
    after it, at an address aligned to `align`, not to 2*align, plus `skew`."""

    def __init__(self, array, align, skew=0, device="cuda"):
        a = np.ascontiguousarray(array)
        raw = a.reshape(-1).view(np.uint8)
        self.nbytes = raw.size
        self.buf = torch.full((64 + 2 * align + skew + self.nbytes + 64,), 0xFF, dtype=torch.uint8, device=device)
        self.start = _place(self.buf.data_ptr(), 64, align, skew)
        if self.nbytes:
            self.buf[self.start:self.start + self.nbytes] = torch.from_numpy(raw.copy()).to(device)
        self.ptr = self.buf.data_ptr() + self.start
