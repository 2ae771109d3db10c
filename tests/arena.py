"""A guarded store arena for the tests: one allocation, sub-buffers packed at
exactly their minimum alignment, and a check that nothing outside the regions
a call may write has changed.

A parity store holds its buffers this way -- data, parity, bitmaps, digests and
scratch carved out of one allocation -- so a store one granule past the end of
a buffer lands in a neighbour, not in slack nobody looks at.  The arena is
filled with a pattern that depends on the byte offset (no 16 consecutive bytes
are constant or zero, so a 16-byte granule of zeros, of one value or of data
meant for another place always differs from it) and keeps a pristine copy.
`check(writable=[...])` compares the two everywhere except inside the named
regions: the guard bands AND every region not named, which is how inputs are
proven unwritten.

What it cannot see: a stray READ, and a stray write that lands outside the
allocation.  The outermost bands are wide (at least `edge` bytes) so that a
near miss of up to one block lands inside.

Works on "cuda" and on "cpu" (tests/test_arena_checker.py runs without a
device).  No library code is involved.
"""
from __future__ import annotations

import bisect

GUARD = 256  # least distance between two regions carved without gap=0


def _torch():
    import torch
    return torch


def pattern_bytes(n, device, start=0):
    """Byte at arena offset o: (167*o + 13*(o >> 8) + 89) mod 256.  167 is odd,
    so neighbours always differ (by 167, or 180 across a 256-byte row)."""
    torch = _torch()
    out = torch.empty(n, dtype=torch.uint8, device=device)
    step = 1 << 22  # int64 temporaries of 32 MiB, not of 8 bytes per arena byte
    for lo in range(0, n, step):
        o = torch.arange(start + lo, start + min(lo + step, n), dtype=torch.int64, device=device)
        out[lo:lo + step] = ((o * 167 + (o >> 8) * 13 + 89) & 0xFF).to(torch.uint8)
    return out


class ArenaError(AssertionError):
    """A byte outside the writable regions changed.  offset: the first such
    arena offset; place: the region or band it falls in; nearest / edge /
    distance: the closest carved region, which of its ends ("start" or "end")
    and how many bytes from it (0 at `end` = the first byte past the region,
    1 before `start` = the last byte in front of it); count: differing bytes."""

    def __init__(self, msg, offset, place, nearest, edge, distance, count):
        super().__init__(msg)
        self.offset, self.place, self.nearest = offset, place, nearest
        self.edge, self.distance, self.count = edge, distance, count


class Arena:
    def __init__(self, nbytes, device, edge=4096, pin=False):
        """edge: least width of the first and of the last band; callers pass
        max(bs, 4096), so a store one whole block off still lands inside.
        pin: a "cpu" arena in page-locked memory (needs a device)."""
        torch = _torch()
        self.nbytes, self.device, self.edge = int(nbytes), device, max(int(edge), 4096)
        self.buf = pattern_bytes(self.nbytes, device)
        if pin:
            self.buf = self.buf.pin_memory()
        self.pristine = self.buf.clone()
        self.base = self.buf.data_ptr()
        self.regions: dict[str, tuple[int, int]] = {}  # name -> (start, end) arena offsets
        self._order: list[str] = []                    # names by start offset (carving order)
        self._cursor = 0                               # end of the last region
        assert torch.equal(self.buf, self.pristine)

    # ---- carving ---------------------------------------------------------
    def carve(self, name, nbytes, align, gap=None, modulus=None):
        """A view of `nbytes` bytes whose address p is at EXACTLY the minimum
        alignment: p % align == 0 and p % (2*align) == align; for align == 1 p
        is odd.  `modulus` (a multiple of 2*align) asks for p % modulus ==
        align instead, for a region whose END must meet a flush neighbour's
        alignment.  At least GUARD bytes (edge bytes in front of the first
        region) separate it from the previous region, unless gap=0: then it
        starts where the previous region ends, and only p % align == 0 holds."""
        assert name not in self.regions and nbytes > 0 and align >= 1 and align & (align - 1) == 0
        if gap == 0:
            assert self._order, "gap=0 needs a previous region"
            start = self._cursor
            assert (self.base + start) % align == 0, f"{name}: a flush start is not {align}-aligned"
        else:
            assert gap is None, "gap is 0 or left out"
            mod = 2 * align if modulus is None else modulus
            assert mod % (2 * align) == 0
            lo = self.base + self._cursor + (GUARD if self._order else self.edge)
            start = lo + (align - lo) % mod - self.base  # the first p >= lo with p % mod == align
        end = start + nbytes
        assert end + self.edge <= self.nbytes, f"arena too small for {name}: {end + self.edge}"
        self.regions[name] = (start, end)
        self._order.append(name)
        self._cursor = end
        return self.buf[start:end]

    def __getitem__(self, name):
        start, end = self.regions[name]
        return self.buf[start:end]

    def ptr(self, name):
        return self.base + self.regions[name][0]

    def size(self, name):
        start, end = self.regions[name]
        return end - start

    @staticmethod
    def room(sizes, edge=4096):
        """Bytes that hold regions of `sizes` (an iterable of (nbytes, align))
        whatever the base address: both outer bands, a guard and the
        alignment slack (up to a whole modulus of 128) per region."""
        edge = max(int(edge), 4096)
        return 2 * edge + sum(n + GUARD + 2 * max(a, 64) for n, a in sizes) + 512

    # ---- the test's own writes --------------------------------------------
    def put(self, name, src):
        """The test's own write: region <- src (a tensor or numpy array of the
        region's size in bytes), adopted as pristine."""
        torch = _torch()
        if not hasattr(src, "data_ptr"):
            import numpy as np
            src = torch.from_numpy(np.ascontiguousarray(src).reshape(-1).view(np.uint8))
        src = src.reshape(-1).view(torch.uint8)
        start, end = self.regions[name]
        assert src.numel() == end - start, (name, src.numel(), end - start)
        self.buf[start:end].copy_(src)
        self.pristine[start:end].copy_(self.buf[start:end])

    def fill(self, name, value):
        """The test's own write: every byte of the region = value, adopted.
        Outputs are prefilled so that a call that writes nothing is seen."""
        start, end = self.regions[name]
        self.buf[start:end].fill_(value)
        self.pristine[start:end].fill_(value)

    def adopt(self, names):
        """The test wrote into these regions through their views."""
        for name in names:
            start, end = self.regions[name]
            self.pristine[start:end].copy_(self.buf[start:end])

    # ---- the check -----------------------------------------------------------
    def describe(self, offset):
        """(place, nearest region, which of its ends, distance) of an arena offset."""
        names = self._order
        starts = [self.regions[n][0] for n in names]
        i = bisect.bisect_right(starts, offset) - 1  # the last region starting at or before
        if i >= 0 and offset < self.regions[names[i]][1]:
            place = f"region '{names[i]}'"
        elif i < 0:
            place = f"the outermost band before '{names[0]}'" if names else "the empty arena"
        elif i == len(names) - 1:
            place = f"the outermost band after '{names[i]}'"
        else:
            place = f"the band between '{names[i]}' and '{names[i + 1]}'"
        best = None
        for n in names:
            s, e = self.regions[n]
            # bytes to the region's first byte / past its last byte
            for edge, d in (("start", abs(s - offset)), ("end", abs(offset - e))):
                if best is None or d < best[2]:
                    best = (n, edge, d)
        return (place,) + (best if best else (None, None, None))

    def check(self, writable, what=""):
        """Every byte outside the `writable` regions equals the pristine copy;
        then the writable regions' content becomes the pristine state.  One
        device synchronisation (the count) when nothing is wrong."""
        torch = _torch()
        for name in writable:
            assert name in self.regions, f"not a region of this arena: {name}"
        diff = self.buf != self.pristine
        for name in writable:
            start, end = self.regions[name]
            diff[start:end] = False
        count = int(diff.sum().item())
        if count:
            offset = int(torch.nonzero(diff)[0].item())
            place, nearest, edge, distance = self.describe(offset)
            side = "" if nearest is None else (
                f", {distance} byte(s) from the {edge} of '{nearest}'")
            raise ArenaError(
                f"{what}: {count} byte(s) changed outside writable={sorted(writable)}; the first "
                f"at arena offset {offset} in {place}{side} (holds "
                f"{int(self.buf[offset].item()):#04x}, was {int(self.pristine[offset].item()):#04x})",
                offset, place, nearest, edge, distance, count)
        self.adopt(writable)
