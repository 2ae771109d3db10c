"""The device parity scrub on an MI355X: xec_verify flags exactly the classes
whose data and parity no longer XOR to zero, counts each once, zeroes its flag
buffer itself and writes nothing else."""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_repair import BS, KM, LAUNCHES, SS, Case, set_shape

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def scrub(xec, c: Case, with_count=True):
    """xec_verify over c; returns (flagged class indices, count or None).  The
    flag buffer starts as 0xFF and the count as 77: the call must set both."""
    torch = _torch()
    flags = torch.full((c.S * c.m + 3,), 0xFF, dtype=torch.uint8, device="cuda")
    count = torch.full((2,), 77, dtype=torch.int32, device="cuda") if with_count else None
    st = xec.verify(c.d, c.p, c.S, c.bs, c.k, c.m, flags, count, c.b.stream)
    assert st == xec.Status.SUCCESS
    torch.cuda.synchronize()
    assert flags[c.S * c.m:].tolist() == [0xFF] * 3, "flags written past S*m"
    got = flags[: c.S * c.m]
    assert int(got.max()) <= 1
    if with_count:
        assert int(count[1].item()) == 77
    return torch.nonzero(got).flatten().tolist(), int(count[0].item()) if with_count else None


class Flip:
    """One bit of one block flipped, and flipped back on exit."""

    def __init__(self, c: Case, stripe, block, byte, bit=0x10):
        # block in [0, k) is a data block, k + j parity block j
        if block < c.k:
            self.cell = c.d.view(c.S, c.k, c.bs)[stripe, block, byte: byte + 1]
        else:
            self.cell = c.p.view(c.S, c.m, c.bs)[stripe, block - c.k, byte: byte + 1]
        self.bit = bit

    def __enter__(self):
        self.cell.bitwise_xor_(self.bit)
        return self

    def __exit__(self, *exc):
        self.cell.bitwise_xor_(self.bit)


@pytest.mark.parametrize("bs", BS)
@pytest.mark.parametrize("k,m", KM)
def test_verify_flags_exactly_the_broken_classes(gpu, oracle, k, m, bs):
    torch = _torch()
    rng = np.random.default_rng(k * 100 + m + bs)
    for S in SS:
        c = Case.get(gpu, oracle, S, k, m, bs)
        assert scrub(gpu, c) == ([], 0)
        assert scrub(gpu, c, with_count=False) == ([], None)  # a NULL d_count is accepted
        cs, j = int(rng.integers(S)), int(rng.integers(m))
        cls = cs * m + j
        last_member = j + m * (k // m - 1)
        places = [(j, 0), (j, bs - 1),            # first byte of a block, last (the ragged granule)
                  (k + j, int(rng.integers(bs))),  # the parity block
                  (last_member, int(rng.integers(bs)))]  # the class's last member
        for block, byte in places:
            with Flip(c, cs, block, byte, bit=1 << int(rng.integers(8))):
                assert scrub(gpu, c) == ([cls], 1), (S, block, byte)
        # two flips of one class, in different chunks where the block has several
        with Flip(c, cs, j, 5), Flip(c, cs, k + j, bs - 3):
            assert scrub(gpu, c) == ([cls], 1)
            assert scrub(gpu, c, with_count=False) == ([cls], None)
        # two errors of one class that cancel are invisible (include/xec.h)
        with Flip(c, cs, j, 9), Flip(c, cs, k + j, 9):
            assert scrub(gpu, c) == ([], 0)
        # one flip in every class
        d3 = c.d.view(S, k, bs)
        cols = torch.from_numpy(rng.integers(bs, size=(S, m))).to("cuda")
        rows = torch.arange(S, device="cuda")[:, None].expand(S, m)
        blks = torch.arange(m, device="cuda")[None, :].expand(S, m)  # member 0 of each class
        d3[rows, blks, cols] ^= 0x80
        try:
            assert scrub(gpu, c) == (list(range(S * m)), S * m)
        finally:
            d3[rows, blks, cols] ^= 0x80
        c.assert_exact("the scrub changed data or parity")


@pytest.mark.parametrize("shape", LAUNCHES, ids=lambda s: "-".join(f"{a}{b}" for a, b in s.items()))
def test_verify_launch_shapes_identical(gpu, oracle, shape):
    try:
        set_shape(gpu, **shape)
        for (k, m, bs, S) in [(12, 3, 4352, 23), (32, 1, 1280, 3), (10, 2, 4352, 3)]:
            c = Case.get(gpu, oracle, S, k, m, bs)
            assert scrub(gpu, c) == ([], 0)
            cs, j = S - 1, m - 1
            with Flip(c, cs, j, bs - 1), Flip(c, 0, k, 1030):
                want = sorted({cs * m + j, 0})
                assert scrub(gpu, c) == (want, len(want))
            c.assert_exact()
    finally:
        set_shape(gpu)


def test_verify_argument_errors_queue_nothing(gpu, oracle):
    torch = _torch()
    S, k, m, bs = 3, 8, 4, 1280
    c = Case.get(gpu, oracle, S, k, m, bs)
    flags = torch.full((S * m,), 0xFF, dtype=torch.uint8, device="cuda")
    count = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    St = gpu.Status
    s = c.b.stream
    assert gpu.verify(c.d, c.p, S, bs, k, m, None, count, s) == St.INVALID_SIZE
    assert gpu.verify(c.d, c.p, S, bs, k, m, flags, count.data_ptr() + 2,
                      s) == St.INVALID_ALIGNMENT
    assert gpu.verify(c.d.data_ptr() + 16, c.p, S, bs, k, m, flags, count,
                      s) == St.INVALID_ALIGNMENT
    assert gpu.verify(c.d, c.p, S, 100, k, m, flags, count, s) == St.INVALID_SIZE
    assert gpu.verify(c.d, c.p, S, bs, 6, 4, flags, count, s) == St.INVALID_COUNTS
    torch.cuda.synchronize()
    assert count.tolist() == [77, 77] and int(flags.min()) == 0xFF
    assert gpu.verify(c.d, c.p, 0, bs, k, m, None, count, s) == St.SUCCESS  # S = 0: count 0
    torch.cuda.synchronize()
    assert count.tolist() == [0, 77] and int(flags.min()) == 0xFF
    c.assert_exact()
