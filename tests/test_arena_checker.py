"""The arena checker (tests/arena.py) has teeth: on a CPU arena, carve gives
exactly the minimum alignments with guard bands between the regions, and every
simulated stray store is reported at the right offset and place.  No device."""
from __future__ import annotations

import pytest

from arena import GUARD, Arena, ArenaError, pattern_bytes

BS = 1280


def _torch():
    import torch
    return torch


def layout():
    """in (64) | w (16) | flush (gap=0 after w) | odd (1) | four (4) | eight (8)"""
    a = Arena(64 << 10, "cpu", edge=max(BS, 4096))
    views = {"in": a.carve("in", 3 * BS, 64), "w": a.carve("w", 2 * BS, 16),
             "flush": a.carve("flush", 48, 16, gap=0), "odd": a.carve("odd", 33, 1),
             "four": a.carve("four", 4, 4), "eight": a.carve("eight", 8 * 7, 8)}
    return a, views


def test_pattern_has_no_constant_granule():
    torch = _torch()
    p = pattern_bytes(1 << 16, "cpu")
    assert bool((p[1:] != p[:-1]).all()), "two neighbouring bytes are equal"
    zeros = torch.nonzero(p == 0).flatten()
    assert bool((zeros[1:] - zeros[:-1] > 16).all())
    # it depends on the offset beyond one 256-byte row
    assert not torch.equal(p[:256], p[256:512])
    assert torch.equal(pattern_bytes(100, "cpu", start=1000), p[1000:1100])


def test_carve_alignments_bands_and_flush():
    a, v = layout()
    want = {"in": 64, "w": 16, "odd": 1, "four": 4, "eight": 8}
    for name, align in want.items():
        p = v[name].data_ptr()
        assert p == a.ptr(name) and v[name].numel() == a.size(name)
        if align == 1:
            assert p % 2 == 1, name
        else:
            assert p % align == 0 and p % (2 * align) == align, (name, p % (2 * align))
    # a modulus puts the region at `align` past a coarser boundary: still exactly minimal
    b = Arena(32 << 10, "cpu")
    assert b.carve("m", 48, 16, modulus=128).data_ptr() % 128 == 16
    # bands: the outer ones at least max(bs, 4096), the inner ones at least GUARD
    order = ["in", "w", "flush", "odd", "four", "eight"]
    spans = [a.regions[n] for n in order]
    assert spans[0][0] >= max(BS, 4096) and a.nbytes - spans[-1][1] >= max(BS, 4096)
    for (n0, (_, e0)), (n1, (s1, _)) in zip(zip(order, spans), zip(order[1:], spans[1:])):
        if n1 == "flush":
            assert s1 == e0, "gap=0 is not flush"
        else:
            assert s1 - e0 >= GUARD, (n0, n1)
    assert v["flush"].data_ptr() == v["w"].data_ptr() + v["w"].numel()
    assert v["flush"].data_ptr() % 16 == 0
    # the views are the arena's memory, and a clean arena checks clean
    v["four"][:] = 7
    assert a.buf[a.regions["four"][0]] == 7
    a.adopt(["four"])
    a.check(writable=[], what="clean")
    # a region that would leave less than the outer band is refused
    with pytest.raises(AssertionError):
        a.carve("big", a.nbytes, 64)


def stray(mutate, writable=("w",)):
    """A clean arena, one simulated stray store, the checker's report."""
    a, _ = layout()
    a.check(writable=[], what="before")
    mutate(a)
    with pytest.raises(ArenaError) as e:
        a.check(writable=list(writable), what="stray")
    return a, e.value


def flip(a, offset, n=1):
    a.buf[offset:offset + n] ^= 0xFF


def test_stray_stores_are_named():
    # one byte at end + 0 of a writable region (w's flush neighbour starts there)
    a, err = stray(lambda a: flip(a, a.regions["w"][1]))
    assert err.offset == a.regions["w"][1] and err.count == 1
    assert err.place == "region 'flush'" and (err.nearest, err.edge, err.distance) in (
        ("w", "end", 0), ("flush", "start", 0))
    # ... and of a writable region followed by a band
    a, err = stray(lambda a: flip(a, a.regions["flush"][1]), writable=("w", "flush"))
    assert err.offset == a.regions["flush"][1] and err.count == 1
    assert err.place == "the band between 'flush' and 'odd'"
    assert (err.nearest, err.edge, err.distance) == ("flush", "end", 0)
    assert "'flush'" in str(err) and f"offset {err.offset}" in str(err) and "1 byte(s)" in str(err)
    # one byte at start - 1
    a, err = stray(lambda a: flip(a, a.regions["w"][0] - 1))
    assert err.offset == a.regions["w"][0] - 1 and err.count == 1
    assert err.place == "the band between 'in' and 'w'"
    assert (err.nearest, err.edge, err.distance) == ("w", "start", 1)
    # 16 bytes one whole block past the end of the last region: the outermost band holds them
    a, err = stray(lambda a: flip(a, a.regions["eight"][1] + BS, 16), writable=("eight",))
    assert err.offset == a.regions["eight"][1] + BS and err.count == 16
    assert err.place == "the outermost band after 'eight'"
    assert (err.nearest, err.edge, err.distance) == ("eight", "end", BS)
    assert "16 byte(s)" in str(err)
    # one whole block past the end of `in`: lands inside w, which is not writable here
    a, err = stray(lambda a: flip(a, a.regions["in"][1] + BS, 16), writable=("in",))
    assert err.offset == a.regions["in"][1] + BS and err.count == 16
    assert err.place == "region 'w'"
    # one byte inside a carved region that was not declared writable
    a, err = stray(lambda a: flip(a, a.regions["in"][0] + 777))
    assert err.offset == a.regions["in"][0] + 777 and err.count == 1
    assert err.place == "region 'in'" and "region 'in'" in str(err)
    assert (err.nearest, err.edge, err.distance) == ("in", "start", 777)
    # one byte in the outermost band, at either end of the arena
    a, err = stray(lambda a: flip(a, 5))
    assert err.offset == 5 and err.place == "the outermost band before 'in'"
    assert (err.nearest, err.edge, err.distance) == ("in", "start", a.regions["in"][0] - 5)
    a, err = stray(lambda a: flip(a, a.nbytes - 1))
    assert err.offset == a.nbytes - 1 and err.place == "the outermost band after 'eight'"
    # the first of several is reported, all are counted
    a, err = stray(lambda a: (flip(a, a.nbytes - 9), flip(a, 100, 3)))
    assert err.offset == 100 and err.count == 4


def test_writes_inside_writable_regions_pass_and_are_adopted():
    a, v = layout()
    v["w"][:] = 0x11
    v["four"][:] = 0x22
    with pytest.raises(ArenaError) as e:
        a.check(writable=["w"], what="four was not declared")
    assert e.value.place == "region 'four'" and e.value.count == 4
    a.check(writable=["w", "four"], what="both declared")
    # adopted: the same content now checks clean with nothing writable ...
    a.check(writable=[], what="adopted")
    # ... and a later change of it is a stray write again
    v["w"][5] = 0x12
    with pytest.raises(ArenaError) as e:
        a.check(writable=[], what="after adoption")
    assert e.value.offset == a.regions["w"][0] + 5
    # a failed check adopts nothing
    with pytest.raises(ArenaError):
        a.check(writable=[], what="again")
    # put and fill are the test's own writes
    a.put("w", _torch().zeros(a.size("w"), dtype=_torch().uint8))
    a.fill("odd", 0xEE)
    a.check(writable=[], what="own writes")
    with pytest.raises(AssertionError):
        a.check(writable=["nobody"], what="unknown name")
