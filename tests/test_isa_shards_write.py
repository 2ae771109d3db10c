"""ISA-level invariants of write_shards_kernel and readv_shards_kernel (CPU only:
hipcc cross-compiles; the listing is `make asm`'s).

* `make asm` shows write_shards_kernel <U, NT, T, DIG, CAP> in 2 unrolls x 2
  policies x 2 workgroup sizes x with / without digest upkeep x 2 table capacities
  = 32, and readv_shards_kernel <NM, U, NT, T, CAP> at every shape and both
  capacities = 112, half per capacity each;
* no instantiation uses scratch memory or spills a vector register;
* every 16-byte load of an NT instantiation carries `nt`;
* an NT write stores through st16_block's buffer store with exactly one policy,
  `sc1` (new data) or `nt` (parity), and issues both; an NT read stores `sc1`;
* a DIG = false write holds no atomic add; a DIG = true one issues 64-bit adds
  only.
Nothing else about the instruction stream is looked at.
"""
from __future__ import annotations

import re

import pytest

import isa_listing
from isa_listing import atomic_adds as _atomic_adds, loads16 as _loads16, stores16 as _stores16


@pytest.fixture(scope="module")
def writes() -> dict[str, dict]:
    out = isa_listing.kernels("write_shards")
    assert len(out) == 32, f"{len(out)} write_shards instantiations in the ISA"
    return out


@pytest.fixture(scope="module")
def reads() -> dict[str, dict]:
    out = isa_listing.kernels("readv_shards")
    # 7 member counts x 2 unrolls x 2 policies x 2 workgroup sizes, x 2 capacities
    assert len(out) == 112, f"{len(out)} readv_shards instantiations in the ISA"
    return out


def _wargs(name: str):
    """(U, NT, T, DIG, CAP) of ...write_shards_kernelILi1ELb1ELi64ELb0ELj64EE..."""
    m = re.search(r"_kernelILi([12])ELb([01])ELi(64|256)ELb([01])ELj(64|256)EE", name)
    assert m, name
    return int(m.group(1)), m.group(2) == "1", int(m.group(3)), m.group(4) == "1", int(m.group(5))


def _rargs(name: str):
    """(NM, U, NT, T, CAP) of ...readv_shards_kernelILi8ELi1ELb1ELi64ELj64EE..."""
    m = re.search(r"_kernelILi(\d+)ELi([12])ELb([01])ELi(64|256)ELj(64|256)EE", name)
    assert m, name
    return int(m.group(1)), int(m.group(2)), m.group(3) == "1", int(m.group(4)), int(m.group(5))


def test_instantiation_count_is_the_template_set(writes, reads):
    combos = [_wargs(n) for n in writes]
    assert len(set(combos)) == 32
    for cap in (64, 256):
        assert sum(1 for c in combos if c[4] == cap) == 16, cap
    for u in (1, 2):
        for nt in (False, True):
            for t in (64, 256):
                for dig in (False, True):
                    assert sum(1 for c in combos if c[:4] == (u, nt, t, dig)) == 2, (u, nt, t, dig)
    combos = [_rargs(n) for n in reads]
    assert len(set(combos)) == 112
    for cap in (64, 256):
        assert sum(1 for c in combos if c[4] == cap) == 56, cap
    assert {c[0] for c in combos} == {0, 1, 2, 4, 8, 16, 32}
    assert sum(c[2] for c in combos) == 56


def test_no_scratch_and_no_vector_spill(writes, reads):
    text = isa_listing.ASM.read_text()
    meta = dict(re.findall(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S))
    for name in list(writes) + list(reads):
        block = meta[name]
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name


def test_nt_instantiations_load_nt(writes, reads):
    for name, k in {**writes, **reads}.items():
        loads = _loads16(k["body"])
        assert loads, name
        is_nt = _wargs(name)[1] if name in writes else _rargs(name)[2]
        if is_nt:
            missing = [i for i in loads if not re.search(r"\bnt\b", i)]
            assert not missing, f"{name}: {missing[:3]}"


def test_write_stores_new_data_sc1_and_parity_nt(writes):
    for name, k in writes.items():
        stores = _stores16(k["body"])
        assert stores, name
        if not _wargs(name)[1]:
            continue
        both = [i for i in stores if re.search(r"\bnt\b", i) and re.search(r"\bsc1\b", i)]
        plain = [i for i in stores if not re.search(r"\b(nt|sc1)\b", i)]
        assert not both and not plain, f"{name}: {(both + plain)[:3]}"
        assert all(i.startswith("buffer_store_dwordx4") for i in stores), name
        assert any(re.search(r"\bsc1\b", i) for i in stores), f"{name}: no sc1 (data) store"
        assert any(re.search(r"\bnt\b", i) for i in stores), f"{name}: no nt (parity) store"


def test_read_stores_sc1(reads):
    for name, k in reads.items():
        stores = _stores16(k["body"])
        assert stores, name
        if _rargs(name)[2]:
            other = [i for i in stores if not re.search(r"\bsc1\b", i) or re.search(r"\bnt\b", i)]
            assert not other, f"{name}: {other[:3]}"


def test_digest_upkeep_is_its_own_instantiation(writes):
    for name, k in writes.items():
        adds = _atomic_adds(k["body"])
        if _wargs(name)[3]:
            assert adds, name
            narrow = [i for i in adds if not re.match(r"\w+_atomic_add_(x2|u64)\b", i)]
            assert not narrow, f"{name}: {narrow[:3]}"
        else:
            assert not adds, f"{name}: {adds[:3]}"


def test_reads_hold_no_atomic(reads):
    for name, k in reads.items():
        assert not _atomic_adds(k["body"]), name
