"""ISA-level invariants of digest_shards_kernel and read_shards_kernel (CPU
only: hipcc cross-compiles; the listing is `make asm`'s).

* `make asm` shows digest_shards_kernel in 2 policies x 2 workgroup sizes x 2
  table capacities and read_shards_kernel at every shape and both capacities;
* no instantiation uses scratch memory or spills a vector register;
* every 16-byte load of an NT instantiation carries `nt`;
* the read stores its 16 bytes `sc1`; the digest stores no 16 bytes and issues
  the one 64-bit atomic add per tile that digest_kernel issues.
"""
from __future__ import annotations

import re

import pytest

import isa_listing
from isa_listing import atomic_adds as _atomic_adds, loads16 as _loads16, stores16 as _stores16


def _nt(name: str) -> bool:
    # NT is the only bool among the template arguments of both kernels
    return re.search(r"Lb1E", name) is not None


@pytest.fixture(scope="module")
def digests() -> dict[str, dict]:
    out = isa_listing.kernels("digest_shards")
    assert len(out) == 8, f"{len(out)} digest_shards instantiations in the ISA"
    return out


@pytest.fixture(scope="module")
def reads() -> dict[str, dict]:
    out = isa_listing.kernels("read_shards")
    # 7 member counts x 2 unrolls x 2 policies x 2 workgroup sizes, x 2 capacities
    assert len(out) == 56 * 2, f"{len(out)} read_shards instantiations in the ISA"
    return out


def test_both_capacities_of_every_shape(digests, reads):
    for group, per_cap in ((digests, 4), (reads, 56)):
        for cap in (64, 256):
            assert sum(1 for n in group if f"ELj{cap}EE" in n) == per_cap, cap
        assert sum(_nt(n) for n in group) == per_cap


def test_no_scratch_and_no_vector_spill(digests, reads):
    text = isa_listing.ASM.read_text()
    meta = dict(re.findall(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S))
    for name in list(digests) + list(reads):
        block = meta[name]
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name


def test_nt_instantiations_load_nt(digests, reads):
    for name, k in {**digests, **reads}.items():
        loads = _loads16(k["body"])
        assert loads, name
        if _nt(name):
            missing = [i for i in loads if not re.search(r"\bnt\b", i)]
            assert not missing, f"{name}: {missing[:3]}"


def test_read_stores_sc1(reads):
    for name, k in reads.items():
        stores = _stores16(k["body"])
        assert stores, name
        if _nt(name):
            other = [i for i in stores if not re.search(r"\bsc1\b", i) or re.search(r"\bnt\b", i)]
            assert not other, f"{name}: {other[:3]}"


def test_digest_stores_nothing_wide_and_adds_once_per_tile(digests):
    batch = isa_listing.kernels("digest")
    assert len(batch) == 4
    for name, k in digests.items():
        assert not re.search(r"_store_dwordx[234]", k["body"]), name
        adds = _atomic_adds(k["body"])
        assert len(adds) == 1 and re.search(r"_atomic_add_(x2|u64)\b", adds[0]), (name, adds)
        # the batch kernel of the same policy and workgroup size issues the same one
        args = re.search(r"digest_shards_kernelI(Lb[01]ELi\d+E)", name).group(1)
        twin = [b for n, b in batch.items() if f"digest_kernelI{args}E" in n]
        assert len(twin) == 1, name
        twin_adds = _atomic_adds(twin[0]["body"])
        assert len(twin_adds) == 1
        assert adds[0].split()[0] == twin_adds[0].split()[0], (name, adds, twin_adds)
