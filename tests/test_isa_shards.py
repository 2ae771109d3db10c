"""ISA-level invariants of the shard-layout kernels (CPU only: hipcc
cross-compiles; the listing is `make asm`'s, as tests/test_isa.py reads it).

* `make asm` shows encode_shards_kernel, repair_shards_kernel and
  verify_shards_kernel at every shape and both table capacities;
* no instantiation uses scratch memory or spills a vector register -- the
  32-member fast path holds 32 wave-uniform 64-bit shard addresses, which is
  where a spill would come from;
* the cache policies are those of the batch kernels: every 16-byte load of an NT
  instantiation `nt`, parity stored `nt`, a rebuilt data block `sc1`, and the
  scrub stores no 16 bytes at all;
* the default-shape instances at 16 and 32 members fit the registers of the
  residency their launch asks for, and the 32-member encode still issues every
  load before its first wait.
"""
from __future__ import annotations

import re

import pytest

import isa_listing
from isa_listing import loads16 as _loads16, nt as _nt, stores16 as _stores16

KINDS = ["encode_shards", "repair_shards", "verify_shards"]
AUTO_OCCUPANCY = {16: 2, 32: 1}  # auto_occupancy, csrc/xec_api.cpp


@pytest.fixture(scope="module")
def kernels() -> dict[str, dict]:
    out = isa_listing.kernels("|".join(KINDS))
    # 7 member counts x 2 unrolls x 2 policies x 2 workgroup sizes x 2 capacities, three kernels
    assert len(out) == 56 * 2 * 3, f"{len(out)} shard instantiations in the ISA"
    return out


def test_no_scratch_and_no_vector_spill(kernels):
    text = isa_listing.ASM.read_text()
    meta = dict(re.findall(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S))
    for name in kernels:
        block = meta[name]
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name


def test_cache_policies_are_the_batch_kernels(kernels):
    for name, k in kernels.items():
        stores = _stores16(k["body"])
        if "verify_shards" in name:
            assert not stores and not re.search(r"_store_dwordx[234]", k["body"]), name
            assert re.search(r"^\s*(?:global|buffer|flat)_store_byte", k["body"], re.M), name
        assert _loads16(k["body"]), name
        if not _nt(name):
            continue
        missing = [i for i in _loads16(k["body"]) if not re.search(r"\bnt\b", i)]
        assert not missing, f"{name}: {missing[:3]}"
        nt = [i for i in stores if re.search(r"\bnt\b", i)]
        sc1 = [i for i in stores if re.search(r"\bsc1\b", i)]
        assert len(nt) + len(sc1) == len(stores), f"{name}: a result store without a policy"
        if "encode_shards" in name:
            assert nt and not sc1, name
        if "repair_shards" in name:  # the parity reduction and the data reduction, the same code
            assert nt and len(nt) == len(sc1), (name, len(nt), len(sc1))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nm", sorted(AUTO_OCCUPANCY))
def test_registers_admit_the_default_residency(kernels, kind, nm):
    hits = [k for n, k in kernels.items() if re.search(rf"{kind}_kernelILi{nm}ELi1ELb1ELi64ELj", n)]
    assert len(hits) == 2  # the two capacities
    for k in hits:
        vgpr_alloc = -(-k["vgpr"] // 8) * 8  # gfx950 allocates VGPRs in blocks of 8
        assert 512 // vgpr_alloc >= AUTO_OCCUPANCY[nm], k["vgpr"]


def test_32_member_encode_issues_every_load_before_the_first_wait(kernels):
    hits = {n: k for n, k in kernels.items()
            if re.search(r"encode_shards_kernelILi32ELi1ELb1ELi64ELj", n)}
    assert len(hits) == 2
    for name, k in hits.items():
        body = k["body"]
        first_load = body.index("global_load_dwordx4")
        first_wait = body.index("s_waitcnt vmcnt", first_load)
        assert body[first_load:first_wait].count("global_load_dwordx4") == 32, name
