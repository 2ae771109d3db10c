"""ISA-level invariants of the vectored-read kernels (CPU only: hipcc
cross-compiles; the listing is `make asm`'s, through tests/isa_listing.py).

For the instantiations the default launch runs -- NT, one wave per workgroup,
one granule per lane -- of readv_list_kernel, readv_arglist_kernel (both
capacities) and readv_dev_kernel at 4, 8, 16 and 32 members per class:

* every 16-byte load carries `nt`;
* every 16-byte store carries `sc1` (kReadStoreAux) and not `nt`;
* the kernel uses no scratch memory;
* its VGPRs, in gfx950's allocation blocks of 8, admit the residency the launch
  asks for (auto_occupancy in csrc/xec_api.cpp, through read_occupancy).
Only cache-policy bits and register counts are looked at.
"""
from __future__ import annotations

import functools
import re

import pytest

import isa_listing
from isa_listing import loads16, stores16

# member count -> resident waves per SIMD (auto_occupancy, csrc/xec_api.cpp)
AUTO_OCCUPANCY = {4: 4, 8: 4, 16: 2, 32: 1}
KINDS = {"readv_list": 1, "readv_arglist": 2, "readv_dev": 1}  # instantiations per shape


@functools.lru_cache(maxsize=None)
def _asm_text() -> str:
    isa_listing.listing()  # `make asm`
    return isa_listing.ASM.read_text()


def _scratch_bytes(name: str) -> int:
    """.private_segment_fixed_size of the kernel's metadata (it follows .name)."""
    m = re.search(rf"\.name:\s+{name}\n\s+\.private_segment_fixed_size:\s+(\d+)", _asm_text())
    assert m, name
    return int(m.group(1))


@pytest.fixture(scope="module")
def by_nm() -> dict[int, dict[str, dict]]:
    every = isa_listing.kernels("|".join(KINDS))
    out = {}
    for nm in AUTO_OCCUPANCY:
        hits = {n: k for n, k in every.items()
                if re.search(rf"_kernelILi{nm}ELi1ELb1ELi64E", n)}
        for kind, want in KINDS.items():
            got = [n for n in hits if re.search(rf"\d\d{kind}_kernelI", n)]
            assert len(got) == want, (nm, kind, got)
        out[nm] = hits
    return out


@pytest.mark.parametrize("nm", list(AUTO_OCCUPANCY))
def test_loads_are_nt_and_stores_sc1(by_nm, nm):
    for name, k in by_nm[nm].items():
        loads, stores = loads16(k["body"]), stores16(k["body"])
        assert loads and stores, name
        missing = [i for i in loads if not re.search(r"\bnt\b", i)]
        assert not missing, f"{name}: {missing[:3]}"
        wrong = [i for i in stores if not re.search(r"\bsc1\b", i) or re.search(r"\bnt\b", i)]
        assert not wrong, f"{name}: {wrong[:3]}"


@pytest.mark.parametrize("nm", list(AUTO_OCCUPANCY))
def test_no_scratch_and_registers_admit_the_residency(by_nm, nm):
    for name, k in by_nm[nm].items():
        assert _scratch_bytes(name) == 0, name
        vgpr_alloc = -(-k["vgpr"] // 8) * 8  # gfx950 allocates VGPRs in blocks of 8
        assert 512 // vgpr_alloc >= AUTO_OCCUPANCY[nm], (name, k["vgpr"])
