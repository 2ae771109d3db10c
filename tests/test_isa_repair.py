"""ISA-level invariants of the repair and verify kernels (CPU only: hipcc
cross-compiles; the listing is `make asm`'s, as tests/test_isa.py reads it).

* every 16-byte load of a non-temporal (NT=true) instantiation carries `nt`;
* the repair kernels' 16-byte result stores carry the policy of their target:
  `nt` for a parity block (encode's), `sc1` for a data block (decode's) -- each
  store exactly one of the two, and both kinds present in every kernel, which
  holds both reductions;
* verify_kernel stores no 16 bytes anywhere: its only store is the flag byte;
* the 16- and 32-member default-shape instances fit the registers of the
  residency their launch asks for (auto_occupancy, csrc/xec_api.cpp).
"""
from __future__ import annotations

import re

import pytest

import isa_listing
from isa_listing import loads16 as _loads16, nt as _nt, stores16 as _stores16

KINDS = ["repair_list", "repair_arglist", "repair_class", "verify"]


@pytest.fixture(scope="module")
def kernels() -> dict[str, dict]:
    out = isa_listing.kernels("|".join(KINDS))
    # 7 member counts x 2 unrolls x 2 policies x 2 workgroup sizes, arglist x 3 capacities
    assert len(out) == 56 * 6, f"{len(out)} repair / verify instantiations in the ISA"
    return out


def test_nt_instantiations_load_nt(kernels):
    for name, k in kernels.items():
        if not _nt(name):
            continue
        loads = _loads16(k["body"])
        assert loads, name
        missing = [i for i in loads if not re.search(r"\bnt\b", i)]
        assert not missing, f"{name}: {missing[:3]}"


def test_repair_stores_carry_their_targets_policy(kernels):
    for name, k in kernels.items():
        if "repair_" not in name or not _nt(name):
            continue
        stores = _stores16(k["body"])
        nt = [i for i in stores if re.search(r"\bnt\b", i)]
        sc1 = [i for i in stores if re.search(r"\bsc1\b", i)]
        assert nt and sc1, name  # the parity reduction and the data reduction
        both = [i for i in stores if re.search(r"\bnt\b", i) and re.search(r"\bsc1\b", i)]
        plain = [i for i in stores if not re.search(r"\b(nt|sc1)\b", i)]
        assert not both and not plain, f"{name}: {(both + plain)[:3]}"
        # the two reductions are the same code with another target: as many stores each
        assert len(nt) == len(sc1), (name, len(nt), len(sc1))


def test_verify_has_no_16_byte_store(kernels):
    hits = {n: k for n, k in kernels.items() if "verify_kernel" in n}
    assert len(hits) == 56
    for name, k in hits.items():
        assert not _stores16(k["body"]), name
        assert not re.search(r"_store_dwordx[234]", k["body"]), name
        assert re.search(r"^\s*(?:global|buffer|flat)_store_byte", k["body"], re.M), name
        assert _loads16(k["body"]), name


# member count -> resident waves per SIMD the launch asks for by default
AUTO_OCCUPANCY = {16: 2, 32: 1}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nm", sorted(AUTO_OCCUPANCY))
def test_registers_admit_the_default_residency(kernels, kind, nm):
    hits = [k for n, k in kernels.items()
            if re.search(rf"{kind}_kernelILi{nm}ELi1ELb1ELi64E", n)]
    assert len(hits) == (3 if kind == "repair_arglist" else 1)
    for k in hits:
        vgpr_alloc = -(-k["vgpr"] // 8) * 8  # gfx950 allocates VGPRs in blocks of 8
        assert 512 // vgpr_alloc >= AUTO_OCCUPANCY[nm], k["vgpr"]
        assert k["sgpr"] <= 96, k["sgpr"]
