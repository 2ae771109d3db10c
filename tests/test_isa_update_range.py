"""ISA-level invariants of the ranged-update kernels, which xec_update and
xec_update_device run too, over [0, bs) with DIG=false (CPU only: hipcc
cross-compiles; the listing is `make asm`'s, as tests/test_isa_repair.py reads
it).

* the kernels are templated <U, NT, T, DIG>: 2 unrolls x 2 policies x 2
  workgroup sizes x with / without digest upkeep = 16 of the list kernel, 16 of
  the class kernel and 16 x 3 capacities of the argument-list kernel;
* every 16-byte load of a non-temporal (NT=true) instantiation carries `nt`;
* every 16-byte store of an NT=true instantiation is st16_block's buffer store
  with exactly one explicit policy, `nt` (parity) or `sc1` (data);
* DIG=false is the d_digests == NULL path and must cost nothing: its body holds
  no vector atomic add.  DIG=true holds a 64-bit one.
Nothing else about the instruction stream is looked at.
"""
from __future__ import annotations

import re

import pytest

import isa_listing
from isa_listing import atomic_adds as _atomic_adds, loads16 as _loads16, stores16 as _stores16

KINDS = {"patch_list": 16, "patch_arglist": 48, "patch_class": 16}


@pytest.fixture(scope="module")
def kernels() -> dict[str, str]:
    out = {n: k["body"] for n, k in isa_listing.kernels("|".join(KINDS)).items()}
    assert len(out) == sum(KINDS.values()), f"{len(out)} ranged-update instantiations in the ISA"
    return out


def _targs(name: str):
    """(U, NT, T, DIG) of ...kernelILi1ELb1ELi64ELb0E..."""
    m = re.search(r"_kernelILi([12])ELb([01])ELi(64|256)ELb([01])E", name)
    assert m, name
    return int(m.group(1)), m.group(2) == "1", int(m.group(3)), m.group(4) == "1"


def test_instantiation_count_is_the_template_set(kernels):
    for kind, want in KINDS.items():
        hits = [n for n in kernels if re.search(rf"\d\d{kind}_kernelI", n)]
        assert len(hits) == want, (kind, len(hits))
        per = want // 16
        combos = [_targs(n) for n in hits]
        for u in (1, 2):
            for nt in (False, True):
                for t in (64, 256):
                    for dig in (False, True):
                        assert combos.count((u, nt, t, dig)) == per, (kind, u, nt, t, dig)


def test_nt_instantiations_load_nt(kernels):
    for name, body in kernels.items():
        loads = _loads16(body)
        assert loads, name
        if not _targs(name)[1]:
            continue
        missing = [i for i in loads if not re.search(r"\bnt\b", i)]
        assert not missing, f"{name}: {missing[:3]}"


def test_nt_stores_are_buffer_stores_with_one_policy(kernels):
    for name, body in kernels.items():
        stores = _stores16(body)
        assert stores, name
        if not _targs(name)[1]:
            continue
        both = [i for i in stores if re.search(r"\bnt\b", i) and re.search(r"\bsc1\b", i)]
        plain = [i for i in stores if not re.search(r"\b(nt|sc1)\b", i)]
        assert not both and not plain, f"{name}: {(both + plain)[:3]}"
        assert all(i.startswith("buffer_store_dwordx4") for i in stores), name


def test_digest_upkeep_is_its_own_instantiation(kernels):
    for name, body in kernels.items():
        adds = _atomic_adds(body)
        if _targs(name)[3]:
            assert any(re.match(r"\w+_atomic_add_x2\b", i) for i in adds), f"{name}: {adds[:3]}"
        else:
            assert not adds, f"{name}: {adds[:3]}"
