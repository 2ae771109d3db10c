"""ISA-level invariants of the kernels xec_update and xec_update_device run
(CPU only: hipcc cross-compiles; the listing is `make asm`'s, as
tests/test_isa.py and tests/test_isa_repair.py read it).

Whole-block update is the ranged update over [0, bs) without digests, so its
kernels are the DIG=false instantiations of patch_list / patch_arglist /
patch_class (<U, NT, T, DIG>); the update_* kernels it had before are gone.

* every 16-byte load of a non-temporal (NT=true) instantiation carries `nt`;
* every 16-byte store of an NT=true instantiation carries exactly one explicit
  policy, `nt` or `sc1`: the new data block and the parity block are both
  stored in place through st16_block, never by a plain store.  The NT=false
  instantiations (xec_set_launch cache_policy 2) store plainly by design, as
  tests/test_isa_repair.py has it, and are only checked to hold stores;
* every instantiation holds loads and stores (it reads old, new and parity and
  writes data and parity) and, being DIG=false, no atomic add;
* the kernels take no member-count parameter, so there are <U, NT, T> = 8 of
  the class kernel, 8 of the list kernel and 8 x 3 capacities of the
  argument-list kernel with DIG=false, and no update_* kernel beside them.
"""
from __future__ import annotations

import re

import pytest

import isa_listing
from isa_listing import atomic_adds as _atomic_adds, loads16 as _loads16, stores16 as _stores16

KINDS = {"patch_list": 8, "patch_arglist": 24, "patch_class": 8}
TARGS = r"_kernelILi([12])ELb([01])ELi(64|256)ELb0E"  # <U, NT, T, DIG=false>


def _nt(name: str) -> bool:
    return re.search(TARGS, name).group(2) == "1"


@pytest.fixture(scope="module")
def kernels() -> dict[str, dict]:
    out = {n: k for n, k in isa_listing.kernels("|".join(KINDS)).items() if re.search(TARGS, n)}
    # 2 unrolls x 2 policies x 2 workgroup sizes, arglist x 3 capacities; no member count
    assert len(out) == sum(KINDS.values()), f"{len(out)} update instantiations in the ISA"
    return out


def test_instantiation_count_is_the_template_set(kernels):
    for kind, want in KINDS.items():
        hits = [n for n in kernels if re.search(rf"\d\d{kind}_kernelI", n)]
        assert len(hits) == want, (kind, len(hits))
        assert sum(_nt(n) for n in hits) == want // 2, kind
        # <U, NT, T, DIG>: the first template argument is the unroll, 1 or 2 -- no NM ahead of it
        combos = [re.search(TARGS, n).groups() for n in hits]
        for u in "12":
            for nt in "01":
                for t in ("64", "256"):
                    assert combos.count((u, nt, t)) == want // 8, (kind, u, nt, t)
    # the whole-block family of its own is gone: one set of kernels serves both calls
    assert not isa_listing.kernels("update_list|update_arglist|update_class")


def test_nt_instantiations_load_nt(kernels):
    for name, k in kernels.items():
        loads = _loads16(k["body"])
        assert loads, name
        assert not _atomic_adds(k["body"]), name  # no digest upkeep on this path
        if not _nt(name):
            continue
        missing = [i for i in loads if not re.search(r"\bnt\b", i)]
        assert not missing, f"{name}: {missing[:3]}"


def test_stores_carry_exactly_one_explicit_policy(kernels):
    for name, k in kernels.items():
        stores = _stores16(k["body"])
        assert stores, name
        if not _nt(name):
            continue
        both = [i for i in stores if re.search(r"\bnt\b", i) and re.search(r"\bsc1\b", i)]
        plain = [i for i in stores if not re.search(r"\b(nt|sc1)\b", i)]
        assert not both and not plain, f"{name}: {(both + plain)[:3]}"
        # st16_block's buffer store, never a global or flat one
        assert all(i.startswith("buffer_store_dwordx4") for i in stores), name
