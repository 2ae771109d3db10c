"""ISA-level invariants of the degraded-write kernels (CPU only: hipcc
cross-compiles; the listing is `make asm`'s, as tests/test_isa_update_range.py reads
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
import subprocess

import pytest

from conftest import PKG_DIR

ASM = PKG_DIR / "build" / "xec_kernels-gfx950.s"
KINDS = {"write_list": 16, "write_arglist": 48, "write_class": 16}


@pytest.fixture(scope="module")
def kernels() -> dict[str, str]:
    subprocess.run(["make", "-C", str(PKG_DIR), "asm"], check=True, capture_output=True)
    text = ASM.read_text()
    out = {}
    for m in re.finditer(r"^(_ZN3xec[12][0-9](?:write_list|write_arglist|write_class)"
                         r"_kernel\w+):.*?^\s*s_endpgm", text, re.S | re.M):
        out[m.group(1)] = m.group(0)
    assert len(out) == sum(KINDS.values()), f"{len(out)} degraded-write instantiations in the ISA"
    return out


def _targs(name: str):
    """(U, NT, T, DIG) of ...kernelILi1ELb1ELi64ELb0E..."""
    m = re.search(r"_kernelILi([12])ELb([01])ELi(64|256)ELb([01])E", name)
    assert m, name
    return int(m.group(1)), m.group(2) == "1", int(m.group(3)), m.group(4) == "1"


def _loads16(body):
    return re.findall(r"^\s*((?:global|buffer)_load_dwordx4[^\n]*)", body, re.M)


def _stores16(body):
    return re.findall(r"^\s*((?:global|buffer|flat|scratch)_store_dwordx4[^\n]*)", body, re.M)


def _atomic_adds(body):
    return re.findall(r"^\s*((?:global|flat|buffer)_atomic_add\w*[^\n]*)", body, re.M)


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
