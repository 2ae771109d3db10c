"""The gfx950 listing of the kernels (`make asm`), compiled and parsed once per
process for every tests/test_isa*.py module (CPU only: hipcc cross-compiles,
and an up-to-date listing is not rebuilt).

listing() maps every kernel symbol to {"body": its text from the label to
s_endpgm, "vgpr": .vgpr_count, "sgpr": .sgpr_count}; kernels(kinds) is the
part of it a module looks at.
"""
from __future__ import annotations

import functools
import re
import subprocess

from conftest import PKG_DIR

ASM = PKG_DIR / "build" / "xec_kernels-gfx950.s"


@functools.lru_cache(maxsize=None)
def listing() -> dict[str, dict]:
    subprocess.run(["make", "-C", str(PKG_DIR), "asm"], check=True, capture_output=True)
    text = ASM.read_text()
    out = {}
    for m in re.finditer(r"^(_ZN3xec\w+):.*?^\s*s_endpgm", text, re.S | re.M):
        out[m.group(1)] = {"body": m.group(0)}
    meta = re.findall(r"\.name:\s+(\S+)\n(.*?)\.vgpr_count:\s+(\d+)", text, re.S)
    for name, block, vgpr in meta:
        if name in out:
            out[name]["vgpr"] = int(vgpr)
            out[name]["sgpr"] = int(re.search(r"\.sgpr_count:\s+(\d+)", block).group(1))
    return out


def kernels(kinds: str) -> dict[str, dict]:
    """The instantiations of `<kind>_kernel`, `kinds` a regex alternation of kinds."""
    name = re.compile(rf"_ZN3xec[12][0-9](?:{kinds})_kernel\w+")
    return {n: k for n, k in listing().items() if name.fullmatch(n)}


def nt(name: str) -> bool:
    # the NT template argument of <NM, U, NT, T> or <U, NT, T>: ...ILi1ELb1ELi64E...
    return re.search(r"ELb1E", name) is not None


def loads16(body):
    return re.findall(r"^\s*((?:global|buffer)_load_dwordx4[^\n]*)", body, re.M)


def stores16(body):
    return re.findall(r"^\s*((?:global|buffer|flat|scratch)_store_dwordx4[^\n]*)", body, re.M)


def atomic_adds(body):
    return re.findall(r"^\s*((?:global|flat|buffer)_atomic_add\w*[^\n]*)", body, re.M)
