#!/usr/bin/env python3
"""Are the kernels of two builds the same instructions?

    tools/isa_symbols.py dump LISTING > manifest.json
    tools/isa_symbols.py compare A B        (each a listing or a manifest)

LISTING is `make asm`'s build/xec_kernels-gfx950.s.  For every `_ZN3xec...`
kernel the manifest holds a hash of its body (label to s_endpgm) and of its
`.amdhsa_kernel` block (registers, LDS, kernarg size), in listing order.
`compare` lists the symbols only in A, only in B, and those whose body or
descriptor differ; it exits 1 if there are any.  Symbol order is reported and
does not count: it follows the order of instantiation in the source.

Before hashing, comments go and local labels lose their function number
(`.LBB<fn>_<n>` becomes `BB_<n>`): the number is the function's position in
the file, and the comments' padding follows the labels' width.  The tool only
hashes and compares; it looks for no particular instruction.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import re
import sys


def _normalise(text: str) -> str:
    lines = []
    for line in text.splitlines():
        line = re.sub(r"\.LBB\d+_(\d+)", r"BB_\1", line.split(";", 1)[0]).strip()
        if line:
            lines.append(" ".join(line.split()))
    return "\n".join(lines)


def _hash(text: str) -> str:
    return hashlib.sha256(_normalise(text).encode()).hexdigest()


def manifest(listing: str) -> dict[str, dict[str, str]]:
    bodies = {m.group(1): m.group(2) for m in re.finditer(
        r"^(_ZN3xec\w+):[^\n]*\n(.*?^\s*s_endpgm)", listing, re.S | re.M)}
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(_ZN3xec\w+)\n(.*?)^\s*\.end_amdhsa_kernel",
                         listing, re.S | re.M):
        name = m.group(1)
        if name not in bodies:
            raise SystemExit(f"{name}: a descriptor without a body")
        out[name] = {"body": _hash(bodies[name]), "descriptor": _hash(m.group(2))}
    if set(out) != set(bodies):
        raise SystemExit(f"bodies without a descriptor: {sorted(set(bodies) - set(out))[:3]}")
    return out


def load(path: str) -> dict[str, dict[str, str]]:
    text = open(path).read()
    return json.loads(text) if text.lstrip().startswith("{") else manifest(text)


def compare(a: dict, b: dict) -> int:
    only_a = [n for n in a if n not in b]
    only_b = [n for n in b if n not in a]
    both = [n for n in a if n in b]
    bodies = [n for n in both if a[n]["body"] != b[n]["body"]]
    descs = [n for n in both if a[n]["descriptor"] != b[n]["descriptor"]]
    print(f"symbols: {len(a)} in A, {len(b)} in B, {len(both)} in both")
    for title, names in (("only in A", only_a), ("only in B", only_b),
                         ("body differs", bodies), ("descriptor differs", descs)):
        print(f"{title}: {len(names)}")
        for n in names:
            print(f"  {n}")
    print("symbol order: " + ("same" if list(a) == list(b) else "differs"))
    return 1 if only_a or only_b or bodies or descs else 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("dump").add_argument("listing")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    if args.cmd == "dump":
        json.dump(manifest(open(args.listing).read()), sys.stdout, indent=0)
        print()
        return 0
    return compare(load(args.a), load(args.b))


if __name__ == "__main__":
    sys.exit(main())
