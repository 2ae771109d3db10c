#!/usr/bin/env python3
"""The degraded read against its partners, in one process on one MI355X.

As tools/digest_bench.py (Shape, time limits and interleaving are
tools/repair_scrub_bench.py's): kernel times come from each call's own dispatch
(xec_set_kernel_events), the operations of a comparison are interleaved round
by round, every figure is the median of a round's launches, and a comparison
reports each operation's per-round medians, the ratio of the overall medians
and the partner's own spread in this process.  A difference inside that spread
is not a difference.

  A  whole lost blocks, one per stripe (block 7c mod k of stripe c), at configs
     2, 3 and 4: xec_read of those blocks against xec_decode's work-list kernel
     (xec_set_decode_tiling(3)) on the same loss set.  Both read k/m blocks and
     write one per lost block; the read writes to d_out, the decode in place;
  B  the same items with no bitmap -- a gather of present whole blocks --
     against ONE device-to-device hipMemcpyAsync (a torch copy_) of the same
     total bytes.  A copy has no kernel dispatch of the library's to time, so
     both sides are also bracketed by two event records on the stream
     ("bracketed_median_us": packet gaps included, on both sides alike);
  C  the point of the feature, at config 3's shape with 1,024 stripes: 1,024
     items of 4 KiB at offset 512 KiB from 1,024 lost 1 MiB blocks against
     xec_repair of the same blocks, with the bytes each moves;
  D  (--sweep) A's read and B's gather under residency caps 1, 2, 4, 8 against
     the shipped choice (0).
The store policy of d_out is a constant of the kernel source
(XEC_READ_STORE_AUX, csrc/xec_kernels.hip): to compare, run the tool once per
library with XEC_LIB naming a library built with -DXEC_READ_STORE_AUX=0, 2 or
16, one after the other, and compare the runs' read times.

Every GPU step runs under a time limit of its own (--step-timeout).  After the
timed launches of a shape what the read delivered is compared with the blocks
themselves (nothing is erased here: "lost" is only what the bitmap says, so a
reconstruction must equal the block it stands for), and the batch is scrubbed.

    python tools/read_bench.py [--rounds 3] [--iters 20] [--sweep] [--only A,B,C] [--out f.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from repair_scrub_bench import CONFIGS, Shape, step  # noqa: E402

POINT = (16, 1, 1 << 20, 1024)  # part C: config 3's stripe, 1,024 of them
POINT_RANGE = (512 << 10, 4 << 10)


class ReadShape(Shape):
    def __init__(self, *a, offset=0, length=None):
        super().__init__(*a)
        import numpy as np
        torch, S, k, m, bs = self.torch, self.S, self.k, self.m, self.bs
        self.offset, self.length = offset, bs if length is None else length
        c = np.arange(S)
        self.lost_i = (7 * c) % k
        self.items = ((c << 8) | self.lost_i).astype(np.uint32)
        self.bm = self.bitmap(lambda b: b.__setitem__((c, self.lost_i), 0))
        self.n = S
        self.out = torch.empty(self.n * self.length, dtype=torch.uint8, device="cuda")
        self.copy_src = torch.empty_like(self.out)
        sb = self.xec.read_scratch_bytes(self.n)
        self.scratch = torch.empty(max(sb, 4), dtype=torch.uint8, device="cuda")
        self.scratch_bytes = sb
        torch.cuda.synchronize()

    def call(self, op, bm=None):
        x, a = self.xec, (self.S, self.bs, self.k, self.m)
        if op in ("read", "gather"):
            return x.read(self.d, self.p, *a, self.bm["h"] if op == "read" else None, self.items,
                          self.n, self.offset, self.length, self.out, self.scratch,
                          self.scratch_bytes, self.s)
        if op == "decode_list":
            x.set_decode_tiling(3)
            try:
                st = x.decode(self.d, self.p, *a, self.bm["h"], self.bm["scratch"], self.s)
                assert st != 0 or x.decode_tiling_used() in (3, 4), x.decode_tiling_used()
                return st
            finally:
                x.set_decode_tiling(0)
        if op == "repair":
            return x.repair(self.d, self.p, *a, self.bm["h"], self.bm["scratch"], self.s)
        if op == "memcpy":
            self.out.copy_(self.copy_src, non_blocking=True)
            return 0
        return super().call(op, bm)

    def bracketed(self, op, iters):
        us = []
        for i in range(iters + 3):
            self.ev[0].record(self.s)
            assert self.call(op) == 0, op
            self.ev[1].record(self.s)
            self.s.synchronize()
            if i >= 3:
                us.append(self.ev[0].elapsed_time(self.ev[1]) * 1e3)
        return statistics.median(us)

    def delivered_is_right(self):
        torch = self.torch
        rows = torch.arange(self.S, device="cuda")
        cols = torch.from_numpy(self.lost_i).to("cuda")
        want = self.d.view(self.S, self.k, self.bs)[rows, cols,
                                                     self.offset:self.offset + self.length]
        for op in ("read", "gather"):
            self.out.fill_(0x5C)
            assert self.call(op) == 0
            torch.cuda.synchronize()
            if not torch.equal(self.out.view(self.n, self.length), want):
                return False
        return self.scrub_is_clean()


def spread(v):
    return round(100 * (max(v) - min(v)) / statistics.median(v), 2)


def ops_row(per):
    return {op: {"round_medians_us": [round(x, 2) for x in v],
                 "median_us": round(statistics.median(v), 2), "spread_pct": spread(v)}
            for op, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sweep", action="store_true", help="residency caps of read and gather")
    ap.add_argument("--only", default="", help="comma list of A,B,C,D (default: A,B,C, and D with --sweep)")
    ap.add_argument("--step-timeout", type=float, default=60.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.rounds >= 3, "at least three interleaved rounds"
    import torch

    import xec
    torch.cuda.set_device(0)
    assert xec.init(0) == 0
    lim = args.step_timeout
    parts = set(args.only.split(",")) if args.only else {"A", "B", "C"} | ({"D"} if args.sweep else set())
    out = {"build_info": xec.build_info(), "lib": Path(xec.LIB_PATH).name, "rounds": args.rounds,
           "iters": args.iters, "rows": []}
    print(json.dumps({"build_info": out["build_info"]}), flush=True)

    def emit(row):
        print(json.dumps(row), flush=True)
        out["rows"].append(row)

    def rounds_of(sh, ops, label, timer="time_round"):
        per = {op: [] for op in ops}
        for r in range(args.rounds):
            for op in ops:
                with step(lim, f"{label} round {r} {op}"):
                    per[op].append(sh.time_round(op, None, args.iters) if timer == "time_round"
                                   else sh.bracketed(op, args.iters))
        return per

    for name, (k, m, bs, S) in (CONFIGS.items() if parts & {"A", "B", "D"} else ()):
        sh = ReadShape(xec, torch, k, m, bs, S, lim)
        moved = S * bs * (k // m + 1)
        if "A" in parts:
            per = rounds_of(sh, ("decode_list", "read"), f"A {name}")
            med = {op: statistics.median(v) for op, v in per.items()}
            emit({"comparison": f"A {name} whole lost blocks, one per stripe: read against the "
                                "list decode", "shape": [k, m, bs, S], "items": sh.n,
                  "bytes_moved_each": moved, "read_tiling": xec.read_tiling_used(),
                  "read_over_decode": round(med["read"] / med["decode_list"], 4),
                  "GBps_read": round(moved / med["read"] / 1e3, 1), "ops": ops_row(per)})
        if "B" in parts:
            per = rounds_of(sh, ("gather",), f"B {name} kernel")
            brk = rounds_of(sh, ("memcpy", "gather"), f"B {name} bracketed", timer="bracketed")
            mb = {op: statistics.median(v) for op, v in brk.items()}
            emit({"comparison": f"B {name} gather of present whole blocks against one D2D "
                                "hipMemcpyAsync", "shape": [k, m, bs, S], "items": sh.n,
                  "bytes_copied": S * bs,
                  "bracketed_gather_over_memcpy": round(mb["gather"] / mb["memcpy"], 4),
                  "gather_kernel": ops_row(per)["gather"], "bracketed": ops_row(brk)})
        if "D" in parts:
            per = {}
            for r in range(args.rounds):
                for w in (0, 1, 2, 4, 8):
                    assert xec.set_occupancy(w) == 0
                    try:
                        for op in ("read", "gather"):
                            with step(lim, f"D {name} round {r} cap {w} {op}"):
                                per.setdefault(f"{op}_cap{w}", []).append(
                                    sh.time_round(op, None, args.iters))
                    finally:
                        xec.set_occupancy(0)
            emit({"comparison": f"D {name} residency caps (0 = the shipped choice)",
                  "shape": [k, m, bs, S], "us": ops_row(per)})
        with step(lim, f"{name} delivered bytes + scrub"):
            assert sh.delivered_is_right(), name
        del sh
        torch.cuda.empty_cache()

    if "C" in parts:
        k, m, bs, S = POINT
        off, ln = POINT_RANGE
        sh = ReadShape(xec, torch, k, m, bs, S, lim, offset=off, length=ln)
        per = rounds_of(sh, ("repair", "read"), "C")
        med = {op: statistics.median(v) for op, v in per.items()}
        emit({"comparison": "C 1,024 items of 4 KiB from lost 1 MiB blocks against xec_repair of "
                            "the same blocks", "shape": [k, m, bs, S], "items": sh.n,
              "range": [off, ln], "read_tiling": xec.read_tiling_used(),
              "bytes_moved": {"read": sh.n * ln * (k // m + 1), "repair": sh.n * bs * (k // m + 1)},
              "repair_over_read": round(med["repair"] / med["read"], 2), "ops": ops_row(per)})
        with step(lim, "C delivered bytes + scrub"):
            assert sh.delivered_is_right()
        del sh
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
