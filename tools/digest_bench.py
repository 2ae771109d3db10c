#!/usr/bin/env python3
"""Block digests and the heal chain against their partners, in one process on
one MI355X, at configs 2, 3 and 4.

As tools/update_bench.py (Shape, time limits and interleaving are
tools/repair_scrub_bench.py's): kernel times come from each call's own dispatch
(xec_set_kernel_events), the operations of a comparison are interleaved round
by round, every figure is the median of a round's launches, and a comparison
reports each operation's per-round medians, the ratio of the overall medians
and the partner's own spread in this process.  A difference inside that spread
is not a difference.

  A  a full xec_digest against xec_verify on the same batch: both read the same
     (k+m)*bs*S bytes once and store next to nothing, so the ratio says what
     the two 64-bit multiplies per word cost;
  B  one block corrupted in 1 stripe in 9, then xec_verify + xec_locate(flags)
     + xec_repair_device, against a full xec_locate.  The chain's kernel time
     is the sum of the three calls' codec kernels (verify, digest, repair),
     each from its own dispatch; "bracketed_median_us" is the whole chain, or
     the whole full locate, between two hipEventRecord packets on the stream,
     small kernels, memsets and packet gaps included.  The blocks are
     corrupted again before every chain (outside the timed interval), and
     after each chain the verdict must be 0 and locate's count the number of
     corrupted blocks;
  D  (--sweep) A's digest under residency caps 1, 2, 4, 8 and none, with nt
     and with default loads; then digest and locate(flags) under xec_set_launch's
     max_grid (GRIDS below; 0 = the library's default).  The segment size is a constant of the kernel
     source (kDigestSegmentBytes, csrc/xec_kernels.h): to compare another
     value, run part A once more with XEC_LIB naming a library built with it
     and compare the two runs' ratios to verify;
  P  (--only P) nothing timed: five xec_digest and five xec_verify launches per
     config, for a counter run of its own --
         rocprofv3 --pmc <counters> -- python tools/digest_bench.py --only P

Every GPU step runs under a time limit of its own (--step-timeout).  After the
timed launches of a shape the batch is scrubbed (xec_verify's count must be 0)
and a full xec_locate against the digests taken at the start must count 0.

    python tools/digest_bench.py [--rounds 3] [--iters 20] [--sweep] [--only A,B] [--out f.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from repair_scrub_bench import CONFIGS, Shape, step  # noqa: E402


class DigestShape(Shape):
    def __init__(self, *a):
        super().__init__(*a)
        torch, n = self.torch, self.S * (self.k + self.m)
        self.dig = torch.empty(8 * n, dtype=torch.uint8, device="cuda")
        self.work = torch.empty(8 * n, dtype=torch.uint8, device="cuda")
        self.timed_dig = torch.empty(8 * n, dtype=torch.uint8, device="cuda")
        self.bitmap = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.lcount = torch.zeros(1, dtype=torch.int32, device="cuda")
        # the stored digests, of the intact batch; the timed xec_digest writes elsewhere
        assert self.xec.digest(self.d, self.p, self.S, self.bs, self.k, self.m, self.dig, None,
                               self.s) == 0
        # 1 stripe in 9: byte 0 of data block (7c) % k
        st = torch.arange(4, self.S, 9, device="cuda")
        self.hit = (st, (7 * st) % self.k)
        self.n_hit = int(st.numel())
        torch.cuda.synchronize()

    def corrupt(self):
        d = self.d.view(self.S, self.k, self.bs)
        d[self.hit[0], self.hit[1], 0] ^= 1

    def call(self, op, bm=None):
        x, a = self.xec, (self.S, self.bs, self.k, self.m)
        if op == "digest":
            return x.digest(self.d, self.p, *a, self.timed_dig, None, self.s)
        if op in ("locate_full", "locate_flags"):
            return x.locate(self.d, self.p, *a, self.dig,
                            self.flags if op == "locate_flags" else None, self.bitmap,
                            self.lcount, self.work, 8 * self.S * (self.k + self.m), self.s)
        if op == "repair_located":
            return x.repair_device(self.d, self.p, *a, self.bitmap, self.status, self.s)
        return super().call(op, bm)

    CHAIN = ("verify", "locate_flags", "repair_located")

    def chain_round(self, iters):
        """Median over `iters` chains (after 3 warm-up ones) of the summed kernel
        times of the three calls (us), and the medians of each."""
        rows = []
        for i in range(iters + 3):
            self.corrupt()
            self.s.synchronize()
            t = []
            for op in self.CHAIN:
                self.xec.set_kernel_events(self.ev[0], self.ev[1])
                assert self.call(op) == 0, op
                self.s.synchronize()
                t.append(self.ev[0].elapsed_time(self.ev[1]) * 1e3)
            assert int(self.status.item()) == 0 and int(self.lcount.item()) == self.n_hit
            assert int(self.count.item()) == self.n_hit
            if i >= 3:
                rows.append(t)
        parts = [statistics.median(r[q] for r in rows) for q in range(3)]
        return statistics.median(sum(r) for r in rows), parts

    def bracketed(self, ops, iters, before=None):
        us = []
        for _ in range(iters):
            if before:
                before()
            self.ev[0].record(self.s)
            for op in ops:
                assert self.call(op) == 0, op
            self.ev[1].record(self.s)
            self.s.synchronize()
            us.append(self.ev[0].elapsed_time(self.ev[1]) * 1e3)
        return statistics.median(us)

    def all_clean(self):
        assert self.call("locate_full") == 0
        self.torch.cuda.synchronize()
        return self.scrub_is_clean() and int(self.lcount.item()) == 0


GRIDS = (0, 2048, 4096, 8192, 16384, 32768, 131072)  # 0 = the library's default


def spread(v):
    return round(100 * (max(v) - min(v)) / statistics.median(v), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sweep", action="store_true", help="digest residency caps x load policy")
    ap.add_argument("--only", default="", help="comma list of A,B,D,P (default: A,B, and D with --sweep)")
    ap.add_argument("--step-timeout", type=float, default=60.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.rounds >= 3, "at least three interleaved rounds"
    import torch

    import xec
    torch.cuda.set_device(0)
    assert xec.init(0) == 0
    lim = args.step_timeout
    parts = set(args.only.split(",")) if args.only else {"A", "B"} | ({"D"} if args.sweep else set())
    out = {"build_info": xec.build_info(), "rounds": args.rounds, "iters": args.iters, "rows": []}
    print(json.dumps({"build_info": out["build_info"]}), flush=True)

    for name, (k, m, bs, S) in CONFIGS.items():
        sh = DigestShape(xec, torch, k, m, bs, S, lim)
        if "P" in parts:
            with step(lim, f"P {name}"):
                for op in ("digest", "verify"):
                    for _ in range(5):
                        assert sh.call(op) == 0
                torch.cuda.synchronize()
        if "A" in parts:
            per = {"verify": [], "digest": []}
            for r in range(args.rounds):
                for op in per:
                    with step(lim, f"A {name} round {r} {op}"):
                        per[op].append(sh.time_round(op, None, args.iters))
            med = {op: statistics.median(v) for op, v in per.items()}
            row = {"comparison": f"A {name} full digest against verify", "shape": [k, m, bs, S],
                   "bytes": sh.bytes, "digest_over_verify": round(med["digest"] / med["verify"], 4),
                   "ops": {op: {"round_medians_us": [round(v, 2) for v in per[op]],
                                "median_us": round(med[op], 2), "spread_pct": spread(per[op]),
                                "GBps_of_batch": round(sh.bytes / med[op] / 1e3, 1)} for op in per}}
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
        if "B" in parts:
            chain, full, pieces = [], [], []
            for r in range(args.rounds):
                with step(lim, f"B {name} round {r} chain"):
                    t, p3 = sh.chain_round(args.iters)
                    chain.append(t)
                    pieces.append(p3)
                with step(lim, f"B {name} round {r} full locate"):
                    full.append(sh.time_round("locate_full", None, args.iters))
            with step(lim, f"B {name} bracketed"):
                b_chain = sh.bracketed(sh.CHAIN, args.iters, sh.corrupt)
                b_full = sh.bracketed(("locate_full",), args.iters)
            mc, mf = statistics.median(chain), statistics.median(full)
            row = {"comparison": f"B {name} heal chain at 1 damaged stripe in 9 against a full locate",
                   "shape": [k, m, bs, S], "damaged_blocks": sh.n_hit,
                   "chain_over_full_locate": round(mc / mf, 4),
                   "bracketed_chain_over_full_locate": round(b_chain / b_full, 4),
                   "chain": {"round_medians_us": [round(v, 2) for v in chain],
                             "median_us": round(mc, 2), "bracketed_median_us": round(b_chain, 2),
                             "verify_locate_repair_us": [round(statistics.median(p[q] for p in pieces), 2)
                                                         for q in range(3)]},
                   "full_locate": {"round_medians_us": [round(v, 2) for v in full],
                                   "median_us": round(mf, 2), "spread_pct": spread(full),
                                   "bracketed_median_us": round(b_full, 2)}}
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
        if "D" in parts:
            per = {}
            for r in range(args.rounds):
                for policy in (1, 2):  # nt, default
                    for w in (0, 1, 2, 4, 8):
                        assert xec.set_occupancy(w) == 0 and xec.set_launch(0, 0, policy, 0) == 0
                        try:
                            with step(lim, f"D {name} round {r} policy {policy} cap {w}"):
                                per.setdefault(f"{'nt' if policy == 1 else 'default'}_cap{w}",
                                               []).append(sh.time_round("digest", None, args.iters))
                        finally:
                            xec.set_occupancy(0)
                            xec.set_launch(0, 0, 0, 0)
                with step(lim, f"D {name} round {r} verify"):
                    per.setdefault("verify", []).append(sh.time_round("verify", None, args.iters))
            # the grid: one workgroup per tile (0) against grid-stride walks of capped grids,
            # for a full digest and for a locate over the flags of 1 damaged stripe in 9
            with step(lim, f"D {name} damage + verify"):
                sh.corrupt()
                assert sh.call("verify") == 0
            for r in range(args.rounds):
                for grid in GRIDS:
                    assert xec.set_launch(0, grid, 0, 0) == 0
                    try:
                        with step(lim, f"D {name} round {r} grid {grid}"):
                            for op in ("digest", "locate_flags"):
                                per.setdefault(f"{op}_grid{grid}", []).append(
                                    sh.time_round(op, None, args.iters))
                    finally:
                        xec.set_launch(0, 0, 0, 0)
            with step(lim, f"D {name} heal"):
                assert sh.call("repair_located") == 0
            row = {"comparison": f"D {name} digest caps x load policy", "shape": [k, m, bs, S],
                   "us": {key: {"round_medians_us": [round(x, 2) for x in v],
                                "median_us": round(statistics.median(v), 2)}
                          for key, v in per.items()},
                   "verify_spread_pct": spread(per["verify"])}
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
        with step(lim, f"{name} scrub + full locate"):
            assert sh.all_clean(), name
        del sh
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
