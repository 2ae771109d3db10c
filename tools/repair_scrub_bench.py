#!/usr/bin/env python3
"""Repair and scrub against their partners, in one process on one MI355X.

Kernel times come from each call's own dispatch (xec_set_kernel_events); the
operations of a comparison are interleaved, round by round, and every figure
is the median of a round's launches.  A comparison reports each operation's
per-round medians, the ratio of the overall medians, and the partner's own
run-to-run spread in this process ((max - min) / median of its round medians):
a difference inside that spread is not a difference.

  A  xec_verify and xec_repair_device (the parity of every class lost) against
     xec_encode at configs 2, 3 and 4: the same (k+m)*bs*S bytes;
  B  xec_repair against xec_decode on the same bitmap, one data block lost per
     stripe at config 3 and two at 16+2 x 1 MiB x 256: the same reduction;
  C  xec_repair with the parity of 1 stripe in 9 lost at config 3 against the
     full xec_encode it replaces;
  D  (--sweep) xec_verify under residency caps 1, 2, 4, 8 and the shipped
     choice at configs 2, 3 and 4.

Every GPU step runs under a time limit of its own (--step-timeout): a step
that overruns ends the process with a traceback instead of queueing more work.
After the timed launches of a shape the batch is scrubbed: count must be 0.

    python tools/repair_scrub_bench.py [--rounds 3] [--iters 20] [--sweep] [--out f.json]
"""
from __future__ import annotations

import argparse
import faulthandler
import json
import statistics
import sys
from contextlib import contextmanager
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "erasure-code-benchmark_amd"))

CONFIGS = {"cfg2": (8, 1, 1 << 16, 1024), "cfg3": (16, 1, 1 << 20, 256),
           "cfg4": (32, 1, 4096, 65536)}  # k, m, bs, S (bench.py WORKLOADS)


@contextmanager
def step(seconds: float, what: str):
    """One GPU step under its own time limit."""
    print(f"# step: {what}", flush=True)
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


class Shape:
    def __init__(self, xec, torch, k, m, bs, S, limit):
        self.xec, self.torch = xec, torch
        self.k, self.m, self.bs, self.S = k, m, bs, S
        self.s = torch.cuda.current_stream()
        self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        with step(limit, f"fill + encode {k}+{m} x {bs} x {S}"):
            for e in self.ev:
                e.record(self.s)
            self.d = torch.empty(S * k * bs, dtype=torch.uint8, device="cuda")
            self.p = torch.empty(S * m * bs, dtype=torch.uint8, device="cuda")
            self.flags = torch.empty(S * m, dtype=torch.uint8, device="cuda")
            self.count = torch.zeros(1, dtype=torch.int32, device="cuda")
            self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
            assert xec.fill_splitmix64(self.d, S, k * bs, 1896, self.s) == 0
            assert xec.encode(self.d, self.p, S, bs, k, m, self.s) == 0
            torch.cuda.synchronize()
        self.bytes = (k + m) * bs * S

    def bitmap(self, rows):
        import numpy as np
        bm = np.ones((self.S, self.k + self.m), np.uint8)
        rows(bm)
        h = self.torch.from_numpy(bm.reshape(-1)).pin_memory()
        return {"h": h, "d": h.to("cuda"), "scratch": self.torch.empty(bm.size, dtype=self.torch.uint8,
                                                                        device="cuda"),
                "lost": int((bm == 0).sum())}

    def call(self, op, bm=None):
        x, a = self.xec, (self.S, self.bs, self.k, self.m)
        if op == "encode":
            return x.encode(self.d, self.p, *a, self.s)
        if op == "verify":
            return x.verify(self.d, self.p, *a, self.flags, self.count, self.s)
        if op == "repair_device":
            return x.repair_device(self.d, self.p, *a, bm["d"], self.status, self.s)
        if op == "repair":
            return x.repair(self.d, self.p, *a, bm["h"], bm["scratch"], self.s)
        if op == "decode":
            return x.decode(self.d, self.p, *a, bm["h"], bm["scratch"], self.s)
        raise ValueError(op)

    def time_round(self, op, bm, iters):
        """Median kernel time (us) of `iters` launches after 3 warm-up ones."""
        us = []
        for i in range(iters + 3):
            self.xec.set_kernel_events(self.ev[0], self.ev[1])
            assert self.call(op, bm) == 0, op
            self.s.synchronize()
            if i >= 3:
                us.append(self.ev[0].elapsed_time(self.ev[1]) * 1e3)
        return statistics.median(us)

    def scrub_is_clean(self):
        assert self.call("verify") == 0
        self.torch.cuda.synchronize()
        return int(self.count.item()) == 0 and int(self.status.item()) == 0


def compare(sh: Shape, ops, rounds, iters, limit, label):
    """ops: [(name, op, bitmap)], the first is the partner.  Interleaved rounds."""
    per = {name: [] for name, _, _ in ops}
    for r in range(rounds):
        for name, op, bm in ops:
            with step(limit, f"{label} round {r} {name}"):
                per[name].append(sh.time_round(op, bm, iters))
    with step(limit, f"{label} scrub"):
        clean = sh.scrub_is_clean()
    partner = ops[0][0]
    med = {n: statistics.median(v) for n, v in per.items()}
    row = {"comparison": label, "shape": [sh.k, sh.m, sh.bs, sh.S], "partner": partner,
           "partner_spread_pct": round(100 * (max(per[partner]) - min(per[partner])) / med[partner], 2),
           "scrub_clean_after": clean, "ops": {}}
    for name, _, bm in ops:
        row["ops"][name] = {"round_medians_us": [round(v, 2) for v in per[name]],
                            "median_us": round(med[name], 2),
                            "GBps_of_batch": round(sh.bytes / med[name] / 1e3, 1),
                            "time_over_partner": round(med[name] / med[partner], 4),
                            "lost_blocks": bm["lost"] if bm else None}
    print(json.dumps(row), flush=True)
    assert clean, label
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sweep", action="store_true", help="verify residency caps 1, 2, 4, 8")
    ap.add_argument("--only", default="", help="comma list of A,B,C,D (default: all asked for)")
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
    out = {"build_info": xec.build_info(), "rounds": args.rounds, "iters": args.iters, "rows": []}
    print(json.dumps({"build_info": out["build_info"]}), flush=True)

    def all_parity(bm):
        bm[:, -1] = 0  # m = 1 in configs 2-4: the parity of every class

    for name, (k, m, bs, S) in CONFIGS.items():
        if not parts & {"A", "D"} and not (name == "cfg3" and parts & {"B", "C"}):
            continue
        sh = Shape(xec, torch, k, m, bs, S, lim)
        if "A" in parts:
            bm = sh.bitmap(all_parity)
            out["rows"].append(compare(sh, [("encode", "encode", None), ("verify", "verify", None),
                                            ("repair_device", "repair_device", bm)],
                                       args.rounds, args.iters, lim, f"A {name}"))
        if "D" in parts:
            ops = [("encode", "encode", None)]
            per = {}
            for r in range(args.rounds):
                for w in (0, 1, 2, 4, 8):
                    assert xec.set_occupancy(w) == 0
                    try:
                        with step(lim, f"D {name} round {r} verify cap {w}"):
                            per.setdefault(w, []).append(sh.time_round("verify", None, args.iters))
                    finally:
                        xec.set_occupancy(0)
                with step(lim, f"D {name} round {r} encode"):
                    per.setdefault("encode", []).append(sh.time_round("encode", None, args.iters))
            row = {"comparison": f"D {name}", "shape": [k, m, bs, S], "members": k // m,
                   "verify_cap_us": {str(w): {"round_medians_us": [round(v, 2) for v in per[w]],
                                              "median_us": round(statistics.median(per[w]), 2)}
                                     for w in (0, 1, 2, 4, 8)},
                   "encode_us": {"round_medians_us": [round(v, 2) for v in per["encode"]],
                                 "median_us": round(statistics.median(per["encode"]), 2)}}
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
            del ops
        if name == "cfg3" and "B" in parts:
            def one_data(bm):
                for c in range(S):
                    bm[c, (7 * c) % k] = 0
            bm = sh.bitmap(one_data)
            out["rows"].append(compare(sh, [("decode", "decode", bm), ("repair", "repair", bm)],
                                       args.rounds, args.iters, lim, "B cfg3 one data block per stripe"))
        if name == "cfg3" and "C" in parts:
            def sparse_parity(bm):
                bm[4::9, -1] = 0
            bm = sh.bitmap(sparse_parity)
            row = compare(sh, [("encode", "encode", None), ("repair", "repair", bm)],
                          args.rounds, args.iters, lim, "C cfg3 parity of 1 stripe in 9")
            row["speedup_over_full_encode"] = round(
                row["ops"]["encode"]["median_us"] / row["ops"]["repair"]["median_us"], 2)
            print(json.dumps({"C_speedup": row["speedup_over_full_encode"]}), flush=True)
            out["rows"].append(row)
        del sh
        torch.cuda.empty_cache()
    if "B" in parts:
        k, m, bs, S = 16, 2, 1 << 20, 256
        sh = Shape(xec, torch, k, m, bs, S, lim)

        def two_data(bm):
            for c in range(S):
                bm[c, 2 * ((3 * c) % (k // 2))] = 0      # class 0
                bm[c, 2 * ((5 * c) % (k // 2)) + 1] = 0  # class 1
        bm = sh.bitmap(two_data)
        out["rows"].append(compare(sh, [("decode", "decode", bm), ("repair", "repair", bm)],
                                   args.rounds, args.iters, lim, "B 16+2 two data blocks per stripe"))
        del sh
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
