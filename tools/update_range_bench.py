#!/usr/bin/env python3
"""Ranged update with digest upkeep against the whole-block paths it replaces,
in one process on one MI355X.

As tools/update_bench.py (whose shapes, time limits and interleaving this
reuses): kernel times come from each call's own dispatch
(xec_set_kernel_events), the operations of a comparison are interleaved round
by round, every figure is the median of a round's launches, and a comparison
reports each operation's per-round medians, the ratio of the overall medians
and the partner's own spread, (max - min) / median of its round medians.  A
difference inside that spread is not a difference.

  P  the point of the feature: 1,024 writes of 4 KiB at offset 512 KiB into
     1 MiB blocks of 16+1 stripes (config 3, four blocks of each stripe):
     xec_update_range without and with upkeep, against xec_update of the same
     blocks whole and against xec_update + xec_digest(select) of those blocks;
  W  whole blocks with upkeep, one block per stripe at configs 2, 3 and 4:
     xec_update_range(0, bs, digests) against xec_update + xec_digest(select),
     the two-pass path;
  N  a sanity row, not a comparison: whole blocks without upkeep at the same
     configs, xec_update_range(0, bs) against xec_update.  Both calls run the
     same kernel (xec_update is the ranged update over [0, bs) without
     digests), so the row shows what two runs of one kernel differ by here.
     It compared two kernels while xec_update had its own (DESIGN.md §3
     *Ranged update*, item 3).

The two-pass figure is the sum of the two calls' kernel times, each from its
own dispatch; the small kernel with which xec_digest zeroes the selected slots
is not in it, which favours the two-pass path.  Successive launches alternate
between two sets of new bytes, so every timed launch changes the bytes it
names.  After the timed launches of a comparison the batch is scrubbed
(xec_verify's count must be 0) and the kept digests are compared with a fresh
xec_digest of the whole batch: they must be equal.

    python tools/update_range_bench.py [--rounds 3] [--iters 20] [--only P,W,N] [--out f.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from repair_scrub_bench import CONFIGS, step  # noqa: E402
from update_bench import UpdateShape  # noqa: E402


class RangeShape(UpdateShape):
    """UpdateShape plus the stored digests of the batch and ranged sets."""

    def __init__(self, *a):
        super().__init__(*a)
        torch = self.torch
        nb = self.S * (self.k + self.m)
        self.dig = torch.zeros(nb, dtype=torch.int64, device="cuda")
        self.fresh_dig = torch.zeros(nb, dtype=torch.int64, device="cuda")
        assert self.xec.digest(self.d, self.p, self.S, self.bs, self.k, self.m, self.dig, None,
                               self.s) == 0
        torch.cuda.synchronize()

    def range_set(self, per_stripe, offset, length):
        """update_set's blocks with `length` new bytes each (two alternating
        sets), and the select mask of the touched data and parity blocks."""
        torch, xec = self.torch, self.xec
        us = self.update_set(per_stripe)
        n = us["n"]
        us["offset"], us["len"] = offset, length
        us["new_range"] = [torch.empty(n * length, dtype=torch.uint8, device="cuda")
                           for _ in range(2)]
        for q, buf in enumerate(us["new_range"]):
            assert xec.fill_splitmix64(buf, n, length, 9090 + q, self.s) == 0
        sel = np.zeros((self.S, self.k + self.m), np.uint8)
        for it in us["items"]:
            c, i = int(it) >> 8, int(it) & 0xFF
            sel[c, i] = 1
            sel[c, self.k + i % self.m] = 1
        us["select"] = torch.from_numpy(sel.reshape(-1)).to("cuda")
        us["selected"] = int(sel.sum())
        torch.cuda.synchronize()
        return us

    def call(self, op, bm=None):
        x, a = self.xec, (self.S, self.bs, self.k, self.m)
        if op in ("range", "range_dig"):
            bm["turn"] ^= 1
            return x.update_range(self.d, self.p, bm["new_range"][bm["turn"]], *a, bm["items"],
                                  bm["n"], bm["offset"], bm["len"],
                                  self.dig if op == "range_dig" else None, bm["scratch"],
                                  4 * bm["n"], self.s)
        if op == "digest_select":
            return x.digest(self.d, self.p, *a, self.dig, bm["select"], self.s)
        return super().call(op, bm)

    def time_round(self, op, bm, iters):
        if op != "update+digest":
            return super().time_round(op, bm, iters)
        us = []
        for i in range(iters + 3):  # two calls, each timed from its own dispatch
            t = 0.0
            for part in ("update", "digest_select"):
                self.xec.set_kernel_events(self.ev[0], self.ev[1])
                assert self.call(part, bm) == 0, part
                self.s.synchronize()
                t += self.ev[0].elapsed_time(self.ev[1]) * 1e3
            if i >= 3:
                us.append(t)
        return statistics.median(us)

    def digests_are_current(self, bm):
        """The kept slots against a fresh xec_digest of the whole batch."""
        x, a = self.xec, (self.S, self.bs, self.k, self.m)
        assert x.digest(self.d, self.p, *a, self.fresh_dig, None, self.s) == 0
        self.torch.cuda.synchronize()
        return bool(self.torch.equal(self.dig, self.fresh_dig))

    def refresh(self, bm):
        assert self.call("digest_select", bm) == 0
        self.torch.cuda.synchronize()


def own_bytes(sh, op, us):
    """Bytes the operation moves: 3 per item and 2 per class touched, times the
    block or the range; the select digest re-reads the whole touched blocks."""
    moved = 3 * us["n"] + 2 * us["classes"]
    if op in ("range", "range_dig"):
        return moved * us["len"]
    if op == "update":
        return moved * sh.bs
    return moved * sh.bs + us["selected"] * sh.bs  # update+digest


def compare(sh, ops, us, rounds, iters, limit, label):
    """ops: [(name, op)], the first is the partner.  Interleaved rounds.  An
    operation without upkeep leaves the kept digests stale, so they are
    refreshed (untimed) after each of its rounds."""
    per = {name: [] for name, _ in ops}
    for r in range(rounds):
        for name, op in ops:
            with step(limit, f"{label} round {r} {name}"):
                per[name].append(sh.time_round(op, us, iters))
                if op in ("range", "update"):
                    sh.refresh(us)
    with step(limit, f"{label} scrub and digests"):
        clean = sh.scrub_is_clean()
        current = sh.digests_are_current(us)
    partner = ops[0][0]
    med = {n: statistics.median(v) for n, v in per.items()}
    row = {"comparison": label, "shape": [sh.k, sh.m, sh.bs, sh.S], "items": us["n"],
           "classes": us["classes"], "offset": us["offset"], "len": us["len"], "partner": partner,
           "scrub_clean_after": clean, "digests_current_after": current, "ops": {}}
    for name, op in ops:
        own = own_bytes(sh, op, us)
        row["ops"][name] = {"round_medians_us": [round(v, 2) for v in per[name]],
                            "median_us": round(med[name], 2),
                            "spread_pct": round(100 * (max(per[name]) - min(per[name])) / med[name], 2),
                            "own_bytes": own,
                            "GBps_of_own_bytes": round(own / med[name] / 1e3, 1),
                            "time_over_partner": round(med[name] / med[partner], 4)}
    print(json.dumps(row), flush=True)
    assert clean and current, label
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="", help="comma list of P,W,N (default: all)")
    ap.add_argument("--step-timeout", type=float, default=60.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.rounds >= 3, "at least three interleaved rounds"
    import torch

    import xec
    torch.cuda.set_device(0)
    assert xec.init(0) == 0
    lim = args.step_timeout
    parts = set(args.only.split(",")) if args.only else {"P", "W", "N"}
    out = {"build_info": xec.build_info(), "rounds": args.rounds, "iters": args.iters, "rows": []}
    print(json.dumps({"build_info": out["build_info"]}), flush=True)

    for name, (k, m, bs, S) in CONFIGS.items():
        if not parts & {"W", "N"} and not (name == "cfg3" and "P" in parts):
            continue
        sh = RangeShape(xec, torch, k, m, bs, S, lim)
        if name == "cfg3" and "P" in parts:
            with step(lim, "P sets"):
                us = sh.range_set(4, 512 << 10, 4 << 10)  # 1,024 items at S = 256
            out["rows"].append(compare(
                sh, [("update", "update"), ("update+digest", "update+digest"),
                     ("update_range", "range"), ("update_range+upkeep", "range_dig")],
                us, args.rounds, args.iters, lim, "P cfg3 1,024 x 4 KiB at 512 KiB"))
            del us
            torch.cuda.empty_cache()
        if parts & {"W", "N"}:
            with step(lim, f"{name} whole-block set"):
                us = sh.range_set(1, 0, bs)
            if "W" in parts:
                out["rows"].append(compare(
                    sh, [("update+digest", "update+digest"), ("update_range+upkeep", "range_dig")],
                    us, args.rounds, args.iters, lim, f"W {name} whole blocks with upkeep"))
            if "N" in parts:
                out["rows"].append(compare(
                    sh, [("update", "update"), ("update_range", "range")],
                    us, args.rounds, args.iters, lim,
                    f"N {name} whole blocks without upkeep (sanity: one kernel twice)"))
            del us
        del sh
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
