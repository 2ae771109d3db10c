#!/usr/bin/env python3
"""Degraded write against the calls it stands beside or replaces, in one
process on one MI355X.

As tools/update_range_bench.py (whose shapes, time limits and interleaving this
reuses): kernel times come from each call's own dispatch
(xec_set_kernel_events), the operations of a comparison are interleaved round
by round, every figure is the median of a round's launches, and a comparison
reports each operation's per-round medians and its spread, (max - min) / median
of its round medians.  A difference inside the partner's spread is not a
difference.

  D  delta mode against xec_update_range: the same items and range under an
     all-present bitmap, without and with upkeep -- 1,024 x 4 KiB at offset
     512 KiB into 1 MiB blocks of 16+1, and one whole block per stripe at
     configs 2, 3 and 4.  The bytes moved are equal;
  R  rebuild-write against the composition it replaces, xec_repair of the lost
     blocks followed by xec_update_range (the sum of the two kernel times):
     1,024 x 4 KiB at 512 KiB with every written block lost (config 3's shape
     with 1,024 stripes, one item each), and one whole lost block per stripe at
     config 3, with the bytes each side moves;
  O  data-only (the parity of every stripe lost) against ONE device-to-device
     hipMemcpyAsync (a torch copy_) of the same bytes, both bracketed by two
     event records on the stream as tools/read_bench.py brackets its gather;
  S  residency of the rebuild mode: xec_set_occupancy 1, 2, 4, 8 and the
     default (uncapped) once each at k/m = 8, 16 and 32 (configs 2, 3 and 4,
     one whole lost block per stripe).

Successive launches alternate between two sets of new bytes.  After a
comparison the batch is repaired under the bitmap in use and scrubbed:
xec_verify's count must be 0.

    python tools/write_bench.py [--rounds 5] [--iters 20] [--only D,R,O,S] [--out f.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from repair_scrub_bench import CONFIGS, Shape, step  # noqa: E402


class WriteShape(Shape):
    def write_set(self, per_stripe, offset, length, lose):
        """Blocks (7c + r) % k, r < per_stripe, of every stripe with `length` new
        bytes each (two alternating sets) and a bitmap: lose = None (all
        present), "written" (every written block) or "parity" (every parity)."""
        torch, xec = self.torch, self.xec
        S, k, m = self.S, self.k, self.m
        blocks = sorted((c, i) for c in range(S)
                        for i in {(7 * c + r) % k for r in range(per_stripe)})
        items = np.array([(c << 8) | i for c, i in blocks], dtype=np.uint32)
        n = len(items)
        bm = np.ones((S, k + m), np.uint8)
        if lose == "written":
            for c, i in blocks:
                bm[c, i] = 0
        elif lose == "parity":
            bm[:, k:] = 0
        new = [torch.empty(n * length, dtype=torch.uint8, device="cuda") for _ in range(2)]
        for q, buf in enumerate(new):
            assert xec.fill_splitmix64(buf, n, length, 5150 + q, self.s) == 0
        nb = S * (k + m)
        ws = {"items": items, "n": n, "offset": offset, "len": length, "new": new, "turn": 0,
              "classes": len({(c, i % m) for c, i in blocks}),
              "h": torch.from_numpy(bm.reshape(-1)).pin_memory(), "lost": int((bm == 0).sum()),
              "scratch": torch.empty(max(xec.write_scratch_bytes(n), nb, 4), dtype=torch.uint8,
                                     device="cuda"),
              "dig": torch.zeros(nb, dtype=torch.int64, device="cuda"),
              "copy_dst": None}
        st, ws["n_rebuild"], ws["n_data_only"] = xec.check_write_items(ws["h"].numpy(), S, k, m,
                                                                       items, n)
        assert st == 0, st
        torch.cuda.synchronize()
        return ws

    def call(self, op, ws=None):
        x, a = self.xec, (self.S, self.bs, self.k, self.m)
        if op in ("range", "range_dig", "write", "write_dig"):
            ws["turn"] ^= 1
            new = ws["new"][ws["turn"]]
            dig = ws["dig"] if op.endswith("_dig") else None
            if op.startswith("range"):
                return x.update_range(self.d, self.p, new, *a, ws["items"], ws["n"], ws["offset"],
                                      ws["len"], dig, ws["scratch"], ws["scratch"].numel(), self.s)
            return x.write(self.d, self.p, new, *a, ws["h"], ws["items"], ws["n"], ws["offset"],
                           ws["len"], dig, ws["scratch"], ws["scratch"].numel(), self.s)
        if op == "repair":
            return x.repair(self.d, self.p, *a, ws["h"], ws["scratch"], self.s)
        if op == "memcpy":
            if ws["copy_dst"] is None:
                ws["copy_dst"] = self.torch.empty_like(ws["new"][0])
            ws["copy_dst"].copy_(ws["new"][0], non_blocking=True)
            return 0
        return super().call(op, ws)

    def time_round(self, op, ws, iters):
        if op != "repair+range":
            return super().time_round(op, ws, iters)
        us = []
        for i in range(iters + 3):  # two calls, each timed from its own dispatch
            t = 0.0
            for part in ("repair", "range"):
                self.xec.set_kernel_events(self.ev[0], self.ev[1])
                assert self.call(part, ws) == 0, part
                self.s.synchronize()
                t += self.ev[0].elapsed_time(self.ev[1]) * 1e3
            if i >= 3:
                us.append(t)
        return statistics.median(us)

    def bracketed(self, op, ws, iters):
        us = []
        for i in range(iters + 3):
            self.ev[0].record(self.s)
            assert self.call(op, ws) == 0, op
            self.ev[1].record(self.s)
            self.s.synchronize()
            if i >= 3:
                us.append(self.ev[0].elapsed_time(self.ev[1]) * 1e3)
        return statistics.median(us)

    def repaired_is_clean(self, ws):
        if ws["lost"]:
            assert self.call("repair", ws) == 0
        return self.scrub_is_clean()


def own_bytes(sh, op, ws):
    """Bytes the operation moves (without upkeep's extra reads)."""
    n, cl, ln = ws["n"], ws["classes"], ws["len"]
    delta = (3 * n + 2 * cl) * ln
    if op in ("range", "range_dig"):
        return delta
    if op == "repair+range":  # k/m blocks read and one written per lost block, then the delta
        return ws["lost"] * (sh.k // sh.m + 1) * sh.bs + delta
    if op == "memcpy":
        return 2 * n * ln
    if ws["n_data_only"]:
        return 2 * n * ln
    if ws["n_rebuild"]:  # per class: its members' sources, the written present ones, the parity
        return (cl * (sh.k // sh.m) + (n - ws["n_rebuild"]) + cl) * ln
    return delta


def compare(sh, ops, ws, rounds, iters, limit, label, timer="time_round"):
    per = {name: [] for name, _ in ops}
    for r in range(rounds):
        for name, op in ops:
            with step(limit, f"{label} round {r} {name}"):
                per[name].append(getattr(sh, timer)(op, ws, iters))
    with step(limit, f"{label} repair and scrub"):
        clean = sh.repaired_is_clean(ws)
    partner = ops[0][0]
    med = {n: statistics.median(v) for n, v in per.items()}
    row = {"comparison": label, "shape": [sh.k, sh.m, sh.bs, sh.S], "items": ws["n"],
           "classes": ws["classes"], "offset": ws["offset"], "len": ws["len"],
           "lost_blocks": ws["lost"], "timer": timer, "partner": partner,
           "tiling": sh.xec.write_tiling_used(), "scrub_clean_after_repair": clean, "ops": {}}
    for name, op in ops:
        own = own_bytes(sh, op, ws)
        row["ops"][name] = {"round_medians_us": [round(v, 2) for v in per[name]],
                            "median_us": round(med[name], 2),
                            "min_us": round(min(per[name]), 2), "max_us": round(max(per[name]), 2),
                            "spread_pct": round(100 * (max(per[name]) - min(per[name])) / med[name], 2),
                            "own_bytes": own,
                            "GBps_of_own_bytes": round(own / med[name] / 1e3, 1),
                            "time_over_partner": round(med[name] / med[partner], 4)}
    print(json.dumps(row), flush=True)
    assert clean, label
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="", help="comma list of D,R,O,S (default: all)")
    ap.add_argument("--step-timeout", type=float, default=60.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.rounds >= 3, "at least three interleaved rounds"
    import torch

    import xec
    torch.cuda.set_device(0)
    assert xec.init(0) == 0
    lim = args.step_timeout
    parts = set(args.only.split(",")) if args.only else {"D", "R", "O", "S"}
    out = {"build_info": xec.build_info(), "rounds": args.rounds, "iters": args.iters, "rows": []}
    print(json.dumps({"build_info": out["build_info"]}), flush=True)
    delta_ops = [("update_range", "range"), ("write", "write")]
    delta_dig = [("update_range+upkeep", "range_dig"), ("write+upkeep", "write_dig")]
    small = (512 << 10, 4 << 10)

    for name, (k, m, bs, S) in CONFIGS.items():
        sh = WriteShape(xec, torch, k, m, bs, S, lim)
        if "D" in parts:
            sets = [("whole blocks, one per stripe", 1, 0, bs)]
            if name == "cfg3":
                sets.insert(0, ("1,024 x 4 KiB at 512 KiB", 4, *small))
            for what, per_stripe, off, ln in sets:
                with step(lim, f"D {name} set"):
                    ws = sh.write_set(per_stripe, off, ln, None)
                for ops in (delta_ops, delta_dig):
                    out["rows"].append(compare(sh, ops, ws, args.rounds, args.iters, lim,
                                               f"D {name} {what}: {ops[1][0]} under an all-present bitmap"))
                del ws
        if "R" in parts and name == "cfg3":
            with step(lim, "R whole set"):
                ws = sh.write_set(1, 0, bs, "written")
            out["rows"].append(compare(sh, [("repair+update_range", "repair+range"), ("write", "write")],
                                       ws, args.rounds, args.iters, lim,
                                       "R cfg3 one whole lost block per stripe"))
            del ws
        if "O" in parts:
            with step(lim, f"O {name} set"):
                ws = sh.write_set(1, 0, bs, "parity")
            out["rows"].append(compare(sh, [("memcpy", "memcpy"), ("write", "write")], ws,
                                       args.rounds, args.iters, lim,
                                       f"O {name} data-only whole blocks against one D2D copy",
                                       timer="bracketed"))
            del ws
        if "S" in parts:
            with step(lim, f"S {name} set"):
                ws = sh.write_set(1, 0, bs, "written")
            sweep = {}
            for w in (0, 1, 2, 4, 8):
                assert xec.set_occupancy(w) == 0
                with step(lim, f"S {name} waves {w}"):
                    sweep[str(w)] = round(sh.time_round("write", ws, args.iters), 2)
            assert xec.set_occupancy(0) == 0
            with step(lim, f"S {name} repair and scrub"):
                clean = sh.repaired_is_clean(ws)
            row = {"comparison": f"S {name} rebuild-write residency sweep (0 = default, uncapped)",
                   "shape": [k, m, bs, S], "members": k // m, "items": ws["n"],
                   "median_us_by_waves_per_simd": sweep, "scrub_clean_after_repair": clean}
            print(json.dumps(row), flush=True)
            assert clean
            out["rows"].append(row)
            del ws
        del sh
        torch.cuda.empty_cache()

    if "R" in parts:  # config 3's blocks, 1,024 stripes: one lost written block in each
        k, m, bs, _ = CONFIGS["cfg3"]
        sh = WriteShape(xec, torch, k, m, bs, 1024, lim)
        with step(lim, "R small set"):
            ws = sh.write_set(1, *small, "written")
        out["rows"].append(compare(sh, [("repair+update_range", "repair+range"), ("write", "write")],
                                   ws, args.rounds, args.iters, lim,
                                   "R 16+1 x 1 MiB x 1,024: 1,024 x 4 KiB at 512 KiB, every written block lost"))
        del ws, sh
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
