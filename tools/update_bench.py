#!/usr/bin/env python3
"""In-place block update against the re-encode it replaces, in one process on
one MI355X.

As tools/repair_scrub_bench.py (whose Shape, time limits and interleaving this
reuses): kernel times come from each call's own dispatch
(xec_set_kernel_events), the operations of a comparison are interleaved round
by round, every figure is the median of a round's launches, and a comparison
reports each operation's per-round medians, the ratio of the overall medians
and the partner's own spread in this process.  A difference inside that spread
is not a difference.

  A  xec_update of one block per stripe at configs 2, 3 and 4 against the
     xec_encode of the same batch (5 / (k+m) of its bytes), with update's rate
     over its own 5*bs per item beside encode's over (k+m)*bs*S;
  B  config 3, g = 1, 2, 4, 8, 16 members of each class updated, against
     encode: the byte counts cross at g > (k/m - 1) / 2 = 7.5;
  C  config 3, xec_update against xec_update_device on the same blocks, one
     stripe in 9 written and every stripe written;
  D  (--sweep) A's update under residency caps 1, 2, 4, 8 and the shipped
     choice.  The parity store's policy is a constant of the kernel source
     (kPatchParityStoreAux, csrc/xec_kernels.hip: xec_update runs the ranged
     update's kernels over whole blocks): to compare another value,
     run part A once more with XEC_LIB naming a library built with it and
     compare the two runs' ratios to encode.

What the times are: the kernel's own dispatch, for update as for encode.  A
list of more than 1,024 items is uploaded into d_scratch on the stream ahead
of the kernel (config 4 in A: 256 KiB), and that copy is NOT in the kernel
time; "bracketed_median_us" beside it is the same call between two
hipEventRecord packets on the stream, copy and packet gaps included, for every
operation alike.

Every GPU step runs under a time limit of its own (--step-timeout).  Successive
launches of an update alternate between two sets of new blocks, so every timed
launch changes the bytes it names.  After the timed launches of a comparison
the batch is scrubbed: xec_verify's count must be 0 -- an update keeps parity
right whatever it wrote.

    python tools/update_bench.py [--rounds 3] [--iters 20] [--sweep] [--only A,B] [--out f.json]
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


class UpdateShape(Shape):
    """Shape plus update sets: {"items", "n", "new", "scratch", "mask", "shadow"}."""

    def update_set(self, per_stripe, stripes=None, device_form=False):
        """Blocks (7c + r) % k, r < per_stripe, of the given stripes (default all)."""
        torch, xec = self.torch, self.xec
        S, k, bs = self.S, self.k, self.bs
        stripes = range(S) if stripes is None else stripes
        blocks = sorted((c, i) for c in stripes
                        for i in {(7 * c + r) % k for r in range(per_stripe)})
        items = np.array([(c << 8) | i for c, i in blocks], dtype=np.uint32)
        n = len(items)
        new = [torch.empty(n * bs, dtype=torch.uint8, device="cuda") for _ in range(2)]
        for q, buf in enumerate(new):
            assert xec.fill_splitmix64(buf, n, bs, 4242 + q, self.s) == 0
        us = {"items": items, "n": n, "new": new, "lost": n, "turn": 0,
              "classes": len({(c, i % self.m) for c, i in blocks}),
              "scratch": torch.empty(max(4 * n, 4), dtype=torch.uint8, device="cuda")}
        if device_form:
            mask = np.zeros((S, k), np.uint8)
            for c, i in blocks:
                mask[c, i] = 1
            us["mask"] = torch.from_numpy(mask.reshape(-1)).to("cuda")
            us["shadow"] = [torch.empty(S * k * bs, dtype=torch.uint8, device="cuda")
                            for _ in range(2)]
            for q, buf in enumerate(us["shadow"]):
                assert xec.fill_splitmix64(buf, S, k * bs, 777 + q, self.s) == 0
        torch.cuda.synchronize()
        return us

    def call(self, op, bm=None):
        x, a = self.xec, (self.S, self.bs, self.k, self.m)
        if op.startswith("update"):
            bm["turn"] ^= 1  # the other set of new blocks: every launch changes the bytes
        if op == "update":
            return x.update(self.d, self.p, bm["new"][bm["turn"]], *a, bm["items"], bm["n"],
                            bm["scratch"], 4 * bm["n"], self.s)
        if op == "update_device":
            return x.update_device(self.d, self.p, bm["shadow"][bm["turn"]], *a, bm["mask"],
                                   self.s)
        return super().call(op, bm)

    def bracketed(self, op, bm, iters):
        """Median time (us) of the call between two event packets on the stream."""
        us = []
        for _ in range(iters):
            self.ev[0].record(self.s)
            assert self.call(op, bm) == 0, op
            self.ev[1].record(self.s)
            self.s.synchronize()
            us.append(self.ev[0].elapsed_time(self.ev[1]) * 1e3)
        return statistics.median(us)


def compare(sh, ops, rounds, iters, limit, label):
    """ops: [(name, op, set)], the first is the partner (encode).  Interleaved rounds."""
    per = {name: [] for name, _, _ in ops}
    tiling = {}
    for r in range(rounds):
        for name, op, us in ops:
            with step(limit, f"{label} round {r} {name}"):
                per[name].append(sh.time_round(op, us, iters))
                if op.startswith("update"):
                    tiling[name] = sh.xec.update_tiling_used()
    with step(limit, f"{label} bracketed"):
        bracketed = {name: sh.bracketed(op, us, iters) for name, op, us in ops}
    with step(limit, f"{label} scrub"):
        clean = sh.scrub_is_clean()
    partner = ops[0][0]
    med = {n: statistics.median(v) for n, v in per.items()}
    row = {"comparison": label, "shape": [sh.k, sh.m, sh.bs, sh.S], "partner": partner,
           "partner_spread_pct": round(100 * (max(per[partner]) - min(per[partner])) / med[partner], 2),
           "scrub_clean_after": clean, "ops": {}}
    for name, op, us in ops:
        # an update reads old and new and writes new per item, and reads and writes the
        # parity block of every class it touches: 5*bs for one item of a class
        own = (3 * us["n"] + 2 * us["classes"]) * sh.bs if op.startswith("update") else sh.bytes
        row["ops"][name] = {"round_medians_us": [round(v, 2) for v in per[name]],
                            "median_us": round(med[name], 2),
                            "bracketed_median_us": round(bracketed[name], 2),
                            "own_bytes": own,
                            "GBps_of_own_bytes": round(own / med[name] / 1e3, 1),
                            "time_over_partner": round(med[name] / med[partner], 4),
                            "items": us["n"] if us else None,
                            "tiling": tiling.get(name)}
    print(json.dumps(row), flush=True)
    assert clean, label
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sweep", action="store_true", help="update residency caps 1, 2, 4, 8")
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

    for name, (k, m, bs, S) in CONFIGS.items():
        if not parts & {"A", "D"} and not (name == "cfg3" and parts & {"B", "C"}):
            continue
        sh = UpdateShape(xec, torch, k, m, bs, S, lim)
        with step(lim, f"{name} update sets"):
            one = sh.update_set(1)
        if "A" in parts:
            row = compare(sh, [("encode", "encode", None), ("update", "update", one)],
                          args.rounds, args.iters, lim, f"A {name} one block per stripe")
            row["bytes_over_encode"] = round(5 / (k + m), 4)
            out["rows"].append(row)
        if "D" in parts:
            per = {}
            for r in range(args.rounds):
                for w in (0, 1, 2, 4, 8):
                    assert xec.set_occupancy(w) == 0
                    try:
                        with step(lim, f"D {name} round {r} update cap {w}"):
                            per.setdefault(w, []).append(sh.time_round("update", one, args.iters))
                    finally:
                        xec.set_occupancy(0)
                with step(lim, f"D {name} round {r} encode"):
                    per.setdefault("encode", []).append(sh.time_round("encode", None, args.iters))
            with step(lim, f"D {name} scrub"):
                assert sh.scrub_is_clean()
            enc = per["encode"]
            row = {"comparison": f"D {name}", "shape": [k, m, bs, S], "items": one["n"],
                   "update_cap_us": {str(w): {"round_medians_us": [round(v, 2) for v in per[w]],
                                              "median_us": round(statistics.median(per[w]), 2)}
                                     for w in (0, 1, 2, 4, 8)},
                   "encode_us": {"round_medians_us": [round(v, 2) for v in enc],
                                 "median_us": round(statistics.median(enc), 2),
                                 "spread_pct": round(100 * (max(enc) - min(enc)) /
                                                     statistics.median(enc), 2)}}
            print(json.dumps(row), flush=True)
            out["rows"].append(row)
        if name == "cfg3" and "B" in parts:
            for g in (1, 2, 4, 8, 16):
                with step(lim, f"B update set g={g}"):
                    us = one if g == 1 else sh.update_set(g)
                row = compare(sh, [("encode", "encode", None), ("update", "update", us)],
                              args.rounds, args.iters, lim, f"B cfg3 {g} of {k // m} members")
                row["members_updated"] = g
                row["bytes_over_encode"] = round((3 * g + 2) / (k // m + 1), 4)
                out["rows"].append(row)
                del us
        if name == "cfg3" and "C" in parts:
            for label, stripes in (("1 stripe in 9", range(4, S, 9)), ("every stripe", None)):
                with step(lim, f"C update set {label}"):
                    us = sh.update_set(1, stripes, device_form=True)
                out["rows"].append(compare(sh, [("encode", "encode", None),
                                                ("update", "update", us),
                                                ("update_device", "update_device", us)],
                                           args.rounds, args.iters, lim, f"C cfg3 {label}"))
                del us
                torch.cuda.empty_cache()
        del sh, one
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
