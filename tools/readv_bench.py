#!/usr/bin/env python3
"""The vectored read against what a caller does without it, in one process on
one MI355X.

As tools/read_bench.py: kernel times come from each call's own dispatch
(xec_set_kernel_events), the two sides of a comparison are interleaved round by
round and every figure is the median of a round's launches.  Beside the kernel
time each side's call-to-sync wall time is taken (time.perf_counter around the
calls and one stream synchronize, at least 20 repetitions after 3 warm-up ones):
the point of the feature is the calls it saves, and those do not show in a
kernel time.

Batch: 16+1 x 1 MiB x 256 stripes, one lost block per stripe (block 7c mod k of
stripe c); 1,024 entries, four per lost block.  xec_read is unchanged code, so
its side is the parent's path measured in the same process.

  a  1,024 lost entries, all (0, 4096): one xec_readv against one xec_read of
     the same items -- the price of the search;
  b  1,024 lost entries over 64 distinct (offset, len) pairs, 16 entries each,
     lengths from {512 B, 4 KiB, 64 KiB}, fixed seed: one xec_readv against the
     64 xec_read calls a caller needs today, back to back on one stream with one
     synchronize (their kernel time is the sum of the 64 kernels);
  c  row b with every entry present (no bitmap);
  d  xec_readv_device on row b's entries against row b's xec_readv;
  scan  (--scan) one xec_readv_device over 2^20 present entries of 16 bytes:
     the whole call bracketed by two event records, and its read kernel alone.

Every GPU step runs under a time limit of its own (--step-timeout).  After the
timed launches what each form delivered is compared with the blocks themselves
(nothing is erased here: "lost" is only what the bitmap says, so a
reconstruction must equal the bytes it stands for), and the batch is scrubbed.

    python tools/readv_bench.py [--rounds 3] [--iters 20] [--scan] [--out f.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from read_bench import ops_row  # noqa: E402
from repair_scrub_bench import Shape, step  # noqa: E402

BATCH = (16, 1, 1 << 20, 256)  # k, m, bs, S
N = 1024
LENGTHS = (512, 4 << 10, 64 << 10)


class ReadvShape(Shape):
    def __init__(self, *a):
        super().__init__(*a)
        import numpy as np
        torch, xec, S, k, bs = self.torch, self.xec, self.S, self.k, self.bs
        self.np = np
        c = np.arange(N) % S
        self.items = ((c << 8) | ((7 * c) % k)).astype(np.uint32)
        self.bm = self.bitmap(lambda b: b.__setitem__((np.arange(S), (7 * np.arange(S)) % k), 0))
        rng = np.random.default_rng(2026)
        pairs = set()
        while len(pairs) < 64:
            ln = int(rng.choice(LENGTHS))
            pairs.add((16 * int(rng.integers(0, (bs - ln) // 16 + 1)), ln))
        self.pairs = sorted(pairs)
        which = rng.permutation(np.repeat(np.arange(64), N // 64))  # 16 entries per pair
        self.uniform = self.iov(self.items, 0, 4096)
        self.mixed = self.iov(self.items, [self.pairs[w][0] for w in which],
                              [self.pairs[w][1] for w in which])
        # the same entries as the 64 calls a caller makes today: per pair, its items
        self.groups = [(off, ln, np.ascontiguousarray(self.items[which == w]))
                       for w, (off, ln) in enumerate(self.pairs)]
        self.total = int(self.mixed["len"].astype(np.int64).sum())
        self.out = torch.empty(max(self.total, N * 4096), dtype=torch.uint8, device="cuda")
        sb = xec.readv_scratch_bytes(N)
        self.scratch = torch.empty(sb, dtype=torch.uint8, device="cuda")
        self.d_mixed = torch.from_numpy(self.mixed.view(np.uint8).reshape(-1).copy()).to("cuda")
        self.work = torch.empty(xec.readv_device_work_bytes(N), dtype=torch.uint8, device="cuda")
        self.evs = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(64)]
        for pair in self.evs:
            for e in pair:
                e.record(self.s)
        torch.cuda.synchronize()

    def iov(self, items, offsets, lengths):
        a = self.np.zeros(len(items), dtype=self.xec.IOV)
        a["item"], a["offset"], a["len"] = items, offsets, lengths
        return a

    def one(self, op, timed=False):
        """Queue `op` once; with `timed` every kernel of it records its own events."""
        x, a, ev = self.xec, (self.S, self.bs, self.k, self.m), self.evs
        lost = not op.endswith("_present")
        h_bm = self.bm["h"] if lost else None
        if op == "read_uniform":
            if timed:
                x.set_kernel_events(*ev[0])
            assert x.read(self.d, self.p, *a, h_bm, self.items, N, 0, 4096, self.out, None, 0,
                          self.s) == 0
            return 1
        if op.startswith("read64"):
            dst = self.out.data_ptr()
            for q, (off, ln, items) in enumerate(self.groups):
                if timed:
                    x.set_kernel_events(*ev[q])
                assert x.read(self.d, self.p, *a, h_bm, items, len(items), off, ln, dst, None, 0,
                              self.s) == 0
                dst += len(items) * ln
            return 64
        if op.startswith("readv_device"):
            if timed:
                x.set_kernel_events(*ev[0])
            assert x.readv_device(self.d, self.p, *a, self.bm["d"] if lost else None, self.d_mixed, N,
                                  self.out, self.total, self.work, self.work.numel(), self.status,
                                  self.s) == 0
            return 1
        iov = self.uniform if op == "readv_uniform" else self.mixed
        if timed:
            x.set_kernel_events(*ev[0])
        assert x.readv(self.d, self.p, *a, h_bm, iov, N, self.out, self.out.numel(), self.scratch,
                       self.scratch.numel(), self.s) == 0
        return 1

    def kernel_round(self, op, iters):
        """Median over `iters` launches of the summed kernel time (us) of one `op`."""
        us = []
        for i in range(iters + 3):
            n = self.one(op, timed=True)
            self.s.synchronize()
            if i >= 3:
                us.append(sum(a.elapsed_time(b) for a, b in self.evs[:n]) * 1e3)
        return statistics.median(us)

    def wall_round(self, op, iters):
        """Median call-to-sync wall time (us) of one `op`: its calls, then one synchronize."""
        us = []
        for i in range(max(iters, 20) + 3):
            self.s.synchronize()
            t0 = time.perf_counter()
            self.one(op)
            self.s.synchronize()
            if i >= 3:
                us.append((time.perf_counter() - t0) * 1e6)
        return statistics.median(us)

    def delivered_is_right(self):
        torch = self.torch
        blocks = self.d.view(self.S, self.k, self.bs)  # every entry names a data block

        def want(iov):
            return torch.cat([blocks[int(e["item"]) >> 8, int(e["item"]) & 0xFF,
                                     int(e["offset"]):int(e["offset"]) + int(e["len"])] for e in iov])

        grouped = self.np.concatenate([self.iov(items, off, ln) for off, ln, items in self.groups])
        for op, iov in (("readv_uniform", self.uniform), ("read_uniform", self.uniform),
                        ("readv_mixed", self.mixed), ("readv_mixed_present", self.mixed),
                        ("readv_device", self.mixed), ("readv_device_present", self.mixed),
                        ("read64", grouped), ("read64_present", grouped)):
            self.out.fill_(0x5C)
            self.one(op)
            torch.cuda.synchronize()
            w = want(iov)
            if int(self.status.item()) != 0 or not torch.equal(self.out[:w.numel()], w):
                print(f"# WRONG BYTES: {op}", flush=True)
                return False
        return self.scrub_is_clean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--scan", action="store_true", help="the device form over 2^20 entries")
    ap.add_argument("--step-timeout", type=float, default=60.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.rounds >= 3, "at least three interleaved rounds"
    import torch

    import xec
    torch.cuda.set_device(0)
    assert xec.init(0) == 0
    lim = args.step_timeout
    out = {"build_info": xec.build_info(), "lib": Path(xec.LIB_PATH).name, "rounds": args.rounds,
           "iters": args.iters, "rows": []}
    print(json.dumps({"build_info": out["build_info"]}), flush=True)
    k, m, bs, S = BATCH
    sh = ReadvShape(xec, torch, k, m, bs, S, lim)

    def compare(label, what, partner, subject):
        kern = {partner: [], subject: []}
        wall = {partner: [], subject: []}
        for r in range(args.rounds):
            for op in (partner, subject):
                with step(lim, f"{label} round {r} {op}"):
                    kern[op].append(sh.kernel_round(op, args.iters))
                    wall[op].append(sh.wall_round(op, args.iters))
        mk = {op: statistics.median(v) for op, v in kern.items()}
        mw = {op: statistics.median(v) for op, v in wall.items()}
        row = {"row": label, "comparison": what, "shape": [k, m, bs, S], "entries": N,
               "partner": partner, "subject": subject,
               "kernel_subject_over_partner": round(mk[subject] / mk[partner], 4),
               "wall_subject_over_partner": round(mw[subject] / mw[partner], 4),
               "kernel_us": ops_row(kern), "call_to_sync_us": ops_row(wall)}
        print(json.dumps(row), flush=True)
        out["rows"].append(row)

    compare("a", "1,024 lost entries, all (0, 4096): xec_readv against xec_read", "read_uniform",
            "readv_uniform")
    compare("b", "1,024 lost entries over 64 (offset, len) pairs: one xec_readv against 64 xec_read "
            "calls and one sync", "read64", "readv_mixed")
    compare("c", "row b, every entry present", "read64_present", "readv_mixed_present")
    compare("d", "xec_readv_device on row b's entries against row b's xec_readv", "readv_mixed",
            "readv_device")
    with step(lim, "delivered bytes + scrub"):
        assert sh.delivered_is_right()
    out["bytes_out_mixed"] = sh.total

    if args.scan:
        import numpy as np
        n = 1 << 20
        rng = np.random.default_rng(5)
        c = rng.integers(0, S, n)
        iov = sh.iov(((c << 8) | rng.integers(0, k, n)).astype(np.uint32),
                     16 * rng.integers(0, bs // 16, n), 16)
        with step(lim, "scan: 2^20 entries"):
            d_iov = torch.from_numpy(iov.view(np.uint8).reshape(-1).copy()).to("cuda")
            work = torch.empty(xec.readv_device_work_bytes(n), dtype=torch.uint8, device="cuda")
            dst = torch.empty(16 * n, dtype=torch.uint8, device="cuda")
            whole, kernel = [], []
            for i in range(8):
                sh.ev[0].record(sh.s)
                xec.set_kernel_events(*sh.evs[0])
                assert xec.readv_device(sh.d, sh.p, S, bs, k, m, None, d_iov, n, dst, dst.numel(),
                                        work, work.numel(), sh.status, sh.s) == 0
                sh.ev[1].record(sh.s)
                sh.s.synchronize()
                if i >= 3:
                    whole.append(sh.ev[0].elapsed_time(sh.ev[1]) * 1e3)
                    kernel.append(sh.evs[0][0].elapsed_time(sh.evs[0][1]) * 1e3)
            assert int(sh.status.item()) == 0
            idx = (torch.from_numpy(((c * k + (iov["item"] & 0xFF).astype(np.int64)) * bs
                                     + iov["offset"].astype(np.int64)) // 16).to("cuda"))
            assert torch.equal(dst.view(n, 16), sh.d.view(-1, 16)[idx]), "scan row: wrong bytes"
        row = {"row": "scan", "entries": n, "entry_bytes": 16,
               "whole_call_bracketed_us": round(statistics.median(whole), 1),
               "read_kernel_us": round(statistics.median(kernel), 1),
               "check_and_scan_at_most_us": round(statistics.median(whole)
                                                  - statistics.median(kernel), 1)}
        print(json.dumps(row), flush=True)
        out["rows"].append(row)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
