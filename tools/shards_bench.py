#!/usr/bin/env python3
"""The shard-major calls against the batch calls, in one process on one MI355X.

For configs 2, 3 and 4 of BASELINE.json each operation -- encode, the scrub, the
device repair with every parity block lost and with one data block lost per
stripe; the digest of every block, the locate over the flags of one class in
64, the degraded read of one whole lost block per stripe and of 4 KiB from each
of min(S, 1024) lost blocks; the degraded write and the vectored read of 4 KiB
of each of min(S, 1024) blocks and of one whole block per stripe, those blocks
lost and present -- runs in four placements of the same bytes:

  batch    the existing batch call (xec_encode, xec_verify, xec_repair_device,
           xec_digest, xec_locate, xec_read_device; xec_write and
           xec_readv_device on the same items);
  alias    the shard call on pointers aliased into that same batch: the same
           addresses, so the difference is the cost of table addressing alone;
  sep      k + m separate allocations, stride = bs;
  pad      the same with a padded stride of bs + 4096.

`sep` puts the members of a class S*bs apart, a large power of two -- the access
pattern column rotation exists for -- so it also runs with rotation off
(sep_rot-1) and on (sep_rot3); rotation applies to none of digest, locate, read,
write and readv, which run in the four placements only.  The writes come last:
they change the store (every placement takes the same new bytes, and the lost
blocks are repaired before the placements are compared).

Kernel times come from each call's own dispatch (xec_set_kernel_events).  The
placements of an operation are interleaved round by round; a figure is the
median of a round's launches after three warm-up launches, and every placement
reports its own spread over the rounds ((max - min) / median): a difference
inside the spreads of the two sides is not a difference.  After the timed
launches of a placement its store is scrubbed: the count must be 0, and what
a digest, locate or read left must equal what the batch call left.

Host cost: the time one xec_encode_shards call takes to return (checks, pair
check, launch) at k + m = 17 and 256, beside xec_encode and beside
xec_check_shards alone, on a tiny batch.

Every GPU step runs under a time limit of its own (--step-timeout): a step that
overruns ends the process with a traceback instead of queueing more work.

    python tools/shards_bench.py [--rounds 3] [--iters 20] [--only cfg3] [--ops digest,read_4k]
                                 [--out f.json]
"""
from __future__ import annotations

import argparse
import faulthandler
import json
import statistics
import sys
import time
from contextlib import contextmanager
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "erasure-code-benchmark_amd"))

CONFIGS = {"cfg2": (8, 1, 1 << 16, 1024), "cfg3": (16, 1, 1 << 20, 256),
           "cfg4": (32, 1, 4096, 65536)}  # k, m, bs, S (bench.py WORKLOADS)
PAD = 4096
# write / readv legs: <call>_<4k | block>_<lost | present>, the items the lost data block of
# each stripe (bitmap given) or the same blocks with everything present (no bitmap)
RW_OPS = [f"{call}_{size}_{state}" for call in ("readv", "write") for size in ("4k", "block")
          for state in ("lost", "present")]
OPS = ["encode", "verify", "repair_parity", "repair_data", "digest", "locate_flags", "read_block",
       "read_4k"] + RW_OPS
NO_ROTATION = OPS[4:]  # xec_set_rotation applies to none of these
READ_4K_ITEMS, READ_4K_LEN = 1024, 4096


@contextmanager
def step(seconds: float, what: str):
    """One GPU step under its own time limit."""
    print(f"# step: {what}", flush=True)
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


class Placement:
    """One placement of a shape's bytes and the calls on it."""

    def __init__(self, xec, torch, name, shape, batch, rotation=0, share=None):
        self.xec, self.torch, self.name, self.rotation = xec, torch, name, rotation
        self.k, self.m, self.bs, self.S = k, m, bs, S = shape
        d, p = batch
        self.batch = batch if name == "batch" else None
        self.keep = []
        if share is not None:  # the allocations of another placement, under another rotation
            self.keep, self.ptrs, self.ds, self.ps = share.keep, share.ptrs, share.ds, share.ps
        elif name in ("batch", "alias"):
            self.ptrs = [d.data_ptr() + i * bs for i in range(k)] + \
                        [p.data_ptr() + j * bs for j in range(m)]
            self.ds, self.ps = k * bs, m * bs
        else:
            stride = bs + (PAD if name == "pad" else 0)
            self.ds = self.ps = stride
            for src, n in ((d, k), (p, m)):
                blocks = src.view(S, n, bs)
                for i in range(n):
                    t = torch.zeros(S * stride, dtype=torch.uint8, device="cuda")
                    t.view(S, stride)[:, :bs] = blocks[:, i, :]
                    self.keep.append(t)
            self.ptrs = [t.data_ptr() for t in self.keep]
        self.table = xec.shard_table(self.ptrs)
        self.flags = torch.empty(S * m, dtype=torch.uint8, device="cuda")
        self.count = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        n = S * (k + m)
        self.digests = torch.empty(n, dtype=torch.int64, device="cuda")
        self.work = torch.empty(n, dtype=torch.int64, device="cuda")
        self.bitmap = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.out = torch.empty(S * bs, dtype=torch.uint8, device="cuda")
        self.rwork = torch.empty(xec.readv_device_work_bytes(S) // 8, dtype=torch.int64,
                                 device="cuda")
        self.scratch = torch.empty(xec.write_scratch_bytes(S) // 4 + 1, dtype=torch.int32,
                                   device="cuda")

    def rw_items(self, op):
        """(items, bytes of each) of a write / readv leg."""
        return (self.S, self.bs) if "_block_" in op else (min(self.S, READ_4K_ITEMS), READ_4K_LEN)

    def data_blocks(self):
        """The data blocks of the batch, or of separate allocations, as (S, k, bs)."""
        S, k, bs = self.S, self.k, self.bs
        if self.batch is not None:
            return self.batch[0].view(S, k, bs)
        return self.torch.stack([t.view(S, self.ds)[:, :bs] for t in self.keep[:k]], dim=1)

    def call_rw(self, op, bm, s):
        x, a = self.xec, (self.S, self.bs, self.k, self.m)
        call, _, state = op.split("_")
        n, length = self.rw_items(op)
        d_bm = bm["repair_data"] if state == "lost" else None
        if call == "readv":
            iov, wb = bm["iov_" + op.split("_")[1]], 8 * self.rwork.numel()
            if self.batch is not None:
                d, p = self.batch
                return x.readv_device(d, p, *a, d_bm, iov, n, self.out, n * length, self.rwork, wb,
                                      self.status, s)
            return x.readv_shards_device(self.table, self.ds, self.ps, *a, d_bm, iov, n, self.out,
                                         n * length, self.rwork, wb, self.status, s)
        if self.batch is not None:
            d, p = self.batch
            return x.write(d, p, bm["new"], *a, bm["h_repair_data"] if state == "lost" else None,
                           bm["h_items"], n, 0, length, None, self.scratch,
                           4 * self.scratch.numel(), s)
        return x.write_shards_device(self.table, self.ds, self.ps, *a, d_bm, bm["items"], n, 0,
                                     length, bm["new"], None, self.status, s)

    def heal(self, bm, s):
        """Put the lost data blocks back after a degraded write."""
        x, a = self.xec, (self.S, self.bs, self.k, self.m)
        if self.batch is not None:
            return x.repair_device(*self.batch, *a, bm["repair_data"], self.status, s)
        return x.repair_shards_device(self.table, self.ds, self.ps, *a, bm["repair_data"],
                                      self.status, s)

    def result(self, op):
        """What the last `op` left, for the comparison with the batch call's."""
        if op in RW_OPS:
            n, length = self.rw_items(op)
            return self.out[:n * length]
        if op == "digest":
            return self.digests
        if op == "locate_flags":
            return self.torch.cat([self.bitmap, self.count.view(self.torch.uint8)])
        n = self.S * self.bs if op == "read_block" else min(self.S, READ_4K_ITEMS) * READ_4K_LEN
        return self.out[:n]

    def call_integrity(self, op, bm, s):
        x, a = self.xec, (self.S, self.bs, self.k, self.m)
        if op in RW_OPS:
            return self.call_rw(op, bm, s)
        if self.batch is not None:
            d, p = self.batch
            if op == "digest":
                return x.digest(d, p, *a, self.digests, None, s)
            if op == "locate_flags":
                return x.locate(d, p, *a, bm["stored"], bm["flags64"], self.bitmap, self.count,
                                self.work, 8 * self.work.numel(), s)
            n, length = (self.S, self.bs) if op == "read_block" else \
                (min(self.S, READ_4K_ITEMS), READ_4K_LEN)
            return x.read_device(d, p, *a, bm["repair_data"], bm["items"], n, 0, length, self.out,
                                 self.status, s)
        t = (self.table, self.ds, self.ps)
        if op == "digest":
            return x.digest_shards(*t, *a, self.digests, None, s)
        if op == "locate_flags":
            return x.locate_shards(*t, *a, bm["stored"], bm["flags64"], self.bitmap, self.count,
                                   self.work, 8 * self.work.numel(), s)
        n, length = (self.S, self.bs) if op == "read_block" else \
            (min(self.S, READ_4K_ITEMS), READ_4K_LEN)
        return x.read_shards_device(*t, *a, bm["repair_data"], bm["items"], n, 0, length, self.out,
                                    self.status, s)

    def call(self, op, bm, s):
        x, a = self.xec, (self.S, self.bs, self.k, self.m)
        if op in NO_ROTATION:
            return self.call_integrity(op, bm, s)
        if self.batch is not None:
            d, p = self.batch
            if op == "encode":
                return x.encode(d, p, *a, s)
            if op == "verify":
                return x.verify(d, p, *a, self.flags, self.count, s)
            return x.repair_device(d, p, *a, bm[op], self.status, s)
        t = (self.table, self.ds, self.ps)
        if op == "encode":
            return x.encode_shards(*t, *a, s)
        if op == "verify":
            return x.verify_shards(*t, *a, self.flags, self.count, s)
        return x.repair_shards_device(*t, *a, bm[op], self.status, s)

    def time_round(self, op, bm, iters, ev, s):
        """Median kernel time (us) of `iters` launches after 3 warm-up ones."""
        assert self.xec.set_rotation(self.rotation) == 0
        try:
            us = []
            for i in range(iters + 3):
                self.xec.set_kernel_events(ev[0], ev[1])
                assert self.call(op, bm, s) == 0, (self.name, op)
                s.synchronize()
                if i >= 3:
                    us.append(ev[0].elapsed_time(ev[1]) * 1e3)
            return statistics.median(us)
        finally:
            self.xec.set_rotation(0)

    def scrub_is_clean(self, s):
        assert self.call("verify", None, s) == 0
        self.torch.cuda.synchronize()
        return int(self.count.item()) == 0 and int(self.status.item()) == 0


def label(pl: Placement):
    return pl.name if pl.rotation == 0 else f"{pl.name}_rot{pl.rotation}"


def run_config(xec, torch, name, shape, rounds, iters, lim, ops):
    import numpy as np
    k, m, bs, S = shape
    s = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with step(lim, f"{name}: fill, encode and lay out {k}+{m} x {bs} x {S}"):
        for e in ev:
            e.record(s)
        d = torch.empty(S * k * bs, dtype=torch.uint8, device="cuda")
        p = torch.empty(S * m * bs, dtype=torch.uint8, device="cuda")
        assert xec.fill_splitmix64(d, S, k * bs, 1896, s) == 0
        assert xec.encode(d, p, S, bs, k, m, s) == 0
        torch.cuda.synchronize()
        pls = [Placement(xec, torch, n, shape, (d, p)) for n in ("batch", "alias", "sep", "pad")]
        pls += [Placement(xec, torch, "sep", shape, (d, p), rot, share=pls[2]) for rot in (-1, 3)]
        parity = np.ones((S, k + m), np.uint8)
        parity[:, k:] = 0
        data = np.ones((S, k + m), np.uint8)
        for c in range(S):
            data[c, (7 * c) % k] = 0
        # the lost data block of every stripe, in stripe order; one class flag in 64
        items = np.array([(c << 8) | ((7 * c) % k) for c in range(S)], np.uint32)
        flags64 = np.zeros(S * m, np.uint8)
        flags64[::64] = 1
        stored = torch.empty(S * (k + m), dtype=torch.int64, device="cuda")
        assert xec.digest(d, p, S, bs, k, m, stored, None, s) == 0
        bm = {"repair_parity": torch.from_numpy(parity.reshape(-1)).to("cuda"),
              "repair_data": torch.from_numpy(data.reshape(-1)).to("cuda"),
              "items": torch.from_numpy(items.view(np.int32)).to("cuda"),
              "flags64": torch.from_numpy(flags64).to("cuda"), "stored": stored}
        if any(op in RW_OPS for op in ops):
            # the same items (ascending: one per stripe) for the write and the vectored read;
            # one range per entry so that the batch and the shard call serve the same queue
            bm["h_items"], bm["h_repair_data"] = items, np.ascontiguousarray(data.reshape(-1))
            for size, length in (("4k", READ_4K_LEN), ("block", bs)):
                iov = np.zeros(S, dtype=xec.IOV)
                iov["item"], iov["len"] = items, length
                bm["iov_" + size] = torch.from_numpy(iov.view(np.uint8).reshape(-1).copy()).to("cuda")
            new = torch.empty(S * bs, dtype=torch.uint8, device="cuda")
            assert xec.fill_splitmix64(new, S, bs, 7321, s) == 0
            bm["new"] = new
        torch.cuda.synchronize()
        torch.cuda.synchronize()
    rows = []
    for op in ops:
        timed = pls[:4] if op in NO_ROTATION else pls
        per = {label(pl): [] for pl in timed}
        for r in range(rounds):
            for pl in timed:
                with step(lim, f"{name} {op} round {r} {label(pl)}"):
                    per[label(pl)].append(pl.time_round(op, bm, iters, ev, s))
        med = {n: statistics.median(v) for n, v in per.items()}
        nbytes = (k + m) * bs * S
        if op in RW_OPS:  # the bytes delivered or taken, not the batch's
            nbytes = pls[0].rw_items(op)[0] * pls[0].rw_items(op)[1]
        row = {"config": name, "shape": list(shape), "op": op, "bytes": nbytes, "placements": {}}
        for n, v in per.items():
            row["placements"][n] = {
                "round_medians_us": [round(x, 2) for x in v], "median_us": round(med[n], 2),
                "spread_pct": round(100 * (max(v) - min(v)) / med[n], 2),
                "time_over_batch": round(med[n] / med["batch"], 4),
                "GBps_of_batch_bytes": round(nbytes / med[n] / 1e3, 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        if op.startswith("write_"):
            with step(lim, f"{name} {op}: repair, then every placement holds the batch's data"):
                n, length = pls[0].rw_items(op)
                for pl in pls[:4]:
                    if op.endswith("_lost"):
                        assert pl.heal(bm, s) == 0
                    torch.cuda.synchronize()
                    assert int(pl.status.item()) == 0, f"{name} {op} {pl.name}"
                want = pls[0].data_blocks()
                c = torch.arange(n, device="cuda")
                i = bm["items"][:n].to(torch.int64) & 0xFF
                assert torch.equal(want[c, i, :length], bm["new"][:n * length].view(n, length))
                for pl in pls[2:4]:
                    assert torch.equal(pl.data_blocks(), want), f"{name} {op} {pl.name}"
        elif op in NO_ROTATION:
            with step(lim, f"{name} {op}: every placement left what the batch call left"):
                torch.cuda.synchronize()
                assert int(pls[0].status.item()) == 0 and int(pls[0].count.item()) == 0
                for pl in pls[1:4]:
                    assert torch.equal(pl.result(op), pls[0].result(op)), f"{name} {op} {pl.name}"
    with step(lim, f"{name}: scrub every placement"):
        for pl in pls[:4]:
            assert pl.scrub_is_clean(s), f"{name} {pl.name}: not clean after the timed launches"
    return rows


def host_cost(xec, torch, lim, calls=2000, group=100):
    """Microseconds for one call to return, queue drained every `group` calls."""
    S, bs = 1, 256
    s = torch.cuda.current_stream()
    rows = []
    for k, m in ((16, 1), (255, 1)):
        with step(lim, f"host cost at k + m = {k + m}"):
            d = torch.zeros(S * k * bs, dtype=torch.uint8, device="cuda")
            p = torch.zeros(S * m * bs, dtype=torch.uint8, device="cuda")
            sep = [torch.zeros(S * bs, dtype=torch.uint8, device="cuda") for _ in range(k + m)]
            tables = {
                "alias": (xec.shard_table([d.data_ptr() + i * bs for i in range(k)] +
                                          [p.data_ptr() + j * bs for j in range(m)]), k * bs, m * bs),
                "sep": (xec.shard_table(sep), bs, bs)}
            fns = {"xec_encode": lambda: xec.encode(d, p, S, bs, k, m, s)}
            for n, t in tables.items():
                fns[f"xec_encode_shards {n}"] = lambda t=t: xec.encode_shards(*t, S, bs, k, m, s)
                fns[f"xec_check_shards {n}"] = lambda t=t: xec.check_shards(*t, S, bs, k, m)
            row = {"k_plus_m": k + m, "us_per_call": {}}
            for n, fn in fns.items():
                per = []
                for _ in range(3):
                    total = 0.0
                    for _ in range(calls // group):
                        t0 = time.perf_counter()
                        for _ in range(group):
                            fn()
                        total += time.perf_counter() - t0
                        torch.cuda.synchronize()
                    per.append(total / calls * 1e6)
                row["us_per_call"][n] = {"rounds": [round(x, 2) for x in per],
                                         "median": round(statistics.median(per), 2)}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="", help="comma list of cfg2,cfg3,cfg4,host (default: all)")
    ap.add_argument("--ops", default="", help=f"comma list of {','.join(OPS)} (default: all)")
    ap.add_argument("--step-timeout", type=float, default=90.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.rounds >= 3, "at least three interleaved rounds"
    import torch

    import xec
    torch.cuda.set_device(0)
    assert xec.init(0) == 0
    want = set(args.only.split(",")) if args.only else set(CONFIGS) | {"host"}
    ops = [op for op in OPS if not args.ops or op in args.ops.split(",")]
    assert ops and (not args.ops or set(args.ops.split(",")) <= set(OPS)), args.ops
    out = {"build_info": xec.build_info(), "rounds": args.rounds, "iters": args.iters, "rows": [],
           "host": []}
    print(json.dumps({"build_info": out["build_info"]}), flush=True)
    for name, shape in CONFIGS.items():
        if name in want:
            out["rows"] += run_config(xec, torch, name, shape, args.rounds, args.iters,
                                      args.step_timeout, ops)
            torch.cuda.empty_cache()
    if "host" in want:
        out["host"] = host_cost(xec, torch, args.step_timeout)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
