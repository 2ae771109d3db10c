#!/usr/bin/env python3
"""What does an xec_verify captured in a hipGraph leave in d_flags / *d_count?

One captured graph per process (`--chain`, a comma list of encode, update,
verify) over a small encoded batch, replayed twice with d_flags pre-filled with
0xFF and *d_count with 77, then the same scrub outside the graph.  `--with`
adds things a process may do around the capture:

  A  a pageable host-to-device copy into the batch before the capture
  C  an xec_verify outside the graph before each replay
  D  a device allocation (a clone of the batch, compared) before each replay
  E  another graph captured, replayed and deleted before this one

Seen on an MI355X (profiles/update/graph_verify_probe.log): with none of them
the captured scrub is exact in both replays (count 0, no flag); with any one
of them the first replay is exact and the second leaves d_flags with bytes
such as 95, 118, 208 -- the kernels only store 0 and 1 there -- or with its
last 5 bytes set, and *d_count to match, while the batch scrubbed clean
outside the graph right after.  The chain encode,verify shows it as update,verify
does.  The cause is not known.

    python tools/lab/graph_verify_probe.py --chain update,verify --with A
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "erasure-code-benchmark_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chain", default="update,verify")
    ap.add_argument("--with", dest="extra", default="")
    args = ap.parse_args()
    import torch

    import xec
    torch.cuda.set_device(0)
    assert xec.init(0) == 0
    S, k, m, bs = 23, 12, 3, 4352
    s0 = torch.cuda.current_stream()
    d = torch.empty(S * k * bs, dtype=torch.uint8, device="cuda")
    p = torch.empty(S * m * bs, dtype=torch.uint8, device="cuda")
    assert xec.fill_splitmix64(d, S, k * bs, 1896, s0) == 0
    assert xec.encode(d, p, S, bs, k, m, s0) == 0
    shadow = torch.empty(S * k * bs, dtype=torch.uint8, device="cuda")
    assert xec.fill_splitmix64(shadow, S, k * bs, 4242, s0) == 0
    rng = np.random.default_rng(23)
    masks = [torch.from_numpy((rng.random(S * k) < 1 / 3).astype(np.uint8)).to("cuda")
             for _ in range(2)]
    mask = masks[0].clone()
    count = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    flags = torch.full((S * m,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if "A" in args.extra:
        d.copy_(torch.from_numpy(d.cpu().numpy().copy()))
    if "E" in args.extra:
        g0 = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g0, stream=torch.cuda.Stream()):
            assert xec.verify(d, p, S, bs, k, m, flags, count, torch.cuda.current_stream()) == 0
        g0.replay()
        torch.cuda.synchronize()
        del g0
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        cs = torch.cuda.current_stream()
        for step in args.chain.split(","):
            if step == "encode":
                assert xec.encode(d, p, S, bs, k, m, cs) == 0
            elif step == "update":
                assert xec.update_device(d, p, shadow, S, bs, k, m, mask, cs) == 0
            elif step == "verify":
                assert xec.verify(d, p, S, bs, k, m, flags, count, cs) == 0
            else:
                raise SystemExit(f"unknown step {step}")
    for rep in range(2):
        mask.copy_(masks[rep])
        if "C" in args.extra:
            assert xec.verify(d, p, S, bs, k, m, flags, count, None) == 0
        if "D" in args.extra:
            d2 = d.clone()
            assert torch.equal(d, d2)
            del d2
        count.fill_(77)
        flags.fill_(0xFF)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        f = flags.cpu().numpy()
        print(f"[{args.chain} +{args.extra or '-'}] replay {rep}: count {int(count.item()):#x} "
              f"flags nonzero at {np.flatnonzero(f).tolist()} values {sorted(set(f.tolist()))}",
              flush=True)
    assert xec.verify(d, p, S, bs, k, m, flags, count, None) == 0
    torch.cuda.synchronize()
    print(f"[{args.chain} +{args.extra or '-'}] the same scrub outside the graph: "
          f"{int(count.item())}", flush=True)


if __name__ == "__main__":
    main()
