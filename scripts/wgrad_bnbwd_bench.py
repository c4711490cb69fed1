"""Per-launch A/B of the fp32 wgrad that produces its dy operand (tmr_conv2d_wgrad_bnbwd) against
the two calls it replaces, over the conv+BN units of the fp32 ResNet-50 step whose masked gradient
comes from a fused dgrad (the shapes of profiles/r6/fwd_epilogue/c2_table.txt).  Per shape:

  two   = bn_bwd_parts (reduction + apply pass writing dy) + conv_wgrad
  fused = bn_bwd_parts_coef (reduction only) + conv_wgrad_bnbwd (dy produced on load, written once)

in ms, and whether the library serves the fused form at all (units on the 256x256 tile do not).

usage: python scripts/wgrad_bnbwd_bench.py [--frames 640] [--reps 10] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tmrnet_amd import ops  # noqa: E402

# (unit, input h, input channels c, output channels k, kernel r, stride)
SHAPES = [
    ("l1.conv1", 56, 256, 64, 1, 1), ("l1.conv2", 56, 64, 64, 3, 1), ("l1.conv3", 56, 64, 256, 1, 1),
    ("l2.0.conv1", 56, 256, 128, 1, 1), ("l2.0.conv2", 56, 128, 128, 3, 2),
    ("l2.conv1", 28, 512, 128, 1, 1), ("l2.conv2", 28, 128, 128, 3, 1), ("l2.conv3", 28, 128, 512, 1, 1),
    ("l3.0.conv1", 28, 512, 256, 1, 1), ("l3.0.conv2", 28, 256, 256, 3, 2),
    ("l3.conv1", 14, 1024, 256, 1, 1), ("l3.conv2", 14, 256, 256, 3, 1), ("l3.conv3", 14, 256, 1024, 1, 1),
    ("l4.0.conv1", 14, 1024, 512, 1, 1), ("l4.0.conv2", 14, 512, 512, 3, 2),
    ("l4.conv1", 7, 2048, 512, 1, 1), ("l4.conv2", 7, 512, 512, 3, 1), ("l4.conv3", 7, 512, 2048, 1, 1),
]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(name, F, h, c, k, r, stride, reps, dev):
    gen = torch.Generator().manual_seed(1)
    pad = r // 2
    ho = (h + 2 * pad - r) // stride + 1
    x = torch.randn(F, h, h, c, generator=gen).to(dev)
    y = torch.randn(F, ho, ho, k, generator=gen).to(dev)
    g = torch.randn(F, ho, ho, k, generator=gen).to(dev)
    g = g * (y > 0)
    nparts = (F * ho * ho + 127) // 128
    parts = torch.randn(nparts, k, 2, generator=gen).to(dev)
    mean = torch.zeros(k, device=dev)
    inv = torch.ones(k, device=dev)
    gam = torch.ones(k, device=dev)

    def two():
        dy, _, _ = ops.bn_bwd_parts(g, y, parts, nparts, mean, inv, gam)
        ops.conv_wgrad(x, dy, r, r, stride, pad)

    def fused():
        coef, _, _ = ops.bn_bwd_parts_coef(y, parts, nparts, mean, inv, gam)
        ops.conv_wgrad_bnbwd(x, g, y, coef, r, r, stride, pad)

    ok = ops.conv_wgrad_bnbwd_ok(x, g, y, r, r, stride, pad)
    row = {"unit": name, "frames": F, "h": h, "c": c, "k": k, "r": r, "stride": stride,
           "served": bool(ok), "two_ms": round(timed(two, reps), 4)}
    if ok:
        row["fused_ms"] = round(timed(fused, reps), 4)
        row["gain_ms"] = round(row["two_ms"] - row["fused_ms"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=640)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for s in SHAPES:
        rows.append(run(s[0], args.frames, *s[1:], args.reps, dev))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
