"""Per-launch A/B of the fp32 wgrad that produces its dy operand (tmr_conv2d_wgrad_bnbwd) against
the two calls it replaces, over the conv+BN units of the fp32 ResNet-50 step whose masked gradient
comes from a fused dgrad (the shapes of profiles/r6/fwd_epilogue/c2_table.txt).  Per shape:

  two   = bn_bwd_parts (reduction + apply pass writing dy) + conv_wgrad
  fused = bn_bwd_parts_coef (reduction only) + conv_wgrad_bnbwd (dy produced on load, written once)

in ms, and whether the library serves the fused form at all.

Then the four downsample blocks (DS_BLOCKS), whose bn3 and downsample BN share one gradient g:

  dual  = bn_bwd_parts_ds (two reductions + one apply writing dy3 and dy_ds) + two conv_wgrads
  fold  = bn_bwd_parts_ds_coef (reductions only) + two conv_wgrad_bnbwds
  half3 / halfd = bn_bwd_parts_ds_coef with bn3's / the downsample BN's dy applied separately + one
          plain and one fused wgrad (the form for a block with one unserved unit)

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


# (block, conv3 input h (= output h), mid channels, output channels k, block input h, block input
# channels, downsample stride)
DS_BLOCKS = [
    ("l1.0", 56, 64, 256, 56, 64, 1), ("l2.0", 28, 128, 512, 56, 256, 2),
    ("l3.0", 14, 256, 1024, 28, 512, 2), ("l4.0", 7, 512, 2048, 14, 1024, 2),
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


def run_ds(name, F, ho, mid, k, hin, cin, stride, reps, dev):
    gen = torch.Generator().manual_seed(1)
    x3 = torch.randn(F, ho, ho, mid, generator=gen).to(dev)
    xd = torch.randn(F, hin, hin, cin, generator=gen).to(dev)
    y3 = torch.randn(F, ho, ho, k, generator=gen).to(dev)
    yd = torch.randn(F, ho, ho, k, generator=gen).to(dev)
    g = torch.randn(F, ho, ho, k, generator=gen).to(dev)
    g = g * (y3 > 0)
    nparts = (F * ho * ho + 127) // 128
    parts = torch.randn(nparts, k, 2, generator=gen).to(dev)
    mean = torch.zeros(k, device=dev)
    inv = torch.ones(k, device=dev)
    gam = torch.ones(k, device=dev)
    bargs = (g, y3, parts, nparts, mean, inv, gam, yd, mean, inv, gam)

    def dual():
        r = ops.bn_bwd_parts_ds(*bargs)
        ops.conv_wgrad(x3, r[0], 1, 1, 1, 0)
        ops.conv_wgrad(xd, r[3], 1, 1, stride, 0)

    def fold():
        r = ops.bn_bwd_parts_ds_coef(*bargs)
        ops.conv_wgrad_bnbwd(x3, g, y3, r[0], 1, 1, 1, 0)
        ops.conv_wgrad_bnbwd(xd, g, yd, r[3], 1, 1, stride, 0)

    def half3():   # bn3 applied separately, the downsample wgrad fused
        r = ops.bn_bwd_parts_ds_coef(*bargs, apply3=True)
        ops.conv_wgrad(x3, r[6], 1, 1, 1, 0)
        ops.conv_wgrad_bnbwd(xd, g, yd, r[3], 1, 1, stride, 0)

    def halfd():   # the downsample BN applied separately, conv3's wgrad fused
        r = ops.bn_bwd_parts_ds_coef(*bargs, applyd=True)
        ops.conv_wgrad_bnbwd(x3, g, y3, r[0], 1, 1, 1, 0)
        ops.conv_wgrad(xd, r[7], 1, 1, stride, 0)

    ok3 = bool(ops.conv_wgrad_bnbwd_ok(x3, g, y3, 1, 1, 1, 0))
    okd = bool(ops.conv_wgrad_bnbwd_ok(xd, g, yd, 1, 1, stride, 0))
    row = {"block": name, "frames": F, "elements": g.numel(), "served3": ok3, "servedd": okd,
           "cfg3": ops.conv_tile(F, ho, ho, mid, k, 1, 1, 1, 0, "wgrad")["cfg"],
           "cfgd": ops.conv_tile(F, hin, hin, cin, k, 1, 1, stride, 0, "wgrad")["cfg"],
           "dual_ms": round(timed(dual, reps), 4)}
    if ok3 and okd:
        row["fold_ms"] = round(timed(fold, reps), 4)
    if okd:
        row["half3_ms"] = round(timed(half3, reps), 4)
    if ok3:
        row["halfd_ms"] = round(timed(halfd, reps), 4)
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
    for b in DS_BLOCKS:
        rows.append(run_ds(b[0], args.frames, *b[1:], args.reps, dev))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
