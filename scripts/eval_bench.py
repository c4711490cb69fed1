"""Split-evaluation throughput on one MI355X: the per-clip loop against the single-pass evaluator,
and the bf16-math eval trunk with fp32 against bf16 activations.

Workload: `--videos` synthetic videos of `--frames` seeded uint8 250x250x3 frames resident in HBM,
random-init ``resnet_lstm`` models, a random bank.  Geometry A: T = 10, L = 40; B: T = 30, L = 300.

Variants (run alternately in one process, `--rounds` rounds after one warm-up of each):
  a  ``PhaseEvaluator`` per-clip loop, 64 clips a batch, fp32 (the reference's loop structure;
     timed on `--per-clip-batches` batches, its clips/s is that sample's)
  b  ``evaluate_split`` fp32
  c  ``evaluate_split`` bf16 math, fp32 activations
  d  ``evaluate_split`` bf16 math, activations="bf16" (``--backbone resnest50``: "bf16-resnest")
Timing: device events around each run, then a synchronise.  One JSON line per variant (median
clips/s and encoded frames/s over the rounds, min / max as the spread) and a summary line with
the ratios b/a (expectation: near T * N_clips / N_frames) and d/c.

``--kernel-table stats.csv`` instead prints the top-kernel table of a
``rocprofv3 --kernel-trace --stats`` run of one variant (``--variants c --rounds 1``).
"""
import argparse
import csv
import json
import os
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

GEOMETRY = {"A": (10, 40), "B": (30, 300)}
NAMES = {"a": "PhaseEvaluator per-clip loop, 64 clips/batch, fp32",
         "b": "evaluate_split fp32",
         "c": "evaluate_split bf16 math, fp32 activations",
         "d": "evaluate_split bf16 math, bf16 activations"}


def kernel_table(path, top):
    from pmc_summary import family
    from top_kernels import pretty
    ns, calls = defaultdict(float), defaultdict(int)
    with open(path) as f:
        for r in csv.DictReader(f):
            fam = family(r["Name"])
            ns[fam] += float(r["TotalDurationNs"])
            calls[fam] += int(r["Calls"])
    tot = sum(ns.values())
    print("%.1f ms of kernels in the profiled run, %d launches" % (tot / 1e6, sum(calls.values())))
    print()
    print("| kernel family | ms | share | launches |")
    print("|---|---:|---:|---:|")
    for fam in sorted(ns, key=ns.get, reverse=True)[:top]:
        print("| %s | %.2f | %.1f%% | %d |" % (pretty(fam), ns[fam] / 1e6, 100 * ns[fam] / tot,
                                              calls[fam]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=sorted(GEOMETRY), default="A")
    ap.add_argument("--backbone", choices=("resnet50", "resnest50"), default="resnet50")
    ap.add_argument("--videos", type=int, default=2)
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--variants", default="a,b,c,d")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--per-clip-batches", type=int, default=4)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--kernel-table", default=None, metavar="STATS_CSV")
    ap.add_argument("--top", type=int, default=12)
    args = ap.parse_args()
    if args.kernel_table:
        return kernel_table(args.kernel_table, args.top)

    import numpy as np
    import torch
    import tmrnet_amd
    from tmrnet_amd import evaluate, lfb_build, ops
    from tmrnet_amd.lfb import LongFeatureBank, get_useful_start_idx

    dev = torch.device("cuda:0")
    T, L = GEOMETRY[args.geometry]
    variants = [v for v in args.variants.split(",") if v]
    lengths = [args.frames] * args.videos
    n_frames = sum(lengths)
    valid = get_useful_start_idx(T, lengths)
    g = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (n_frames, 250, 250, 3), generator=g, dtype=torch.uint8).to(dev)
    labels = torch.randint(0, 7, (n_frames,), generator=g).to(dev)
    bank = LongFeatureBank(torch.rand(len(valid), 512, generator=g) * 2 - 1, valid, L, dev)
    models = {}
    for prec, users in (("fp32", {"a", "b"}), ("bf16", {"c", "d"})):
        if users & set(variants):
            torch.manual_seed(0)
            models[prec] = tmrnet_amd.resnet_lstm(seq_len=T, precision=prec,
                                                  backbone=args.backbone).to(dev).eval()

    B = 64
    nb = max(1, min(args.per_clip_batches, len(valid) // B))
    off = torch.full((B, 2), lfb_build.center_offset(250), dtype=torch.int32, device=dev)

    def run_a():
        ev = evaluate.PhaseEvaluator(models["fp32"], bank)
        for i in range(nb):
            starts = valid[i * B:(i + 1) * B]
            idx = torch.tensor([s + j for s in starts for j in range(T)], device=dev)
            x4 = ops.crop_normalize(frames.index_select(0, idx), off, T)
            ev.step(x4, labels.index_select(0, idx), clip_starts=starts)
        ev.result()
        return nb * B, nb * B * T

    def split(prec, act):
        def run():
            r = evaluate.evaluate_split(models[prec], bank, frames, lengths, labels, activations=act)
            return r["clips"], r["frames_encoded"]
        return run

    runs = {"a": run_a, "b": split("fp32", "fp32"), "c": split("bf16", "fp32"),
            "d": split("bf16", "bf16-resnest" if args.backbone == "resnest50" else "bf16")}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        clips, enc = fn()
        e1.record()
        torch.cuda.synchronize()
        return clips, enc, e0.elapsed_time(e1) / 1e3

    for v in variants:           # warm-up: every shape of every variant
        timed(runs[v])
    secs = {v: [] for v in variants}
    count = {}
    for _ in range(args.rounds):
        for v in variants:
            clips, enc, s = timed(runs[v])
            secs[v].append(s)
            count[v] = (clips, enc)
    lines = []
    med = {}
    for v in variants:
        clips, enc = count[v]
        cps = sorted(clips / s for s in secs[v])
        med[v] = float(np.median(cps))
        lines.append({"geometry": args.geometry, "backbone": args.backbone, "seq_len": T,
                      "lfb_length": L, "variant": v,
                      "name": NAMES[v], "clips": clips, "frames_encoded": enc,
                      "seconds": [round(s, 4) for s in secs[v]],
                      "clips_per_s": round(med[v], 1), "clips_per_s_min": round(cps[0], 1),
                      "clips_per_s_max": round(cps[-1], 1),
                      "frames_encoded_per_s": round(med[v] * enc / clips, 1),
                      "spread_pct": round(100 * (cps[-1] - cps[0]) / med[v], 2),
                      "data": "synthetic (%d videos x %d uint8 250x250x3 frames in HBM, "
                              "random-init weights)" % (args.videos, args.frames)})
    summary = {"geometry": args.geometry, "backbone": args.backbone, "summary": True,
               "expected_b_over_a": round(T * len(valid) / n_frames, 2),
               "b_over_a": round(med["b"] / med["a"], 2) if {"a", "b"} <= set(med) else "not measured",
               "d_over_c": round(med["d"] / med["c"], 3) if {"c", "d"} <= set(med) else "not measured"}
    lines.append(summary)
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
