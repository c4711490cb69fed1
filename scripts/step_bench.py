"""Train-step time of the three trunk precisions on one MI355X: "fp32", "bf16-bwd" (the fp32
forward with bf16 operands in the backward convs only, tmrnet_amd/trunk.py BWD16) and "bf16".

The step is bench.py's own (its synthetic resident inputs, `bench.synth_inputs`; the train
transform or crop + normalize -> LFB rows -> forward -> CE-sum -> backward -> SGD with the
reference's parameter groups), at C2 (64 clips x 10 frames, L = 40) or C5 (64 x 30, L = 300).
bench.py's `--precision` choices are fixed, so the new value is measured here.

Protocol: `--rounds` rounds (3), each running every precision's leg in turn inside one process:
`--warmup` (5) untimed + `--steps` (20) timed steps, timed by device events around the timed
steps.  Per precision one JSON line: the median over the rounds of ms/step and frames/s, spread =
(max - min) / median, torch.cuda.max_memory_allocated of its legs, and the per-view conv times
(ops.PROF) of one instrumented step after the timed region.  A leg that runs out of memory is
recorded as such.  `--out FILE` also appends the lines to FILE.

`--kernel-table STATS_CSV` instead prints the per-kernel table of a
`rocprofv3 --kernel-trace --stats` run of one leg (`--precisions bf16-bwd --rounds 1 --no-prof`):
ms per step, share, launches per step and, for the BatchNorm / pooling passes whose bytes per
element are known, the algorithmic GB/s at `--config`'s frame count (no counters involved).
"""
import argparse
import csv
import json
import os
import statistics
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

CONFIGS = {"C2": (64, 10, 40), "C5": (64, 30, 300)}   # clips, frames per clip, LFB length
PRECISIONS = ("fp32", "bf16-bwd", "bf16")


# ---------------------------------------------------------------- kernel table
def _elements(frames):
    """Per frame-batch element counts of ResNet-50's BatchNorm outputs at 224x224 -> dict:
    block (16 block outputs), ds (the 4 downsample blocks' outputs), inner (bn1 / bn2 outputs),
    stem (the stem conv's output), pooled (the maxpool's)."""
    n = dict(block=0, ds=0, inner=0, stem=frames * 112 * 112 * 64, pooled=frames * 56 * 56 * 64)
    hw = 56
    for planes, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
        for b in range(blocks):
            s = stride if b == 0 else 1
            n["inner"] += frames * hw * hw * planes           # bn1's output
            hw //= s
            n["inner"] += frames * hw * hw * planes           # bn2's
            n["block"] += frames * hw * hw * planes * 4
            if b == 0:
                n["ds"] += frames * hw * hw * planes * 4
    return n


def kernel_table(path, frames, top):
    """Families the bf16-bwd step's elementwise passes run in, with their algorithmic bytes per
    step: (elements, bytes per element).  bn_bwd_apply8_k: every unit but the downsample blocks'
    two and the last block's bn3 (fp32 g, y in, bf16 dy out)."""
    from pmc_summary import family
    from top_kernels import pretty
    e = _elements(frames)
    last = frames * 7 * 7 * 2048
    alg = {"bn_apply_bits8_k": e["block"] * (4 + 4 + 4 + 2 + 0.125),
           "bn_apply_dual8_k": e["inner"] * (4 + 4 + 2),
           "bn_bwd_apply_ds8": e["ds"] * (3 * 4 + 2 * 2),
           "bn_bwd_apply8_k": (e["inner"] + e["block"] - e["ds"] - last) * (4 + 4 + 2),
           "maxpool_fwd_bn8": e["stem"] * 4 + e["pooled"] * (4 + 2 + 1),
           "stem_bwd_apply8q": e["stem"] * (4 + 2) + e["pooled"] * (4 + 1)}
    ns, calls, steps = defaultdict(float), defaultdict(int), 0
    with open(path) as f:
        for r in csv.DictReader(f):
            fam = pretty(family(r["Name"]))
            ns[fam] += float(r["TotalDurationNs"])
            calls[fam] += int(r["Calls"])
            if fam == "sgd_multi_k":
                steps += int(r["Calls"])
    if steps == 0:
        raise SystemExit("no sgd_multi_k launches: cannot count the profiled steps")
    tot = sum(ns.values()) / steps / 1e6
    print("%d profiled steps at %d frames, %.1f ms of kernels per step" % (steps, frames, tot))
    print()
    print("| kernel family | ms / step | share | launches / step | algorithmic GB/s |")
    print("|---|---|---|---|---|")
    for fam in sorted(ns, key=lambda k: -ns[k])[:top]:
        ms = ns[fam] / steps / 1e6
        gbs = "%.0f" % (alg[fam] / (ms * 1e-3) / 1e9) if fam in alg and ms > 0 else "-"
        print("| `%s` | %.2f | %.1f%% | %.0f | %s |" % (fam, ms, 100 * ms / tot,
                                                     calls[fam] / steps, gbs))


# ---------------------------------------------------------------- the legs
def add_protocol_args(ap):
    ap.add_argument("--config", choices=sorted(CONFIGS), default="C2")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--augment", choices=["reference", "crop"], default="reference",
                    help="bench.py's --augment (its default: the reference train transform)")
    ap.add_argument("--no-prof", action="store_true", help="skip the instrumented step")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")


def main():
    ap = argparse.ArgumentParser()
    add_protocol_args(ap)
    ap.add_argument("--precisions", default=",".join(PRECISIONS))
    ap.add_argument("--kernel-table", default=None, metavar="STATS_CSV")
    ap.add_argument("--top", type=int, default=16)
    args = ap.parse_args()
    clips, T, L = CONFIGS[args.config]
    if args.kernel_table:
        kernel_table(args.kernel_table, clips * T, args.top)
        return
    precs = [p for p in args.precisions.split(",") if p]
    for p in precs:
        if p not in PRECISIONS:
            raise SystemExit("unknown precision %r" % p)
    run_legs(args, [(p, p, None) for p in precs])


def run_legs(args, specs):
    """The protocol above over `specs` = [(leg name, trunk precision, prepare)]: prepare(model),
    when given, runs on the leg's fresh train-mode model before its optimizer is built (other
    benchmarks' legs: scripts/frozen_bench.py).  One JSON line per leg, its name under
    "precision"."""
    clips, T, L = CONFIGS[args.config]
    import torch
    import bench
    import tmrnet_amd
    from tmrnet_amd import ops, LFBRows
    from tmrnet_amd.augment import ClipAugment
    from tmrnet_amd.optim import sgd_param_groups

    precs = [name for name, _, _ in specs]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    per_leg = args.warmup + args.steps
    nsteps = args.rounds * per_leg + 1
    inp = argparse.Namespace(clips=clips, seq=T, lfb=L, warmup=0, steps=nsteps)
    frames, bank, vs_d, offs, starts, labels = bench.synth_inputs(inp, 0, 1, dev)
    aug = ClipAugment(seq_len=T, use_flip=1) if args.augment == "reference" else None
    crit = tmrnet_amd.CrossEntropyLoss(size_average=False)
    lr = 5e-7   # bench.py's (the reference default)

    legs = {}
    for p, trunk_precision, prepare in specs:
        torch.manual_seed(0)
        model = tmrnet_amd.resnet_lstm(seq_len=T, precision=trunk_precision).to(dev).train()
        if prepare is not None:
            prepare(model)
        opt = tmrnet_amd.SGD(sgd_param_groups(model, lr), lr=lr / 10, momentum=0.9,
                             weight_decay=5e-4)
        legs[p] = dict(model=model, opt=opt, ms=[], mem=0, oom=False, i=0)

    def step(leg):
        i = leg["i"]
        leg["i"] += 1
        leg["opt"].zero_grad(set_to_none=True)
        if aug is not None:
            x4 = aug(frames[i % len(frames)])
        else:
            x4 = ops.crop_normalize(frames[i % len(frames)], offs[i], T)
        rows = ops.lfb_index(vs_d, starts[i], L)
        loss = crit(leg["model"](x4, LFBRows(bank, rows)), labels[i])
        loss.backward()
        leg["opt"].step()
        return loss

    for _ in range(args.rounds):
        for p in precs:
            leg = legs[p]
            if leg["oom"]:
                continue
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            try:
                for _ in range(args.warmup):
                    step(leg)
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    loss = step(leg)
                e1.record()
                torch.cuda.synchronize()
            except torch.cuda.OutOfMemoryError:
                leg["oom"] = True
                leg["opt"].zero_grad(set_to_none=True)
                torch.cuda.empty_cache()
                continue
            leg["ms"].append(e0.elapsed_time(e1) / args.steps)
            leg["mem"] = max(leg["mem"], torch.cuda.max_memory_allocated(dev))
            leg["loss"] = float(loss.item())
            del loss
            leg["opt"].zero_grad(set_to_none=True)   # the next leg starts without this one's grads
            torch.cuda.empty_cache()

    fh = open(args.out, "a") if args.out else None
    for p in precs:
        leg = legs[p]
        rec = {"config": args.config, "clips": clips, "seq": T, "lfb": L, "precision": p,
               "augment": args.augment, "rounds": args.rounds, "warmup": args.warmup,
               "steps": args.steps, "oom": leg["oom"]}
        if leg["ms"]:
            med = statistics.median(leg["ms"])
            rec.update(ms_per_step=round(med, 3), frames_per_s=round(clips * T / med * 1e3, 1),
                       spread=round((max(leg["ms"]) - min(leg["ms"])) / med, 4),
                       ms_rounds=[round(v, 3) for v in leg["ms"]],
                       max_memory_allocated=leg["mem"], last_loss=leg["loss"])
        if leg["ms"] and not leg["oom"] and not args.no_prof:
            ops.PROF = []
            torch.cuda.synchronize()
            step(leg)
            torch.cuda.synchronize()
            recs, ops.PROF = ops.PROF, None
            views = {}
            for kind, fl, a, b, _, _ in recs:
                v = views.setdefault(kind, {"launches": 0, "ms": 0.0, "flops": 0.0})
                v["launches"] += 1
                v["ms"] += a.elapsed_time(b)
                v["flops"] += fl
            rec["conv_views"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 2),
                                     "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1)}
                                 for k, v in views.items()}
            leg["opt"].zero_grad(set_to_none=True)
            torch.cuda.empty_cache()
        line = json.dumps(rec)
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()
    if fh:
        fh.close()


if __name__ == "__main__":
    main()
