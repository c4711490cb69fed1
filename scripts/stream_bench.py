"""Online recognition latency on one MI355X: what a live caller pays per pushed frame.

Workload: `--streams` live videos of seeded uint8 250x250x3 frames (a pool resident in HBM, read
round-robin), random-init ``resnet_lstm`` + ``resnet_lstm_LFB`` (`--backbone`, `--precision`).  Geometry A: T = 10, L = 40;
B: T = 30, L = 300.  A tick is one new frame for every stream; the host synchronises after every
tick, because an online caller reads each answer.

Variants (run alternately in one process, `--rounds` rounds of `--ticks` ticks after the rings
are full):
  a  the public modules alone: per tick ``model_lfb`` and ``model`` run on the last T frames of
     every stream, with a dense ``long_feature`` assembled from the rows kept so far
     (`--ticks-a` ticks a round: every frame is encoded T times by each model)
  b  ``OnlineRecognizer(window="steps")``
  c  ``OnlineRecognizer(window="kernel")``
  d  ``OnlineRecognizer(window="kernel", activations=--activations)``: the bf16-activation trunk
     of the backbone ("bf16" for resnet50, "bf16-resnest" for resnest50; needs --precision bf16)
One JSON line per variant (median per-tick latency and ticks/s over the rounds' medians, spread =
(max - min) / median), for (b) and (c) the phases of a tick (device events between the phases, one
extra round), and a summary line with b/a, c/b and d/c.

``--kernel-table stats.csv`` instead prints the top-kernel table of a
``rocprofv3 --kernel-trace --stats`` run of one variant (``--variants c --rounds 1``).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

GEOMETRY = {"A": (10, 40), "B": (30, 300)}
NAMES = {"a": "public modules on the last T frames, dense long_feature",
         "b": "OnlineRecognizer window=steps",
         "c": "OnlineRecognizer window=kernel",
         "d": "OnlineRecognizer window=kernel, bf16 activations"}
PHASES = ("input", "trunks", "projection", "recurrences", "head")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=sorted(GEOMETRY), default="A")
    ap.add_argument("--streams", type=int, default=1)
    ap.add_argument("--backbone", choices=("resnet50", "resnest50"), default="resnet50")
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--activations", default=None,
                    help="variant d's activations (default: the backbone's bf16 value)")
    ap.add_argument("--variants", default="a,b,c")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--ticks-a", type=int, default=None, help="ticks a round of variant a")
    ap.add_argument("--pool", type=int, default=64, help="distinct frames per stream")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--kernel-table", default=None, metavar="STATS_CSV")
    ap.add_argument("--top", type=int, default=12)
    args = ap.parse_args()
    if args.kernel_table:
        from eval_bench import kernel_table
        return kernel_table(args.kernel_table, args.top)

    import numpy as np
    import torch
    import tmrnet_amd
    from tmrnet_amd import lfb, lfb_build, ops
    from tmrnet_amd.stream import OnlineRecognizer

    dev = torch.device("cuda:0")
    T, L = GEOMETRY[args.geometry]
    S = args.streams
    variants = [v for v in args.variants.split(",") if v]
    ticks = {v: (args.ticks_a or args.ticks) if v == "a" else args.ticks for v in variants}
    g = torch.Generator().manual_seed(1)
    pool = torch.randint(0, 256, (args.pool, S, 250, 250, 3), generator=g, dtype=torch.uint8).to(dev)
    torch.manual_seed(0)
    kw = {"backbone": args.backbone, "precision": args.precision}
    model = tmrnet_amd.resnet_lstm(seq_len=T, **kw).to(dev).eval()
    model_lfb = tmrnet_amd.resnet_lstm_LFB(seq_len=T, **kw).to(dev).eval()
    act_d = args.activations or ("bf16-resnest" if args.backbone == "resnest50" else "bf16")

    class ModulesLoop:
        """Variant a.  Bank rows are kept per stream in one device tensor that grows by a row a
        tick; the last T frames of every stream are re-encoded by both models."""

        def __init__(self):
            self.n = 0
            self.rows = torch.rand(S, L, 512, generator=g).to(dev) * 2 - 1   # as if L ticks ran
            self.off = torch.full((S, 2), lfb_build.center_offset(250), dtype=torch.int32,
                                  device=dev)

        @torch.no_grad()
        def tick(self):
            idx = [(self.n + j) % args.pool for j in range(T)]
            clip = pool[idx].transpose(0, 1).reshape(S * T, 250, 250, 3).contiguous()
            self.n += 1
            x4 = ops.crop_normalize(clip, self.off, T)
            row = model_lfb(x4)                                        # (S, 512)
            self.rows = torch.cat([self.rows, row.reshape(S, 1, 512)], 1)
            s = self.rows.shape[1] - 1
            tab = lfb.lfb_row_table(np.arange(s + 1), [s], L)[0]       # newest first
            lt = self.rows[:, torch.from_numpy(tab).to(dev)].contiguous()
            probs, scores, preds = ops.softmax_max(model(x4, lt).contiguous())
            if self.rows.shape[1] > 4 * L:
                self.rows = self.rows[:, -L - 1:].contiguous()
            return preds

    class RecLoop:
        def __init__(self, window, activations="fp32"):
            self.rec = OnlineRecognizer(model, model_lfb, L, streams=S, window=window,
                                        activations=activations)
            self.n = 0
            for _ in range(T + L + 2):                                 # fill both rings
                self.tick()

        def tick(self):
            out = self.rec.push(pool[self.n % args.pool])
            self.n += 1
            return out["preds"]

    loops = {}
    for v in variants:
        loops[v] = (ModulesLoop() if v == "a" else RecLoop("kernel", act_d) if v == "d"
                    else RecLoop("steps" if v == "b" else "kernel"))

    def timed_round(v):
        """Per-tick host latency (push to answer on the host), seconds."""
        lat = []
        loop = loops[v]
        torch.cuda.synchronize()
        for _ in range(ticks[v]):
            t0 = time.perf_counter()
            loop.tick()
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t0)
        return float(np.median(lat)), float(np.percentile(lat, 99))

    def phase_round(v):
        """Device time between the phase marks of a tick, median over the ticks (ms)."""
        rec = loops[v].rec
        acc = {p: [] for p in PHASES}
        for _ in range(min(ticks[v], 100)):
            evs = []

            def mark(name):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                evs.append((name, e))

            rec.mark = mark
            mark("start")
            loops[v].tick()
            rec.mark = None
            torch.cuda.synchronize()
            per = {p: 0.0 for p in PHASES}
            for (_, e0), (name, e1) in zip(evs[:-1], evs[1:]):
                per[name] += e0.elapsed_time(e1)
            for p in PHASES:
                acc[p].append(per[p])
        return {p: round(float(np.median(acc[p])), 4) for p in PHASES}

    for v in variants:                      # warm-up: every shape of every variant
        for _ in range(3):
            loops[v].tick()
        torch.cuda.synchronize()
    med = {v: [] for v in variants}
    p99 = {v: [] for v in variants}
    for _ in range(args.rounds):
        for v in variants:
            m, p = timed_round(v)
            med[v].append(m)
            p99[v].append(p)
    lines, mid = [], {}
    for v in variants:
        mid[v] = float(np.median(med[v]))
        ln = {"geometry": args.geometry, "backbone": args.backbone, "precision": args.precision,
              "seq_len": T, "lfb_length": L, "streams": S,
              "variant": v, "name": NAMES[v], "ticks_per_round": ticks[v],
              "round_median_ms": [round(1e3 * m, 4) for m in med[v]],
              "round_p99_ms": [round(1e3 * m, 4) for m in p99[v]],
              "tick_ms": round(1e3 * mid[v], 4), "ticks_per_s": round(1.0 / mid[v], 1),
              "frames_per_s": round(S / mid[v], 1),
              "spread_pct": round(100 * (max(med[v]) - min(med[v])) / mid[v], 2),
              "data": "synthetic (%d uint8 250x250x3 frames per stream in HBM, random-init "
                      "weights)" % args.pool}
        if v != "a":
            ln["phase_ms"] = phase_round(v)
        lines.append(ln)

    def ratio(x, y):
        return round(mid[y] / mid[x], 3) if {x, y} <= set(mid) else "not measured"

    lines.append({"geometry": args.geometry, "backbone": args.backbone,
                  "precision": args.precision, "streams": S, "summary": True,
                  "b_over_a_ticks_per_s": ratio("b", "a"), "c_over_b_ticks_per_s": ratio("c", "b"),
                  "d_over_c_ticks_per_s": ratio("d", "c")})
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
