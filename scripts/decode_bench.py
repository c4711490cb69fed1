"""Throughput of the frames-from-files stage: files -> decoded -> HBM ->
tmr_resize_u8 (Resize((250, 250)), train_only_non-local_pretrained.py:336), next to the train
step's consumption rate.

Variants, each at every --workers count:
  threads    decode_frames: pil_loader (:96-99) in a thread pool into a pinned batch
  processes  DecodePool: pil_loader in worker processes into a pinned shared-memory batch
  device     tmrnet_amd.jpeg.DeviceJpegDecoder: entropy decode in threads, the rest in jpeg.hip
  device_entropy  the same with entropy="device": the threads only pack the scans, the Huffman
             decode runs in jpeg_entropy.hip
`processes` and `device` submit batch i + 1 before they take batch i (their submit / result
pairs), `threads` has no such pair and runs batch after batch.

Protocol (DESIGN.md §18's): one warm-up of every variant, then --rounds rounds in which the
variants run alternately, all in this process tree; per variant the median frames/s to the resized
device batch and spread = (max - min) / median.  `device` also reports its host pass alone
(entropy decode into pinned memory, no copy, no kernels) and the time of the reconstruction
kernels per frame from device events; `device_entropy` splits that time into the entropy and the
reconstruction kernels and adds the median and maximum number of re-decode rounds a frame needed.
The last lines compare `device` and `device_entropy` with `processes`, and `device_entropy` with
`device`, at the largest worker count of the same run.  --out appends every line to a file
(profiles/jpeg_decode/entropy.jsonl holds the run DESIGN.md §25 quotes).

Synthetic JPEGs (smooth colour field + noise, quality 95, written to a temp dir) at Cholec80's
native 854x480 and at a pre-resized 250x250.  One JSON line per (size, variant, workers)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_jpegs(d, n, w, h, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    paths = []
    for i in range(n):
        base = np.stack([(xx * (1 + i % 5) + yy) % 256, (yy * 2 + i * 7) % 256,
                         (xx + yy * 3 + i * 13) % 256], -1).astype(np.float32)
        img = np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
        p = os.path.join(d, "%05d.jpg" % i)
        Image.fromarray(img).save(p, quality=95)
        paths.append(p)
    return paths


class Variant:
    """One (mode, workers): run(paths, batches) -> the last resized device batch (or host batch
    without a GPU)."""

    def __init__(self, mode, nw, dev):
        from tmrnet_amd import frames
        self.mode, self.nw, self.dev, self.frames = mode, nw, dev, frames
        self.pool = self.dec = None
        if mode == "processes":
            self.pool = frames.DecodePool(workers=nw)
        elif mode in ("device", "device_entropy"):
            from tmrnet_amd.jpeg import DeviceJpegDecoder
            self.dec = DeviceJpegDecoder(workers=nw, device=dev,
                                         entropy="device" if mode == "device_entropy" else "host")

    def _finish(self, dev_batch):
        if tuple(dev_batch.shape[1:3]) == tuple(self.frames.RESIZE):
            return dev_batch
        return self.frames.resize_frames(dev_batch)

    def run(self, paths, batches):
        if self.mode == "threads":
            for _ in range(batches):
                out = self.frames.load_frames(paths, device=self.dev, workers=self.nw)
            return out
        src = self.pool if self.mode == "processes" else self.dec
        job = src.submit(paths)
        for b in range(batches):
            nxt = src.submit(paths) if b + 1 < batches else None
            out = self._finish(job.to(self.dev) if self.mode == "processes" else job.result())
            job = nxt
        return out

    def close(self):
        if self.pool is not None:
            self.pool.close()
        if self.dec is not None:
            self.dec.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=640, help="one C2 step's frames per batch")
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workers", default="8,16")
    ap.add_argument("--sizes", default="854x480,250x250")
    ap.add_argument("--modes", default="threads,processes,device,device_entropy")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench: the resized batch lives on the device; no GPU is visible")
    dev = torch.device("cuda:0")
    workers = [int(v) for v in args.workers.split(",")]
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        with tempfile.TemporaryDirectory() as d:
            paths = write_jpegs(d, args.frames, w, h)
            mb = sum(os.path.getsize(p) for p in paths) / 1e6
            variants = [Variant(m, nw, dev) for m in args.modes.split(",") for nw in workers]
            try:
                for v in variants:          # warm: page cache, worker processes, pinned buffers
                    v.run(paths, 1)
                torch.cuda.synchronize()
                rates = {id(v): [] for v in variants}
                for _ in range(args.rounds):
                    for v in variants:
                        t0 = time.perf_counter()
                        out = v.run(paths, args.batches)
                        torch.cuda.synchronize()
                        dt = time.perf_counter() - t0
                        assert tuple(out.shape) == (args.frames, 250, 250, 3)
                        rates[id(v)].append(args.frames * args.batches / dt)
                summary = {}
                for v in variants:
                    r = sorted(rates[id(v)])
                    med = float(np.median(r))
                    rec = {"stage": "frames-from-files", "mode": v.mode, "size": size,
                           "workers": v.nw, "frames": args.frames, "batches": args.batches,
                           "rounds": args.rounds, "jpeg_mb": round(mb, 1),
                           "frames_per_s": round(med, 1), "min": round(r[0], 1), "max": round(r[-1], 1),
                           "spread_pct": round(100 * (r[-1] - r[0]) / med, 2),
                           "host_cpus": len(os.sched_getaffinity(0))}
                    if v.dec is not None:
                        hp = []
                        for _ in range(args.rounds):
                            t0 = time.perf_counter()
                            nbytes = v.dec.host_pass(paths)
                            hp.append(args.frames / (time.perf_counter() - t0))
                        rec["host_pass_frames_per_s"] = round(float(np.median(hp)), 1)
                        rec["upload_bytes_per_frame"] = nbytes // args.frames
                        v.dec.kernel_events, v.dec.entropy_events, v.dec.entropy_rounds = [], [], []
                        for _ in range(args.rounds):
                            v.dec.decode(paths)
                        torch.cuda.synchronize()
                        ms = [a.elapsed_time(b) for a, b in v.dec.kernel_events]
                        v.dec.kernel_events = None
                        rec["kernels_us_per_frame"] = round(1e3 * float(np.median(ms)) / args.frames, 3)
                        if v.dec.entropy_events:
                            ems = [a.elapsed_time(b) for a, b in v.dec.entropy_events]
                            e_us = 1e3 * float(np.median(ems)) / args.frames
                            rec["entropy_kernels_us_per_frame"] = round(e_us, 3)
                            rec["reconstruct_kernels_us_per_frame"] = round(
                                rec["kernels_us_per_frame"] - e_us, 3)
                            rec["rounds_median"] = float(np.median(v.dec.entropy_rounds))
                            rec["rounds_max"] = int(max(v.dec.entropy_rounds))
                        rec["entropy_device_frames"] = v.dec.stats["entropy_device"]
                        rec["device_frames"] = v.dec.stats["device"]
                        rec["fallback_frames"] = v.dec.stats["fallback"]
                    summary[(v.mode, v.nw)] = rec
                    emit(rec)
                top = max(workers)
                for x, y in (("device", "processes"), ("device_entropy", "processes"),
                             ("device_entropy", "device")):
                    a, b = summary.get((x, top)), summary.get((y, top))
                    if a and b:
                        gain = 100 * (a["frames_per_s"] / b["frames_per_s"] - 1)
                        noise = max(a["spread_pct"], b["spread_pct"])
                        emit({"stage": "frames-from-files", "size": size, "workers": top,
                              "%s_over_%s_pct" % (x, y): round(gain, 2), "larger_spread_pct": noise,
                              "verdict": "gain" if gain > noise else
                                         ("loss" if -gain > noise else "no difference")})
            finally:
                for v in variants:
                    v.close()


if __name__ == "__main__":
    main()
