"""What the black-margin cut costs on one MI355X.

Synthetic frames: a bright textured disc on black plus 3% salt noise, at 854x480 and 1920x1080.
Per size, after a warm-up, `--rounds` alternating rounds; each figure is the median over the
rounds' medians, spread = (max - min) / median:

  margin_boxes        us per frame of ``frames.margin_boxes`` on a batch resident in HBM
                      (device events around `--reps` calls)
  resize dense/boxed  us per frame of ``resize_frames`` to 250 x 250 without and with boxes (the
                      boxed call includes its host read of the boxes and the table upload)
  load_frames         us per frame of ``load_frames(paths, decoder=DeviceJpegDecoder())`` with and
                      without ``cut_margin`` on the same JPEG files (host wall time, synchronised)

``--stream`` instead times the ``OnlineRecognizer`` tick at one stream with and without
``cut_margin`` (scripts/stream_bench.py's protocol: host latency per synchronised tick, rings full,
alternating rounds) on bordered 250 x 250 frames.  One JSON line per figure, appended to `--out`.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"854x480": (480, 854), "1920x1080": (1080, 1920)}
GEOMETRY = {"A": (10, 40), "B": (30, 300)}


def disc_frames(n, h, w, seed, salt=0.03):
    import numpy as np
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((n, h, w, 3), dtype=np.uint8)
    for i in range(n):
        cy, cx = h * (0.48 + 0.04 * rng.random()), w * (0.48 + 0.04 * rng.random())
        inside = (yy - cy) ** 2 + (xx - cx) ** 2 <= (0.47 * h) ** 2
        tex = rng.integers(60, 256, size=(h, w, 3), dtype=np.uint8)
        out[i][inside] = tex[inside]
        s = rng.random((h, w)) < salt
        out[i][s] = rng.integers(128, 256, size=(int(s.sum()), 3), dtype=np.uint8)
    return out


def summary(name, per_round, unit, **extra):
    import numpy as np
    mid = float(np.median(per_round))
    ln = {"figure": name, "rounds": [round(v, 3) for v in per_round], unit: round(mid, 3),
          "spread_pct": round(100 * (max(per_round) - min(per_round)) / mid, 2)}
    ln.update(extra)
    return ln


def bench_size(args, name, emit):
    import numpy as np
    import torch
    from PIL import Image
    from tmrnet_amd import frames
    from tmrnet_amd.jpeg import DeviceJpegDecoder

    dev = torch.device("cuda:0")
    h, w = SIZES[name]
    n = args.frames
    x = disc_frames(n, h, w, seed=h)
    xd = torch.from_numpy(x).to(dev)
    boxes = frames.margin_boxes(xd)
    info = {"size": name, "frames": n, "first_box": boxes[0].tolist(),
            "data": "synthetic (bright disc on black, 3% salt)"}
    ws = torch.empty((frames.query("tmr_margin_ws_bytes", n, h, w) + 7) // 8, dtype=torch.int64,
                     device=dev)

    def device_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / (args.reps * n)

    def host_us(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / (reps * n)

    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for i in range(n):
            p = os.path.join(tmp, "%04d.jpg" % i)
            Image.fromarray(x[i], "RGB").save(p, quality=90)
            paths.append(p)
        dec = DeviceJpegDecoder()
        variants = {
            "margin_boxes": lambda: device_us(lambda: frames.margin_boxes(xd, ws=ws)),
            "resize_dense": lambda: host_us(lambda: frames.resize_frames(xd), args.reps),
            "resize_boxed": lambda: host_us(lambda: frames.resize_frames(xd, boxes=boxes), args.reps),
            "load_frames": lambda: host_us(lambda: frames.load_frames(paths, decoder=dec), 2),
            "load_frames_cut_margin": lambda: host_us(
                lambda: frames.load_frames(paths, decoder=dec, cut_margin=True), 2),
        }
        for fn in variants.values():          # warm-up: every shape, table and buffer
            fn()
        rounds = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                rounds[k].append(fn())
    mid = {}
    for k in variants:
        ln = summary(k, rounds[k], "us_per_frame", **info)
        mid[k] = ln["us_per_frame"]
        emit(ln)
    emit({"summary": True, "size": name,
          "cut_margin_extra_us_per_frame": round(mid["load_frames_cut_margin"] - mid["load_frames"], 3),
          "boxed_minus_dense_resize_us_per_frame": round(mid["resize_boxed"] - mid["resize_dense"], 3)})


def bench_stream(args, emit):
    import numpy as np
    import torch
    import tmrnet_amd
    from tmrnet_amd.stream import OnlineRecognizer

    dev = torch.device("cuda:0")
    T, L = GEOMETRY[args.geometry]
    pool = torch.from_numpy(disc_frames(args.pool, 250, 250, seed=1)).to(dev)
    torch.manual_seed(0)
    model = tmrnet_amd.resnet_lstm(seq_len=T).to(dev).eval()
    model_lfb = tmrnet_amd.resnet_lstm_LFB(seq_len=T).to(dev).eval()

    class Loop:
        def __init__(self, cut):
            self.rec = OnlineRecognizer(model, model_lfb, L, window="kernel", cut_margin=cut)
            self.n = 0
            for _ in range(T + L + 5):        # fill both rings, warm every shape
                self.tick()

        def tick(self):
            i = self.n % args.pool
            self.n += 1
            return self.rec.push(pool[i:i + 1])["preds"]

    loops = {"plain": Loop(False), "cut_margin": Loop(True)}

    def timed_round(loop):
        lat = []
        torch.cuda.synchronize()
        for _ in range(args.ticks):
            t0 = time.perf_counter()
            loop.tick()
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(lat))

    rounds = {k: [] for k in loops}
    for _ in range(args.rounds):
        for k, loop in loops.items():
            rounds[k].append(timed_round(loop))
    mid = {}
    for k in loops:
        ln = summary("stream_tick_" + k, rounds[k], "tick_ms", geometry=args.geometry, seq_len=T,
                     lfb_length=L, streams=1, ticks_per_round=args.ticks,
                     data="synthetic (bordered 250x250 frames in HBM, random-init fp32 weights)")
        mid[k] = (ln["tick_ms"], ln["spread_pct"])
        emit(ln)
    diff = 100 * (mid["cut_margin"][0] - mid["plain"][0]) / mid["plain"][0]
    emit({"summary": True, "geometry": args.geometry, "cut_margin_over_plain_pct": round(diff, 2),
          "beyond_both_spreads": bool(abs(diff) > mid["plain"][1] + mid["cut_margin"][1])})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="854x480,1920x1080")
    ap.add_argument("--frames", type=int, default=16, help="frames per batch")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--geometry", choices=sorted(GEOMETRY), default="A")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--pool", type=int, default=64)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    def emit(ln):
        print(json.dumps(ln), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(ln) + "\n")

    if args.stream:
        return bench_stream(args, emit)
    for name in [s for s in args.sizes.split(",") if s]:
        bench_size(args, name, emit)


if __name__ == "__main__":
    main()
