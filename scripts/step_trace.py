"""Launch trace and result digests of one seeded trunk step per step kind, on one MI355X.

A tool for changes to the host logic of the trunk steps (tmrnet_amd/trunk.py, resnest.py) that
must leave the launches and the bits alone.  For each kind below it builds a fresh seeded share,
wraps `ops.call` and `resnest.call` by a recorder, runs one step (4 frames of 64x64, seeded as
tests/test_wgrad_bnbwd_gpu.py::test_wgrad_bnbwd_step_bit_identical does; a kind whose extras carry
"input": (frames, side) runs that size instead) and prints one JSON line:

  kind      the kind's name
  calls     the number of library calls
  trace     sha256 over the ordered calls: entry name and every non-address argument (integers,
            floats, the fields of descriptor structs, 0/1 for an absent / present tensor)
  names     the distinct entry names in order of first use; "order" indexes it, call by call
  digests   sha256 of the feature tensor, of every parameter gradient and of every buffer, folded
            into one sha256 each for "feat", "grads" and "buffers" (`--full`: every tensor's own)
  peak      torch.cuda.max_memory_allocated of the step, and the bytes allocated before it

Run it before and after the change and compare the files line by line (`--diff A B` does, and
says which field of which kind differs); `--dump KIND` writes the kind's full call list instead.

`--host-bench` times the host-bound case instead: eval-mode `features_nhwc4` of one 224x224
frame (ResNet-50 fp32 and infer_act16, ResNeSt-50 infer_act16), 20 warm-up calls, then `--rounds`
rounds of 200 calls each ended by a device synchronise; one JSON line per case with the median.

  python scripts/step_trace.py --out profiles/trunk_units/head.jsonl
  python scripts/step_trace.py --diff profiles/trunk_units/parent_a.jsonl profiles/trunk_units/head.jsonl
"""
import argparse
import contextlib
import ctypes
import gc
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# ---------------------------------------------------------------- the kinds
# (name, backbone, precision, mode, {trunk switch: value}, extras)
# mode: "train" (forward + backward), "nograd" (train-mode forward under no_grad), "eval"
# extras: "freeze": the keywords of tmrnet_amd.freeze_bn; "input": (frames, side) where the kind
# refuses the default 4 frames of 64x64
def _frozen(precision, affine, backward=None, forward=None, mode="train"):
    fz = {"affine": affine}
    if backward:
        fz["backward"] = backward
    if forward:
        fz["forward"] = forward
    name = "r50 %s frozen %s" % (precision, " ".join("%s=%s" % kv for kv in fz.items()))
    if mode == "nograd":
        name += " no_grad"
    return (name, "resnet50", precision, mode, {}, {"freeze": fz})


def _kinds():
    R, S = "resnet50", "resnest50"
    B, F = "bf16", "fused"
    return [
        ("r50 fp32 train", R, "fp32", "train", {}, {}),
        ("r50 fp32 train WGRAD_BNBWD_DS_MIN=0", R, "fp32", "train", {"WGRAD_BNBWD_DS_MIN": 0}, {}),
        ("r50 fp32 train WGRAD_BNBWD=False", R, "fp32", "train", {"WGRAD_BNBWD": False}, {}),
        ("r50 fp32 train DS_DUAL=False", R, "fp32", "train", {"DS_DUAL": False}, {}),
        ("r50 fp32 train no_grad", R, "fp32", "nograd", {}, {}),
        ("r50 bf16 train", R, "bf16", "train", {}, {}),
        ("r50 bf16 train engine_only", R, "bf16", "train", {}, {"engine_only": True}),
        ("r50 bf16 train ACT16=False", R, "bf16", "train", {"ACT16": False}, {}),
        ("r50 bf16 train FULL16=False G16=False", R, "bf16", "train",
         {"FULL16": False, "G16": False}, {}),
        ("r50 bf16 train FULL16=False G16=False BF16_STORE=False", R, "bf16", "train",
         {"FULL16": False, "G16": False, "BF16_STORE": False}, {}),
        ("r50 bf16-bwd train", R, "bf16-bwd", "train", {}, {}),
        _frozen("fp32", True),
        _frozen("fp32", False),
        _frozen("fp32", True, B),
        _frozen("fp32", False, B),
        _frozen("bf16-bwd", True, B),
        _frozen("fp32", False, None, F),
        _frozen("fp32", False, B, F),
        _frozen("bf16-bwd", False, B, F),
        _frozen("fp32", True, mode="nograd"),
        # (without a backward to record the forward is the unfused one)
        _frozen("fp32", False, None, F, mode="nograd"),
        ("r50 fp32 eval", R, "fp32", "eval", {}, {}),
        ("r50 bf16 eval", R, "bf16", "eval", {}, {}),
        ("r50 bf16 eval infer_act16", R, "bf16", "eval", {}, {"infer_act16": True}),
        ("rs50 fp32 train", S, "fp32", "train", {}, {}),
        ("rs50 bf16 train", S, "bf16", "train", {}, {}),
        ("rs50 fp32 eval", S, "fp32", "eval", {}, {}),
        ("rs50 bf16 eval infer_act16", S, "bf16", "eval", {}, {"infer_act16": True}),
    ]


def _make_share(backbone, precision, dev):
    import torch
    from tmrnet_amd import trunk, resnest
    torch.manual_seed(0)
    cls = trunk.ResNet50Share if backbone == "resnet50" else resnest.ResNeSt50Share
    return cls(precision=precision).to(dev)


# ---------------------------------------------------------------- the recorder
def _plain(v):
    """A ctypes value as JSON: integers / floats as they are, arrays as lists."""
    if isinstance(v, ctypes.Array):
        return [_plain(e) for e in v]
    return v


def _arg(a, typ):
    import torch
    from tmrnet_amd import _lib
    if typ is _lib.P:   # an address: present or not
        if isinstance(a, torch.Tensor):
            return 1
        if isinstance(a, ctypes.c_void_p):
            return int(bool(a.value))
        return int(bool(a))
    obj = getattr(a, "_obj", None)   # ctypes.byref(struct)
    if isinstance(obj, ctypes.Structure):
        if all(f[1] is ctypes.c_void_p for f in obj._fields_):   # a table of addresses
            return {f[0]: int(bool(getattr(obj, f[0]))) for f in obj._fields_}
        return {f[0]: _plain(getattr(obj, f[0])) for f in obj._fields_}
    if obj is not None:
        return 1
    if isinstance(a, (bool, int, float)):
        return a
    return getattr(a, "value", repr(type(a)))


@contextlib.contextmanager
def _recording(log):
    from tmrnet_amd import ops, resnest, _lib

    def wrap(real):
        def rec(name, *args):
            types = _lib.SIGNATURES[name]
            log.append([name] + [_arg(a, t) for a, t in zip(args, types)])
            return real(name, *args)
        return rec
    saved = ops.call, resnest.call
    ops.call, resnest.call = wrap(saved[0]), wrap(saved[1])
    try:
        yield
    finally:
        ops.call, resnest.call = saved


def _sha(t):
    import torch
    raw = t.detach().contiguous().reshape(-1).view(torch.uint8)
    return hashlib.sha256(raw.cpu().numpy().tobytes()).hexdigest()


def _fold(d):
    h = hashlib.sha256()
    for k in sorted(d):
        h.update(("%s=%s\n" % (k, d[k])).encode())
    return h.hexdigest()


def run_kind(spec, dev, full=False, dump=None):
    import torch
    import tmrnet_amd
    from tmrnet_amd import ops, trunk
    name, backbone, precision, mode, switches, extra = spec
    gen = torch.Generator().manual_seed(3)
    frames, side = extra.get("input", (4, 64))
    x4 = torch.randn(frames, side, side, 4, generator=gen).to(dev)
    x4[..., 3] = 0
    w = torch.randn(frames, 2048, generator=gen).to(dev)
    saved = {k: getattr(trunk, k) for k in switches}
    log = []
    try:
        for k, v in switches.items():
            setattr(trunk, k, v)
        share = _make_share(backbone, precision, dev)
        share.train(mode != "eval")
        if "freeze" in extra:
            tmrnet_amd.freeze_bn(share, **extra["freeze"])
        if extra.get("infer_act16"):
            share.infer_act16 = True
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        with contextlib.ExitStack() as st:
            if extra.get("engine_only"):
                st.enter_context(ops.engine_only())
            if mode != "train":
                st.enter_context(torch.no_grad())
            st.enter_context(_recording(log))
            feat = share.features_nhwc4(x4)
            if mode == "train":
                (feat * w).sum().backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev)
    finally:
        for k, v in saved.items():
            setattr(trunk, k, v)
    grads = {n: _sha(p.grad) for n, p in share.named_parameters() if p.grad is not None}
    bufs = {n: _sha(b) for n, b in share.named_buffers()}
    names = list(dict.fromkeys(c[0] for c in log))
    index = {n: i for i, n in enumerate(names)}
    out = {"kind": name, "calls": len(log),
           "trace": hashlib.sha256(json.dumps(log, sort_keys=True).encode()).hexdigest(),
           "names": names, "order": [index[c[0]] for c in log],
           "digests": {"feat": _sha(feat), "grads": _fold(grads), "ngrads": len(grads),
                       "buffers": _fold(bufs), "nbuffers": len(bufs)},
           "peak": {"max_memory_allocated": peak, "allocated_before": before}}
    if full:
        out["digests"].update(grad=grads, buffer=bufs)
    if dump:
        with open(dump, "w") as f:
            for c in log:
                f.write(json.dumps(c, sort_keys=True) + "\n")
    del share, feat
    gc.collect()
    torch.cuda.empty_cache()
    return out


# ---------------------------------------------------------------- the host-bound case
def host_bench(dev, rounds, out):
    import torch
    cases = [("r50 fp32 eval 1x224", "resnet50", "fp32", False),
             ("r50 bf16 eval infer_act16 1x224", "resnet50", "bf16", True),
             ("rs50 bf16 eval infer_act16 1x224", "resnest50", "bf16", True)]
    gen = torch.Generator().manual_seed(3)
    x4 = torch.randn(1, 224, 224, 4, generator=gen).to(dev)
    x4[..., 3] = 0
    for name, backbone, precision, i16 in cases:
        share = _make_share(backbone, precision, dev).eval()
        share.infer_act16 = i16
        us = []
        with torch.no_grad():
            for _ in range(20):
                share.features_nhwc4(x4)
            torch.cuda.synchronize()
            for _ in range(rounds):
                t0 = time.perf_counter()
                for _ in range(200):
                    share.features_nhwc4(x4)
                torch.cuda.synchronize()
                us.append((time.perf_counter() - t0) / 200 * 1e6)
        med = statistics.median(us)
        _emit({"case": name, "warmup": 20, "calls": 200, "rounds": rounds,
               "us_per_call": round(med, 2), "us_rounds": [round(v, 2) for v in us],
               "spread": round((max(us) - min(us)) / med, 4)}, out)
        del share


def _emit(rec, out):
    line = json.dumps(rec, sort_keys=True)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def diff(a, b):
    """Compare two outputs kind by kind -> the number of differing kinds."""
    def load(path):
        with open(path) as f:
            return {r["kind"]: r for r in map(json.loads, f) if "kind" in r}
    ra, rb = load(a), load(b)
    bad = 0
    for kind in sorted(set(ra) | set(rb)):
        if kind not in ra or kind not in rb:
            print("%-60s only in %s" % (kind, a if kind in ra else b))
            bad += 1
            continue
        x, y = ra[kind], rb[kind]
        fields = [k for k in ("calls", "trace", "names", "order", "digests", "peak", "error")
                  if x.get(k) != y.get(k)]
        print("%-60s %s" % (kind, "differs: " + ", ".join(fields) if fields else "equal"))
        bad += bool(fields)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default=None, help="comma separated kind names (default: all)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--full", action="store_true", help="every tensor's own digest")
    ap.add_argument("--input", default=None, metavar="FRAMES,SIDE",
                    help="run the chosen kinds at this input size (to find the smallest a kind "
                         "takes); a kind that raises prints its error instead")
    ap.add_argument("--dump", default=None, metavar="KIND",
                    help="write this kind's full call list to --out (one call per line)")
    ap.add_argument("--host-bench", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.diff:
        raise SystemExit(1 if diff(*args.diff) else 0)
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.host_bench:
        host_bench(dev, args.rounds, args.out)
        return
    kinds = _kinds()
    if args.dump:
        spec = [k for k in kinds if k[0] == args.dump]
        if not spec or not args.out:
            raise SystemExit("--dump takes a kind's name and needs --out")
        run_kind(spec[0], dev, dump=args.out)
        return
    if args.kinds:
        want = [k for k in args.kinds.split(",") if k]
        known = {k[0] for k in kinds}
        for k in want:
            if k not in known:
                raise SystemExit("unknown kind %r (have: %s)" % (k, "; ".join(sorted(known))))
        kinds = [k for k in kinds if k[0] in want]
    for spec in kinds:
        if args.input:
            size = tuple(int(v) for v in args.input.split(","))
            spec = spec[:5] + (dict(spec[5], input=size),)
        try:
            _emit(run_kind(spec, dev, full=args.full), args.out)
        except RuntimeError as e:
            if not args.input:
                raise
            _emit({"kind": spec[0], "input": args.input, "error": str(e)}, args.out)


if __name__ == "__main__":
    main()
