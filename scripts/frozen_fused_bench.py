"""Train-step time and peak memory of the frozen-BatchNorm step with BN folded into the conv
forward (tmrnet_amd.freeze_bn(model, affine=False, forward="fused")) beside its unfused partner,
for both backwards, on one MI355X.

The legs and the protocol are scripts/step_bench.py's (bench.py's own step and resident inputs;
5 untimed + 20 timed steps per leg, 3 rounds alternating the legs in one process; the median and
spread = (max - min) / median per leg, torch.cuda.max_memory_allocated of its legs):

  fp32 frozen no-affine              freeze_bn(model, affine=False)
  fp32 frozen no-affine fused        freeze_bn(model, affine=False, forward="fused")
  bf16-bwd frozen no-affine          freeze_bn(model, affine=False, backward="bf16")
  bf16-bwd frozen no-affine fused    freeze_bn(model, affine=False, backward="bf16", forward="fused")

  python scripts/frozen_fused_bench.py --config C2 --out profiles/frozen_fused/step_C2.jsonl

`--legs` selects legs by name (comma separated): a `rocprofv3 --kernel-trace --stats` run of one
leg (`--legs "bf16-bwd frozen no-affine fused" --rounds 1 --no-prof`) gives the per-kernel table
through `scripts/step_bench.py --kernel-table`.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import step_bench  # noqa: E402


def _freeze(backward, forward):
    def prepare(model):
        import tmrnet_amd
        tmrnet_amd.freeze_bn(model, affine=False, backward=backward, forward=forward)
    return prepare


LEGS = [("fp32 frozen no-affine", "fp32", _freeze(None, None)),
        ("fp32 frozen no-affine fused", "fp32", _freeze(None, "fused")),
        ("bf16-bwd frozen no-affine", "bf16-bwd", _freeze("bf16", None)),
        ("bf16-bwd frozen no-affine fused", "bf16-bwd", _freeze("bf16", "fused"))]


def main():
    ap = argparse.ArgumentParser()
    step_bench.add_protocol_args(ap)
    ap.add_argument("--legs", default=",".join(n for n, _, _ in LEGS))
    args = ap.parse_args()
    names = [n for n in args.legs.split(",") if n]
    known = {spec[0]: spec for spec in LEGS}
    for n in names:
        if n not in known:
            raise SystemExit("unknown leg %r (have: %s)" % (n, ", ".join(known)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    step_bench.run_legs(args, [known[n] for n in names])


if __name__ == "__main__":
    main()
