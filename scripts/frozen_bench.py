"""Train-step time and peak memory of the frozen-BatchNorm steps (tmrnet_amd.freeze_bn) beside
their yardsticks on one MI355X, one family of legs per run (`--family`):

  bn      the fp32 frozen step beside the "fp32" step
            fp32                        the batch-statistics step (the yardstick)
            fp32 frozen affine          freeze_bn(model): BN weights and biases still train
            fp32 frozen no-affine       freeze_bn(model, affine=False)
  bwd16   bf16 backward convs, beside the "bf16-bwd" step
            bf16-bwd                    the batch-statistics step with bf16 backward convs
            bf16-bwd frozen             freeze_bn(model, backward="bf16"): BN weights, biases train
            bf16-bwd frozen no-affine   freeze_bn(model, affine=False, backward="bf16")
  fused   BN folded into the conv forward, beside its unfused partner, for both backwards
            fp32 frozen no-affine              freeze_bn(model, affine=False)
            fp32 frozen no-affine fused        freeze_bn(model, affine=False, forward="fused")
            bf16-bwd frozen no-affine          freeze_bn(model, affine=False, backward="bf16")
            bf16-bwd frozen no-affine fused    freeze_bn(model, affine=False, backward="bf16",
                                                         forward="fused")

The legs and the protocol are scripts/step_bench.py's (bench.py's own step and resident inputs;
5 untimed + 20 timed steps per leg, 3 rounds alternating the legs in one process; the median and
spread = (max - min) / median per leg, torch.cuda.max_memory_allocated of its legs):

  python scripts/frozen_bench.py --family bn --config C2 --out profiles/frozen_bn/step_C2.jsonl
  python scripts/frozen_bench.py --family bwd16 --config C2 --out profiles/frozen_bwd16/step_C2.jsonl
  python scripts/frozen_bench.py --family fused --config C2 --out profiles/frozen_fused/step_C2.jsonl

`--legs` selects legs by name (comma separated): a `rocprofv3 --kernel-trace --stats` run of one
leg (`--family bn --legs "fp32 frozen affine" --rounds 1 --no-prof`) gives the per-kernel table
through `scripts/step_bench.py --kernel-table`.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import step_bench  # noqa: E402


def _freeze(**kw):
    def prepare(model):
        import tmrnet_amd
        tmrnet_amd.freeze_bn(model, **kw)
    return prepare


# family -> [(leg name, trunk precision, prepare)]
LEGS = {
    "bn": [("fp32", "fp32", None),
           ("fp32 frozen affine", "fp32", _freeze(affine=True)),
           ("fp32 frozen no-affine", "fp32", _freeze(affine=False))],
    "bwd16": [("bf16-bwd", "bf16-bwd", None),
              ("bf16-bwd frozen", "bf16-bwd", _freeze(affine=True, backward="bf16")),
              ("bf16-bwd frozen no-affine", "bf16-bwd", _freeze(affine=False, backward="bf16"))],
    "fused": [("fp32 frozen no-affine", "fp32", _freeze(affine=False)),
              ("fp32 frozen no-affine fused", "fp32", _freeze(affine=False, forward="fused")),
              ("bf16-bwd frozen no-affine", "bf16-bwd", _freeze(affine=False, backward="bf16")),
              ("bf16-bwd frozen no-affine fused", "bf16-bwd",
               _freeze(affine=False, backward="bf16", forward="fused"))],
}


def main():
    ap = argparse.ArgumentParser()
    step_bench.add_protocol_args(ap)
    ap.add_argument("--family", choices=sorted(LEGS), required=True)
    ap.add_argument("--legs", default=None, help="legs of the family by name (default: all)")
    args = ap.parse_args()
    known = {spec[0]: spec for spec in LEGS[args.family]}
    names = [n for n in args.legs.split(",") if n] if args.legs else list(known)
    for n in names:
        if n not in known:
            raise SystemExit("unknown leg %r (have: %s)" % (n, ", ".join(known)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    step_bench.run_legs(args, [known[n] for n in names])


if __name__ == "__main__":
    main()
