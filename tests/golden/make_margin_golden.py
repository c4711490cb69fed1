"""Writes tests/golden/margin_cases.npz: for the disc-plus-salt frames of tests/_margin_emu.py
(every shape of SHAPES, seeds 0..2) the seed, the shape, the expected box and the SHA-256 of the
mask after the median.  The file pins the emulation: tests/test_margin_cpu.py compares the
emulation with it, tests/test_margin_gpu.py compares the kernels with both.

    python tests/golden/make_margin_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _margin_emu as emu  # noqa: E402

SEEDS = (0, 1, 2)


def main():
    seeds, shapes, boxes, shas = [], [], [], []
    for h, w in emu.SHAPES:
        for seed in SEEDS:
            f = emu.disc_frame(h, w, seed)
            seeds.append(seed)
            shapes.append((h, w))
            boxes.append(emu.box(f))
            shas.append(emu.mask_sha(f))
    out = os.path.join(HERE, "margin_cases.npz")
    np.savez_compressed(out, seeds=np.array(seeds, np.int32), shapes=np.array(shapes, np.int32),
                        boxes=np.array(boxes, np.int32), mask_sha256=np.array(shas))
    for s, hw, b in zip(seeds, shapes, boxes):
        print(hw, s, b)


if __name__ == "__main__":
    main()
