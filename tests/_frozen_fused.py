"""Shared pieces of the tests of the frozen-BatchNorm step with BN folded into the conv forward
(tmrnet_amd.freeze_bn(affine=False, forward="fused"); tests/test_frozen_fused_cpu.py, _gpu.py).

The contract (tmrnet_amd/trunk.py "_frozen_fused"): every non-stem unit is one launch
z = [relu](fmaf(acc, scale, shift) [+ residual]); with a bf16 backward the launch also writes
z16 = bf16(z), rounded to nearest even once, after the residual and the ReLU; a dgrad that
produces a unit's gradient masks it by that unit's stored output, z > 0 (z16 > 0).

Three parts:
  * grid_case / emu_dual / compare_dual / compare_mask: operands fp32 holds exactly, a numpy
    emulation of the dual epilogue and the comparisons the GPU tests use;
    tests/test_frozen_fused_cpu.py plants errors in the emulation's outputs to show that the
    comparisons can fail.
  * trunk_convs: the non-stem ResNet-50 convs the step sends to the fused forward.
  * folded(): the float64 frozen oracle with BN folded into the conv as the step folds it."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn

from tests import _bwd16 as H
from tests import _frozen_bn as F
from tests import _frozen_bwd16 as X

rne_bf16, trunc_bf16, half_up_bf16 = H.rne_bf16, H.trunc_bf16, X.half_up_bf16
bits16, bits32 = X.bits16, X.bits32


def widen(b):
    """uint16 bf16 bit patterns -> the fp32 values they stand for."""
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


# ---------------------------------------------------------------- the dual epilogue
def grid_case(rows, c, seed, res=True):
    """An epilogue case on exact grids (float64 arrays that fp32 holds exactly): acc -- what the
    conv accumulates -- integers / 16 in [-64, 64]; scale +-2^-j (j = 0..3), shift on the 1/16
    grid: fmaf(acc, scale, shift) is exact in fp32.  Planted, where the residual allows it:
      column 0: pre-activations that are exact bf16 ties of both parities (scale 1, shift 0,
                residual 0; the odd rows' kept mantissa ends in 1, the even rows' in 0);
      column 1: fmaf(acc, scale, shift) == 0 exactly on every fourth row (the ReLU's argument is
                zero without a residual);
      column 2: a residual that cancels the pre-activation to zero on every fourth row."""
    g = np.random.default_rng(seed)
    acc = g.integers(-1024, 1025, (rows, c)) / 16.0
    scale = (2.0 ** -g.integers(0, 4, c)) * np.where(g.random(c) < 0.5, -1.0, 1.0)
    shift = g.integers(-64, 65, c) / 16.0
    r = g.integers(-256, 257, (rows, c)) / 16.0 if res else None
    # ties: 1.xxxxxxx1 / 1.xxxxxxx0 followed by the half bit, exponents near 1 (needs c >= 3)
    scale[0], shift[0] = 1.0, 0.0
    acc[:, 0] = X.ties(g, rows, 0).astype(np.float64)
    acc[1::2, 0] = X.ties(g, rows, 1)[1::2].astype(np.float64)
    scale[1] = 0.5
    acc[::4, 1] = -shift[1] / scale[1]
    if res:
        r[:, 0] = 0.0
        r[::4, 1] = 0.0
        r[::4, 2] = -(acc[::4, 2] * scale[2] + shift[2])
    k = dict(acc=acc, scale=scale, shift=shift, res=r)
    for v in k.values():
        assert v is None or np.array_equal(v, v.astype(np.float32).astype(np.float64))
    return k


def emu_dual(k, relu=True, copy="after"):
    """-> (z fp32, z16 uint16 bit patterns) of one case.  copy: "after" (the contract: the copy is
    of the stored z), "pre_relu" / "pre_res" (planted: the copy taken before the ReLU / before the
    residual add)."""
    v = k["acc"] * k["scale"] + k["shift"]
    assert np.array_equal(v, v.astype(np.float32).astype(np.float64))   # the fmaf is exact
    pre_res = v
    if k["res"] is not None:
        v = (v.astype(np.float32) + k["res"].astype(np.float32)).astype(np.float64)
    pre_relu = v
    if relu:
        v = np.maximum(v, 0.0)
    z = v.astype(np.float32)
    src = {"after": z, "pre_relu": pre_relu.astype(np.float32),
           "pre_res": (np.maximum(pre_res, 0.0) if relu else pre_res).astype(np.float32)}[copy]
    return z, rne_bf16(src)


def compare_dual(z, z16, ref_z):
    """A dual launch's outputs (numpy: z fp32, z16 uint16 bit patterns) against the reference z
    (fp32, bit for bit) -> list of what differs.  z16 is always held to RNE of the z it came with."""
    bad = []
    if np.isnan(z).any():
        bad.append("z has NaN")
    if not np.array_equal(bits32(z), bits32(ref_z)):
        bad.append("z != reference")
    if not np.array_equal(np.asarray(z16, np.uint16), rne_bf16(z)):
        bad.append("z16 != RNE(z)")
    return bad


def compare_mask(dx, full, z):
    """A masked dgrad's dx against the unmasked dgrad `full` and the stored output z (numpy,
    widened to fp32): dx must be full where z > 0 and exactly 0 elsewhere -> list of what
    differs."""
    want = np.where(np.asarray(z, np.float32) > 0, full, np.float32(0)).astype(np.float32)
    bad = []
    if not np.array_equal(bits32(np.abs(dx)), bits32(np.abs(want))):
        bad.append("dx != where(z > 0, dgrad, 0)")
    return bad


# ---------------------------------------------------------------- routing
def trunk_convs():
    """The non-stem ResNet-50 convs (tests/_bwd16.resnet50_convs rows): the fused forward's."""
    return [c for c in H.resnet50_convs() if c[0] != "stem"]


# ---------------------------------------------------------------- the folded oracle
class _FoldConv(nn.Conv2d):
    """conv + frozen BN as the step folds them: z = conv(x, w) * scale + shift with the
    coefficients of tmr_bn_frozen_params, scale = gamma * inv, shift = beta - mean * scale."""

    def forward(self, x):
        bn = self._bn[0]
        scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
        shift = bn.bias.detach() - bn.running_mean * scale
        y = Fn.conv2d(x, self.weight, None, self.stride, self.padding)
        return y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)


class _FoldBN(nn.BatchNorm2d):
    def forward(self, x):   # (applied inside its conv)
        return x


def folded(r, stem=False):
    """Switch the frozen oracle model r's trunk to folded units (class swaps: parameters, buffers
    and state_dict keys stay); the stem stays conv + BN unless `stem`."""
    share = r.share
    blocks = [b for n in ("layer1", "layer2", "layer3", "layer4") for b in getattr(share, n)]
    units = [(share.conv1, share.bn1)] if stem else []
    for b in blocks:
        units += [(b.conv1, b.bn1), (b.conv2, b.bn2), (b.conv3, b.bn3)]
        if b.downsample is not None:
            units.append((b.downsample[0], b.downsample[1]))
    assert len(units) == (53 if stem else 52)
    for conv, bn in units:
        assert not bn.training
        conv.__class__ = _FoldConv
        conv._bn = (bn,)   # (a tuple: the BN is not registered a second time)
        bn.__class__ = _FoldBN
    return r


def bn_names(named_parameters):
    return {n for n, _ in named_parameters
            if n.startswith("share.") and (".bn" in n or ".downsample.1." in n)}
