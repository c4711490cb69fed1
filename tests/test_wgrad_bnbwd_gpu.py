"""The fp32 wgrad that produces its dy operand from the BatchNorm backward's coefficients while
loading it (tmr_conv2d_wgrad_bnbwd; gemm16_kernel.h BNW) against the two calls it replaces.

Kernel level: tmr_bn_bwd_parts (dy, dgamma, dbeta) + tmr_conv2d_wgrad (dW) -- both pinned to
float64 by test_bn_f64_gpu.py / test_kernels_gpu.py -- against the coefficient-only backward
(tmr_bn_bwd_parts_x without dy) + the fused wgrad.  The fused kernel evaluates bn_bwd_apply8_k's
expression per element and reduces in the plain wgrad's k order and split plan, so everything must
match bit for bit; tmr_wgrad_bnbwd_launches tells that the fused kernel ran.  Step level: the fp32
ResNet-50 trunk train step with trunk.WGRAD_BNBWD on and off.
Reference: the backward of torchvision Bottleneck's conv + BatchNorm2d units that
code/Training TMRNet/train_only_non-local_pretrained.py:724-725 (loss.backward) runs.
"""
import ctypes

import pytest
import torch

from tmrnet_amd import ops
from tmrnet_amd._lib import lib

pytestmark = pytest.mark.gpu


def _launches():
    return int(lib().tmr_wgrad_bnbwd_launches())


def _operands(dev, frames, h, c, k, r, stride, seed=7, nparts=5):
    """x, masked g (about half zero), y and the (sum g, sum g*(y - mean)) partials of g."""
    gen = torch.Generator().manual_seed(seed)
    ho = (h + 2 * (r // 2) - r) // stride + 1
    x = torch.randn(frames, h, h, c, generator=gen).to(dev)
    y = (torch.randn(frames, ho, ho, k, generator=gen) * 1.5 + 0.25).to(dev)
    g = torch.randn(frames, ho, ho, k, generator=gen).to(dev)
    g = g * (torch.rand(frames, ho, ho, k, generator=gen).to(dev) > 0.5)
    y2, g2 = y.view(-1, k), g.view(-1, k)
    mean = y2.mean(0)
    inv = 1.0 / torch.sqrt(y2.var(0, unbiased=False) + 1e-5)
    gamma = (torch.rand(k, generator=gen) + 0.5).to(dev)
    rows = y2.shape[0]
    parts = torch.zeros(nparts, k, 2, device=dev)
    step = (rows + nparts - 1) // nparts
    for p in range(nparts):
        gs, ys = g2[p * step:(p + 1) * step], y2[p * step:(p + 1) * step]
        parts[p, :, 0] = gs.sum(0)
        parts[p, :, 1] = (gs * (ys - mean)).sum(0)
    return x, g, y, parts.contiguous(), nparts, mean, inv, gamma


# (name, r, stride, h, frames, c, k): the smallest shapes that reach each path of the fused form
CASES = [
    ("a", 1, 1, 14, 11, 64, 64),     # 64x64 tile, >= 2 splits, last split partial (2,156 rows)
    ("b", 1, 1, 14, 11, 64, 256),    # N <= 64 rule, four m-tiles
    ("c", 1, 1, 7, 45, 256, 128),    # 128x128 eight-wave tile; 2,205 rows, no multiple of 32
    ("d", 3, 1, 14, 11, 128, 128),   # multi-tap, several n-tiles: only n-tile 0 writes dy
    ("e", 3, 2, 14, 45, 128, 128),   # strided
    ("f", 1, 1, 7, 2, 64, 64),       # one split, fewer rows than one k-tile past the first
    ("g", 1, 1, 14, 11, 256, 64),    # 64x256 tile (64 output channels, 64 < N < 512)
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_wgrad_bnbwd_vs_two_calls(dev, case):
    _, r, stride, h, frames, c, k = case
    pad = r // 2
    x, g, y, parts, nparts, mean, inv, gamma = _operands(dev, frames, h, c, k, r, stride)
    dy_ref, dg_ref, db_ref = ops.bn_bwd_parts(g, y, parts, nparts, mean, inv, gamma)
    dw_ref = ops.conv_wgrad(x, dy_ref, r, r, stride, pad)
    torch.cuda.synchronize()
    assert ops.conv_wgrad_bnbwd_ok(x, g, y, r, r, stride, pad)
    n0 = _launches()
    coef, dg, db = ops.bn_bwd_parts_coef(y, parts, nparts, mean, inv, gamma)
    dw, dy = ops.conv_wgrad_bnbwd(x, g, y, coef, r, r, stride, pad)
    torch.cuda.synchronize()
    assert _launches() == n0 + 1
    assert torch.equal(dg, dg_ref) and torch.equal(db, db_ref)
    assert torch.equal(dy, dy_ref)
    assert torch.equal(dw, dw_ref)


def test_wgrad_bnbwd_refuses_bf16_operand(dev):
    x, g, y, parts, nparts, mean, inv, gamma = _operands(dev, 2, 7, 64, 64, 1, 1)
    n0 = _launches()
    assert not ops.conv_wgrad_bnbwd_ok(x.to(torch.bfloat16), g, y, 1, 1, 1, 0, math="bf16")
    assert not ops.conv_wgrad_bnbwd_ok(x, g, y, 1, 1, 1, 0, math="bf16")
    d = ops.conv_desc(2, 7, 7, 64, 64, 1, 1, 1, 0, math="bf16", io=ops.IO_X)
    assert lib().tmr_conv2d_wgrad_bnbwd_ok(ctypes.byref(d), None, None, None, None) == 0
    assert _launches() == n0


def test_wgrad_bnbwd_refuses_groups(dev):
    x, g, y, parts, nparts, mean, inv, gamma = _operands(dev, 2, 7, 64, 64, 1, 1)
    n0 = _launches()
    assert not ops.conv_wgrad_bnbwd_ok(x, g, y, 1, 1, 1, 0, groups=2)
    assert _launches() == n0


def test_wgrad_bnbwd_refuses_misaligned(dev):
    x, g, y, parts, nparts, mean, inv, gamma = _operands(dev, 2, 7, 64, 64, 1, 1)
    n0 = _launches()
    buf = torch.zeros(g.numel() + 4, device=dev)
    g1 = buf[1:1 + g.numel()].view(g.shape)   # 4 bytes past a 16-B boundary
    g1.copy_(g)
    assert g1.data_ptr() % 16 == 4
    assert not ops.conv_wgrad_bnbwd_ok(x, g1, y, 1, 1, 1, 0)
    coef, _, _ = ops.bn_bwd_parts_coef(y, parts, nparts, mean, inv, gamma)
    with pytest.raises(RuntimeError, match="no fused form"):   # the call never falls back
        ops.conv_wgrad_bnbwd(x, g1, y, coef, 1, 1, 1, 0)
    torch.cuda.synchronize()
    assert _launches() == n0


def test_wgrad_bnbwd_step_bit_identical(dev):
    """The fp32 ResNet-50 trunk train step (2 clips x 2 frames of 64x64) with the fused wgrads
    and with the separate apply passes: features, every gradient, every buffer bit-identical.

    Covered units: every conv+BN unit whose masked gradient comes from a fused dgrad.  Of the
    16 Bottlenecks each conv1 and conv2 has one (32); so has conv3 of the blocks without a
    downsample (12) but for the last block, whose gradient comes from the average pool (11); the
    four downsample blocks' bn3 goes through tmr_bn_bwd_parts_ds, the stem through the maxpool
    backward.  At this size no wgrad reaches the 100-GFLOP rule of the 256x256 tile, and fp32
    has no direct wgrad kernel: 32 + 11 = 43."""
    from tmrnet_amd import trunk
    covered = 16 + 16 + (16 - 4 - 1)
    gen = torch.Generator().manual_seed(3)
    x4 = torch.randn(4, 64, 64, 4, generator=gen).to(dev)
    x4[..., 3] = 0
    w = torch.randn(4, 2048, generator=gen).to(dev)
    res = {}
    saved = trunk.WGRAD_BNBWD
    try:
        for on in (True, False):
            trunk.WGRAD_BNBWD = on
            torch.manual_seed(0)
            share = trunk.ResNet50Share(precision="fp32").to(dev).train()
            n0 = _launches()
            feat = share.features_nhwc4(x4)
            (feat * w).sum().backward()
            torch.cuda.synchronize()
            assert _launches() - n0 == (covered if on else 0)
            res[on] = (feat.detach().clone(),
                       {n: p.grad.clone() for n, p in share.named_parameters()},
                       {n: b.clone() for n, b in share.named_buffers()})
    finally:
        trunk.WGRAD_BNBWD = saved
    assert torch.equal(res[True][0], res[False][0])
    assert len(res[True][1]) > 100
    for n in res[True][1]:
        assert torch.equal(res[True][1][n], res[False][1][n]), n
    for n in res[True][2]:
        assert torch.equal(res[True][2][n], res[False][2][n]), n
