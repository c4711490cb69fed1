"""The bf16-activation inference path: tmr_conv2d_fwd_fused with TMR_IO_Y_BF16 (bf16 residual in,
one RNE rounding, bf16 y out) and the ResNet-50 eval trunk built on it
(ResNet50Share.infer_act16)."""
import pytest
import torch

import tmrnet_amd
from tmrnet_amd import ops
from tmrnet_amd.trunk import ResNet50Share
from oracle import tmrnet_ref as ref
from tests._infer16_emu import randomize_bn, hooked_share, features

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16

# (n, h, w, cin, cout, r, stride, pad, max_frames)
CASES_1X1 = [(5, 14, 14, 64, 256, 1), (2, 13, 9, 64, 128, 1), (3, 9, 9, 128, 64, 1),
             (3, 9, 9, 64, 64, 1), (2, 9, 9, 64, 200, 1), (3, 7, 7, 32, 96, 1),
             (2, 12, 12, 64, 512, 2)]   # the cases of test_bf16_gpu.test_gemm16_y16_store_forms
CASES = ([c[:5] + (1, c[5], 0, 0) for c in CASES_1X1]
         + [(2, 9, 9, 64, 64, 3, 1, 1, 0),        # 3x3, pad 1
            (1, 224, 224, 8, 64, 7, 2, 3, 0),     # the NHWC8 stem: k-tiles spanning taps
            (3, 9, 9, 64, 64, 1, 1, 0, 1)])       # one frame per launch (chunked)


def _operands(dev, case):
    n, h, w, cin, cout, r, st, pad, _ = case
    g = torch.Generator().manual_seed(11 + cin + cout + r)
    if cin == 8:   # the stem: 3 real channels, stored 4 -> 8
        wt = torch.randn(cout, 3, r, r, generator=g) / (3 * r * r) ** 0.5
        x4 = torch.randn(n, h, w, 4, generator=g)
        x4[..., 3] = 0
        x16 = ops.nhwc4_to_bf16x8(x4.to(dev))
        w16 = ops.weight_to_krsc(wt.to(dev), cpad=8, bf16=True)
    else:
        wt = torch.randn(cout, cin, r, r, generator=g) / (cin * r * r) ** 0.5
        x16 = torch.randn(n, h, w, cin, generator=g).to(dev).to(BF16)
        w16 = ops.weight_to_krsc(wt.to(dev), bf16=True)
    scale = (torch.rand(cout, generator=g) + 0.5).to(dev)
    shift = (torch.randn(cout, generator=g) * 0.1).to(dev)
    ho = (h + 2 * pad - r) // st + 1
    wo = (w + 2 * pad - r) // st + 1
    res16 = torch.randn(n, ho, wo, cout, generator=g).to(dev).to(BF16)
    return x16, w16, scale, shift, res16


def _both(case, x16, w16, scale, shift, res16, relu):
    """(bf16 output of the new epilogue, fp32 output of the fp32 epilogue) on the same operands."""
    st, pad, mf = case[6], case[7], case[8]
    saved = ops.MAX_FRAMES
    ops.MAX_FRAMES = mf
    try:
        yb = ops.conv_fwd_fused(x16, w16, st, pad, scale, shift, res16, relu, math="bf16", y16=True)
        y32 = ops.conv_fwd_fused(x16, w16, st, pad, scale, shift,
                                 res16.float() if res16 is not None else None, relu, math="bf16")
    finally:
        ops.MAX_FRAMES = saved
    return yb, y32


@pytest.mark.parametrize("case", CASES)
def test_infer16_bit_exact(dev, case):
    """The bf16 output's bytes are those of the fp32 inference epilogue's output rounded to bf16:
    same engine, same tile, same accumulators, the same fp32 operations, one rounding."""
    x16, w16, scale, shift, res16 = _operands(dev, case)
    for has_res in (False, True):
        for relu in (False, True):
            yb, y32 = _both(case, x16, w16, scale, shift, res16 if has_res else None, relu)
            assert yb.dtype == BF16 and yb.shape == y32.shape
            assert torch.equal(yb.view(torch.int16), y32.to(BF16).view(torch.int16)), \
                (case, has_res, relu)


@pytest.mark.parametrize("case", [CASES[0], CASES[7]])
def test_infer16_vs_float64(dev, case):
    """Each output element within 2^-8 |v| (half an ulp of the one RNE rounding) + 1e-5 max|v|
    (twice the 5e-6 tests/test_bf16_gpu.py grants this engine's summation order: the fma added)
    of the float64 conv of the rounded operands, scale/shift, residual and ReLU."""
    n, h, w, cin, cout, r, st, pad, _ = case
    x16, w16, scale, shift, res16 = _operands(dev, case)
    acc = torch.nn.functional.conv2d(x16.double().cpu().permute(0, 3, 1, 2),
                                     w16.double().cpu().permute(0, 3, 1, 2), stride=st,
                                     padding=pad).permute(0, 2, 3, 1)
    for has_res in (False, True):
        for relu in (False, True):
            yb, _ = _both(case, x16, w16, scale, shift, res16 if has_res else None, relu)
            v = acc * scale.double().cpu() + shift.double().cpu()
            if has_res:
                v = v + res16.double().cpu()
            if relu:
                v = v.clamp_min(0)
            err = (yb.double().cpu() - v).abs()
            bound = 2.0 ** -8 * v.abs() + 1e-5 * v.abs().max()
            print("infer16 vs f64", case, has_res, relu, "max err/bound",
                  (err / bound).max().item())
            assert (err <= bound).all(), (case, has_res, relu, (err / bound).max().item())


def test_infer16_trunk(dev):
    """The bf16-activation eval trunk against its float64 emulation (criterion of
    test_bf16_gpu.test_tmrnet_bf16_eval_logits on the features), and the default path's bits
    unchanged by switching it on and off again (no layout-cache leak)."""
    torch.manual_seed(71)
    share = ResNet50Share(precision="bf16").to(dev)
    randomize_bn(share, 72)
    share.eval()
    g = torch.Generator().manual_seed(73)
    x = torch.randn(4, 3, 224, 224, generator=g)
    x4 = ops.nchw_to_nhwc(x.to(dev), cpad=4)
    with torch.no_grad():
        f_off = share.features_nhwc4(x4)
        share.infer_act16 = True
        f_on = share.features_nhwc4(x4)
        share.infer_act16 = False
        f_off2 = share.features_nhwc4(x4)
    assert torch.equal(f_off, f_off2)
    assert not torch.equal(f_off, f_on)   # the switch took effect
    e32, e64 = hooked_share(share.state_dict())
    f32 = features(e32, x).double()
    f64 = features(e64, x.double())
    e_hip = (f_on.double().cpu() - f64).abs().max().item()
    e_cpu = (f32 - f64).abs().max().item()
    print("infer16 trunk e_hip %.3g e_cpu %.3g max|f64| %.3g" % (e_hip, e_cpu, f64.abs().max().item()))
    assert e_hip < max(5e-4 * max(1.0, f64.abs().max().item()), 3 * e_cpu), (e_hip, e_cpu)


def test_infer16_refusals(dev):
    """ResNeSt-50 has no bf16-activation eval path; a bf16 output takes a bf16 residual (checked
    before any library call)."""
    from tmrnet_amd import evaluate
    from tmrnet_amd.lfb import LongFeatureBank
    m = tmrnet_amd.resnet_lstm(seq_len=3, backbone="resnest50", precision="bf16")
    bank = LongFeatureBank(torch.zeros(1, 512), [0], 5, "cpu")
    with pytest.raises(ValueError, match="ResNet-50"):
        evaluate.evaluate_split(m, bank, torch.zeros(3, 250, 250, 3, dtype=torch.uint8), [3],
                                torch.zeros(3, dtype=torch.int64), activations="bf16")
    case = CASES[3]
    x16, w16, scale, shift, res16 = _operands(dev, case)
    calls = []
    real = ops.call
    ops.call = lambda *a, **k: calls.append(a[0]) or real(*a, **k)
    try:
        with pytest.raises(RuntimeError, match="bf16 residual"):
            ops.conv_fwd_fused(x16, w16, 1, 0, scale, shift, res16.float(), True, math="bf16",
                               y16=True)
    finally:
        ops.call = real
    assert calls == []
