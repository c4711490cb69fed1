"""The bf16-activation inference trunk of ResNeSt-50 (ResNeSt50Share.infer_act16):
the grouped form of the fused inference unit (tmr_conv2d_fwd_fused, groups + TMR_IO_Y_BF16), the
one-launch attention MLP (tmr_splat_attn_inf), the weighted sum with the avd pool
(tmr_splat_combine_a16) and the trunk built on them against its float64 emulation."""
import pytest
import torch
import torch.nn.functional as F

from tmrnet_amd import ops
from tmrnet_amd.resnest import ResNeSt50Share
from tests._infer16_resnest_emu import randomize_bn, hooked_share, features

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16

# ------------------------------------------------------------------ grouped fused unit
# (n, h, w, cin, cout, stride, max_frames): groups = 2, 3x3, pad 1
GROUPED = [(2, 9, 9, 64, 128, 1, 0), (1, 7, 5, 128, 256, 1, 0), (2, 9, 9, 64, 128, 2, 0),
           (3, 9, 9, 64, 128, 1, 1)]


@pytest.mark.parametrize("case", GROUPED)
def test_grouped_fused_unit(dev, case):
    """groups = 2 with a bf16 output: the bytes of the grouped fp32 fused epilogue's output rounded
    to bf16 (the criterion of test_infer16_bit_exact), and each element within 2^-8 |v| + 1e-5 max|v|
    of the float64 grouped conv of the rounded operands (the bound test_infer16_vs_float64 grants
    this engine)."""
    n, h, w, cin, cout, st, mf = case
    g = torch.Generator().manual_seed(31 + cin + cout + st + n)
    wt = torch.randn(cout, cin // 2, 3, 3, generator=g) / (cin // 2 * 9) ** 0.5
    x16 = torch.randn(n, h, w, cin, generator=g).to(dev).to(BF16)
    w16 = ops.weight_to_krsc(wt.to(dev), bf16=True)
    assert tuple(w16.shape) == (cout, 3, 3, cin // 2)
    scale = (torch.rand(cout, generator=g) + 0.5).to(dev)
    shift = (torch.randn(cout, generator=g) * 0.1).to(dev)
    acc = F.conv2d(x16.double().cpu().permute(0, 3, 1, 2), w16.double().cpu().permute(0, 3, 1, 2),
                   stride=st, padding=1, groups=2).permute(0, 2, 3, 1)
    saved = ops.MAX_FRAMES
    ops.MAX_FRAMES = mf
    try:
        for relu in (False, True):
            yb = ops.conv_fwd_fused(x16, w16, st, 1, scale, shift, None, relu, math="bf16",
                                    y16=True, groups=2)
            y32 = ops.conv_fwd_fused(x16, w16, st, 1, scale, shift, None, relu, math="bf16",
                                     groups=2)
            assert yb.dtype == BF16 and y32.dtype == torch.float32 and yb.shape == y32.shape
            assert tuple(yb.shape) == (n,) + tuple(acc.shape[1:3]) + (cout,)
            assert torch.equal(yb.view(torch.int16), y32.to(BF16).view(torch.int16)), (case, relu)
            v = acc * scale.double().cpu() + shift.double().cpu()
            if relu:
                v = v.clamp_min(0)
            err = (yb.double().cpu() - v).abs()
            bound = 2.0 ** -8 * v.abs() + 1e-5 * v.abs().max()
            print("grouped infer16 vs f64", case, relu, "max err/bound", (err / bound).max().item())
            assert (err <= bound).all(), (case, relu, (err / bound).max().item())
    finally:
        ops.MAX_FRAMES = saved


# ------------------------------------------------------------------ tmr_splat_attn_inf
@pytest.mark.parametrize("n,C", [(1, 64), (5, 128), (17, 256), (3, 512)])
def test_splat_attn_inf(dev, n, C):
    """One launch against float64: its maximum error at most 3x that of the four-launch route
    (gemm_nt, bn_apply, gemm_nt, splat_att) on the same inputs against the same float64 (the
    margin test_infer16_trunk grants over its reference route)."""
    inter = C // 2
    g = torch.Generator().manual_seed(500 + n + C)
    gap = torch.rand(n, C, generator=g) * 2
    w1 = torch.randn(inter, C, generator=g) / C ** 0.5
    b1 = torch.randn(inter, generator=g) * 0.1
    gamma = torch.rand(inter, generator=g) * 0.5 + 0.75
    beta = torch.randn(inter, generator=g) * 0.2
    mean = torch.randn(inter, generator=g) * 0.5
    var = torch.rand(inter, generator=g) + 0.5
    w2 = torch.randn(2 * C, inter, generator=g) * (2.0 / inter) ** 0.5
    b2 = torch.randn(2 * C, generator=g) * 0.1
    d = [t.to(dev) for t in (gap, w1, b1, gamma, beta, mean, var, w2, b2)]
    gap_d, w1_d, b1_d, gamma_d, beta_d, mean_d, var_d, w2_d, b2_d = d
    sc, sh = ops.bn_eval_params(gamma_d, beta_d, mean_d, var_d, 1e-5)
    att = ops.splat_attn_inf(gap_d, w1_d, b1_d, sc, sh, w2_d, b2_d)
    h1 = ops.gemm_nt(gap_d, w1_d, bias=b1_d)
    a1 = ops.bn_apply(h1, sc, sh, None, True)
    old = ops.splat_att(ops.gemm_nt(a1, w2_d, bias=b2_d))
    h64 = gap.double() @ w1.double().t() + b1.double()
    h64 = ((h64 - mean.double()) / (var.double() + 1e-5).sqrt() * gamma.double()
           + beta.double()).clamp_min(0)
    z64 = h64 @ w2.double().t() + b2.double()
    ref = torch.softmax(z64.view(n, 2, C), 1).reshape(n, 2 * C)
    assert att.shape == old.shape == ref.shape
    e_new = (att.double().cpu() - ref).abs().max().item()
    e_old = (old.double().cpu() - ref).abs().max().item()
    print("splat_attn_inf n %d C %d: e_new %.3g e_old %.3g" % (n, C, e_new, e_old))
    assert e_new <= 3 * e_old, (e_new, e_old)


# ------------------------------------------------------------------ tmr_splat_combine_a16
@pytest.mark.parametrize("n,h,w,C,pool", [(2, 5, 7, 64, 0), (2, 5, 7, 64, 1), (3, 9, 6, 128, 2),
                                          (1, 7, 7, 512, 2), (2, 1, 1, 64, 2)])
def test_splat_combine_a16(dev, n, h, w, C, pool):
    """Within 2^-8 |v| (half an ulp of the one rounding) + 19 * 2^-24 max|x2| (18 fp32
    multiply-adds and the division over values bounded by max|x2|: the attention weights sum to 1)
    of float64; the padded border checked on its own; nothing written outside the tensor."""
    g = torch.Generator().manual_seed(900 + n + h + w + C + pool)
    x2 = torch.randn(n, h, w, 2 * C, generator=g).clamp_min(0).to(BF16)
    att = torch.softmax(torch.randn(n, 2, C, generator=g) * 2, 1).reshape(n, 2 * C)
    v = (att[:, :C].double().view(n, 1, 1, C) * x2[..., :C].double()
         + att[:, C:].double().view(n, 1, 1, C) * x2[..., C:].double())
    if pool:
        v = F.avg_pool2d(v.permute(0, 3, 1, 2), 3, pool, 1,
                         count_include_pad=True).permute(0, 2, 3, 1)
    ho, wo = v.shape[1], v.shape[2]
    assert (ho, wo) == (((h - 1) // pool + 1, (w - 1) // pool + 1) if pool else (h, w))
    guard, pat = 64, 0x7B7B
    numel = n * ho * wo * C
    buf = torch.full((numel + 2 * guard,), pat, dtype=torch.int16, device=dev)
    out = buf[guard:guard + numel].view(BF16).view(n, ho, wo, C)
    got = ops.splat_combine_a16(x2.to(dev), att.to(dev), pool=pool, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert (buf[:guard] == pat).all() and (buf[guard + numel:] == pat).all()
    y = out.double().cpu()
    bound = 2.0 ** -8 * v.abs() + 19 * 2.0 ** -24 * x2.double().abs().max()
    err = (y - v).abs()
    print("splat_combine_a16", (n, h, w, C, pool), "max err/bound", (err / bound).max().item())
    assert (err <= bound).all(), (err / bound).max().item()
    if pool:
        # the padded border by hand, independent of avg_pool2d: real cells summed, 9 counted
        full = (att[:, :C].double().view(n, 1, 1, C) * x2[..., :C].double()
                + att[:, C:].double().view(n, 1, 1, C) * x2[..., C:].double())

        def window(oy, ox):
            ys = slice(max(oy * pool - 1, 0), min(oy * pool + 2, h))
            xs = slice(max(ox * pool - 1, 0), min(ox * pool + 2, w))
            return full[:, ys, xs].sum((1, 2)) / 9.0

        for oy in range(ho):            # first / last output rows and columns
            for ox in range(wo):
                if oy in (0, ho - 1) or ox in (0, wo - 1):
                    assert ((y[:, oy, ox] - window(oy, ox)).abs() <= bound[:, oy, ox]).all(), (oy, ox)
    # without `out` the wrapper allocates the output itself: the same bytes
    again = ops.splat_combine_a16(x2.to(dev), att.to(dev), pool=pool)
    assert torch.equal(again.view(torch.int16), out.view(torch.int16))


def test_new_entry_points_refuse_bad_arguments(dev):
    x2 = torch.zeros(1, 2, 2, 128, dtype=BF16, device=dev)
    att = torch.zeros(1, 128, device=dev)
    with pytest.raises(RuntimeError, match="pool stride"):
        ops.splat_combine_a16(x2, att, pool=3)
    with pytest.raises(RuntimeError, match="x2 must be"):
        ops.splat_combine_a16(x2.float(), att)
    gap = torch.zeros(2, 96, device=dev)
    z = torch.zeros(48, device=dev)
    with pytest.raises(RuntimeError, match="tmr_splat_attn_inf: bad shape"):
        ops.splat_attn_inf(gap, torch.zeros(48, 96, device=dev), z, z, z,
                           torch.zeros(192, 48, device=dev), torch.zeros(192, device=dev))


# ------------------------------------------------------------------ the trunk
@pytest.fixture(scope="module")
def trunk_case(dev):
    torch.manual_seed(171)
    share = ResNeSt50Share(precision="bf16").to(dev)
    randomize_bn(share, 172)
    share.eval()
    g = torch.Generator().manual_seed(173)
    # 72 x 56: maps of 36 / 18 / 9 / 5 / 3 rows (ceil_mode pools, odd avd windows)
    x = torch.randn(3, 3, 72, 56, generator=g)
    return share, x, ops.nchw_to_nhwc(x.to(dev), cpad=4)


def test_infer16_resnest_trunk(trunk_case):
    """The features against the float64 emulation (criterion of test_infer16_trunk); the default
    path's bits unchanged by switching the route on and off again, and different from it."""
    share, x, x4 = trunk_case
    assert share.infer_act16 is False
    with torch.no_grad():
        f_off = share.features_nhwc4(x4)
        share.infer_act16 = True
        try:
            f_on = share.features_nhwc4(x4)
        finally:
            share.infer_act16 = False
        f_off2 = share.features_nhwc4(x4)
    assert f_on.dtype == torch.float32 and tuple(f_on.shape) == (3, 2048)
    assert torch.equal(f_off, f_off2)
    assert not torch.equal(f_off, f_on)   # the switch took effect
    e32, e64 = hooked_share(share.state_dict())
    f32 = features(e32, x).double()
    f64 = features(e64, x.double())
    e_hip = (f_on.double().cpu() - f64).abs().max().item()
    e_cpu = (f32 - f64).abs().max().item()
    print("infer16 resnest trunk e_hip %.3g e_cpu %.3g max|f64| %.3g"
          % (e_hip, e_cpu, f64.abs().max().item()))
    assert e_hip < max(5e-4 * max(1.0, f64.abs().max().item()), 3 * e_cpu), (e_hip, e_cpu)


def test_infer16_resnest_batch_of_one(trunk_case):
    """A frame alone (an online tick) gives the bits of the same frame in a batch of 3: no kernel
    of the route sums over frames, and no tile choice changes a conv's summation order."""
    share, _, x4 = trunk_case
    share.infer_act16 = True
    try:
        with torch.no_grad():
            f3 = share.features_nhwc4(x4)
            f1 = share.features_nhwc4(x4[:1].contiguous())
    finally:
        share.infer_act16 = False
    assert torch.equal(f1[0], f3[0])
