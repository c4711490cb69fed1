"""The downsample blocks' dual BatchNorm backward folded into their two wgrads, and the 256x256
sixteen-wave form of the wgrad that produces its dy operand.

A downsample Bottleneck's bn3 and downsample BN share the block's masked gradient g.  The present
calls are tmr_bn_bwd_parts_ds (two reductions, one apply pass writing dy3 and dy_ds) and two plain
wgrads; the fold runs the reductions only (dy == dy_ds == NULL), or one single-output apply, and
lets tmr_conv2d_wgrad_bnbwd produce each served unit's dy from (g, y, coefficients).  Same fmaf
sequence per element, same k order and split plan: everything must match bit for bit (compared as
integers, so a NaN or a signed zero cannot hide), and tmr_wgrad_bnbwd_launches counts the fused
kernels.  Step level: the fp32 ResNet-50 trunk with trunk.WGRAD_BNBWD_DS on and off.
Reference: the backward of torchvision Bottleneck's `out += identity` with a `downsample`
Sequential, which code/Training TMRNet/train_only_non-local_pretrained.py:724-725 (loss.backward)
runs.
"""
import ctypes

import pytest
import torch

from tmrnet_amd import ops
from tmrnet_amd._lib import lib
from tests import _conv_engine_cases as T

pytestmark = pytest.mark.gpu


def _launches():
    return int(lib().tmr_wgrad_bnbwd_launches())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _bn_stats(y2, gen, dev):
    k = y2.shape[1]
    mean = y2.mean(0)
    inv = 1.0 / torch.sqrt(y2.var(0, unbiased=False) + 1e-5)
    gamma = (torch.rand(k, generator=gen) + 0.5).to(dev)
    return mean, inv, gamma


def _parts(g2, y2, mean, nparts):
    """The (sum g, sum g * (y - mean)) partial rows a fused dgrad leaves for bn3."""
    rows, k = y2.shape
    parts = torch.zeros(nparts, k, 2, device=y2.device)
    step = (rows + nparts - 1) // nparts
    for p in range(nparts):
        gs, ys = g2[p * step:(p + 1) * step], y2[p * step:(p + 1) * step]
        parts[p, :, 0] = gs.sum(0)
        parts[p, :, 1] = (gs * (ys - mean)).sum(0)
    return parts.contiguous()


# (name, frames, h, block input channels, mid channels, k, downsample stride)
BLOCKS = [
    ("s2_128_256", 11, 14, 128, 128, 256, 2),   # 128x128 eight-wave tile, 539 rows: no multiple of 32
    ("s1_128_256", 11, 14, 128, 128, 256, 1),   # the same at stride 1: 2,156 rows
    ("s1_64_256", 11, 14, 64, 64, 256, 1),      # 64-wide tile, four m-tiles
]
_CACHE = {}


def _block(dev, name):
    """Operands of one downsample block and the present calls' results, computed once."""
    if name in _CACHE:
        return _CACHE[name]
    _, frames, h, cin, mid, k, stride = next(b for b in BLOCKS if b[0] == name)
    gen = torch.Generator().manual_seed(11)
    ho = (h - 1) // stride + 1
    xd = torch.randn(frames, h, h, cin, generator=gen).to(dev)        # the block input
    x3 = torch.randn(frames, ho, ho, mid, generator=gen).to(dev)      # conv3's input
    y3 = (torch.randn(frames, ho, ho, k, generator=gen) * 1.5 + 0.25).to(dev)
    yd = (torch.randn(frames, ho, ho, k, generator=gen) * 0.75 - 0.5).to(dev)
    g = torch.randn(frames, ho, ho, k, generator=gen).to(dev)
    g = g * (torch.rand(frames, ho, ho, k, generator=gen).to(dev) > 0.5)
    m3, i3, g3 = _bn_stats(y3.view(-1, k), gen, dev)
    md, idv, gd = _bn_stats(yd.view(-1, k), gen, dev)
    nparts = 5
    parts = _parts(g.view(-1, k), y3.view(-1, k), m3, nparts)
    bargs = (g, y3, parts, nparts, m3, i3, g3, yd, md, idv, gd)
    dy3, dg3, db3, dyd, dgd, dbd = ops.bn_bwd_parts_ds(*bargs)
    dw3 = ops.conv_wgrad(x3, dy3, 1, 1, 1, 0)
    dwd = ops.conv_wgrad(xd, dyd, 1, 1, stride, 0)
    torch.cuda.synchronize()
    _CACHE[name] = dict(xd=xd, x3=x3, y3=y3, yd=yd, g=g, stride=stride, bargs=bargs,
                        ref=dict(dy3=dy3, dg3=dg3, db3=db3, dyd=dyd, dgd=dgd, dbd=dbd, dw3=dw3,
                                 dwd=dwd))
    return _CACHE[name]


@pytest.mark.parametrize("name", [b[0] for b in BLOCKS])
def test_ds_fold_vs_present_calls(dev, name):
    b = _block(dev, name)
    ref, g = b["ref"], b["g"]
    assert ops.conv_wgrad_bnbwd_ok(b["x3"], g, b["y3"], 1, 1, 1, 0)
    assert ops.conv_wgrad_bnbwd_ok(b["xd"], g, b["yd"], 1, 1, b["stride"], 0)
    n0 = _launches()
    c3, dg3, db3, cd, dgd, dbd, dy3, dyd = ops.bn_bwd_parts_ds_coef(*b["bargs"])
    assert dy3 is None and dyd is None
    assert c3.data_ptr() % 16 == 0 and cd.data_ptr() % 16 == 0
    assert _launches() == n0
    dw3, dy3 = ops.conv_wgrad_bnbwd(b["x3"], g, b["y3"], c3, 1, 1, 1, 0)
    dwd, dyd = ops.conv_wgrad_bnbwd(b["xd"], g, b["yd"], cd, 1, 1, b["stride"], 0)
    torch.cuda.synchronize()
    assert _launches() == n0 + 2
    got = dict(dy3=dy3, dg3=dg3, db3=db3, dyd=dyd, dgd=dgd, dbd=dbd, dw3=dw3, dwd=dwd)
    for key in ref:
        assert _same(got[key], ref[key]), key


@pytest.mark.parametrize("name", [b[0] for b in BLOCKS])
def test_ds_half_forms(dev, name):
    """Exactly one output: a single-output apply; the BN gradients and the written output are the
    full call's, the other unit's coefficients are the coefficient-only call's."""
    b = _block(dev, name)
    ref = b["ref"]
    c3, _, _, cd, _, _, _, _ = ops.bn_bwd_parts_ds_coef(*b["bargs"])
    c3, cd = c3.clone(), cd.clone()
    a = ops.bn_bwd_parts_ds_coef(*b["bargs"], apply3=True)
    d = ops.bn_bwd_parts_ds_coef(*b["bargs"], applyd=True)
    torch.cuda.synchronize()
    assert a[7] is None and _same(a[6], ref["dy3"]) and _same(a[3], cd)
    assert d[6] is None and _same(d[7], ref["dyd"]) and _same(d[0], c3)
    for r in (a, d):
        assert _same(r[1], ref["dg3"]) and _same(r[2], ref["db3"])
        assert _same(r[4], ref["dgd"]) and _same(r[5], ref["dbd"])
    with pytest.raises(RuntimeError):
        ops.bn_bwd_parts_ds_coef(*b["bargs"], apply3=True, applyd=True)


def test_ds_coef_forms_refuse_bf16(dev):
    """The NULL-output forms are fp32 only: the C entry point refuses bf16 operands with a NULL
    dy and launches nothing (dgamma keeps its fill)."""
    b = _block(dev, "s1_64_256")
    g, y3, parts, nparts, m3, i3, g3, yd, md, idv, gd = b["bargs"]
    k = y3.shape[-1]
    rows = y3.numel() // k
    g16, y16, yd16 = (t.to(torch.bfloat16) for t in (g, y3, yd))
    nb = int(lib().tmr_bn_bwd_parts_ds_ws_bytes(nparts, rows, k))
    ws = torch.empty(nb // 8 + 1, dtype=torch.float64, device=dev)
    out = [torch.full((k,), 7.0, device=dev) for _ in range(4)]
    dyd = torch.empty_like(yd16)
    with pytest.raises(RuntimeError, match="fp32 only"):
        ops.call("tmr_bn_bwd_parts_ds", g16, y16, parts, nparts, m3, i3, g3, None, out[0], out[1],
                 yd16, md, idv, gd, dyd, out[2], out[3], rows, k, 1, ws,
                 ctypes.c_size_t(ws.numel() * 8), ops.stream_ptr())
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in out)
    assert int(lib().tmr_bn_bwd_parts_ds_coef_offset(nparts, rows, k, 2)) == 0
    assert int(lib().tmr_bn_bwd_parts_ds_coef_offset(nparts, rows, k, 0)) == \
        int(lib().tmr_bn_parts_coef_offset(nparts, k))


def test_ds_fused_refusals(dev):
    """The fused call refuses what the query refuses -- a bf16 operand, groups, a misaligned g --
    on a downsample unit (1x1 stride 2), and launches nothing."""
    b = _block(dev, "s2_128_256")
    xd, g, yd, s = b["xd"], b["g"], b["yd"], b["stride"]
    cd = ops.bn_bwd_parts_ds_coef(*b["bargs"])[3]
    n0 = _launches()
    assert not ops.conv_wgrad_bnbwd_ok(xd.to(torch.bfloat16), g, yd, 1, 1, s, 0, math="bf16")
    assert not ops.conv_wgrad_bnbwd_ok(xd, g, yd, 1, 1, s, 0, math="bf16")
    assert not ops.conv_wgrad_bnbwd_ok(xd, g, yd, 1, 1, s, 0, groups=2)
    buf = torch.zeros(g.numel() + 4, device=dev)
    g1 = buf[1:1 + g.numel()].view(g.shape)   # 4 bytes past a 16-B boundary
    g1.copy_(g)
    assert g1.data_ptr() % 16 == 4
    assert not ops.conv_wgrad_bnbwd_ok(xd, g1, yd, 1, 1, s, 0)
    with pytest.raises(RuntimeError, match="no fused form"):
        ops.conv_wgrad_bnbwd(xd, g1, yd, cd, 1, 1, s, 0)
    with pytest.raises(RuntimeError, match="no fused form"):
        ops.conv_wgrad_bnbwd(xd, g, yd, cd, 1, 1, s, 0, math="bf16")
    d = ops.conv_desc(11, 14, 14, 128, 256, 1, 1, s, 0, math="fp32", io=0, groups=2)
    assert lib().tmr_conv2d_wgrad_bnbwd_ok(ctypes.byref(d), None, None, None, None) == 0
    torch.cuda.synchronize()
    assert _launches() == n0


def test_wgrad_bnbwd_256x256_tile(dev):
    """The sixteen-wave 256x256 form (gemm16_wgrad_bnbwd16_kernel) at the smallest reduction that
    selects config 6: 61 frames of 14x14, 2048 -> 2048, 1x1 (11,956 rows, no multiple of 32;
    2*M*N*K = 100.3e9).  dW and dy bit-identical to tmr_bn_bwd_parts + tmr_conv2d_wgrad.

    dy against float64: the kernel computes fl(A*g + fl(B*y + C)) with fused multiply-adds, two
    roundings of relative size u = 2^-24, so with the fp32 coefficients taken as exact
    |dy - ref| <= u * (|B*y + C| + |ref|) + O(u^2) <= 2u * (|A*g| + |B*y| + |C|); asserted with
    the factor (1 + 2^-20) for the second-order term.  (test_wgrad_bnbwd_gpu.py itself compares
    bit for bit and has no float64 bound to borrow.)"""
    c = next(r for r in T.CASES if r.name == "c2048_2048_big")
    assert ops.conv_tile(c.n, c.h, c.w, c.cin, c.cout, c.r, c.r, c.stride, c.pad, "wgrad")["cfg"] == 6
    gen = torch.Generator(device=dev).manual_seed(5)
    k = c.cout
    x = torch.randn(c.n, c.h, c.w, c.cin, generator=gen, device=dev)
    y = torch.randn(c.n, c.h, c.w, k, generator=gen, device=dev) * 1.5 + 0.25
    g = torch.randn(c.n, c.h, c.w, k, generator=gen, device=dev)
    g = g * (torch.rand(c.n, c.h, c.w, k, generator=gen, device=dev) > 0.5)
    y2, g2 = y.view(-1, k), g.view(-1, k)
    mean = y2.mean(0)
    inv = 1.0 / torch.sqrt(y2.var(0, unbiased=False) + 1e-5)
    gamma = torch.rand(k, generator=gen, device=dev) + 0.5
    nparts = 5
    parts = _parts(g2, y2, mean, nparts)
    if not ops.conv_wgrad_bnbwd_ok(x, g, y, 1, 1, 1, 0):
        pytest.skip("the 256x256 sixteen-wave dy-producing form was not built "
                    "(wgrad_bnbwd_cfg has no config 6)")
    dy_ref, dg_ref, db_ref = ops.bn_bwd_parts(g, y, parts, nparts, mean, inv, gamma)
    dw_ref = ops.conv_wgrad(x, dy_ref, 1, 1, 1, 0)
    n0 = _launches()
    coef, dg, db = ops.bn_bwd_parts_coef(y, parts, nparts, mean, inv, gamma)
    dw, dy = ops.conv_wgrad_bnbwd(x, g, y, coef, 1, 1, 1, 0)
    torch.cuda.synchronize()
    assert _launches() == n0 + 1
    assert _same(dg, dg_ref) and _same(db, db_ref)
    assert _same(dy, dy_ref)
    assert _same(dw, dw_ref)
    A, B, C = coef.double().view(3, k)
    ref = A * g2.double() + (B * y2.double() + C)
    bound = 2.0 * 2.0 ** -24 * (1 + 2.0 ** -20) * ((A * g2.double()).abs() + (B * y2.double()).abs()
                                                   + C.abs())
    err = (dy.view(-1, k).double() - ref).abs()
    print("256x256 form: max |dy - f64| / bound = %.3f" % float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())


def test_ds_fold_step_bit_identical(dev):
    """The fp32 ResNet-50 trunk train step (2 clips x 2 frames of 64x64) with the downsample
    blocks' fold on (every size: WGRAD_BNBWD_DS_MIN = 0) and off: features, every gradient, every
    buffer bit-identical; on, the four blocks add their eight fused launches (bn3's conv3 and the
    downsample conv each) to the 43 of the other units."""
    from tmrnet_amd import trunk
    gen = torch.Generator().manual_seed(3)
    x4 = torch.randn(4, 64, 64, 4, generator=gen).to(dev)
    x4[..., 3] = 0
    w = torch.randn(4, 2048, generator=gen).to(dev)
    res = {}
    saved = (trunk.WGRAD_BNBWD_DS, trunk.WGRAD_BNBWD_DS_MIN)
    try:
        trunk.WGRAD_BNBWD_DS_MIN = 0
        for on in (True, False):
            trunk.WGRAD_BNBWD_DS = on
            torch.manual_seed(0)
            share = trunk.ResNet50Share(precision="fp32").to(dev).train()
            n0 = _launches()
            feat = share.features_nhwc4(x4)
            (feat * w).sum().backward()
            torch.cuda.synchronize()
            assert _launches() - n0 == 43 + (8 if on else 0)
            res[on] = (feat.detach().clone(),
                       {n: p.grad.clone() for n, p in share.named_parameters()},
                       {n: b.clone() for n, b in share.named_buffers()})
    finally:
        trunk.WGRAD_BNBWD_DS, trunk.WGRAD_BNBWD_DS_MIN = saved
    assert _same(res[True][0], res[False][0])
    assert len(res[True][1]) > 100
    for n in res[True][1]:
        assert _same(res[True][1][n], res[False][1][n]), n
    for n in res[True][2]:
        a, b = res[True][2][n], res[False][2][n]
        assert torch.equal(a, b) if a.dtype != torch.float32 else _same(a, b), n
