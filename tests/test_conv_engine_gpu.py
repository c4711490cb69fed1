"""The LDS-DMA implicit-GEMM conv engine against float64, at every tile config its fp32 rules can
select (tests/_conv_engine_cases.py; test_conv_engine_cpu.py proves the coverage) and at the tile
edges: two passes per case and view.

Exact pass.  Every operand (x, w, dy, bias, the old output of the accumulating forms) is an integer
drawn uniformly from {-3, ..., 3}.  A product is at most 9 in magnitude and a sum of K of them at
most 9*K < 2^24 (asserted), so every product and every partial sum -- in any summation order,
across split-K slabs, frame chunks and the wgrad reduce -- is an integer fp32 holds exactly: the
result must equal the float64 reference bit for bit (torch.equal).  One dropped, duplicated or
misplaced term changes an integer.  Outputs are pre-filled with NaN (beta = 0 must not read them,
and an element never written stays NaN); the channels of a wider tensor around a channel slice
must keep their NaN.
  Zeros: the reference should be non-zero nearly everywhere, so that a tile of zeros cannot pass.
  For integers in [-3, 3] a sum of K products is zero with probability about 0.1 / sqrt(K) (a
  lattice variable of variance 16*K), which is above 1 in 1000 for every K < 10^4 whatever the
  seed; the tests therefore require the zero fraction among outputs that have any tap to stay
  below max(1e-3, 0.2 / sqrt(K1)) -- twice the expected rate at K1, the shortest reduction an
  output of the view has (one tap's channels; the wgrad's rows, halved where taps can fall into
  the padding) -- regenerate with another seed otherwise, and rely on the NaN pre-fill for
  missing stores.

Rounding pass.  randn operands rounded to fp32, weights scaled by 1/sqrt(K).  Per element
|got - ref| <= (K + splits + 2) * 2^-24 * S, S the float64 sum of |a|*|b| over the same taps: the
standard bound for K correctly rounded fma / add steps in any order, no measurement in it.  splits
is 0 for the forward and the dgrad and the split-K count for the wgrad; on the frame-chunked row
the wgrad reduces its splits once per chunk and adds the chunks into dW, so there splits counts
every chunk's plus one add per further chunk.  In max-norm, max|err| / max|ref| must stay within 3x that of a torch fp32
computation of the same operands against the same float64 reference, floor 2e-6 (the factor and
floor of test_kernels_gpu.py / test_bf16_gpu.py).

Reference: float64 F.conv2d / torch.nn.grad on the CPU below 1 GFLOP; above, a float64
torch.matmul on the device over an im2col built here with plain torch slicing (a reshape for
1x1).  test_im2col_reference_matches_conv2d requires the two equal to 1e-12 on a 3x3 stride-2
case.  Nothing from libtmr is in the reference.
"""
import json
import math
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

from tmrnet_amd import ops
from tests import _conv_engine_cases as T
from tests._bits import pack_bits

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS = 2.0 ** -24
VIEWS = ("fwd", "dgrad", "wgrad")
ROWS = [(c, v) for c in T.CASES for v in VIEWS if v in c.expect]
IDS = ["%s-%s-cfg%d" % (c.name, v, c.expect[v][1]) for c, v in ROWS]


BF16_ROWS = T.bf16_rows(ops)   # (case, view, cfg under bf16 rules); the 4-channel rows are left out


# ------------------------------------------------------------------ float64 reference (plain torch)
def im2col(x, r, stride, pad):
    """x (n, h, w, c) -> (n*ho*wo, r*r*c), taps outermost (the KRSC order)."""
    n, h, w, c = x.shape
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1
    if r == 1 and stride == 1 and pad == 0:
        return x.reshape(-1, c)
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    cols = [xp[:, i:i + stride * (ho - 1) + 1:stride, j:j + stride * (wo - 1) + 1:stride, :]
            for i in range(r) for j in range(r)]
    return torch.cat(cols, dim=3).reshape(n * ho * wo, r * r * c)


def ref_matmul(c, view, x, w, dy):
    """x (n,h,w,cin), w (cout,cin,r,r), dy (n,ho,wo,cout) -> y NHWC / dx NHWC / dW OIHW."""
    ho, wo = T.out_hw(c)
    wk = w.permute(0, 2, 3, 1).reshape(c.cout, -1)            # (cout, r*r*cin)
    if view == "fwd":
        return (im2col(x, c.r, c.stride, c.pad) @ wk.t()).view(c.n, ho, wo, c.cout)
    if view == "wgrad":
        dw = dy.reshape(-1, c.cout).t() @ im2col(x, c.r, c.stride, c.pad)
        return dw.view(c.cout, c.r, c.r, c.cin).permute(0, 3, 1, 2).contiguous()
    dcol = (dy.reshape(-1, c.cout) @ wk).view(c.n, ho, wo, c.r, c.r, c.cin)
    dxp = torch.zeros(c.n, c.h + 2 * c.pad, c.w + 2 * c.pad, c.cin, dtype=x.dtype, device=x.device)
    for i in range(c.r):
        for j in range(c.r):
            dxp[:, i:i + c.stride * (ho - 1) + 1:c.stride,
                j:j + c.stride * (wo - 1) + 1:c.stride, :] += dcol[:, :, :, i, j, :]
    return dxp[:, c.pad:c.pad + c.h, c.pad:c.pad + c.w, :].contiguous()


def ref_conv2d(c, view, x, w, dy):
    """The same through torch's own conv ops (NCHW)."""
    xn, dyn = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
    if view == "fwd":
        return F.conv2d(xn, w, stride=c.stride, padding=c.pad).permute(0, 2, 3, 1).contiguous()
    if view == "wgrad":
        return torch.nn.grad.conv2d_weight(xn, w.shape, dyn, stride=c.stride, padding=c.pad)
    return torch.nn.grad.conv2d_input(xn.shape, w, dyn, stride=c.stride,
                                      padding=c.pad).permute(0, 2, 3, 1).contiguous()


def reference(c, view, x, w, dy, dev):
    """float64 reference and S = sum |a|*|b| of the view, on the device."""
    if T.flops(c) < 1e9:
        a = [t.double().cpu() for t in (x, w, dy)]
        return (ref_conv2d(c, view, *a).to(dev),
                ref_conv2d(c, view, *[t.abs() for t in a]).to(dev))
    a = [t.double() for t in (x, w, dy)]
    return ref_matmul(c, view, *a), ref_matmul(c, view, *[t.abs() for t in a])


# ------------------------------------------------------------------ operands, shared per (case, kind)
_CACHE = {}


def gen(c, tag, dev):
    """A generator of its own per (case, purpose): the data of a test does not depend on which
    tests ran before it."""
    return torch.Generator(device=dev).manual_seed(zlib.crc32(("%s/%s" % (c.name, tag)).encode()))


def ints(g, shape, dev, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g, device=dev).float()


def operands(c, kind, dev, attempt=0):
    """Operands and lazily computed references of one case; one case is kept at a time.
    attempt: another seed (the exact pass regenerates when too many reference outputs are zero)."""
    key = (c.name, kind, attempt)
    if _CACHE.get("key") != key:
        _CACHE.clear()
        torch.cuda.empty_cache()
        g = gen(c, "%s/%d" % (kind, attempt), dev)
        ho, wo = T.out_hw(c)

        def draw(shape, scale=1.0):
            if kind == "exact":
                return ints(g, shape, dev)
            return torch.randn(shape, generator=g, device=dev) * scale
        k_all = c.r * c.r * c.cin
        _CACHE.update(key=key, attempt=attempt, x=draw((c.n, c.h, c.w, c.cin)),
                      w=draw((c.cout, c.cin, c.r, c.r), 1.0 / math.sqrt(k_all)),
                      dy=draw((c.n, ho, wo, c.cout)), bias=draw((c.cout,)), ref={})
    return _CACHE


def ref_of(c, view, kind, dev, attempt=0):
    o = operands(c, kind, dev, attempt)
    if view not in o["ref"]:
        o["ref"][view] = reference(c, view, o["x"], o["w"], o["dy"], dev)
    return o["ref"][view]


def in_slice(t, ld, fill):
    """t (n, h, w, c) as a channel slice at offset 8 of a (n, h, w, ld) tensor filled by fill."""
    if not ld:
        return None, t.contiguous()
    full = fill(t.shape[:3] + (ld,))
    full[..., 8:8 + t.shape[3]] = t
    return full, full[..., 8:8 + t.shape[3]]


def run_view(c, view, o, dev, beta=0.0, old=None, bias=None, dtype=torch.float32):
    """One launch of the view on the case's operands (dtype: their storage) -> the output."""
    math_ = "fp32" if dtype == torch.float32 else "bf16"
    ho, wo = T.out_hw(c)
    x_ld, y_ld = c.extras.get("x_ld", 0), c.extras.get("y_ld", 0)
    garbage = lambda s: torch.full(s, 7.0, device=dev, dtype=dtype)   # channels outside the slice
    x = in_slice(o["x"].to(dtype), x_ld, garbage)[1]
    dy = in_slice(o["dy"].to(dtype), y_ld, garbage)[1]
    nan = lambda s: torch.full(s, float("nan"), device=dev)
    with T.run_form(ops, c):
        if view == "fwd":
            full, out = in_slice(old if old is not None else nan((c.n, ho, wo, c.cout)), y_ld, nan)
            wk = o["w"].permute(0, 2, 3, 1).contiguous().to(dtype)
            ops.conv_fwd(x, wk, c.stride, c.pad, bias=bias, out=out, beta=beta, math=math_)
        elif view == "dgrad":
            full, out = in_slice(old if old is not None else nan((c.n, c.h, c.w, c.cin)), x_ld, nan)
            wc = o["w"].permute(1, 2, 3, 0).contiguous().to(dtype)     # (cin, r, s, cout)
            ops.conv_dgrad(dy, wc, (c.h, c.w), c.stride, c.pad, out=out, beta=beta, math=math_,
                           wt=True)
        else:
            full, out = None, (old.clone() if old is not None else nan((c.cout, c.cin, c.r, c.r)))
            ops.conv_wgrad(x, dy, c.r, c.r, c.stride, c.pad, out=out, beta=beta, math=math_)
    torch.cuda.synchronize()
    if full is not None:    # the wider tensor's other channels keep their NaN
        rest = torch.ones(full.shape[3], dtype=torch.bool, device=dev)
        rest[8:8 + out.shape[3]] = False
        assert torch.isnan(full[..., rest]).all(), "wrote outside the channel slice"
    return out


def check_exact(c, view, dev, dtype):
    k = T.gemm_k(c, view)
    assert 9 * k + 6 < 2 ** 24
    # zeros: at most twice the expected rate 0.1 / sqrt(K1), K1 the shortest reduction of an output
    # that has a tap (one tap's channels; the wgrad's rows, half of them where a tap can fall
    # into the padding); another seed otherwise
    k1 = {"fwd": c.cin, "dgrad": c.cout, "wgrad": k if c.pad == 0 else max(1, k // 2)}[view]
    for attempt in range(4):
        o = operands(c, "exact", dev, attempt)
        ref, s = ref_of(c, view, "exact", dev, attempt)
        zeros = ((ref == 0) & (s > 0)).double().mean().item()
        print("%s %s: zero fraction %.3g (seed %d)" % (c.name, view, zeros, attempt))
        if zeros < max(1e-3, 0.2 / math.sqrt(k1)):
            break
    assert zeros < max(1e-3, 0.2 / math.sqrt(k1))
    got = run_view(c, view, o, dev, dtype=dtype)
    assert not torch.isnan(got).any(), "%d elements never written" % torch.isnan(got).sum().item()
    bad = (got.double() != ref).sum().item()
    assert torch.equal(got.double(), ref), "%d of %d elements differ" % (bad, ref.numel())
    # accumulating forms: beta = 1 into a prefilled integer output, fwd with an integer bias
    old = ints(gen(c, "old/" + view, dev), tuple(ref.shape), dev)
    bias = o["bias"] if view == "fwd" else None
    got = run_view(c, view, o, dev, beta=1.0, old=old.clone(), bias=bias, dtype=dtype)
    want = ref + old.double() + (bias.double() if bias is not None else 0.0)
    assert torch.equal(got.double(), want), "beta = 1%s" % (" + bias" if bias is not None else "")
    if view == "fwd":      # bias alone (beta = 0)
        got = run_view(c, view, o, dev, bias=bias, dtype=dtype)
        assert torch.equal(got.double(), ref + bias.double()), "bias"


@pytest.mark.parametrize("case,view", ROWS, ids=IDS)
def test_exact(dev, case, view):
    check_exact(case, view, dev, torch.float32)


@pytest.mark.parametrize("case,view,cfg", BF16_ROWS,
                         ids=["%s-%s-cfg%d" % (c.name, v, k) for c, v, k in BF16_ROWS])
def test_exact_bf16(dev, case, view, cfg):
    """The exact pass with bf16 math on bf16-stored operands (small integers are exact in bf16);
    cfg: the tile config the bf16 rules take (in the test id; no coverage requirement)."""
    check_exact(case, view, dev, torch.bfloat16)


@pytest.mark.parametrize("case,view", ROWS, ids=IDS)
def test_rounding(dev, case, view):
    c = case
    o = operands(c, "round", dev)
    ref, s = ref_of(c, view, "round", dev)
    got = run_view(c, view, o, dev).double()
    assert not torch.isnan(got).any()
    plan = T.tile(ops, c, view)
    # K + splits + 2 steps, splits = 0 for fwd / dgrad.  Frame chunks (the `chunks` row) change
    # the wgrad only: each chunk reduces its own splits and adds into dW, so its splits count per
    # chunk plus one add per further chunk
    splits = plan["splits"] if view == "wgrad" else 0
    if view == "wgrad" and "max_frames" in c.extras:
        nchunks = -(-c.n // c.extras["max_frames"])
        splits = splits * nchunks + nchunks - 1
    steps = T.gemm_k(c, view) + splits + 2
    err = (got - ref).abs()
    excess = (err - steps * EPS * s).max().item()
    worst = (err / (steps * EPS * s).clamp_min(1e-300)).max().item()
    # torch fp32 of the same operands against the same reference
    base = ref_matmul(c, view, o["x"], o["w"], o["dy"])
    rel = (err.max() / ref.abs().max()).item()
    rel_t = ((base.double() - ref).abs().max() / ref.abs().max()).item()
    rec = {"case": c.name, "view": view, "cfg": plan["cfg"], "rel": rel, "rel_torch": rel_t,
           "ratio": rel / max(rel_t, 1e-30), "elem_bound_used": worst}
    print(json.dumps(rec))
    if os.environ.get("TMR_CONV_ENGINE_RATIOS"):
        with open(os.environ["TMR_CONV_ENGINE_RATIOS"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert excess <= 0, "element error %.3g of its bound" % worst
    assert rel <= max(3 * rel_t, 2e-6), (rel, rel_t)


def test_im2col_reference_matches_conv2d(dev):
    """The two references on a mid-size 3x3 stride-2 pad-1 case, every view, to 1e-12."""
    c = T.Case("im2col", 4, 29, 27, 64, 96, 3, 2, 1, {}, {})
    g = torch.Generator().manual_seed(3)
    ho, wo = T.out_hw(c)
    x = torch.randn(c.n, c.h, c.w, c.cin, generator=g, dtype=F64)
    w = torch.randn(c.cout, c.cin, 3, 3, generator=g, dtype=F64) / 24
    dy = torch.randn(c.n, ho, wo, c.cout, generator=g, dtype=F64)
    for view in VIEWS:
        a = ref_conv2d(c, view, x, w, dy)
        b = ref_matmul(c, view, x.to(dev), w.to(dev), dy.to(dev)).cpu()
        assert a.shape == b.shape
        assert ((a - b).abs().max() / a.abs().max()).item() < 1e-12, view


# ------------------------------------------------------------------ fused forms on the large tiles
BY_NAME = {c.name: c for c in T.CASES}


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30)).item()


def _krsc(o):
    return o["w"].permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("name", ["c64_64_ragM", "c8_128_tapv8", "c64_256_cfg1", "c64_256_cfg6"])
def test_fwd_bnstats_large_tiles(dev, name):
    """conv_fwd_bnstats on configs 3, 7, 1, 6: y bit-identical to conv_fwd, the statistics against
    float64 of y with the tolerances of test_conv_fused_bn_stats."""
    c = BY_NAME[name]
    assert c.expect["fwd"][1] in (3, 7, 1, 6)
    o = operands(c, "round", dev)
    x = torch.relu(o["x"]) + 0.5            # non-zero-mean input
    y_ref = ops.conv_fwd(x, _krsc(o), c.stride, c.pad)
    y, stats, nparts = ops.conv_fwd_bnstats(x, _krsc(o), c.stride, c.pad)
    assert torch.equal(y, y_ref)
    yd = y_ref.double().view(-1, c.cout)
    rm, rv = torch.zeros(c.cout, device=dev), torch.ones(c.cout, device=dev)
    mean, inv, _, _ = ops.bn_finalize(stats, nparts, torch.ones(c.cout, device=dev),
                                      torch.zeros(c.cout, device=dev), rm, rv, 0.1, 1e-5)
    assert _rel(mean, yd.mean(0)) < 1e-6
    assert _rel(inv, 1 / torch.sqrt(yd.var(0, unbiased=False) + 1e-5)) < 1e-5
    assert _rel(rv, 0.9 + 0.1 * yd.var(0, unbiased=True)) < 1e-6


@pytest.mark.parametrize("name", ["c8_128_tapv8", "c64_256_cfg6"])
@pytest.mark.parametrize("res,relu", [(True, True), (False, False)])
def test_fwd_fused_large_tiles(dev, name, res, relu):
    """conv_fwd_fused on configs 7 and 6: bit-identical to conv_fwd + bn_apply, and within 1e-5
    of float64 (test_conv_fused_eval_bn)."""
    c = BY_NAME[name]
    assert c.expect["fwd"][1] in (7, 6)
    o = operands(c, "round", dev)
    ref, _ = ref_of(c, "fwd", "round", dev)
    g = gen(c, "fwd_fused", dev)
    scale = torch.rand(c.cout, generator=g, device=dev) + 0.5
    shift = torch.randn(c.cout, generator=g, device=dev)
    y = ops.conv_fwd(o["x"], _krsc(o), c.stride, c.pad)
    resid = torch.randn(y.shape, generator=g, device=dev) if res else None
    z_ref = ops.bn_apply(y, scale, shift, resid, relu)
    z = ops.conv_fwd_fused(o["x"], _krsc(o), c.stride, c.pad, scale, shift, resid, relu)
    torch.cuda.synchronize()
    assert torch.equal(z, z_ref)
    zd = ref * scale.double() + shift.double()
    if res:
        zd = zd + resid.double()
    if relu:
        zd = zd.clamp_min(0)
    assert _rel(z, zd) < 1e-5


# (row, mask, tiles): masks 0-3 on configs 3 and 7 and on the two rows the wave-specialised launch
# takes (configs 7 and 2; gemm16_ws.h: mask bits, beta 1), those also one tile per workgroup
DGRAD_FUSED = ([(n, m, False) for n in ("c64_64_ragM", "c512_128") for m in range(4)] +
               [(c.name, m, t) for c in T.CASES if c.extras.get("ws") for m in range(4)
                for t in (False, True)])


@pytest.mark.parametrize("name,mask,tiles", DGRAD_FUSED,
                         ids=["%s-mask%d%s" % (n, m, "-tiles" if t else "") for n, m, t in DGRAD_FUSED])
def test_dgrad_bnbwd_large_tiles(dev, name, mask, tiles):
    """conv_dgrad_bnbwd (fp32 LDS-DMA engine, beta = 1 into a prefilled dx) on configs 3, 7 and 2
    against the float64 closed form: dx = mask * (old + dgrad), parts = per-channel sums of dx and
    dx * (y - mean).  Integer operands (y in halves, scale a power of two, shift k + 1/4): every
    value is exact, so dx must match bit for bit and the mask has no borderline element.  On the
    rows marked ws, mask 3 must run the wave-specialised persistent kernel (tmr_dgrad_ws_launches
    counts it) and, with tiles (TMR_IO_TILES), the one-tile-per-workgroup launch; every other
    combination must not count a wave-specialised launch."""
    from tmrnet_amd import _lib
    c = BY_NAME[name]
    assert c.expect["dgrad"][1] in (3, 7, 2) and (c.r, c.stride) == (1, 1)
    o = operands(c, "exact", dev)
    dxr, _ = ref_of(c, "dgrad", "exact", dev)
    g = gen(c, "dgrad_bnbwd", dev)
    shp = (c.n, c.h, c.w, c.cin)
    y = torch.randint(-6, 7, shp, generator=g, device=dev).float() / 2
    mean = torch.randint(-1, 2, (c.cin,), generator=g, device=dev).float()
    scale = torch.tensor([1.0, 2.0, 0.5, -1.0], device=dev).repeat(c.cin // 4)
    shift = torch.randint(-2, 3, (c.cin,), generator=g, device=dev).float() + 0.25
    zint = torch.randint(-3, 4, shp, generator=g, device=dev).float()
    old = torch.randint(-3, 4, shp, generator=g, device=dev).float()
    z = None
    if mask == 0:
        m = torch.ones(shp, device=dev, dtype=torch.bool)
    elif mask == 2:
        m = (y.double() * scale.double() + shift.double()) > 0
    else:
        m = zint > 0
        z = torch.relu(zint) if mask == 1 else pack_bits(m)
    want = (old.double() + dxr) * m
    wc = o["w"].permute(1, 2, 3, 0).contiguous()
    before = _lib.query("tmr_dgrad_ws_launches")
    with (ops.dgrad_tile_launches() if tiles else T.run_form(ops, c)):
        dz, parts, nparts = ops.conv_dgrad_bnbwd(o["dy"], wc, (c.h, c.w), 1, 0, y, mean, mask, z=z,
                                                 scale=scale, shift=shift, out=old.clone(), beta=1.0,
                                                 wt=True)
    torch.cuda.synchronize()
    ws = _lib.query("tmr_dgrad_ws_launches") - before
    print("%s mask %d tiles %s: wave-specialised launches %d, %d part rows" % (name, mask, tiles, ws, nparts))
    assert ws == (1 if c.extras.get("ws") and mask == 3 and not tiles else 0)
    assert torch.equal(dz.double(), want)
    p = parts[:nparts].double().sum(0)
    s0 = want.view(-1, c.cin).sum(0)
    s1 = (want * (y.double() - mean.double())).view(-1, c.cin).sum(0)
    assert _rel(p[:, 0], s0) < 1e-5 and _rel(p[:, 1], s1) < 1e-5


@pytest.mark.parametrize("name", ["c64_64_ragM", "c256_64_w4", "wsplit_cfg4", "c512_128",
                                  "c32_200_3x3", "wsplit_cfg7"])
def test_wgrad_bnbwd_against_float64(dev, name):
    """conv_wgrad_bnbwd on its three configs (64x64, 64x256, 128x128 as 8 waves; ragged tiles and
    the short last split among them): dy = A*g + B*y + C and dW against float64 directly.  Small
    integer g, y, coefficients and x: |dy| <= 13, |x * dy| <= 39 and 39*K < 2^24, so both are
    exact and must match bit for bit."""
    c = BY_NAME[name]
    cfg = c.expect["wgrad"][1]
    assert cfg in (5, 4, 7) and 39 * T.gemm_k(c, "wgrad") < 2 ** 24
    o = operands(c, "exact", dev)
    ho, wo = T.out_hw(c)
    gn = gen(c, "wgrad_bnbwd", dev)
    g = o["dy"]
    y = torch.randint(-3, 4, g.shape, generator=gn, device=dev).float()
    coef = torch.cat([torch.tensor([1.0, -1.0, 2.0, 1.0], device=dev).repeat(c.cout // 4),
                      torch.tensor([2.0, 1.0, -1.0, -1.0], device=dev).repeat(c.cout // 4),
                      torch.randint(-1, 2, (c.cout,), generator=gn, device=dev).float()])
    assert ops.conv_wgrad_bnbwd_ok(o["x"], g, y, c.r, c.r, c.stride, c.pad)
    A, B, C = coef.double().view(3, c.cout)
    dy_ref = A * g.double() + B * y.double() + C
    big = T.flops(c) >= 1e9
    f = ref_matmul if big else ref_conv2d
    args = [o["x"].double(), o["w"].double(), dy_ref]
    dw_ref = f(c, "wgrad", *(args if big else [t.cpu() for t in args])).to(dev)
    dw, dy = ops.conv_wgrad_bnbwd(o["x"], g, y, coef, c.r, c.r, c.stride, c.pad)
    torch.cuda.synchronize()
    assert torch.equal(dy.double(), dy_ref)
    assert torch.equal(dw.double(), dw_ref)
