"""freeze_bn(affine=False, forward="fused") on the GPU: the fp32 fused forward that also writes a
bf16 copy (tmr_conv2d_fwd_fused_dual) at every tile config and launch form an fp32 forward takes,
the masked dgrad (ops.conv_dgrad_relu), and the 2-frame step against the unfused affine=False step
bit for bit and against the float64 oracle / emulation (tests/_frozen_fused.py)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import tmrnet_amd
from tmrnet_amd import ops, trunk, _lib
from tmrnet_amd._lib import stream_ptr
from tests import _conv_engine_cases as T
from tests import _frozen_bn as F
from tests._frozen_bn import SENT, intact, _buffers, _keep
from tests import _frozen_bwd16 as X
from tests import _frozen_fused as Z

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "frozen_fused")
BF16 = torch.bfloat16
F64 = torch.float64
EPS = 2.0 ** -24
BY_NAME = {c.name: c for c in T.CASES}


def record(key, value):
    """Merge one figure into profiles/frozen_fused/step_parity.json (a read-only checkout keeps
    the committed record)."""
    path = os.path.join(OUT, "step_parity.json")
    try:
        os.makedirs(OUT, exist_ok=True)
        rec = {}
        if os.path.exists(path):
            with open(path) as f:
                rec = json.load(f)
        rec[key] = value
        with open(path, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
    except (OSError, ValueError):
        pass


def guarded(shape, dev, dtype=torch.float32):
    """A NaN-filled tensor between two sentinel zones -> (whole buffer, view)."""
    return F.guarded(shape, dev, float("nan"), dtype)


# ------------------------------------------------------------------ the dual forward
# one row per fp32 forward config and launch form: (row, config, TAPV)
DUAL_ROWS = [("tiny", 5, 0), ("c64_128_3x3", 2, 0), ("c64_64_ragM", 3, 0), ("c8_128_tapv8", 7, 1),
             ("c4_128_k4", 7, 0), ("c64_256_cfg1", 1, 0), ("c64_256_cfg6", 6, 0),
             ("c32_200_ragN", 2, 0), ("c16_128_tapv16", 2, 1), ("chunks", 2, 0)]
VARIANTS = [(True, True), (True, False), (False, True), (False, False)]   # (residual, relu)


def im2col(x, r, stride, pad):
    n, h, w, c = x.shape
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1
    if r == 1 and stride == 1 and pad == 0:
        return x.reshape(-1, c)
    xp = Fn.pad(x, (0, 0, pad, pad, pad, pad))
    cols = [xp[:, i:i + stride * (ho - 1) + 1:stride, j:j + stride * (wo - 1) + 1:stride, :]
            for i in range(r) for j in range(r)]
    return torch.cat(cols, dim=3).reshape(n * ho * wo, r * r * c)


def conv64(c, x, wk):
    """float64 conv on the device: x (n,h,w,cin), wk KRSC -> (n,ho,wo,cout).  Plain torch."""
    ho, wo = T.out_hw(c)
    return (im2col(x.double(), c.r, c.stride, c.pad) @ wk.double().reshape(c.cout, -1).t()).view(
        c.n, ho, wo, c.cout)


def run_dual(c, dev, x, wk, scale, shift, res, relu):
    """One tmr_conv2d_fwd_fused_dual call between sentinels -> (z, z16)."""
    ho, wo = T.out_hw(c)
    with T.run_form(ops, c):
        d = ops.conv_desc(c.n, c.h, c.w, c.cin, c.cout, c.r, c.r, c.stride, c.pad)
        zf, z = guarded((c.n, ho, wo, c.cout), dev)
        hf, z16 = guarded((c.n, ho, wo, c.cout), dev, BF16)
        _lib.call("tmr_conv2d_fwd_fused_dual", ctypes.byref(d), x, wk, scale, shift, res, z, z16,
                  int(relu), stream_ptr())
    torch.cuda.synchronize()
    assert intact(zf) and intact(hf), "wrote outside z / z16"
    assert not torch.isnan(z).any() and not torch.isnan(z16.float()).any(), "elements never written"
    return z, z16


_EXACT = {}


def exact_case(c, dev):
    """Exact-grid operands of one row and their float64 reference pieces, computed once per row
    and shared by its four variants (never written).  x, w: integers in [-3, 3] (9*K < 2^24: the
    accumulator is an exact integer); scale +-2^-j, shift on the 1/16 grid: fmaf(acc, scale,
    shift) is exact in fp32 (9*K*16 < 2^24, asserted).  Planted: channel 0 scale 2^-4, shift 24 --
    its outputs (acc + 384) / 16 are exact bf16 ties of both parities wherever acc is odd;
    channel 1 scale 1, shift 0 with the input zeroed under output pixel (0, 0, 0): the ReLU's
    argument is exactly 0; the residual cancels channel 2 to zero and plants ties of both
    parities in channel 3."""
    if _EXACT.get("name") != c.name:
        _EXACT.clear()
        torch.cuda.empty_cache()
        g = torch.Generator(device=dev).manual_seed(1000 + len(c.name) * 37 + c.cin)
        k = c.r * c.r * c.cin
        assert 9 * k * 16 + 64 * 16 < 2 ** 24
        ho, wo = T.out_hw(c)
        x = torch.randint(-3, 4, (c.n, c.h, c.w, c.cin), generator=g, device=dev).float()
        x[0, :2, :2, :] = 0.0
        w = torch.randint(-3, 4, (c.cout, c.r, c.r, c.cin), generator=g, device=dev).float()
        j = torch.randint(0, 4, (c.cout,), generator=g, device=dev)
        sign = torch.randint(0, 2, (c.cout,), generator=g, device=dev).float() * 2 - 1
        scale = sign * torch.pow(2.0, -j.float())
        shift = torch.randint(-64, 65, (c.cout,), generator=g, device=dev).float() / 16
        scale[0], shift[0] = 2.0 ** -4, 24.0
        scale[1], shift[1] = 1.0, 0.0
        acc = conv64(c, x, w)
        pre = acc * scale.double() + shift.double()
        assert torch.equal(pre, pre.float().double())            # the fmaf is exact
        res = torch.randint(-256, 257, (c.n, ho, wo, c.cout), generator=g, device=dev).double() / 16
        res[..., 0] = 0.0
        res[0, 0, 0, 1] = 0.0
        res[..., 2] = -pre[..., 2]
        m = torch.randint(128, 256, (c.n, ho, wo), generator=g, device=dev).double() * 2 + 1
        res[..., 3] = m / 16 - pre[..., 3]                       # z = m / 16, m odd in [257, 511]
        assert torch.equal(res, res.float().double())
        assert torch.equal(pre + res, (pre + res).float().double())
        _EXACT.update(name=c.name, x=x, w=w, scale=scale, shift=shift, pre=pre, res=res)
    return _EXACT


def _ties(z):
    u = torch.from_numpy(Z.bits32(z.cpu().numpy()).astype(np.int64))
    tie = ((u & 0xFFFF) == 0x8000) & (z.cpu() != 0)
    return int((tie & ((u >> 16) & 1 == 0)).sum()), int((tie & ((u >> 16) & 1 == 1)).sum())


@pytest.mark.parametrize("res,relu", VARIANTS, ids=["res-relu", "res", "relu", "plain"])
@pytest.mark.parametrize("name,cfg,tapv", DUAL_ROWS, ids=[r[0] for r in DUAL_ROWS])
def test_dual_exact(dev, name, cfg, tapv, res, relu):
    """z bit for bit the float64 reference, z16 bit for bit its round-to-nearest-even, on exact
    grids with planted ties, zeros of the ReLU's argument and a cancelling residual."""
    c = BY_NAME[name]
    plan = T.tile(ops, c, "fwd")
    assert (plan["engine"], plan["cfg"], plan["tapv"]) == (2, cfg, tapv), plan
    o = exact_case(c, dev)
    want = o["pre"] + (o["res"] if res else 0.0)
    if relu:
        want = want.clamp_min(0.0)
    want = want.float()
    even, odd = _ties(want[..., 0] if not res else want[..., 3])
    assert even > 0 and odd > 0, "no planted ties of both parities"
    assert want[0, 0, 0, 1] == 0                                  # the ReLU's argument is 0
    if res:
        assert (want[..., 2] == 0).all() and (o["res"][..., 2] != 0).any()
    z, z16 = run_dual(c, dev, o["x"], o["w"], o["scale"], o["shift"],
                      o["res"].float() if res else None, relu)
    bad = Z.compare_dual(z.cpu().numpy(), Z.bits16(z16), want.cpu().numpy())
    assert bad == [], (name, res, relu, bad)
    assert torch.equal(z16, want.to(BF16))


@pytest.mark.parametrize("res,relu", VARIANTS, ids=["res-relu", "res", "relu", "plain"])
@pytest.mark.parametrize("name,cfg,tapv", DUAL_ROWS, ids=[r[0] for r in DUAL_ROWS])
def test_dual_against_the_existing_ops(dev, name, cfg, tapv, res, relu):
    """Random operands: z is conv_fwd_fused's z and conv_fwd + bn_apply's (with residual and
    ReLU: bn_apply_bits's) bit for bit, z16 is ops.to_bf16(z); the wrapper gives the same."""
    c = BY_NAME[name]
    g = torch.Generator(device=dev).manual_seed(7 + c.cin * 3 + c.cout)
    ho, wo = T.out_hw(c)
    x = torch.randn(c.n, c.h, c.w, c.cin, generator=g, device=dev)
    wk = torch.randn(c.cout, c.r, c.r, c.cin, generator=g, device=dev) / math.sqrt(c.r * c.r * c.cin)
    scale = torch.rand(c.cout, generator=g, device=dev) + 0.5
    shift = torch.randn(c.cout, generator=g, device=dev)
    resid = torch.randn(c.n, ho, wo, c.cout, generator=g, device=dev) if res else None
    z, z16 = run_dual(c, dev, x, wk, scale, shift, resid, relu)
    with T.run_form(ops, c), ops.engine_only():
        zf = ops.conv_fwd_fused(x, wk, c.stride, c.pad, scale, shift, resid, relu)
        y = ops.conv_fwd(x, wk, c.stride, c.pad)
        za, zb = ops.conv_fwd_fused_dual(x, wk, c.stride, c.pad, scale, shift, resid, relu)
    assert torch.equal(z, zf)
    assert torch.equal(z16, ops.to_bf16(z)) and torch.equal(z16, z.to(BF16))
    assert torch.equal(z, ops.bn_apply(y, scale, shift, resid, relu))
    if res and relu and c.cout % 8 == 0 and (ho * wo * c.cout) % 32 == 0:
        assert torch.equal(z, ops.bn_apply_bits(y, scale, shift, resid)[0])
    assert torch.equal(za, z) and torch.equal(zb, z16)


def test_dual_refusals(dev):
    """Each refusal by name, nothing written: z and z16 keep their fill."""
    c = BY_NAME["tiny"]
    x = torch.randn(c.n, c.h, c.w, c.cin, device=dev)
    wk = torch.randn(c.cout, 1, 1, c.cin, device=dev)
    sc, sh = torch.ones(c.cout, device=dev), torch.zeros(c.cout, device=dev)
    shape = (c.n, c.h, c.w, c.cout)
    zf, z = guarded(shape, dev)
    hf, z16 = guarded(shape, dev, BF16)
    res = torch.randn(shape, device=dev)

    def call(d=None, x=x, wk=wk, res=None, z=z, z16=z16):
        d = d or ops.conv_desc(c.n, c.h, c.w, c.cin, c.cout, 1, 1, 1, 0)
        _lib.call("tmr_conv2d_fwd_fused_dual", ctypes.byref(d), x, wk, sc, sh, res, z, z16, 1,
                  stream_ptr())
    P = "tmr_conv2d_fwd_fused_dual: "
    with pytest.raises(RuntimeError, match=P + "fp32 operands in fp32 math only"):
        call(ops.conv_desc(c.n, c.h, c.w, c.cin, c.cout, 1, 1, 1, 0, math="bf16"))
    with pytest.raises(RuntimeError, match="bf16-stored operands|fp32 operands in fp32 math only"):
        call(ops.conv_desc(c.n, c.h, c.w, c.cin, c.cout, 1, 1, 1, 0, math="bf16",
                           io=ops.IO_X | ops.IO_W))
    with pytest.raises(RuntimeError, match=P + "no grouped conv"):
        call(ops.conv_desc(c.n, c.h, c.w, c.cin, c.cout, 1, 1, 1, 0, groups=2))
    d = ops.conv_desc(c.n, c.h, c.w, c.cin, c.cout, 1, 1, 1, 0, y_ld=c.cout + 8)
    with pytest.raises(RuntimeError, match=P + "z and z16 must be dense"):
        call(d)
    with pytest.raises(RuntimeError, match=P + "output channels 15 must be even"):
        call(ops.conv_desc(c.n, c.h, c.w, c.cin, 15, 1, 1, 1, 0))
    with pytest.raises(RuntimeError, match=P + "null z16"):
        call(z16=None)
    with pytest.raises(RuntimeError, match=P + "z16 overlaps z or the residual"):
        call(z16=z)
    with pytest.raises(RuntimeError, match=P + "z16 overlaps z or the residual"):
        call(res=res, z16=res)
    with pytest.raises(RuntimeError, match=P + "residual must not alias z"):
        call(res=z)
    off = torch.full((z16.numel() + 8,), SENT, dtype=BF16, device=dev)
    with pytest.raises(RuntimeError, match=P + ".*16-B aligned"):
        call(z16=off[2:2 + z16.numel()])
    # a shape the LDS-DMA engine does not serve: a misaligned x (no two-pass fall-back)
    xo = torch.zeros(x.numel() + 4, device=dev)[1:1 + x.numel()].view(x.shape)
    with pytest.raises(RuntimeError, match=P + "not a shape of the fp32 LDS-DMA forward"):
        call(x=xo)
    torch.cuda.synchronize()
    assert torch.isnan(z).all() and torch.isnan(z16.float()).all() and (off == SENT).all()
    assert intact(zf) and intact(hf)
    # the wrapper's own checks come before any library call
    with pytest.raises(RuntimeError, match="conv_fwd_fused_dual: fp32 operands in fp32 math only"):
        ops.conv_fwd_fused_dual(x.to(BF16), wk.to(BF16), 1, 0, sc, sh)
    with pytest.raises(RuntimeError, match="conv_fwd_fused_dual: the residual stays fp32"):
        ops.conv_fwd_fused_dual(x, wk, 1, 0, sc, sh, res.to(BF16))
    with pytest.raises(RuntimeError, match="conv_fwd_fused_dual: output channels 15 must be even"):
        ops.conv_fwd_fused_dual(x, wk[:15].contiguous(), 1, 0, sc[:15], sh[:15])
    call()                                                        # the plain call goes through
    torch.cuda.synchronize()
    assert not torch.isnan(z).any() and intact(zf) and intact(hf)


# ------------------------------------------------------------------ the masked dgrad
DGRAD_ROWS = ["c64_128_3x3", "c512_128", "c512_2048_l4", "c256_64_ws", "s2_odd"]


def dgrad64(c, dy, w_oihw):
    """float64 dgrad and S = sum |dy| |w| on the device (1x1 stride 1: a matmul) or the CPU."""
    if c.r == 1 and c.stride == 1:
        wm = w_oihw.double().view(c.cout, c.cin)
        a = dy.double().reshape(-1, c.cout)
        return ((a @ wm).view(c.n, c.h, c.w, c.cin), (a.abs() @ wm.abs()).view(c.n, c.h, c.w, c.cin))
    f = lambda a, b: torch.nn.grad.conv2d_input(
        (c.n, c.cin, c.h, c.w), b, a.permute(0, 3, 1, 2), stride=c.stride,
        padding=c.pad).permute(0, 2, 3, 1).contiguous()
    a, b = dy.double().cpu(), w_oihw.double().cpu()
    return f(a, b).to(dy.device), f(a.abs(), b.abs()).to(dy.device)


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
@pytest.mark.parametrize("name", DGRAD_ROWS)
def test_dgrad_relu(dev, name, kind):
    """ops.conv_dgrad_relu, beta 0 and 1, fp32 z and bf16 z with bf16 dy / weights: on exact-grid
    operands dx is conv_dgrad followed by an explicit where(z > 0, ., 0) bit for bit (z == 0
    planted: it passes nothing); on random operands dx stays within (K + 2) * 2^-24 * sum|a||b| of
    the float64 dgrad of the operands as stored (test_conv_engine_gpu's dgrad bound)."""
    c = BY_NAME[name]
    dt = torch.float32 if kind == "fp32" else BF16
    mth = "fp32" if kind == "fp32" else "bf16"
    ho, wo = T.out_hw(c)
    g = torch.Generator(device=dev).manual_seed(31 + c.cin + 7 * c.cout)
    shp = (c.n, c.h, c.w, c.cin)
    ri = lambda s, lo=-3, hi=3: torch.randint(lo, hi + 1, s, generator=g, device=dev).float()
    assert 9 * T.gemm_k(c, "dgrad") + 6 < 2 ** 24
    dy, w = ri((c.n, ho, wo, c.cout)).to(dt), ri((c.cout, c.cin, c.r, c.r))
    wc = w.permute(1, 2, 3, 0).contiguous().to(dt)                # (cin, r, s, cout)
    z = torch.relu(ri(shp)).to(dt)
    assert (z == 0).any() and (z > 0).any()
    old = ri(shp)
    kw = dict(math=mth, wt=True)
    with T.run_form(ops, c):
        for beta in (0.0, 1.0):
            plain = ops.conv_dgrad(dy, wc, (c.h, c.w), c.stride, c.pad,
                                   out=old.clone() if beta else None, beta=beta, **kw)
            want = torch.where(z > 0, plain, torch.zeros_like(plain))
            got = ops.conv_dgrad_relu(dy, wc, (c.h, c.w), c.stride, c.pad, z,
                                      out=old.clone() if beta else None, beta=beta, **kw)
            torch.cuda.synchronize()
            assert got.dtype == torch.float32
            bad = Z.compare_mask(got.cpu().numpy(), plain.cpu().numpy(), z.float().cpu().numpy())
            assert bad == [] and torch.equal(got, want), (name, kind, beta, bad)
            assert (got[z == 0] == 0).all()
        if kind == "bf16":      # the non-residual units' form: g stored bf16, rounded once
            g16 = ops.conv_dgrad_relu(dy, wc, (c.h, c.w), c.stride, c.pad, z, g16=True, **kw)
            want = torch.where(z > 0, ops.conv_dgrad(dy, wc, (c.h, c.w), c.stride, c.pad, **kw),
                               torch.zeros(shp, device=dev))
            assert g16.dtype == BF16 and torch.equal(g16, want.to(BF16))
        # random operands (as stored: the bf16 ones are the rounded values)
        dy = (torch.randn(c.n, ho, wo, c.cout, generator=g, device=dev) * 0.5).to(dt)
        w = (torch.randn(c.cout, c.cin, c.r, c.r, generator=g, device=dev)
             / math.sqrt(c.r * c.r * c.cout)).to(dt)
        wc = w.permute(1, 2, 3, 0).contiguous()
        zr = torch.relu(torch.randn(shp, generator=g, device=dev)).to(dt)
        got = ops.conv_dgrad_relu(dy, wc, (c.h, c.w), c.stride, c.pad, zr, **kw).double()
    ref, s = dgrad64(c, dy, w)
    on = zr.double() > 0
    steps = T.gemm_k(c, "dgrad") + 2
    err = (got - ref * on).abs()
    worst = (err / (steps * EPS * s).clamp_min(1e-300)).max().item()
    print("conv_dgrad_relu %s %s: element error %.3g of its bound" % (name, kind, worst))
    assert (err - steps * EPS * s).max().item() <= 0, worst
    assert (got[~on] == 0).all()


# ------------------------------------------------------------------ the step
MODES = [None, "bf16"]
IDS = ["bwd-fp32", "bwd-bf16"]


NOAFF = dict(affine=False)                      # the unfused partner's freeze_bn keywords
FUSED = dict(affine=False, forward="fused")     # the fused step's


_RUNS = {}


@pytest.fixture(scope="module")
def runs(dev):
    """Per backward: one step of the unfused affine=False model and of the fused one (computed
    once, never written) -> {backward: dict}."""
    def get(backward):
        if backward not in _RUNS:
            ref = _keep(F.hip_step(F.hip_model(dev, backward=backward, **NOAFF), dev))
            m = F.hip_model(dev, backward=backward, **FUSED)
            before = _buffers(m)
            got = _keep(F.hip_step(m, dev))
            _RUNS[backward] = {"m": m, "before": before, "ref": ref, "got": got}
        return _RUNS[backward]
    return get


@pytest.mark.parametrize("backward", MODES, ids=IDS)
def test_step_is_the_unfused_step_bit_for_bit(runs, backward):
    """Logits, loss and every gradient torch.equal to the unfused affine=False step of the same
    backward; no statistic or counter moves."""
    r = runs(backward)
    (l0, loss0, g0), (l1, loss1, g1) = r["ref"], r["got"]
    assert torch.equal(l1, l0) and loss1 == loss0
    bn = Z.bn_names(r["m"].named_parameters())
    assert len(bn) == 106
    differ = []
    for n, g in g1.items():
        if n in bn:
            assert g is None and g0[n] is None, n
        elif not torch.equal(g, g0[n]):
            differ.append((n, (g - g0[n]).abs().max().item()))
    record("bit_identical_%s" % (backward or "fp32"), {"gradients": len(g1) - len(bn),
                                                       "differ": differ[:8], "loss": loss1})
    assert not differ, differ[:8]
    after = _buffers(r["m"])
    n = 0
    for name, b in r["before"].items():
        assert torch.equal(after[name], b), name
        n += name.endswith(("running_mean", "running_var", "num_batches_tracked"))
    assert n == 3 * 53


@pytest.mark.parametrize("backward", MODES, ids=IDS)
def test_step_gradients_against_float64(runs, backward):
    """Under _assert_vs_fp64 with the bounds of the unfused tests: the float64 oracle for the fp32
    backward (tests/test_frozen_bn_gpu.py), the float64 emulation of the bf16 contract with its
    fp32 run as the yardstick for the bf16 backward (tests/test_frozen_bwd16_gpu.py)."""
    from tests.test_model_parity_gpu import _assert_vs_fp64, l2_err
    r = runs(backward)
    logits, loss, grads = r["got"]
    bn = Z.bn_names(r["m"].named_parameters())
    if backward is None:
        rows = []
        F.assert_step(grads, logits, what="fused frozen step", record="frozen_fused_step",
                      rows_out=rows, absent=bn)
        worst = max(rows, key=lambda x: x["e_hip"] / max(x["e_cpu"], 1e-30))
        record("vs_fp64_fp32", {"worst": worst, "loss": loss})
        return
    e64, e32 = X.emu_step(torch.float64), X.emu_step(torch.float32)
    have = {n: g for n, g in grads.items() if n not in bn}
    assert all(g is not None for g in have.values()) and all(grads[n] is None for n in bn)
    rows = [(n, l2_err(g, e64["grads"][n]), l2_err(e32["grads"][n], e64["grads"][n]))
            for n, g in have.items() if not n.endswith("linear2.bias")]
    agg = (sum(x[1] ** 2 for x in rows) / sum(x[2] ** 2 for x in rows)) ** 0.5
    record("vs_fp64_bf16", {"agg_ratio_vs_fp64": agg, "loss": loss,
                            "max_ratio_vs_fp64": max(x[1] / max(x[2], 1e-12) for x in rows)})
    err = (logits.double().cpu() - e64["logits"]).abs().max().item()
    assert err < 1e-4, err
    _assert_vs_fp64(have, {n: e32["grads"][n] for n in have}, {n: e64["grads"][n] for n in have},
                    "frozen_fused16_grads")


@pytest.mark.parametrize("backward", MODES, ids=IDS)
def test_step_launches_and_records(runs, dev, backward, monkeypatch):
    """The step completes with every BatchNorm apply pass, the statistics forms and the finalizes
    replaced by functions that raise, and conv_fwd only for the stem; every non-stem record has
    no y and no mask bits, and its mask source is the tensor the next unit keeps as x."""
    def refuse(name):
        def f(*a, **k):
            raise AssertionError("the fused frozen step called ops.%s" % name)
        return f
    for name in ("bn_apply", "bn_apply_bits", "bn_apply2", "bn_apply2_bits", "bn_apply_dual",
                 "bn_apply_bits_dual", "bn_apply2_bits_dual", "conv_fwd_bnstats", "bn_finalize",
                 "bn_frozen_finalize", "bn_fwd_train", "bn_bwd", "bn_bwd_parts", "bn_bwd_parts_ds",
                 "counters_add_one"):
        monkeypatch.setattr(ops, name, refuse(name))
    real_fwd, stem_calls = ops.conv_fwd, []

    def conv_fwd(x, w, *a, **k):
        assert x.shape[-1] == 4 and tuple(w.shape[1:3]) == (7, 7), "conv_fwd for a non-stem conv"
        stem_calls.append(tuple(x.shape))
        return real_fwd(x, w, *a, **k)
    monkeypatch.setattr(ops, "conv_fwd", conv_fwd)
    seen = {"dual": 0, "fused": 0, "relu": 0, "bnbwd": 0}
    for key, name in (("dual", "conv_fwd_fused_dual"), ("fused", "conv_fwd_fused"),
                      ("relu", "conv_dgrad_relu")):
        orig = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _o=orig, _k=key, **k:
                            (seen.__setitem__(_k, seen[_k] + 1), _o(*a, **k))[1])
    recs, stems = [], []
    real_fused, real_run = trunk._TrainUnits.fused, trunk._TrainUnits._run
    monkeypatch.setattr(trunk._TrainUnits, "fused", lambda self, *a, **k:
                        (lambda out: (recs.append(out[2]), out)[1])(real_fused(self, *a, **k)))
    monkeypatch.setattr(trunk._TrainUnits, "_run", lambda self, *a, **k:
                        (lambda out: (stems.append(out[3]), out)[1])(real_run(self, *a, **k)))
    r = runs(backward)
    logits, loss, grads = F.hip_step(r["m"], dev)
    assert torch.equal(logits, r["got"][0])
    for n, g in grads.items():
        assert (g is None and r["got"][2][n] is None) or torch.equal(g, r["got"][2][n]), n
    assert len(stem_calls) == 1 and len(stems) == 1 and len(recs) == 52
    assert stems[0].y is not None                                 # the one unit that stores y
    b16 = backward == "bf16"
    # bf16 backward: every unit but the downsample branches and the last block's conv3 is dual
    assert (seen["dual"], seen["fused"]) == ((52 - 4 - 1, 5) if b16 else (0, 52))
    # every dgrad that produces a unit's gradient masks by that unit's output: 3 per block but the
    # first block's conv1 (its dx is the stem's pooled gradient); the 4 downsample dgrads are plain
    assert seen["relu"] == 3 * 16 - 1
    for i, rec in enumerate(recs):
        assert rec.y is None and rec.zbits is None, i
        if rec.relu:
            last = i == len(recs) - 1
            assert rec.z is not None
            assert rec.z.dtype == (BF16 if b16 and not last else torch.float32), i
        else:
            assert rec.z is None and not rec.res                  # a downsample branch
    # the mask source is the next conv's operand itself: no extra memory
    by_conv = {id(rec.conv): rec for rec in recs}
    for blk in [b for l in r["m"].share.trunk_parts()[2] for b in l]:
        r1, r2 = by_conv[id(blk.conv1)], by_conv[id(blk.conv2)]
        assert r2.x is r1.z and by_conv[id(blk.conv3)].x is r2.z


def test_both_share_kinds_and_unfreeze(dev, runs):
    """backward="bf16": the "fp32" and the "bf16-bwd" share give the same bits; unfreeze_bn gives
    back the share's own step, torch.equal to a never-frozen model's."""
    want = runs("bf16")["got"]
    m = F.hip_model(dev, backward="bf16", precision="bf16-bwd", **FUSED)
    logits, _, grads = F.hip_step(m, dev)
    assert torch.equal(logits, want[0])
    for n, g in grads.items():
        assert (g is None and want[2][n] is None) or torch.equal(g, want[2][n]), n
    for precision, mm in (("bf16-bwd", m), ("fp32", F.hip_model(dev, **FUSED))):
        a = F.hip_model(dev, frozen=False, precision=precision)
        b = tmrnet_amd.unfreeze_bn(mm)
        assert b.share.bn_frozen_fwd is None
        la, _, ga = F.hip_step(a, dev)
        lb, _, gb = F.hip_step(b, dev)
        assert torch.equal(la, lb)
        for n in ga:
            assert torch.equal(ga[n], gb[n]), n
        for (n, x), (_, y) in zip(a.named_buffers(), b.named_buffers()):
            assert torch.equal(x, y), n
        assert int(b.share.bn1.num_batches_tracked) == 1


@pytest.mark.parametrize("backward", MODES, ids=IDS)
def test_batch_independence(dev, runs, backward):
    """2 clips x 2 frames: clip A's logits bit-identical in (A, B), in (A, C) and alone;
    grad(A + B) against grad(A) + grad(B) within the relative gap the unfused tests allow
    (GRAD_RATIO x the fp32 CPU run's distance of its grad(A + B) from the float64 sum -- of the
    oracle for the fp32 backward, of the emulation for the bf16 backward; linear2.bias, whose exact
    gradient is 0, 1e-5 of the largest norm)."""
    from tests.test_model_parity_gpu import GRAD_RATIO, AGG_RATIO, l2_err
    r = runs(backward)
    m = r["m"]
    bn = Z.bn_names(m.named_parameters())
    keep = lambda t: (t[0].clone(), {n: g.detach().clone() for n, g in t[2].items() if n not in bn})
    l_ab, g_ab = keep(F.hip_step(m, dev, (0, 1)))
    l_ac, _ = keep(F.hip_step(m, dev, (0, 2)))
    l_b, g_b = keep(F.hip_step(m, dev, (1,)))
    l_a, g_a = r["got"][0], r["got"][2]
    assert torch.equal(l_ab[0], l_ac[0]) and torch.equal(l_ab[0], l_a[0])
    assert torch.equal(l_ab[1], l_b[0])
    step = F.oracle_step if backward is None else X.emu_step
    e64 = {k: step(torch.float64, k) for k in ((0,), (1,))}
    e32 = step(torch.float32, (0, 1))
    summed64 = {n: e64[(0,)]["grads"][n] + e64[(1,)]["grads"][n] for n in g_ab}
    gmax = max(g.norm().item() for g in g_ab.values())
    rows, bad = [], []
    for n, g in g_ab.items():
        s = g_a[n].double() + g_b[n].double()
        e_acc = l2_err(g, summed64[n])
        e_cpu = l2_err(e32["grads"][n], summed64[n])
        if n.endswith("linear2.bias"):
            ok = (g.double() - s).norm().item() <= 1e-5 * gmax
        else:
            e_hip = l2_err(g, s)
            ok = e_hip <= GRAD_RATIO * e_cpu
            rows.append((n, e_hip, e_cpu, e_acc))
        if not ok:
            bad.append((n, l2_err(g, s), e_cpu))
    agg = (sum(x[3] ** 2 for x in rows) / sum(x[2] ** 2 for x in rows)) ** 0.5
    worst = max(rows, key=lambda x: x[1] / x[2])
    record("batch_independence_%s" % (backward or "fp32"),
           {"worst": worst[0], "defect": worst[1], "yardstick": worst[2], "agg_vs_fp64": agg})
    assert not bad, bad[:5]
    assert agg <= AGG_RATIO, agg


@pytest.mark.parametrize("backward", MODES, ids=IDS)
def test_short_trajectory(dev, backward):
    """Five SGD steps: the fused run's losses equal the unfused run's, and no statistic moves."""
    from oracle import tmrnet_ref as ref
    x4, lt, labels, masks = F.hip_inputs(dev)
    crit = tmrnet_amd.CrossEntropyLoss(size_average=False)
    traj = {}
    for key in ("unfused", "fused"):
        m = F.hip_model(dev, backward=backward, **(FUSED if key == "fused" else NOAFF))
        m.nl_block.forced_mask, m.forced_head_mask = masks["nl"], masks["head"]
        opt = tmrnet_amd.SGD(ref.sgd_param_groups(m, F.LR), lr=F.LR / 10, momentum=0.9,
                             weight_decay=5e-4)
        before = _buffers(m)
        losses = []
        for _ in range(F.STEPS):
            opt.zero_grad()
            loss = crit(m(x4, lt), labels)
            loss.backward()
            opt.step()
            losses.append(float(loss.item()))
        traj[key] = losses
        after = _buffers(m)
        assert all(torch.equal(after[n], b) for n, b in before.items())
    record("trajectory_%s" % (backward or "fp32"), traj)
    assert traj["fused"] == traj["unfused"], traj
    assert (np.diff(np.asarray(traj["fused"])) < 0).all(), traj


@pytest.mark.parametrize("backward", MODES, ids=IDS)
def test_peak_memory_is_below_the_unfused_step(dev, backward):
    """One step at 8 frames (after a first step, so that weight copies and workspaces exist on both
    sides): max_memory_allocated of the fused step is strictly below the unfused affine=False
    step's.  The measured ratio goes to profiles/frozen_fused/step_parity.json; no ratio is fixed."""
    g = torch.Generator().manual_seed(5)
    clips = 8 // F.T
    x4 = torch.randn(8, 224, 224, 4, generator=g)
    x4[..., 3] = 0
    x4, lt = x4.to(dev), (torch.rand(clips, F.L, 512, generator=g) * 2 - 1).to(dev)
    labels = torch.randint(0, 7, (clips,), generator=g).to(dev)
    crit = tmrnet_amd.CrossEntropyLoss(size_average=False)
    peak = {}
    for key in ("unfused", "fused"):
        m = F.hip_model(dev, backward=backward, **(FUSED if key == "fused" else NOAFF))
        for it in range(2):
            for p in m.parameters():
                p.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            crit(m(x4, lt), labels).backward()
            torch.cuda.synchronize()
            peak[key] = (torch.cuda.max_memory_allocated(), base)
        del m
        torch.cuda.empty_cache()
    rec = {"frames": 8, "unfused": peak["unfused"][0], "fused": peak["fused"][0],
           "resident_before": {k: v[1] for k, v in peak.items()},
           "ratio": peak["fused"][0] / peak["unfused"][0],
           "ratio_above_resident": (peak["fused"][0] - peak["fused"][1])
           / max(1, peak["unfused"][0] - peak["unfused"][1])}
    print("fused frozen step memory (%s):" % (backward or "fp32"), json.dumps(rec))
    record("memory_%s" % (backward or "fp32"), rec)
    assert peak["fused"][0] < peak["unfused"][0], rec
