"""Shared pieces of the tests of the frozen-BatchNorm step with bf16 backward convs
(tmrnet_amd.freeze_bn(backward="bf16"), "frozen16"; tests/test_frozen_bwd16_cpu.py, _gpu.py).

The contract (tmrnet_amd/trunk.py "_frozen16"): the fp32 frozen forward bit for
bit; every trunk conv's dgrad / wgrad on bf16 operands with three roundings, RNE, each once:
  x    the conv's input;
  w    a folded unit's dgrad reads bf16(w[k] * scale[k]), the product formed in fp32; the
       single-pass units (the last block's bn3 / downsample BN, the stem) bf16(w);
  g    a folded unit's convs take bf16(g), the masked gradient unscaled (dW rows are scaled in
       fp32 afterwards); a single-pass unit's take bf16(g * scale).
BN sums (dgamma, dbeta) are of the rounded g for bn1 / bn2 -- the fused dgrad stores that g bf16
-- and of the unrounded g elsewhere (the residual stream stays fp32).

Three parts:
  * x_case / emu_x / compare_x: operands, a numpy emulation and the comparison of the
    tmr_bn_frozen_bwd*_x entry points against their fp32 siblings; compare_wscaled for
    ops.weight_to_crsk_scaled(bf16=True).  tests/test_frozen_bwd16_cpu.py plants errors in the
    emulation's outputs to show that the comparisons can fail.
  * g16_dgrads: the ResNet-50 dgrads the step sends with TMR_IO_G16.
  * emulate(): the oracle's conv + frozen-BN units with the contract's backward, float64 or
    float32, on tests/_frozen_bn's model and step_case()."""
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn

from tests import _bwd16 as H
from tests import _frozen_bn as F

rne_bf16, trunc_bf16, pack_bits = H.rne_bf16, H.trunc_bf16, H.pack_bits


def half_up_bf16(x):
    """The wrong rounding that takes an exact tie away from zero whatever the parity."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x8000) >> 16).astype(np.uint16)


def bits16(t):
    """bf16 torch tensor -> uint16 bit patterns (numpy)."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- the _x entry points
def ties(gen, n, parity):
    """n fp32 values exactly halfway between two bf16 values whose kept mantissa ends in
    `parity` (0: RNE rounds down in magnitude, 1: up), random sign and exponent near 1."""
    top = gen.integers(0, 64, n).astype(np.uint32) * 2 + np.uint32(parity)      # 7 mantissa bits
    exp = gen.integers(125, 130, n).astype(np.uint32)
    sign = gen.integers(0, 2, n).astype(np.uint32)
    return ((sign << 31) | (exp << 23) | (top << 16) | np.uint32(0x8000)).view(np.float32)


def x_case(rows, c, seed):
    """Operands of one case (numpy fp32): g and y random (products with the random scales are
    not bf16 values), channel 0's scales 0.5 so that the exact ties planted in g[:, 0] (both
    parities) stay ties in g * scale; z / y planted so that the mask's argument is exactly 0
    (z == 0; y = 0 under shift 0 in channel 1) on ~1/8 of the elements."""
    gen = np.random.default_rng(seed)
    f = lambda *s: gen.standard_normal(s).astype(np.float32)
    k = dict(g=f(rows, c), y=f(rows, c), yd=f(rows, c), z=f(rows, c),
             scale=(0.5 + gen.random(c)).astype(np.float32),
             scale_d=(0.5 + gen.random(c)).astype(np.float32),
             shift=(0.1 * f(c)), mean=0.2 * f(c), mean_d=0.2 * f(c))
    k["scale"][0] = k["scale_d"][0] = 0.5
    k["shift"][1] = 0.0
    k["g"][:, 0] = ties(gen, rows, 0)
    k["g"][1::2, 0] = ties(gen, rows, 1)[1::2]
    zero = gen.random((rows, c)) < 0.125
    k["z"] = np.where(zero, np.float32(0), np.maximum(k["z"], 0)).astype(np.float32)
    k["y"][:, 1] = np.where(zero[:, 1], np.float32(0), k["y"][:, 1])
    k["zero"] = zero
    return k


def mask_of(k, mask):
    if mask == 0:
        return np.ones_like(k["g"], dtype=bool)
    if mask == 2:   # the forward's fmaf, exactly: float64 holds the product and the sum's rounding
        v = (k["y"].astype(np.float64) * k["scale"].astype(np.float64)
             + k["shift"].astype(np.float64)).astype(np.float32)
        return v > 0
    return k["z"] > 0


def emu_x(k, mask, dual):
    """The fp32 entry point's dres / dy / dy_ds and the _x form's bf16 outputs (uint16 bits)."""
    gm = np.where(mask_of(k, mask), k["g"], np.float32(0)).astype(np.float32)
    dy = (gm * k["scale"]).astype(np.float32)
    out = dict(dres=gm, dy=dy, dy16=rne_bf16(dy), g16=rne_bf16(gm))
    if dual:
        dyd = (gm * k["scale_d"]).astype(np.float32)
        out.update(dyd=dyd, dyd16=rne_bf16(dyd))
    return out


def compare_x(got, ref):
    """An _x call (dict of numpy arrays: dy16 / dyd16 / g16 uint16 bits, dres, parts, parts_d fp32;
    absent or None: not produced) against the fp32 entry point's outputs (dy, dyd, dres, parts,
    parts_d) -> list of what differs."""
    bad = []
    for name, src in (("dy16", "dy"), ("dyd16", "dyd"), ("g16", "dres")):
        if got.get(name) is not None and not np.array_equal(got[name], rne_bf16(ref[src])):
            bad.append("%s != RNE(fp32 call's %s)" % (name, src))
    for name in ("dres", "parts", "parts_d"):
        if got.get(name) is not None and not np.array_equal(bits32(got[name]), bits32(ref[name])):
            bad.append("%s != fp32 call's" % name)
    return bad


def wscaled_want(w, scale):
    """(K, C, R, S) fp32 w, (K,) scale -> the bf16 bits of CRSK(w) * scale[k], the product formed
    in fp32 and rounded once."""
    p = (np.asarray(w, np.float32) * np.asarray(scale, np.float32)[:, None, None, None])
    return rne_bf16(np.ascontiguousarray(p.astype(np.float32).transpose(1, 2, 3, 0)))


def compare_wscaled(got_bits, w, scale):
    return [] if np.array_equal(got_bits, wscaled_want(w, scale)) else \
        ["scaled CRSK copy != RNE(fp32 w * scale)"]


# ---------------------------------------------------------------- routing
def g16_dgrads():
    """The ResNet-50 dgrads the step sends with TMR_IO_G16: every block's conv3 (it produces
    bn2's masked gradient) and conv2 (bn1's)."""
    return [c for c in H.resnet50_convs() if c[0].endswith((".conv2", ".conv3"))]


# ---------------------------------------------------------------- the emulation step
def _r16(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _UnitFn(torch.autograd.Function):
    """conv + eval-mode BatchNorm of the oracle as one node whose backward is the contract's.
    kind: "mid" (bn1 / bn2: g itself is stored bf16), "out" (a folded block output: bn3 or a
    downsample BN but the last block's), "single" (the last block's bn3 / downsample BN, the
    stem).  plant: None, or one of PLANTS."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, mean, var, eps, stride, padding, kind, plant):
        y = Fn.conv2d(x, w, None, stride, padding)
        ctx.save_for_backward(x, w, gamma, mean, var, y)
        ctx.cfg = (eps, stride, padding, kind, plant)
        return Fn.batch_norm(y, mean, var, gamma, beta, False, 0.0, eps)

    @staticmethod
    def backward(ctx, g):
        x, w, gamma, mean, var, y = ctx.saved_tensors
        eps, stride, padding, kind, plant = ctx.cfg
        dt = g.dtype
        v = lambda t: t.view(1, -1, 1, 1)
        # the coefficients as the device forms them: fp32 (tmr_bn_frozen_params)
        inv32 = 1.0 / torch.sqrt(var.float() + eps)
        scale32 = gamma.float() * inv32
        inv, scale = inv32.to(dt), scale32.to(dt)
        rnd = (lambda t: (t.float().view(torch.int32) & -65536).view(torch.float32).to(t.dtype)) \
            if plant == "trunc" else _r16
        g16 = rnd(g)
        gs = g16 if (kind == "mid" or plant == "sums_rounded") else g
        dgamma = (gs * (y - v(mean))).sum((0, 2, 3)) * inv
        dbeta = gs.sum((0, 2, 3))
        xb = rnd(x)
        if kind == "single":
            gop, wb, post = rnd(g * v(scale)), rnd(w), None
        else:
            gop = rnd(g * v(scale)) if plant == "g16_scaled" else g16
            if plant == "w_rounded_first":
                wb = rnd(w) * v(scale).view(-1, 1, 1, 1)
            else:
                wb = rnd((w.float() * scale32.view(-1, 1, 1, 1)).to(dt))
            post = None if plant == "g16_scaled" else scale
        dx = None
        if ctx.needs_input_grad[0]:
            wd = rnd(w) if plant == "g16_scaled" and kind != "single" else wb
            dx = torch.nn.grad.conv2d_input(x.shape, wd, gop, stride, padding)
        dw = torch.nn.grad.conv2d_weight(xb, w.shape, gop, stride, padding)
        if post is not None:
            dw = dw * post.view(-1, 1, 1, 1)
        return dx, dw, dgamma, dbeta, None, None, None, None, None, None, None


# (the step-level plants: the emulation's gradients must move when the contract is broken)
PLANTS = ("trunc", "g16_scaled", "w_rounded_first", "sums_rounded")


class _UnitConv(nn.Conv2d):
    def forward(self, x):
        bn = self._unit[0]
        return _UnitFn.apply(x, self.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                             bn.eps, self.stride, self.padding, self._unit[1], self._unit[2])


class _UnitBN(nn.BatchNorm2d):
    def forward(self, x):   # (applied inside its conv's node)
        return x


def emulate(r, plant=None):
    """Switch the frozen oracle model r's trunk to the frozen16 contract (class swaps: the
    parameters, buffers and state_dict keys stay)."""
    share = r.share
    blocks = [b for n in ("layer1", "layer2", "layer3", "layer4") for b in getattr(share, n)]
    units = [(share.conv1, share.bn1, "single")]
    for b in blocks:
        last = b is blocks[-1]
        units += [(b.conv1, b.bn1, "mid"), (b.conv2, b.bn2, "mid"),
                  (b.conv3, b.bn3, "single" if last else "out")]
        if b.downsample is not None:
            units.append((b.downsample[0], b.downsample[1], "single" if last else "out"))
    assert len(units) == 53
    for conv, bn, kind in units:
        assert not bn.training
        conv.__class__ = _UnitConv
        conv._unit = (bn, kind, plant)   # (a tuple: the BN is not registered a second time)
        bn.__class__ = _UnitBN
    return r


def emu_model(dtype=torch.float64, plant=None):
    return emulate(F.oracle_model(dtype), plant)


@functools.lru_cache(maxsize=None)
def emu_step(dtype=torch.float64, clips=(0,), plant=None):
    """The cached emulation step (read-only: shared between tests) -> F.run_step's dict."""
    return F.run_step(emu_model(dtype, plant), clips, dtype)


def trunk_rel(ga, gb):
    """|ga - gb| / |gb| per trunk group (tests/_bwd16.group_rel)."""
    return H.group_rel(ga, gb)
