"""The bounds of tests/_splat_ref.py are fair and sharp (no GPU).

Fair: an emulation of each kernel of csrc/resnest.hip in torch ops -- fp32 where the kernel computes
in fp32, float64 where it accumulates in double, fmaf as the exactly rounded a * b + c -- stays inside
every bound at every SMALL shape.  Sharp: the same emulation with one planted error leaves its
bound, one test per error.
"""
import pytest
import torch

from tests import _splat_ref as R
from tests._splat_ref import BF16, f32, halves, ratio

ONE = torch.tensor(1.0, dtype=f32)


def fma32(a, b, c):
    """fmaf: the product of two fp32 is exact in float64, the sum carries 2^-53"""
    return (a.double() * b.double() + c.double()).float()


def ops32(k, *names):
    """the case's operands as the kernel holds them: fp32 (a bf16 y widened: the same values)"""
    return [k[n].float() for n in names]


# ------------------------------------------------------------------ emulations
def emu_bnrelu(y, sc, sh, bf16, ge=False):
    v = fma32(y, sc, sh)
    x = torch.relu(v)
    if bf16:
        x = x.to(BF16).float()
    return x, (v >= 0 if ge else v > 0)


def emu_gap(x, C, skip_last=False):
    hw = x.shape[1]
    xs = x.double()[:, :hw - 1] if skip_last else x.double()
    x0, x1 = halves(xs, C)
    return ((x0.sum(1) + x1.sum(1)) * (1.0 / hw)).float()


def emu_att(z, C):
    z0, z1 = halves(z, C)
    m = torch.maximum(z0, z1)
    e0, e1 = torch.exp(z0 - m), torch.exp(z1 - m)
    inv = ONE / (e0 + e1)
    return torch.cat([e0 * inv, e1 * inv], -1)


def emu_combine(x, z, C):
    att = emu_att(z, C)
    (a0, a1), (x0, x1) = halves(att, C), halves(x, C)
    return att, a0.unsqueeze(1) * x0 + a1.unsqueeze(1) * x1


def emu_combine_bn(y, sc, sh, att, C, bf16, swap_last_quad=False):
    x, _ = emu_bnrelu(y, sc, sh, bf16)
    a0, a1 = (t.clone() for t in halves(att, C))
    if swap_last_quad:
        a0[:, C - 4:], a1[:, C - 4:] = att[:, 2 * C - 4:], att[:, C - 4:C]
    x0, x1 = halves(x, C)
    out = fma32(a1.unsqueeze(1), x1, a0.unsqueeze(1) * x0)
    return out.to(BF16) if bf16 else out


def _emu_softmax_bwd(dout, x, att, C):
    x0, x1 = halves(x.double(), C)
    a0, a1 = halves(att.double(), C)
    p0, p1 = (dout.double() * x0).sum(1), (dout.double() * x1).sum(1)
    dot = a0 * p0 + a1 * p1
    return torch.cat([a0 * (p0 - dot), a1 * (p1 - dot)], -1).float()


def emu_bwd(dout, x, att, C):
    return _emu_softmax_bwd(dout, x, att, C)


def emu_reduce_bn(dout, y, sc, sh, mean, att, C, bf16, ge=False, s4_unmasked=False):
    x, m = emu_bnrelu(y, sc, sh, bf16, ge)
    m = m.double()
    g2 = torch.cat([dout, dout], -1).double()
    d = (y - mean).double()                 # the fp32 subtraction
    sums = torch.stack([(m * g2).sum(1), m.sum(1), (m * g2 * d).sum(1),
                        (d if s4_unmasked else m * d).sum(1)]).float()
    return _emu_softmax_bwd(dout, x, att, C), sums


def emu_coefs(att, dgap, sums, invstd, gamma, n, hw, C, swap12=False):
    a, s = att.double(), sums.double()
    dg = torch.cat([dgap, dgap], -1).double() * (1.0 / hw)
    sg = (a * s[0] + dg * s[1]).sum(0)
    sgx = (a * s[2] + dg * s[3]).sum(0)
    inv, N = invstd.double(), float(n * hw)
    rows = [gamma.double() * inv, sg / N, inv * inv * sgx / N]
    if swap12:
        rows = [rows[0], rows[2], rows[1]]
    return {"dbeta": sg.float(), "dgamma": (sgx * inv).float(), "coef0": rows[0].float(),
            "coef1": rows[1].float(), "coef2": rows[2].float()}


def emu_apply(dout, att, dgap, hw):
    inv = ONE / torch.tensor(float(hw), dtype=f32)
    return att.unsqueeze(1) * torch.cat([dout, dout], -1) + (torch.cat([dgap, dgap], -1) * inv).unsqueeze(1)


def emu_apply_bn(dout, y, sc, sh, mean, att, dgap, coef, hw, bf16, ge=False, frame0=False):
    _, m = emu_bnrelu(y, sc, sh, bf16, ge)
    ihw = ONE / torch.tensor(float(hw), dtype=f32)
    dg = torch.cat([dgap, dgap], -1) * ihw
    if frame0:
        dg = dg[:1].expand_as(dg)
    gg = fma32(att.unsqueeze(1), torch.cat([dout, dout], -1), dg.unsqueeze(1))
    gg = torch.where(m, gg, torch.zeros_like(gg))
    out = coef[0] * (gg - coef[1] - (y - mean) * coef[2])
    return out.to(BF16) if bf16 else out


def emu_center(x):
    m = (x.double().sum(0) / x.shape[0]).float()
    return m, x - m


def emu_axpy(alpha, x, y):
    return fma32(torch.tensor(alpha, dtype=f32), x, y)


def _divisor(ho, wo, h, w, k, s, p, incl, kk):
    """fp32 1 / divisor per output [ho][wo]: nn.AvgPool2d's rule, restated; kk: the k * k mistake"""
    y0 = torch.arange(ho).view(ho, 1) * s - p
    x0 = torch.arange(wo).view(1, wo) * s - p
    if incl and kk:
        div = torch.full((ho, wo), k * k)
    elif incl:
        div = ((y0 + k).clamp(max=h + p) - y0) * ((x0 + k).clamp(max=w + p) - x0)
    else:
        div = ((y0 + k).clamp(max=h) - y0.clamp(min=0)) * ((x0 + k).clamp(max=w) - x0.clamp(min=0))
    return ONE / div.float()


def _taps(ho, wo, h, w, k, s, p, dy, dx):
    """the outputs whose tap (dy, dx) is inside the input, and the input cell it reads"""
    oy, ox = torch.arange(ho), torch.arange(wo)
    iy, ix = oy * s - p + dy, ox * s - p + dx
    vy, vx = (iy >= 0) & (iy < h), (ix >= 0) & (ix < w)
    return oy[vy].view(-1, 1), ox[vx].view(1, -1), iy[vy].view(-1, 1), ix[vx].view(1, -1)


def emu_pool_fwd(x, ho, wo, k, s, p, incl, kk=False):
    """fp32 sums of the taps in window order (x fp32, or bf16 widened), times the fp32 reciprocal"""
    n, h, w, c = x.shape
    acc = torch.zeros(n, ho, wo, c)
    for dy in range(k):
        for dx in range(k):
            oy, ox, iy, ix = _taps(ho, wo, h, w, k, s, p, dy, dx)
            acc[:, oy, ox] = acc[:, oy, ox] + x[:, iy, ix].float()
    out = acc * _divisor(ho, wo, h, w, k, s, p, incl, kk).view(1, ho, wo, 1)
    return out.to(BF16) if x.dtype == BF16 else out


def emu_pool_bwd(dy_, h, w, k, s, p, incl, kk=False):
    """per input cell, dy * (1 / div) of the windows that hold it, outputs in ascending order"""
    n, ho, wo, c = dy_.shape
    t = dy_ * _divisor(ho, wo, h, w, k, s, p, incl, kk).view(1, ho, wo, 1)
    dx_ = torch.zeros(n, h, w, c)
    for dy in reversed(range(k)):
        for dx in reversed(range(k)):
            oy, ox, iy, ix = _taps(ho, wo, h, w, k, s, p, dy, dx)
            dx_[:, iy, ix] = dx_[:, iy, ix] + t[:, oy, ox]
    return dx_


# ------------------------------------------------------------------ fair
def _sp(shape):
    k = R.splat_case(*shape)
    return k, k["n"], k["hw"], k["C"]


@pytest.mark.parametrize("shape", R.SMALL)
def test_emulation_within_bounds_unfused(shape):
    """tmr_splat_gap / att / combine / bwd / bwd_apply"""
    k, n, hw, C = _sp(shape)
    x, z, att, dout, dgap = ops32(k, "x", "z", "att", "dout", "dgap")
    assert ratio(emu_gap(x, C), *R.ref_gap(k["x"], C)) <= 1
    a = emu_att(z, C)
    assert ratio(a, *R.ref_att(k["z"], C)) <= 1
    assert (a[:, :C].double() + a[:, C:].double() - 1).abs().max().item() <= 2 * R.U
    (ra, ro), (ea, eo) = R.ref_combine(k["x"], k["z"], C), emu_combine(x, z, C)
    assert ratio(ea, *ra) <= 1 and ratio(eo, *ro) <= 1
    assert ratio(emu_bwd(dout, x, att, C), *R.ref_bwd(k["dout"], k["x"], k["att"], C)) <= 1
    assert ratio(emu_apply(dout, att, dgap, hw), *R.ref_bwd_apply(k["dout"], k["att"], k["dgap"], hw)) <= 1


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", R.SMALL)
def test_emulation_within_bounds_bn(shape, bf16):
    """the `_bn` entry points and tmr_splat_bn0_coefs; a share of the pre-activations is 0"""
    k, n, hw, C = _sp(shape)
    y, sc, sh, mean, att, dout, dgap, coef, sums, invstd, gamma = ops32(
        k, "y", "scale", "shift", "mean", "att", "dout", "dgap", "coef", "sums", "invstd", "gamma")
    if n * hw * C >= 2000:
        zero = (k["y"] * k["scale"] + k["shift"] == 0).double().mean().item()
        assert 0.03 < zero < 0.12, zero
    assert ratio(emu_gap(emu_bnrelu(y, sc, sh, bf16)[0], C),
                 *R.ref_gap_bn(k["y"], k["scale"], k["shift"], C, bf16)) <= 1
    assert ratio(emu_combine_bn(y, sc, sh, att, C, bf16),
                 *R.ref_combine_bn(k["y"], k["scale"], k["shift"], k["att"], C, bf16)) <= 1
    dzl, s = emu_reduce_bn(dout, y, sc, sh, mean, att, C, bf16)
    rd, rs = R.ref_bwd_reduce_bn(k["dout"], k["y"], k["scale"], k["shift"], k["mean"], k["att"], C, bf16)
    assert ratio(dzl, *rd) <= 1 and ratio(s, *rs) <= 1
    assert torch.equal(s[1].double(), rs[0][1])
    got = emu_coefs(att, dgap, sums, invstd, gamma, n, hw, C)
    ref = R.ref_bn0_coefs(k["att"], k["dgap"], k["sums"], k["invstd"], k["gamma"], n, hw, C)
    for name, rb in ref.items():
        assert ratio(got[name], *rb) <= 1, name
    assert ratio(emu_apply_bn(dout, y, sc, sh, mean, att, dgap, coef, hw, bf16),
                 *R.ref_bwd_apply_bn(k["dout"], k["y"], k["scale"], k["shift"], k["mean"], k["att"],
                                     k["dgap"], k["coef"], hw, bf16)) <= 1


def test_emulation_within_bounds_att_many():
    """2 M pairs of N(0, 3) logits (the GPU file's BIG att case): the relative bound and the 2U
    bound of a0 + a1 - 1 hold for every one"""
    n, C = R.BIG_ATT
    z = R.logits(n, C, torch.Generator().manual_seed(5))
    a = emu_att(z.float(), C)
    assert ratio(a, *R.ref_att(z, C)) <= 1
    assert (a[:, :C].double() + a[:, C:].double() - 1).abs().max().item() <= 2 * R.U


@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("cols", R.COLS)
def test_emulation_within_bounds_center(rows, cols):
    x = R.center_case(rows, cols)
    m, xc = emu_center(x.float())
    assert ratio(m, *R.ref_center_cols(x)) <= 1
    assert torch.equal(xc, x.float() - m)


@pytest.mark.parametrize("n", R.AXPY_N[:4])
def test_emulation_within_bounds_axpy(n):
    g = torch.Generator().manual_seed(n)
    x, y = R.rnd(n, g=g), R.rnd(n, g=g)
    alpha = float(torch.tensor(0.37, dtype=f32))
    assert ratio(emu_axpy(alpha, x.float(), y.float()), *R.ref_axpy(alpha, x, y)) <= 1


pool_case = R.pool_case


@pytest.mark.parametrize("case", R.POOL_SMALL)
def test_emulation_within_bounds_pool(case):
    n, h, w, c, k, s, p, incl, ceil = case
    x, x16, g = pool_case(case)
    ref, bound = R.ref_avgpool2d_fwd(x, k, s, p, incl, ceil)
    ho, wo = ref.shape[1:3]
    assert ratio(emu_pool_fwd(x.float(), ho, wo, k, s, p, incl), ref, bound) <= 1
    assert ratio(emu_pool_fwd(x16.to(BF16), ho, wo, k, s, p, incl),
                 *R.ref_avgpool2d_fwd(x16, k, s, p, incl, ceil, bf16=True)) <= 1
    dy = R.rnd(n, ho, wo, c, g=g)
    assert ratio(emu_pool_bwd(dy.float(), h, w, k, s, p, incl),
                 *R.ref_avgpool2d_bwd(dy, (h, w), k, s, p, incl, ceil)) <= 1


# ------------------------------------------------------------------ sharp
MUT = (5, 7, 7, 40)


@pytest.mark.parametrize("case", R.POOL_OVERHANG)
def test_planted_kk_divisor(case):
    """the k * k divisor on a window that hangs over the padded extent: forward, bf16, backward"""
    n, h, w, c, k, s, p, incl, ceil = case
    x, x16, g = pool_case(case)
    ref, bound = R.ref_avgpool2d_fwd(x, k, s, p, incl, ceil)
    ho, wo = ref.shape[1:3]
    assert ratio(emu_pool_fwd(x.float(), ho, wo, k, s, p, incl, kk=True), ref, bound) > 1
    assert ratio(emu_pool_fwd(x16.to(BF16), ho, wo, k, s, p, incl, kk=True),
                 *R.ref_avgpool2d_fwd(x16, k, s, p, incl, ceil, bf16=True)) > 1
    dy = R.rnd(n, ho, wo, c, g=g)
    assert ratio(emu_pool_bwd(dy.float(), h, w, k, s, p, incl, kk=True),
                 *R.ref_avgpool2d_bwd(dy, (h, w), k, s, p, incl, ceil)) > 1


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_planted_mask_ge(bf16):
    """mask `>= 0`: the planted zero pre-activations enter S1..S4 and the apply"""
    k, n, hw, C = _sp(MUT)
    y, sc, sh, mean, att, dout, dgap, coef = ops32(k, "y", "scale", "shift", "mean", "att", "dout",
                                                   "dgap", "coef")
    _, s = emu_reduce_bn(dout, y, sc, sh, mean, att, C, bf16, ge=True)
    _, (rs, bs) = R.ref_bwd_reduce_bn(k["dout"], k["y"], k["scale"], k["shift"], k["mean"], k["att"], C, bf16)
    assert not torch.equal(s[1].double(), rs[1])
    for i in (0, 2, 3):
        assert ratio(s[i], rs[i], bs[i]) > 1, i
    assert ratio(emu_apply_bn(dout, y, sc, sh, mean, att, dgap, coef, hw, bf16, ge=True),
                 *R.ref_bwd_apply_bn(k["dout"], k["y"], k["scale"], k["shift"], k["mean"], k["att"],
                                     k["dgap"], k["coef"], hw, bf16)) > 1


def test_planted_s4_unmasked():
    k, n, hw, C = _sp(MUT)
    y, sc, sh, mean, att, dout = ops32(k, "y", "scale", "shift", "mean", "att", "dout")
    _, s = emu_reduce_bn(dout, y, sc, sh, mean, att, C, False, s4_unmasked=True)
    _, (rs, bs) = R.ref_bwd_reduce_bn(k["dout"], k["y"], k["scale"], k["shift"], k["mean"], k["att"],
                                      C, False)
    assert ratio(s[3], rs[3], bs[3]) > 1
    assert max(ratio(s[i], rs[i], bs[i]) for i in (0, 1, 2)) <= 1


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_planted_dgap_frame0(bf16):
    """dgap / hw of frame 0 used for every frame (a frame cache that never refreshes)"""
    k, n, hw, C = _sp(MUT)
    y, sc, sh, mean, att, dout, dgap, coef = ops32(k, "y", "scale", "shift", "mean", "att", "dout",
                                                   "dgap", "coef")
    out = emu_apply_bn(dout, y, sc, sh, mean, att, dgap, coef, hw, bf16, frame0=True)
    ref, bound = R.ref_bwd_apply_bn(k["dout"], k["y"], k["scale"], k["shift"], k["mean"], k["att"],
                                    k["dgap"], k["coef"], hw, bf16)
    assert ratio(out[:1], ref[:1], bound[:1]) <= 1 and ratio(out[1:], ref[1:], bound[1:]) > 1


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_planted_att_halves_swapped_last_quad(bf16):
    """only the last four channels are wrong: an L2 norm over the tensor would not see it"""
    k, n, hw, C = _sp(MUT)
    y, sc, sh, att = ops32(k, "y", "scale", "shift", "att")
    out = emu_combine_bn(y, sc, sh, att, C, bf16, swap_last_quad=True)
    ref, bound = R.ref_combine_bn(k["y"], k["scale"], k["shift"], k["att"], C, bf16)
    assert ratio(out[..., :C - 4], ref[..., :C - 4], bound[..., :C - 4]) <= 1
    assert ratio(out[..., C - 4:], ref[..., C - 4:], bound[..., C - 4:]) > 1


def test_planted_coef_rows_exchanged():
    k, n, hw, C = _sp(MUT)
    att, dgap, sums, invstd, gamma = ops32(k, "att", "dgap", "sums", "invstd", "gamma")
    got = emu_coefs(att, dgap, sums, invstd, gamma, n, hw, C, swap12=True)
    ref = R.ref_bn0_coefs(k["att"], k["dgap"], k["sums"], k["invstd"], k["gamma"], n, hw, C)
    assert ratio(got["coef1"], *ref["coef1"]) > 1 and ratio(got["coef2"], *ref["coef2"]) > 1
    assert max(ratio(got[m], *ref[m]) for m in ("dbeta", "dgamma", "coef0")) <= 1


@pytest.mark.parametrize("bf16", [None, False, True], ids=["unfused", "fp32", "bf16"])
def test_planted_gap_without_last_pixel(bf16):
    k, n, hw, C = _sp(MUT)
    if bf16 is None:
        out, rb = emu_gap(k["x"].float(), C, skip_last=True), R.ref_gap(k["x"], C)
    else:
        y, sc, sh = ops32(k, "y", "scale", "shift")
        out = emu_gap(emu_bnrelu(y, sc, sh, bf16)[0], C, skip_last=True)
        rb = R.ref_gap_bn(k["y"], k["scale"], k["shift"], C, bf16)
    assert ratio(out, *rb) > 1
