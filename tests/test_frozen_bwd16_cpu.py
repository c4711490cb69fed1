"""freeze_bn(backward="bf16") without a GPU: the interface, the routing of the step's G16
dgrads, the emulation step, and planted errors that the comparison helpers must flag."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import tmrnet_amd
from tmrnet_amd import ops
from tests import _frozen_bn as F
from tests import _frozen_bwd16 as X


def _bns(share):
    return [m for m in share.modules() if isinstance(m, nn.BatchNorm2d)]


# ------------------------------------------------------------------ 1. the interface
@pytest.mark.parametrize("precision", ["fp32", "bf16-bwd"])
def test_backward_bf16_sets_and_clears_the_flag(precision):
    torch.manual_seed(0)
    m = tmrnet_amd.resnet_lstm(seq_len=2, precision=precision).train()
    share = m.share
    assert share.bn_frozen is False and share.bn_frozen_bwd is None
    keys = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert tmrnet_amd.freeze_bn(m, backward="bf16") is m
    assert share.bn_frozen is True and share.bn_frozen_bwd == "bf16" and share.training
    assert not any(b.training for b in _bns(share))
    assert all(b.weight.requires_grad and b.bias.requires_grad for b in _bns(share))
    m.eval(), m.train()
    assert not any(b.training for b in _bns(share))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == keys
    assert tmrnet_amd.unfreeze_bn(m) is m
    assert share.bn_frozen is False and share.bn_frozen_bwd is None
    assert all(b.training for b in _bns(share))
    tmrnet_amd.freeze_bn(m, affine=False, backward="bf16")
    assert not any(b.weight.requires_grad or b.bias.requires_grad for b in _bns(share))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == keys


def test_default_backward_is_todays_behaviour():
    for kw in ({}, {"backward": None}, {"backward": "fp32"}):
        m = tmrnet_amd.resnet_lstm(seq_len=2).train()
        tmrnet_amd.freeze_bn(m, **kw)
        assert m.share.bn_frozen is True and m.share.bn_frozen_bwd is None
        for prec in ("bf16", "bf16-bwd"):
            p = tmrnet_amd.resnet_lstm(seq_len=2, precision=prec).train()
            with pytest.raises(ValueError, match="precision 'fp32' only, not for '%s'" % prec):
                tmrnet_amd.freeze_bn(p, **kw)
            assert p.share.bn_frozen is False and all(b.training for b in _bns(p.share))
    # a second call without the flag goes back to the fp32 backward
    m = tmrnet_amd.freeze_bn(tmrnet_amd.resnet_lstm(seq_len=2).train(), backward="bf16")
    tmrnet_amd.freeze_bn(m)
    assert m.share.bn_frozen is True and m.share.bn_frozen_bwd is None


def test_new_refusals():
    with pytest.raises(ValueError, match='backward="bf16".*ResNeSt-50'):
        tmrnet_amd.freeze_bn(tmrnet_amd.resnet_lstm(seq_len=2, backbone="resnest50"),
                             backward="bf16")
    m = tmrnet_amd.resnet_lstm(seq_len=2, precision="bf16").train()
    with pytest.raises(ValueError, match='backward="bf16".*not for \'bf16\''):
        tmrnet_amd.freeze_bn(m, backward="bf16")
    assert m.share.bn_frozen is False and all(b.training for b in _bns(m.share))
    for bad in ("bf16-bwd", "fp16", True, 16):
        m = tmrnet_amd.resnet_lstm(seq_len=2).train()
        with pytest.raises(ValueError, match="backward must be"):
            tmrnet_amd.freeze_bn(m, backward=bad)
        assert m.share.bn_frozen is False and m.share.bn_frozen_bwd is None


def test_which_step_runs():
    from tmrnet_amd import trunk
    for prec in ("fp32", "bf16-bwd"):
        s = tmrnet_amd.ResNet50Share(precision=prec).train()
        assert not trunk._frozen_step(s) and not trunk._frozen16(s)
        tmrnet_amd.freeze_bn(s, backward="bf16")
        assert trunk._frozen_step(s) and trunk._frozen16(s)
        s.eval()
        assert not trunk._frozen_step(s) and not trunk._frozen16(s)
        tmrnet_amd.unfreeze_bn(s.train())
        assert not trunk._frozen_step(s) and not trunk._frozen16(s)
    s = tmrnet_amd.freeze_bn(tmrnet_amd.ResNet50Share().train())
    assert trunk._frozen_step(s) and not trunk._frozen16(s)


# ------------------------------------------------------------------ 2. routing
@pytest.mark.parametrize("n", [2, 640])
def test_g16_dgrads_plan_an_lds_staged_tile(n):
    """Every dgrad the step sends with TMR_IO_G16 (bf16 dy, bf16 CRSK weights; conv2 and conv3 of
    the 16 blocks) plans the LDS-DMA engine on a tile other than 256x256, which the library
    refuses for a bf16 masked gradient."""
    convs = X.g16_dgrads()
    assert len(convs) == 32
    for name, h, w, c, k, r, stride, pad in convs:
        t = ops.conv_tile(n, h, w, c, k, r, r, stride, pad, "dgrad", math="bf16",
                          io=ops.IO_DY | ops.IO_WT | ops.IO_G16)
        assert t["engine"] == 2, (name, t)
        assert (t["bm"], t["bn"]) != (256, 256), (name, t)


# ------------------------------------------------------------------ 3. the helpers can fail
@pytest.mark.parametrize("mask,dual", [(0, False), (1, True), (2, False), (3, True)])
def test_compare_x_catches_planted_errors(mask, dual):
    k = X.x_case(98, 24, 7)
    e = X.emu_x(k, mask, dual)
    m = X.mask_of(k, mask)
    assert (~m).sum() >= (k["zero"].sum() if mask == 1 else 0) and (mask == 0 or (~m).any())
    parts = np.stack([e["dres"].sum(0), (e["dres"] * (k["y"] - k["mean"])).sum(0)], -1)
    ref = dict(dy=e["dy"], dyd=e.get("dyd"), dres=e["dres"], parts=parts, parts_d=parts)
    good = dict(dy16=e["dy16"], dyd16=e.get("dyd16"), g16=e["g16"], dres=e["dres"], parts=parts)
    assert X.compare_x(good, ref) == []
    # the planted ties are there, of both parities, where the mask passes
    u = X.bits32(e["dres"][:, 0])
    tie = (u & 0xFFFF) == 0x8000
    assert (tie & ((u >> 16) & 1 == 0)).any() and (tie & ((u >> 16) & 1 == 1)).any()
    # truncation instead of RNE
    assert X.compare_x(dict(good, dy16=X.trunc_bf16(e["dy"])), ref)
    assert X.compare_x(dict(good, g16=X.trunc_bf16(e["dres"])), ref)
    # round-half-up: differs from RNE on the even-parity ties only
    hu = X.half_up_bf16(e["dres"])
    assert (hu != e["g16"]).sum() == (tie & ((u >> 16) & 1 == 0)).sum() > 0
    assert X.compare_x(dict(good, g16=hu), ref) == ["g16 != RNE(fp32 call's dres)"]
    assert X.compare_x(dict(good, dy16=X.half_up_bf16(e["dy"])), ref)
    # g16 carrying the scale
    assert X.compare_x(dict(good, g16=e["dy16"]), ref) == ["g16 != RNE(fp32 call's dres)"]
    # sums taken from the rounded g where the contract says fp32
    g16f = (e["g16"].astype(np.uint32) << 16).view(np.float32)
    p16 = np.stack([g16f.sum(0), (g16f * (k["y"] - k["mean"])).sum(0)], -1)
    assert X.compare_x(dict(good, parts=p16), ref) == ["parts != fp32 call's"]
    # the unmasked gradient
    if mask:
        assert X.compare_x(dict(good, g16=X.rne_bf16(k["g"])), ref)
    if dual:
        assert X.compare_x(dict(good, dyd16=e["dy16"]), ref) == ["dyd16 != RNE(fp32 call's dyd)"]


def test_compare_wscaled_catches_a_weight_rounded_before_the_multiply():
    gen = np.random.default_rng(5)
    w = gen.standard_normal((24, 16, 3, 3)).astype(np.float32)
    scale = (0.5 + gen.random(24)).astype(np.float32)
    want = X.wscaled_want(w, scale)
    assert want.shape == (16, 3, 3, 24)
    assert X.compare_wscaled(want, w, scale) == []
    w16 = (X.rne_bf16(w).astype(np.uint32) << 16).view(np.float32)
    first = X.rne_bf16(np.ascontiguousarray(
        (w16 * scale[:, None, None, None]).transpose(1, 2, 3, 0)))
    assert X.compare_wscaled(first, w, scale)
    assert X.compare_wscaled(X.trunc_bf16(np.ascontiguousarray(
        (w * scale[:, None, None, None]).transpose(1, 2, 3, 0))), w, scale)
    assert X.compare_wscaled(X.rne_bf16(np.ascontiguousarray(w.transpose(1, 2, 3, 0))), w, scale)


# ------------------------------------------------------------------ 4. the emulation step
def test_emulation_step_keeps_the_forward_and_the_statistics():
    """At step_case() (2 frames) the fp32 emulation gives the fp32 frozen oracle's logits bit for
    bit, writes no statistic, and moves only trunk gradients."""
    base = F.oracle_step(torch.float32)
    r = X.emu_model(torch.float32)
    before = {n: b.detach().clone() for n, b in r.named_buffers()}
    keys = list(r.state_dict().keys())
    assert keys == list(F.step_case()["sd"].keys())
    got = F.run_step(r, (0,), torch.float32)
    assert torch.equal(got["logits"], base["logits"]) and got["loss"] == base["loss"]
    for n, b in got["buffers"].items():
        assert torch.equal(b, before[n]), n
    moved = 0
    for n, g in got["grads"].items():
        if n.startswith("share."):
            moved += not torch.equal(g, base["grads"][n])
        else:
            assert torch.equal(g, base["grads"][n]), n
    assert moved >= 150
    rel = X.trunk_rel(got["grads"], base["grads"])
    assert all(1e-4 < v < 0.1 for v in rel.values()), rel


def test_emulation_gradients_are_additive_over_clips():
    """Frozen BN: every frame's rounded operands are its own, so grad(A + B) = grad(A) + grad(B)
    within float64 rounding."""
    a, b = X.emu_step(torch.float64, (0,)), X.emu_step(torch.float64, (1,))
    ab = X.emu_step(torch.float64, (0, 1))
    assert (ab["logits"][0] - a["logits"][0]).abs().max() < 1e-12
    for n, g in ab["grads"].items():
        s = a["grads"][n] + b["grads"][n]
        assert (g - s).norm() <= 1e-9 * max(s.norm().item(), 1e-30) + 1e-14, n


@pytest.mark.parametrize("plant", ["g16_scaled", "sums_rounded"])
def test_emulation_plants_move_the_gradients(plant):
    """A broken contract is another function: g16 carrying the scale moves the conv gradients,
    sums of the rounded g move a block output's BN gradients."""
    good = X.emu_step(torch.float64)
    bad = F.run_step(X.emu_model(torch.float64, plant), (0,), torch.float64)
    assert torch.equal(bad["logits"], good["logits"])
    name = "share.layer2.1.conv3.weight" if plant == "g16_scaled" else "share.layer2.1.bn3.weight"
    assert not torch.equal(bad["grads"][name], good["grads"][name])
    if plant == "sums_rounded":   # (bn1 / bn2 already sum the rounded g: unchanged)
        assert torch.equal(bad["grads"]["share.layer2.1.bn1.weight"],
                           good["grads"]["share.layer2.1.bn1.weight"])
