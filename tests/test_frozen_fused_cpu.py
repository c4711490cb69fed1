"""freeze_bn(forward="fused") without a GPU: the interface, the routing of the step's forwards and
dgrads, planted errors that the comparison helpers must flag, and the float64 oracle with BN
folded into the conv."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import tmrnet_amd
from tmrnet_amd import ops, trunk
from tests import _frozen_bn as F
from tests import _frozen_fused as Z


def _bns(share):
    return [m for m in share.modules() if isinstance(m, nn.BatchNorm2d)]


def _untouched(share):
    return (share.bn_frozen is False and share.bn_frozen_bwd is None
            and share.bn_frozen_fwd is None and all(b.training for b in _bns(share))
            and all(b.weight.requires_grad and b.bias.requires_grad for b in _bns(share)))


# ------------------------------------------------------------------ 1. the interface
@pytest.mark.parametrize("precision,backward", [("fp32", None), ("fp32", "fp32"), ("fp32", "bf16"),
                                                ("bf16-bwd", "bf16")])
def test_forward_fused_sets_and_clears_the_flag(precision, backward):
    torch.manual_seed(0)
    m = tmrnet_amd.resnet_lstm(seq_len=2, precision=precision).train()
    plain = tmrnet_amd.resnet_lstm(seq_len=2).train()
    share = m.share
    assert _untouched(share)
    keys = {k: tuple(v.shape) for k, v in plain.state_dict().items()}
    assert tmrnet_amd.freeze_bn(m, affine=False, backward=backward, forward="fused") is m
    assert share.bn_frozen is True and share.bn_frozen_fwd == "fused" and share.training
    assert share.bn_frozen_bwd == ("bf16" if backward == "bf16" else None)
    assert trunk._frozen_step(share) and trunk._frozen_fused(share)
    assert trunk._frozen16(share) == (backward == "bf16")
    assert not any(b.training for b in _bns(share))
    assert not any(b.weight.requires_grad or b.bias.requires_grad for b in _bns(share))
    m.eval()
    assert not trunk._frozen_fused(share)          # eval mode is the eval path
    m.train()
    assert trunk._frozen_fused(share) and not any(b.training for b in _bns(share))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == keys
    # a later call without the keyword goes back to the apply-pass forward, as backward does
    tmrnet_amd.freeze_bn(m, affine=False, backward=backward)
    assert share.bn_frozen is True and share.bn_frozen_fwd is None
    tmrnet_amd.freeze_bn(m, affine=False, backward=backward, forward="fused")
    assert tmrnet_amd.unfreeze_bn(m) is m
    assert _untouched(share) and not trunk._frozen_fused(share)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == keys


def test_defaults_leave_the_flag_at_none():
    for prec, kws in (("fp32", ({}, {"forward": None}, {"forward": "apply"},
                                {"backward": "bf16", "forward": "apply"},
                                {"affine": False, "forward": "apply"})),
                      ("bf16-bwd", ({"backward": "bf16"}, {"backward": "bf16", "forward": None},
                                    {"backward": "bf16", "forward": "apply"}))):
        for kw in kws:
            m = tmrnet_amd.resnet_lstm(seq_len=2, precision=prec).train()
            assert m.share.bn_frozen_fwd is None
            tmrnet_amd.freeze_bn(m, **kw)
            assert m.share.bn_frozen is True and m.share.bn_frozen_fwd is None
            assert not trunk._frozen_fused(m.share)
            assert m.share.bn_frozen_bwd == kw.get("backward")


@pytest.mark.parametrize("precision,backward", [("fp32", None), ("fp32", "bf16"),
                                                ("bf16-bwd", "bf16")])
def test_affine_true_is_refused_and_leaves_the_share_untouched(precision, backward):
    m = tmrnet_amd.resnet_lstm(seq_len=2, precision=precision).train()
    for kw in ({}, {"affine": True}):
        with pytest.raises(ValueError, match="dgamma needs the conv output, which this step does "
                                             "not store"):
            tmrnet_amd.freeze_bn(m, backward=backward, forward="fused", **kw)
        assert _untouched(m.share)


def test_bad_values_of_forward_are_refused():
    for bad in ("fuse", "bf16", True, 1, "FUSED"):
        m = tmrnet_amd.resnet_lstm(seq_len=2).train()
        with pytest.raises(ValueError, match="forward must be"):
            tmrnet_amd.freeze_bn(m, affine=False, forward=bad)
        assert _untouched(m.share)
    with pytest.raises(ValueError, match="backward must be"):   # (the earlier check stays first)
        tmrnet_amd.freeze_bn(tmrnet_amd.resnet_lstm(seq_len=2), backward="fp16", forward="nope")


@pytest.mark.parametrize("forward", ["fused", "apply", None])
def test_pinned_refusals_keep_their_messages(forward):
    kw = dict(affine=False, forward=forward)
    with pytest.raises(ValueError, match="ResNet-50 trunk \\(precision 'fp32'\\) only, not for a "
                                         "ResNeSt-50 share"):
        tmrnet_amd.freeze_bn(tmrnet_amd.resnet_lstm(seq_len=2, backbone="resnest50"), **kw)
    with pytest.raises(ValueError, match='backward="bf16".*ResNeSt-50'):
        tmrnet_amd.freeze_bn(tmrnet_amd.resnet_lstm(seq_len=2, backbone="resnest50"),
                             backward="bf16", **kw)
    for prec in ("bf16", "bf16-bwd"):
        m = tmrnet_amd.resnet_lstm(seq_len=2, precision=prec).train()
        with pytest.raises(ValueError, match="precision 'fp32' only, not for '%s'" % prec):
            tmrnet_amd.freeze_bn(m, **kw)
        assert _untouched(m.share)
    m = tmrnet_amd.resnet_lstm(seq_len=2, precision="bf16").train()
    with pytest.raises(ValueError, match='backward="bf16".*not for \'bf16\''):
        tmrnet_amd.freeze_bn(m, backward="bf16", **kw)
    assert _untouched(m.share)
    # the share kind is judged before affine: the pinned message, not the new one
    with pytest.raises(ValueError, match="ResNeSt-50"):
        tmrnet_amd.freeze_bn(tmrnet_amd.resnet_lstm(seq_len=2, backbone="resnest50"),
                             forward="fused")


def test_ops_wrappers_refuse_before_any_library_call(monkeypatch):
    """conv_fwd_fused_dual's Python-side checks and the y=None rule of bn_frozen_bwd (fp32 and
    dy16 forms) raise without calling the library (CPU tensors would be refused there anyway)."""
    def no_call(*a, **k):
        raise AssertionError("library call")
    monkeypatch.setattr(ops, "call", no_call)
    monkeypatch.setattr(ops, "query", no_call)
    x, w = torch.zeros(1, 4, 4, 8), torch.zeros(8, 1, 1, 8)
    sc = torch.ones(8)
    with pytest.raises(RuntimeError, match="fp32 operands in fp32 math only, x is torch.bfloat16"):
        ops.conv_fwd_fused_dual(x.bfloat16(), w, 1, 0, sc, sc)
    with pytest.raises(RuntimeError, match="fp32 operands in fp32 math only, w is torch.bfloat16"):
        ops.conv_fwd_fused_dual(x, w.bfloat16(), 1, 0, sc, sc)
    g = torch.zeros(4, 8)
    for dy16 in (False, True):
        with pytest.raises(RuntimeError, match="y=None needs want_sums=False"):
            ops.bn_frozen_bwd(g, None, sc, sc, sc, mask=1, z=g, want_sums=True, dy16=dy16)
        with pytest.raises(RuntimeError, match="y=None needs want_sums=False"):
            ops.bn_frozen_bwd(g, None, sc, sc, sc, mask=2, want_sums=False, dy16=dy16)


# ------------------------------------------------------------------ 2. routing
@pytest.mark.parametrize("n", [2, 640])
def test_every_non_stem_forward_plans_the_lds_dma_engine(n):
    """The dual form exists on the LDS-DMA engine only and on the six tile configs an fp32 forward
    can take: every non-stem ResNet-50 conv must plan one of them, so that it serves the whole
    trunk (layer1's 3x3 convs included: the fused entry points skip the direct kernels)."""
    convs = Z.trunk_convs()
    assert len(convs) == 52
    with ops.engine_only():   # (the fused entry points never take a direct kernel)
        for name, h, w, c, k, r, stride, pad in convs:
            t = ops.conv_tile(n, h, w, c, k, r, r, stride, pad, "fwd", math="fp32")
            assert t["engine"] == 2, (name, t)
            assert t["cfg"] in (5, 2, 7, 3, 1, 6), (name, t)
            assert c % 8 == 0 and k % 8 == 0, name


@pytest.mark.parametrize("n", [2, 640])
def test_dgrads_plan_the_engines_of_the_unfused_steps(n):
    """The masked dgrads are the unfused frozen steps' calls with another mask source: the same
    descriptor bits but TMR_IO_BN_BF16 | TMR_IO_ENGINE (a bf16 mask source, kept off the direct bf16
    3x3 dgrad that would take layer1's conv2 otherwise), so the same engine, tile and class count -- fp32 with the transposed fp32 weights, bf16 with bf16 dy / CRSK weights, the
    non-residual units' g stored bf16."""
    for name, h, w, c, k, r, stride, pad in Z.trunk_convs():
        a = ops.conv_tile(n, h, w, c, k, r, r, stride, pad, "dgrad", math="fp32", io=ops.IO_WT32)
        assert a["engine"] in (0, 2), (name, a)
        mid = name.endswith((".conv2", ".conv3"))
        io = ops.IO_DY | ops.IO_WT | (ops.IO_G16 if mid else 0)
        b = ops.conv_tile(n, h, w, c, k, r, r, stride, pad, "dgrad", math="bf16", io=io)
        f = ops.conv_tile(n, h, w, c, k, r, r, stride, pad, "dgrad", math="bf16",
                          io=io | ops.IO_BN | ops.IO_ENGINE)
        d = ops.conv_tile(n, h, w, c, k, r, r, stride, pad, "dgrad", math="bf16",
                          io=io | ops.IO_BN)
        assert d == f or (d["engine"] == 0 and name.startswith("layer1.") and r == 3), (name, d)
        assert b == f, (name, b, f)
        assert f["engine"] in (0, 2), (name, f)
        if mid and f["engine"] == 2:
            assert (f["bm"], f["bn"]) != (256, 256), (name, f)


# ------------------------------------------------------------------ 3. the helpers can fail
@pytest.mark.parametrize("res,relu", [(True, True), (True, False), (False, True), (False, False)])
def test_compare_dual_catches_planted_errors(res, relu):
    k = Z.grid_case(96, 24, 5, res)
    z, z16 = Z.emu_dual(k, relu)
    assert Z.compare_dual(z, z16, z) == []
    # the planted ties are there, of both parities, where the ReLU passes them
    u = Z.bits32(z)
    tie = ((u & 0xFFFF) == 0x8000) & (z != 0)
    assert (tie & ((u >> 16) & 1 == 0))[:, 0].any() and (tie & ((u >> 16) & 1 == 1))[:, 0].any()
    assert (z[::4, 1] == 0).all()                          # zeros of the ReLU's argument
    if res:
        assert (z[::4, 2] == 0).all() and (k["res"][::4, 2] != 0).any()   # the cancelling residual
    # truncation instead of round to nearest even
    assert Z.compare_dual(z, Z.trunc_bf16(z), z) == ["z16 != RNE(z)"]
    # round-half-up: differs from RNE on the even-parity ties only
    hu = Z.half_up_bf16(z)
    assert (hu != z16).sum() == (tie & ((u >> 16) & 1 == 0)).sum() > 0
    assert Z.compare_dual(z, hu, z) == ["z16 != RNE(z)"]
    # the copy taken before the ReLU / before the residual
    if relu:
        assert Z.compare_dual(z, Z.emu_dual(k, relu, "pre_relu")[1], z) == ["z16 != RNE(z)"]
    if res:
        assert Z.compare_dual(z, Z.emu_dual(k, relu, "pre_res")[1], z) == ["z16 != RNE(z)"]
    # a wrong z with its own faithful copy
    z2 = z.copy()
    z2[3, 5] += 1.0
    assert Z.compare_dual(z2, Z.rne_bf16(z2), z) == ["z != reference"]


def test_compare_mask_catches_a_mask_that_passes_zero():
    g = np.random.default_rng(3)
    full = g.integers(1, 8, (64, 16)).astype(np.float32) * np.where(g.random((64, 16)) < 0.5, -1, 1)
    z = np.maximum(g.integers(-3, 4, (64, 16)), 0).astype(np.float32)
    assert (z == 0).any() and (z > 0).any()
    good = np.where(z > 0, full, 0).astype(np.float32)
    assert Z.compare_mask(good, full, z) == []
    assert Z.compare_mask(np.where(z >= 0, full, 0).astype(np.float32), full, z)   # passes z == 0
    assert Z.compare_mask(full, full, z)                                            # no mask
    assert Z.compare_mask(np.zeros_like(full), full, z)
    # the bf16 mask source: the same predicate on the widened values
    z16 = Z.widen(Z.rne_bf16(z))
    assert Z.compare_mask(good, full, z16) == []


# ------------------------------------------------------------------ 4. the folded oracle
def test_folded_oracle_gives_the_unfolded_oracle():
    """The float64 frozen oracle with BN folded into the conv as the step folds it (scale = gamma *
    inv, shift = beta - mean * scale on every non-stem unit) gives the unfolded oracle's logits
    and gradients within float64 rounding; the BN parameters get no gradient (affine=False is the
    only form the fold has)."""
    base = F.oracle_step(torch.float64)
    r = Z.folded(F.oracle_model(torch.float64))
    assert list(r.state_dict().keys()) == list(F.step_case()["sd"].keys())
    got = F.run_step(r, (0,), torch.float64)
    assert (got["logits"] - base["logits"]).abs().max() < 1e-10
    assert abs(got["loss"] - base["loss"]) < 1e-10 * max(1.0, abs(base["loss"]))
    for n, b in got["buffers"].items():
        assert torch.equal(b, base["buffers"][n]), n
    bn = Z.bn_names(r.named_parameters())
    assert len(bn) == 106
    checked = 0
    for n, g in got["grads"].items():
        if n in bn and not n.startswith(("share.bn1.",)):
            assert g is None, n                             # folded: no BN gradient
            continue
        ref = base["grads"][n]
        assert (g - ref).norm() <= 1e-9 * max(ref.norm().item(), 1e-30) + 1e-14, n
        checked += 1
    assert checked >= 53 + 2
