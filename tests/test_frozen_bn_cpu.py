"""Frozen BatchNorm without a GPU: the freeze_bn / unfreeze_bn interface, the float64 oracle's
properties of a frozen step, and the comparison (tests/_frozen_bn.assert_step) that the GPU tests
rely on -- it must flag a step on batch statistics, a dy without the scale and a ReLU mask that
passes the gradient where z == 0."""
import pytest
import torch
import torch.nn as nn

import tmrnet_amd
from tmrnet_amd import lfb_build
from tests import _frozen_bn as F


def _bns(share):
    return [m for m in share.modules() if isinstance(m, nn.BatchNorm2d)]


def _share(model):
    return getattr(model, "share", None) or getattr(model, "res", None) or model


def _models():
    import types
    from tmrnet_amd.compat import models as cm
    return [tmrnet_amd.ResNet50Share(), tmrnet_amd.resnet_lstm(seq_len=2),
            tmrnet_amd.resnet_lstm_LFB(seq_len=2), tmrnet_amd.MemoryBankModel(seq_len=2),
            cm.resnet_lstm(types.SimpleNamespace(seq=2), 7)]


@pytest.mark.parametrize("i", range(5))
def test_freeze_sets_flags_and_survives_train_eval(i):
    m = _models()[i]
    share = _share(m)
    assert isinstance(share, tmrnet_amd.ResNet50Share) and share.bn_frozen is False
    keys = list(m.state_dict().keys())
    shapes = [tuple(v.shape) for v in m.state_dict().values()]
    m.train()
    assert tmrnet_amd.freeze_bn(m) is m
    assert share.bn_frozen is True and share.training
    assert len(_bns(share)) == 53 and not any(b.training for b in _bns(share))
    assert all(b.weight.requires_grad and b.bias.requires_grad for b in _bns(share))
    for mode in (True, False, True):
        m.train(mode)
        assert share.training is mode and not any(b.training for b in _bns(share))
    m.eval()
    assert not share.training and not any(b.training for b in _bns(share))
    m.train()
    if hasattr(m, "share"):   # (inference_mode takes the models that hold a .share)
        with lfb_build.inference_mode(m):
            assert not share.training and not any(b.training for b in _bns(share))
    assert share.training and not any(b.training for b in _bns(share))
    assert list(m.state_dict().keys()) == keys
    assert [tuple(v.shape) for v in m.state_dict().values()] == shapes
    # round trip
    assert tmrnet_amd.unfreeze_bn(m) is m
    assert share.bn_frozen is False and all(b.training for b in _bns(share))
    m.eval()
    assert not any(b.training for b in _bns(share))
    tmrnet_amd.freeze_bn(m)
    tmrnet_amd.unfreeze_bn(m)   # in eval mode: the BN modules follow share.training
    assert not share.training and not any(b.training for b in _bns(share))
    m.train()
    assert all(b.training for b in _bns(share))


def test_affine_false_stops_bn_parameters_only():
    m = tmrnet_amd.resnet_lstm(seq_len=2)
    tmrnet_amd.freeze_bn(m, affine=False)
    bn_params = {id(p) for b in _bns(m.share) for p in (b.weight, b.bias)}
    for p in m.parameters():
        assert p.requires_grad is (id(p) not in bn_params)
    assert len(bn_params) == 106
    tmrnet_amd.unfreeze_bn(m)
    assert all(p.requires_grad for p in m.parameters())
    assert list(m.state_dict()) == list(tmrnet_amd.resnet_lstm(seq_len=2).state_dict())


def test_refusals():
    with pytest.raises(ValueError, match="ResNeSt-50"):
        tmrnet_amd.freeze_bn(tmrnet_amd.resnet_lstm(seq_len=2, backbone="resnest50"))
    for prec in ("bf16", "bf16-bwd"):
        m = tmrnet_amd.resnet_lstm(seq_len=2, precision=prec)
        with pytest.raises(ValueError, match="precision 'fp32' only, not for '%s'" % prec):
            tmrnet_amd.freeze_bn(m)
        assert m.share.bn_frozen is False and all(b.training for b in _bns(m.share))
    with pytest.raises(TypeError, match="ResNet50Share"):
        tmrnet_amd.freeze_bn(nn.Linear(2, 2))


def test_mixed_mode_share_raises_at_forward():
    x4 = torch.zeros(1, 224, 224, 4)
    share = tmrnet_amd.ResNet50Share().train()
    share.layer2[1].bn2.eval()
    with pytest.raises(RuntimeError, match="BatchNorm modules disagree"):
        share.features_nhwc4(x4)
    share = tmrnet_amd.freeze_bn(tmrnet_amd.ResNet50Share().train())
    for b in _bns(share):
        b.train()                 # put back by hand: the flag now contradicts the modules
    with pytest.raises(RuntimeError, match="bn_frozen is set"):
        share.features_nhwc4(x4)


# ---- the float64 oracle's frozen step ---------------------------------------------------------
def test_oracle_step_writes_no_statistics():
    o = F.oracle_step(torch.float64)
    sd = F.step_case()["sd"]
    n = 0
    for name, b in o["buffers"].items():
        if name.startswith("share.") and name.split(".")[-1] in (
                "running_mean", "running_var", "num_batches_tracked"):
            assert torch.equal(b, sd[name].to(b.dtype)), name
            n += 1
    assert n == 3 * 53
    assert abs(o["loss"] - F.oracle_step(torch.float32)["loss"]) < 1e-4


def test_oracle_gradients_are_additive_over_clips():
    """Frozen BN makes a clip's gradient independent of the batch: grad(A + B) = grad(A) + grad(B)
    (CE summed), in float64 to its rounding."""
    ab = F.oracle_step(torch.float64, (0, 1))
    a, b = F.oracle_step(torch.float64, (0,)), F.oracle_step(torch.float64, (1,))
    assert torch.allclose(ab["logits"][0], a["logits"][0], rtol=0, atol=1e-12)
    assert torch.allclose(ab["logits"][1], b["logits"][0], rtol=0, atol=1e-12)
    for n, g in ab["grads"].items():
        s = a["grads"][n] + b["grads"][n]
        # (1e-15 absolute: nl_block.linear2.bias has an exactly zero gradient, 1e-17 of noise)
        assert (g - s).norm() <= 1e-11 * s.norm() + 1e-15, n


# ---- the comparison flags planted errors ------------------------------------------------------
def test_comparison_accepts_the_fp32_oracle():
    o = F.oracle_step(torch.float32)
    F.assert_step(o["grads"], o["logits"], what="fp32 oracle", record="frozen_cpu_self")


@pytest.mark.parametrize("plant", ["batch_stats", "no_scale", "mask_zero"])
def test_comparison_flags_planted_error(plant):
    bad = F.run_step(F.oracle_model(torch.float32, plant))
    with pytest.raises(AssertionError):
        F.assert_step(bad["grads"], bad["logits"], what=plant, record="frozen_cpu_" + plant)
    if plant != "batch_stats":
        # the forward is right: the gradients alone give it away
        good = F.oracle_step(torch.float32)
        assert torch.allclose(bad["logits"], good["logits"], atol=1e-5)
        from tests.test_model_parity_gpu import _assert_vs_fp64
        with pytest.raises(AssertionError):
            _assert_vs_fp64(bad["grads"], good["grads"], F.oracle_step(torch.float64)["grads"],
                            plant, record="frozen_cpu_" + plant)
