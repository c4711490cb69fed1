"""The public surface of the bf16-activation inference trunk of ResNeSt-50:
activations="bf16-resnest" through lfb_build.check_activations / inference_mode.  No device work."""
import pytest

import tmrnet_amd
from tmrnet_amd import lfb_build
from tmrnet_amd.stream import OnlineRecognizer


def _model(backbone, precision, lfb=False):
    cls = tmrnet_amd.resnet_lstm_LFB if lfb else tmrnet_amd.resnet_lstm
    return cls(seq_len=3, backbone=backbone, precision=precision)


@pytest.fixture(scope="module")
def rst16():
    return _model("resnest50", "bf16")


def test_accepts_resnest_bf16(rst16):
    assert rst16.share.infer_act16 is False
    lfb_build.check_activations(rst16, "bf16-resnest")
    lfb_build.check_activations(rst16, "fp32")
    lfb_build.LFBBuilder(_model("resnest50", "bf16", lfb=True), activations="bf16-resnest")


def test_refuses_other_trunks_and_precisions(rst16):
    with pytest.raises(ValueError, match="ResNeSt-50"):
        lfb_build.check_activations(_model("resnet50", "bf16"), "bf16-resnest")
    with pytest.raises(ValueError, match="ResNeSt-50"):
        lfb_build.check_activations(_model("resnest50", "fp32"), "bf16-resnest")
    # the ResNet-50 contract keeps its name and its refusal of ResNeSt
    with pytest.raises(ValueError, match="ResNet-50"):
        lfb_build.check_activations(rst16, "bf16")
    with pytest.raises(ValueError, match="activations must be"):
        lfb_build.check_activations(rst16, "bf16-resnet")
    # OnlineRecognizer checks both of its models
    with pytest.raises(ValueError, match="ResNeSt-50"):
        OnlineRecognizer(rst16, _model("resnet50", "bf16", lfb=True), 5,
                         activations="bf16-resnest")


def test_inference_mode_sets_and_restores(rst16):
    m = rst16
    m.train()
    with lfb_build.inference_mode(m, "bf16-resnest"):
        assert not m.training and not m.share.training and m.share.infer_act16 is True
    assert m.training and m.share.training and m.share.infer_act16 is False
    with pytest.raises(OSError):
        with lfb_build.inference_mode(m, "bf16-resnest"):
            assert m.share.infer_act16 is True
            raise OSError("decoder failed")
    assert m.training and m.share.training and m.share.infer_act16 is False
    with lfb_build.inference_mode(m, "fp32"):
        assert not m.training and m.share.infer_act16 is False
    m.eval()
    with lfb_build.inference_mode(m, "bf16-resnest"):
        assert m.share.infer_act16 is True
    assert not m.training and m.share.infer_act16 is False
