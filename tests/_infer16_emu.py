"""CPU emulation of the bf16-activation inference trunk (ResNet50Share.infer_act16), shared by
tests/test_infer16_gpu.py and tests/test_evaluate_split_gpu.py.

The contract: bf16 conv operands (oracle emulate_bf16_convs) and every stored activation rounded
once to bf16 after BN (+residual) (+ReLU).  The emulation is the oracle's eval-mode ResNet-50 with
forward hooks that round the outputs of the stem ReLU, of every downsample branch and of every
Bottleneck; the other unit outputs feed only convs, which round their operands anyway."""
import copy

import torch

from oracle import tmrnet_ref as ref


def randomize_bn(model, seed):
    """Non-trivial BatchNorm parameters and running statistics (as tests/test_lfb_build_gpu.py)."""
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            c = m.num_features
            m.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
            with torch.no_grad():
                m.weight.copy_(torch.rand(c, generator=g) * 0.5 + 0.25)
                m.bias.copy_(torch.randn(c, generator=g) * 0.1)


def _round_hook(mod, inp, out):
    return ref.bf16_round(out)


def hooked_share(state_dict, prefix=""):
    """(share fp32, share float64): the emulation loaded from `state_dict` (keys under prefix)."""
    share = ref.emulate_bf16_convs(ref.resnet50_share()).eval()
    share.load_state_dict({k[len(prefix):]: v.detach().cpu() for k, v in state_dict.items()
                           if k.startswith(prefix)})
    share.relu.register_forward_hook(_round_hook)
    for m in share.modules():
        if isinstance(m, ref.Bottleneck):
            m.register_forward_hook(_round_hook)
            if m.downsample is not None:
                m.downsample.register_forward_hook(_round_hook)
    return share, copy.deepcopy(share).double()


def features(share, x_nchw):
    """(F, 2048) features of the emulated trunk for NCHW frames of the share's dtype."""
    with torch.no_grad():
        return share(x_nchw).flatten(1)
