"""CPU emulation of the bf16-activation inference trunk of ResNeSt-50
(ResNeSt50Share.infer_act16), shared by the tests of that route.

The contract: bf16 conv operands (oracle emulate_bf16_convs; fc1 / fc2 stay fp32) and every stored
activation rounded once to bf16 where it is stored.  The emulation is the oracle's eval-mode
ResNeSt-50 with forward hooks that round
  * each SplAtConv2d.bn0 output -- the stored tensor is relu(bn0(.)); RNE is monotone and keeps 0,
    so rounding commutes with the ReLU that follows, and the oracle's `relu` module is shared with
    the attention MLP, which stays fp32;
  * the SplAtConv2d output in blocks without avd, the avd_layer output in blocks with it (there
    the un-pooled weighted sum is never stored);
  * share.relu (the stem's last unit), every downsample branch and its pool, every BottleneckS.
The other unit outputs feed only convs, which round their operands anyway."""
import copy

import torch

from oracle import tmrnet_ref as ref
from tests._infer16_emu import randomize_bn, features   # noqa: F401  (re-exported)


def _round_hook(mod, inp, out):
    return ref.bf16_round(out)


def hooked_share(state_dict, prefix=""):
    """(share fp32, share float64): the emulation loaded from `state_dict` (keys under prefix)."""
    share = ref.emulate_bf16_convs(ref.resnest50_share()).eval()
    share.load_state_dict({k[len(prefix):]: v.detach().cpu() for k, v in state_dict.items()
                           if k.startswith(prefix)})
    share.relu.register_forward_hook(_round_hook)
    for m in share.modules():
        if isinstance(m, ref.BottleneckS):
            m.register_forward_hook(_round_hook)
            m.conv2.bn0.register_forward_hook(_round_hook)
            if m.avd:
                m.avd_layer.register_forward_hook(_round_hook)
            else:
                m.conv2.register_forward_hook(_round_hook)
            if m.downsample is not None:
                m.downsample.register_forward_hook(_round_hook)
                m.downsample[0].register_forward_hook(_round_hook)
    return share, copy.deepcopy(share).double()
