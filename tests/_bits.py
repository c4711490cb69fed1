"""ReLU-mask bits as the kernels read them (tmr_bn_apply_bits, mask 3 of the fused dgrad)."""
import torch


def pack_bits(m):
    """(numel,) bool -> int32 words, element e = bit e % 32 of word e // 32 (zero-padded)."""
    m = m.reshape(-1).to(torch.int64)
    m = torch.cat([m, m.new_zeros((-m.numel()) % 32)]).view(-1, 32)
    w = (m << torch.arange(32, dtype=torch.int64, device=m.device)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
