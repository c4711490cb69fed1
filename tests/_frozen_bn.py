"""Shared pieces of the frozen-BatchNorm tests (tests/test_frozen_bn_*.py, test_frozen_bwd16_*.py,
test_frozen_fused_*.py).

step_case(): one seeded 2-frame TMRNet step whose trunk BatchNorms are frozen -- eval mode, every
BN's running statistics and affine parameters randomised so that a step on batch statistics, a dy
without the scale or a wrong ReLU mask cannot pass for it.  oracle_step() runs it on the CPU oracle
(oracle.TMRNetRef) in fp32 or float64 once per (dtype, clips, plant) and caches the result; the
cached tensors are shared between tests and never written.
"""
import functools
import math

import torch
import torch.nn as nn

from oracle import tmrnet_ref as ref

T, L = 2, 3          # frames per clip, long-feature rows
CLIPS = 3            # clip 0 is step_case()'s batch; 1 and 2 serve the batch-independence test


def randomise_bn(module, seed=11):
    """running_mean ~ 0.2 N(0,1), running_var ~ U(0.5, 2), gamma ~ U(0.5, 1.5),
    beta ~ 0.1 N(0,1) for every BatchNorm2d of `module`, from one seeded generator."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                c = m.num_features
                m.running_mean.copy_(0.2 * torch.randn(c, generator=g))
                m.running_var.copy_(0.5 + 1.5 * torch.rand(c, generator=g))
                m.weight.copy_(0.5 + torch.rand(c, generator=g))
                m.bias.copy_(0.1 * torch.randn(c, generator=g))


@functools.lru_cache(maxsize=None)
def step_case():
    """The seeded case: state_dict (fp32), CLIPS clips of T frames (x: (CLIPS, T, 3, 224, 224)),
    long features, labels and explicit dropout masks.  The step of the issue is clip 0 alone
    (B = 1); see batch()."""
    torch.manual_seed(21)
    r = ref.TMRNetRef(seq_len=T)
    randomise_bn(r.share)
    g = torch.Generator().manual_seed(22)
    case = {
        "sd": {k: v.detach().clone() for k, v in r.state_dict().items()},
        "x": torch.randn(CLIPS, T, 3, 224, 224, generator=g),
        "lt": torch.rand(CLIPS, L, 512, generator=g) * 2 - 1,
        "labels": torch.randint(0, 7, (CLIPS,), generator=g),
        "nl": (torch.rand(CLIPS, 512, generator=g) >= 0.2).float() / 0.8,
        "head": (torch.rand(CLIPS, 512, generator=g) >= 0.5).float() / 0.5,
    }
    return case


def batch(clips=(0,), dtype=torch.float32):
    """(x (B,T,3,224,224), lt, labels, masks) of the chosen clips."""
    c = step_case()
    idx = torch.tensor(list(clips))
    f = lambda t: t[idx].to(dtype) if t.is_floating_point() else t[idx]
    return f(c["x"]), f(c["lt"]), f(c["labels"]), {"nl": f(c["nl"]), "head": f(c["head"])}


def freeze_oracle(r):
    """The oracle's form of freeze_bn: train mode, the trunk's BatchNorm modules in eval."""
    r.train()
    for m in r.share.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.eval()
    return r


# ---- planted errors (the comparison must flag each) ------------------------------------------
class _BNNoScale(torch.autograd.Function):
    """Eval-mode BN whose backward forgets the scale: dx = g instead of g * gamma * inv."""

    @staticmethod
    def forward(ctx, x, gamma, beta, mean, inv):
        v = lambda t: t.view(1, -1, 1, 1)
        ctx.save_for_backward(x, mean, inv)
        return (x - v(mean)) * v(inv) * v(gamma) + v(beta)

    @staticmethod
    def backward(ctx, g):
        x, mean, inv = ctx.saved_tensors
        v = lambda t: t.view(1, -1, 1, 1)
        dgamma = (g * (x - v(mean)) * v(inv)).sum((0, 2, 3))
        return g, dgamma, g.sum((0, 2, 3)), None, None


class _ReluPassZero(torch.autograd.Function):
    """ReLU whose backward passes the gradient where z == 0 (mask z >= 0)."""

    @staticmethod
    def forward(ctx, x):
        z = x.clamp(min=0)
        ctx.save_for_backward(z)
        return z

    @staticmethod
    def backward(ctx, g):
        (z,) = ctx.saved_tensors
        return g * (z >= 0).to(g.dtype)


class _ReluPassZeroModule(nn.Module):
    def forward(self, x):
        return _ReluPassZero.apply(x)


def _plant(r, plant):
    if plant == "batch_stats":
        for m in r.share.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.train()
    elif plant == "no_scale":
        for m in r.share.modules():
            if isinstance(m, nn.BatchNorm2d):
                def fwd(x, m=m):
                    inv = (m.running_var + m.eps).rsqrt()
                    return _BNNoScale.apply(x, m.weight, m.bias, m.running_mean, inv)
                m.forward = fwd
    elif plant == "mask_zero":
        for m in list(r.share.modules()):
            for name, child in list(m.named_children()):
                if isinstance(child, nn.ReLU):
                    setattr(m, name, _ReluPassZeroModule())
    elif plant is not None:
        raise ValueError(plant)


def oracle_model(dtype=torch.float32, plant=None):
    r = ref.TMRNetRef(seq_len=T)
    r.load_state_dict(step_case()["sd"])
    if dtype == torch.float64:
        r = r.double()
    freeze_oracle(r)
    _plant(r, plant)
    return r


def run_step(r, clips=(0,), dtype=torch.float32):
    """One forward + CE-sum backward of model `r` on the chosen clips -> dict of detached
    logits, loss, grads {name: tensor or None} and buffers {name: tensor} after the step."""
    x, lt, labels, masks = batch(clips, dtype)
    for p in r.parameters():
        p.grad = None
    out = r(x, lt, masks=masks)
    loss = ref.ce_sum_ref(out, labels)
    loss.backward()
    return {"logits": out.detach().clone(), "loss": float(loss.item()),
            "grads": {n: (p.grad.detach().clone() if p.grad is not None else None)
                      for n, p in r.named_parameters()},
            "buffers": {n: b.detach().clone() for n, b in r.named_buffers()}}


@functools.lru_cache(maxsize=None)
def oracle_step(dtype=torch.float32, clips=(0,), plant=None):
    """The cached oracle step (read-only: shared between tests)."""
    return run_step(oracle_model(dtype, plant), clips, dtype)


# ---- comparison -------------------------------------------------------------------------------
def assert_step(got_grads, got_logits, clips=(0,), what="frozen step", record=None, rows_out=None,
                absent=()):
    """A candidate step against the float64 oracle under tests.test_model_parity_gpu's
    _assert_vs_fp64 (its constants unchanged; the fp32 CPU oracle is the yardstick), and its logits
    by that module's step-parity rule (1e-4 absolute, equal argmax).  rows_out: a list that
    receives the per-parameter (name, e_hip, e_cpu) rows.  absent: parameter names whose gradient
    must be None (affine=False); every other parameter must have one."""
    from tests.test_model_parity_gpu import _assert_vs_fp64, l2_err
    o32, o64 = oracle_step(torch.float32, clips), oracle_step(torch.float64, clips)
    absent = set(absent)
    missing = [n for n in o64["grads"] if n not in absent and got_grads.get(n) is None]
    assert not missing, (what, "no gradient for", missing[:5])
    present = [n for n in absent if got_grads.get(n) is not None]
    assert not present, (what, "unexpected gradient for", present[:5])
    got_grads = {n: g for n, g in got_grads.items() if n not in absent}
    if rows_out is not None:
        for n, g in got_grads.items():
            rows_out.append({"name": n, "e_hip": l2_err(g, o64["grads"][n]),
                             "e_cpu": l2_err(o32["grads"][n], o64["grads"][n])})
    err = (got_logits.detach().double().cpu() - o64["logits"]).abs().max().item()
    assert err < 1e-4, (what, "logits", err)
    assert torch.equal(got_logits.detach().cpu().argmax(1), o64["logits"].argmax(1)), what
    _assert_vs_fp64(got_grads, o32["grads"], o64["grads"], what, record=record or what)


# ---- the HIP model ----------------------------------------------------------------------------
def to_nhwc4(x):
    """(F,3,H,W) -> the HIP step's (F,H,W,4) NHWC4 input (channel 3 zero)."""
    f, _, h, w = x.shape
    out = torch.zeros(f, h, w, 4, dtype=x.dtype)
    out[..., :3] = x.permute(0, 2, 3, 1)
    return out


def hip_model(dev, frozen=True, affine=True, backward=None, forward=None, precision="fp32"):
    import tmrnet_amd
    m = tmrnet_amd.resnet_lstm(seq_len=T, precision=precision).to(dev)
    m.load_state_dict(step_case()["sd"])
    m.train()
    if frozen:
        tmrnet_amd.freeze_bn(m, affine=affine, backward=backward, forward=forward)
    return m


def _buffers(m):
    return {n: b.detach().clone() for n, b in m.named_buffers()}


def _keep(t):
    """A hip_step result whose tensors the next step cannot overwrite."""
    return t[0].clone(), t[1], {n: (g.detach().clone() if g is not None else None)
                                for n, g in t[2].items()}


PAD, SENT = 64, 12345.0


def guarded(shape, dev, fill=None, dtype=torch.float32):
    """A tensor between two PAD-element sentinel zones -> (whole buffer, view); the view is 16-B
    aligned (PAD elements into an aligned allocation).  fill: a tensor copied into the view, or
    a number (NaN) it is filled with; None leaves the sentinel value."""
    n = math.prod(shape)
    full = torch.full((n + 2 * PAD,), SENT, dtype=dtype, device=dev)
    view = full[PAD:PAD + n].view(shape)
    if isinstance(fill, torch.Tensor):
        view.copy_(fill)
    elif fill is not None:
        view.fill_(fill)
    return full, view


def intact(full):
    return bool((full[:PAD] == SENT).all() and (full[-PAD:] == SENT).all())


def hip_inputs(dev, clips=(0,)):
    x, lt, labels, masks = batch(clips)
    x4 = to_nhwc4(x.reshape(-1, 3, 224, 224)).to(dev)
    return x4, lt.to(dev), labels.to(dev), {k: v.to(dev) for k, v in masks.items()}


def hip_step(m, dev, clips=(0,)):
    """One forward + CE-sum backward of the HIP model -> (logits, loss, {name: grad or None})."""
    import tmrnet_amd
    x4, lt, labels, masks = hip_inputs(dev, clips)
    m.nl_block.forced_mask = masks["nl"]
    m.forced_head_mask = masks["head"]
    for p in m.parameters():
        p.grad = None
    out = m(x4, lt)
    loss = tmrnet_amd.CrossEntropyLoss(size_average=False)(out, labels)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach(), float(loss.item()), {n: p.grad for n, p in m.named_parameters()}


STEPS, LR = 5, 1e-4


@functools.lru_cache(maxsize=None)
def oracle_trajectory(dtype=torch.float64):
    """Losses of STEPS SGD steps (the reference's parameter groups at lr LR, momentum 0.9, weight
    decay 5e-4) of the frozen oracle on clip 0 -> tuple of floats."""
    r = oracle_model(dtype)
    opt = torch.optim.SGD(ref.sgd_param_groups(r, LR), lr=LR / 10, momentum=0.9, weight_decay=5e-4)
    x, lt, labels, masks = batch((0,), dtype)
    losses = []
    for _ in range(STEPS):
        opt.zero_grad()
        loss = ref.ce_sum_ref(r(x, lt, masks=masks), labels)
        loss.backward()
        opt.step()
        losses.append(float(loss.item()))
    return tuple(losses)
