"""ResNet-50 frame encoder (`share`) on libtmr's NHWC implicit-GEMM kernels.

Drop-in for the `share` nn.Sequential of the reference's inline TMRNet model
(code/Training TMRNet/train_only_non-local_pretrained.py:204-214, built from
torchvision resnet50): same child names (conv1, bn1, relu, maxpool,
layer1..4, avgpool), same Bottleneck sub-module names and therefore identical
``state_dict`` keys ("share.layer1.0.conv1.weight", "share.bn1.running_mean",
...).  nn.Conv2d / nn.BatchNorm2d modules are kept as parameter/buffer
containers only (their torch forward is never called); the whole trunk runs
as ONE autograd node (`TrunkFn`) that keeps activations NHWC in HBM and drives
conv -> BN(batch stats) -> ReLU(+residual) on the HIP kernels, with the
backward pass (BN backward, dgrad, wgrad) in reverse layer order.

BN semantics follow nn.BatchNorm2d in train mode: batch mean / biased variance
for normalisation, running stats updated with momentum and the unbiased
variance, num_batches_tracked += 1; eval mode uses running stats.

The other step kinds, each specified by the block comment named:
  * precision "bf16": bf16 conv operands and activations (BF16_STORE, FULL16, ACT16, G16, R16);
  * precision "bf16-bwd": the fp32 forward, bf16 operands in the backward convs only (BWD16);
  * frozen BatchNorm (freeze_bn): a train step on the running statistics ("frozen BatchNorm");
    with backward="bf16" its backward convs in bf16 math (_frozen16); with forward="fused" BN
    folded into the conv forward, no conv output stored (_frozen_fused).  One backward walk
    (TrunkFn._backward_frozen) and one per-unit helper (_frozen_unit_bwd) serve them all: the
    units' records say which forward ran;
  * infer16: eval mode with bf16 activations, opt-in (_infer16, TrunkFn._forward_eval).
How the units of a step are put together: "the conv+BN unit" below, DESIGN.md §29.
"""
import os
import weakref

import torch
import torch.nn as nn

from . import ops


class Bottleneck(nn.Module):
    """torchvision v1.5 Bottleneck (stride on the 3x3) as a parameter container."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


def _make_layer(inplanes, planes, blocks, stride):
    downsample = None
    if stride != 1 or inplanes != planes * 4:
        downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False),
                                   nn.BatchNorm2d(planes * 4))
    layers = [Bottleneck(inplanes, planes, stride, downsample)]
    for _ in range(1, blocks):
        layers.append(Bottleneck(planes * 4, planes))
    return nn.Sequential(*layers)


# --------------------------------------------------------------------- engine
# share module -> callable(pairs) told each block's final gradients during the backward
# (ddp.GradAllReduce registers itself here).  A weak side table rather than a module attribute,
# so deepcopy / torch.save of the model never see the reducer or its process group.
_GRAD_READY = weakref.WeakKeyDictionary()


def set_grad_ready(share, fn):
    """Register (fn) or clear (None) the per-block gradient hook of a trunk module."""
    if fn is None:
        _GRAD_READY.pop(share, None)
    else:
        _GRAD_READY[share] = fn


def get_grad_ready(share):
    return _GRAD_READY.get(share, getattr(share, "grad_ready", None))

def _bn_momentum(bn):
    if bn.momentum is None:
        raise NotImplementedError("BatchNorm2d(momentum=None) (cumulative average) is not supported")
    return bn.momentum


# bf16 math (configs C4/C5): the tensors consumed only as conv operands -- the KRSC weights, the
# BN+ReLU outputs of each Bottleneck's first two units, every BatchNorm-backward output dy -- are
# stored as bf16 (tmr_conv_desc.io).  Exact: the bf16 convs round those operands to bf16 (RNE)
# when staging them anyway, so results are bit-identical to fp32 storage; the convs read half the
# bytes with no conversion.  TMR_BF16_STORE=0 keeps them fp32 (A/B measurements).
BF16_STORE = os.environ.get("TMR_BF16_STORE", "1") != "0"


def _store16(math):
    return math == "bf16" and BF16_STORE


# bf16 math with EVERY conv operand bf16 in HBM (train mode): the block outputs are written fp32
# (identity residual, ReLU mask) and as a bf16 copy in the same pass (bn_apply_dual / bn_apply2
# dual), the stem maxpool output as bf16 only (layer1.0 has a downsample, so it is never a
# residual), and each conv's dgrad reads a transposed bf16 weight copy (weight_to_crsk).  Every conv
# but the 4-channel stem then runs on the LDS-DMA engine (gemm16_kernel.h).  Same rounding of the
# same operands as the register-staged bf16 path, tests/test_bf16_gpu.py.  (A module attribute, no
# environment switch: tests/test_bf16_gpu.py turns it off to reach the fp32-storage forms.)
FULL16 = True

# bf16 activations (train mode, on top of FULL16; TMR_BF16_ACT=0 turns it off): every conv output
# y is stored rounded to bf16 by its epilogue (the BN statistics are those of the rounded values)
# and every BatchNorm(+residual)(+ReLU) output z is computed in fp32 and stored rounded to bf16 --
# block outputs included, so the identity residual is the bf16 block output.  Gradients stay fp32
# (dy, a conv operand, bf16).  This changes the numerics contract of the bf16 step (the oracle's
# emulate_bf16_convs(activations=True) restates it); the HBM traffic of every BatchNorm pass and of
# the conv epilogues halves.
ACT16 = os.environ.get("TMR_BF16_ACT", "1") != "0"


# bf16-activation step: the masked BN-output gradient of the non-residual units (bn1, bn2 of every
# Bottleneck) stored bf16 by the fused dgrad (TMR_IO_G16; the residual stream's gradient stays
# fp32) -- halves the bytes of the dgrad store and of the BN-backward apply's read of g.  The
# contract (oracle.emulate_bf16_convs(grads=True)) rounds the gradient at those two points.
G16 = os.environ.get("TMR_G16", "1") != "0"

# bf16-activation step (ResNet-50 and ResNeSt-50 trunks): the residual stream's gradient -- the
# masked gradient of every Bottleneck's sum bn3(y3) + identity but the last block's -- is stored
# bf16 too
# (TMR_BF16_RESGRAD=0: fp32).  Each block's conv1 dgrad adds its part to the identity branch's
# gradient (read bf16, or fp32 from the downsample dgrad / the last block), masks it by the previous
# block's ReLU and rounds once (tmr_conv2d_dgrad_bnbwd_acc); the BN backward of bn3 and of the
# downsample BN read it bf16 (tmr_bn_bwd_parts_g16, tmr_bn_bwd_g16).  12-14 -> 6-7 B per element on
# the residual dgrads' epilogue.  The contract (oracle.emulate_bf16_convs(grads=True)) rounds the
# gradient of every block output but the last.
R16 = os.environ.get("TMR_BF16_RESGRAD", "1") != "0"

# downsample blocks: the BatchNorm backward of bn3 and of the downsample BN -- both take the
# block's masked pre-ReLU gradient g -- in one call whose apply pass reads g once for both dy's
# (tmr_bn_bwd_parts_ds: the values of the two separate passes; C2 174.2 -> 173.6 ms/step, C5
# 161.8 -> 161.5, profiles/r5/ds_dual/.  A module attribute for the bit-identity test.)
DS_DUAL = True

# fp32 step: a unit whose masked gradient comes from a fused dgrad (parts) lets its wgrad produce
# dy = A*g + B*y + C while loading its dy operand (tmr_conv2d_wgrad_bnbwd) instead of a separate
# BatchNorm-backward apply pass: the same dy and dW bit for bit, 12 instead of 16 B moved per dy
# element (profiles/wgrad_bnbwd/, profiles/wgrad_bnbwd_ds/ for the 256x256 tile's form).  Units
# the fused form does not serve (ops.conv_wgrad_bnbwd_ok: direct kernels, misaligned or chunked
# operands) keep the two calls.  A module attribute for the bit-identity test.
WGRAD_BNBWD = True

# fp32 step, downsample blocks: the same fold for bn3 and the downsample BN, which share the
# block's masked gradient g.  tmr_bn_bwd_parts_ds then runs its two reductions only (or one
# single-output apply for a unit the fused wgrad does not take), and each served unit's wgrad
# produces its own dy from (g, its y, its coefficients): dy3, dy_ds, both dW and the four BN
# gradients bit for bit (profiles/wgrad_bnbwd_ds/).  WGRAD_BNBWD_DS_MIN: dy elements from which a
# block takes the route.  Per launch, at 640 and at 40 frames of 224x224, the fold won on every
# block of 8.0e6 elements and more (0.02-0.83 ms) and broke even at 4.0e6 (l4.0 at 40 frames:
# 0.331 against 0.323 ms); below that nothing was measured and the dual apply stays.  Module
# attributes for the bit-identity test.
WGRAD_BNBWD_DS = True
WGRAD_BNBWD_DS_MIN = 8_000_000


def _ds_fold(g, r3, rd):
    """Which of a downsample block's two units (bn3's conv3, the downsample conv) let their wgrad
    produce dy (WGRAD_BNBWD_DS) -> (fold3, foldd)."""
    # (fp32 math only: the BWD16 step's g is fp32 but its wgrads run in bf16 math on a bf16 dy)
    if not (WGRAD_BNBWD and WGRAD_BNBWD_DS and g.dtype == torch.float32
            and r3.math == "fp32" and rd.math == "fp32" and g.numel() >= WGRAD_BNBWD_DS_MIN):
        return False, False
    return _wgrad_dy_ok(r3, g), _wgrad_dy_ok(rd, g)


def _ds_dual(g, r3, rd):
    """DS_DUAL applies: g, y3 and y_ds of one dtype, which is also the dy dtype the separate passes
    would write (fp32 y under bf16 storage writes bf16 dy: not this path -- except the BWD16
    step's records, whose fp32 g / y / y_ds in, bf16 dy's out form is _ds_dy16), 8-channel
    multiples."""
    y = r3.y
    return (DS_DUAL and g.is_contiguous() and g.dtype == y.dtype == rd.y.dtype
            and y.shape == rd.y.shape and y.shape[-1] % 8 == 0
            and (_ds_dy16(r3, rd) or not (_store16(r3.math) and y.dtype == torch.float32)))


def _ds_dy16(r3, rd):
    """The BWD16 step's downsample blocks: fp32 g, y3, y_ds, both dy's stored bf16
    (ops.bn_bwd_parts_ds(dy16=True))."""
    return bool(r3.dy16 and rd.dy16 and r3.y.dtype == torch.float32)

# the fp32 block outputs' ReLU masks as bits for the mask-3 dgrads (round 2: 3622 -> 3634 frames/s,
# profiles/r2/bench_r3a/).  The bf16-activation step re-reads its 2-byte z instead: bits measured no
# faster there (profiles/r3/bench_r4i/, round-4 A/B under R16: the step unchanged) and were retired.


# fp32 math: the dgrad view runs on the fp32 form of the LDS-DMA engine, reading a transposed fp32
# weight copy (TMR_IO_WT_F32; the forward view takes that engine by itself)
def _dma32(math):
    return math == "fp32"


# bf16 activations: the direct bf16 stem takes the NHWC4 fp32 input itself (stem16.hip, round 4:
# 147 of 176 multiplies useful instead of 147 of 392); on the implicit-GEMM engine
# (ops.engine_only, tests) the stem reads an NHWC8 bf16 copy of it (LDS-DMA engine pieces)


def _full16(math):
    return _store16(math) and FULL16


# precision "bf16-bwd" (ResNet-50 only): the forward is the fp32 step's, bit for bit -- the same
# conv kernels on fp32 operands, BN statistics, z, running statistics; eval mode is the fp32 path.
# Every trunk conv's dgrad and wgrad run with math "bf16" and fp32 accumulation on three roundings
# (the oracle's emulate_bf16_convs(ops=("dy", "bx", "bw"))): dy stored bf16 (RNE) by the BN
# backward that produces it; the wgrad reads a bf16 copy of the conv's input, written in the
# forward by the pass that writes the fp32 value (bn_apply_dual, bn_apply(2)_bits_dual,
# maxpool_fwd_bn_dual; the stem's NHWC4 fp32 input is rounded on load by the direct bf16 wgrad);
# the dgrad reads the bf16 CRSK weight copy.  BN statistics, y, the ReLU masks (bits for block
# outputs, y*scale+shift otherwise), the masked gradients g, the residual-stream gradient, dW and
# the BN gradients stay fp32: no G16 / R16 here.  Saved per unit: the bf16 input copy, fp32 y, bits
# for block outputs, statistics and coefficients -- the fp32 z of a non-residual unit is dropped
# once the next conv's forward has read it, and the block outputs' fp32 z after the forward (mask 3
# reads the bits; the last block's stays for the first BN backward's mask).
BWD16 = "bf16-bwd"


def _fwd_math(precision):
    """The math mode of the forward convs (ops.MATH) under ResNet50Share.precision."""
    return "fp32" if precision == BWD16 else precision


def _act16(math):
    return _full16(math) and ACT16


def _infer16(share):
    """The bf16-activation inference trunk applies: eval mode, every conv operand bf16 in HBM
    (_full16) and the opt-in switch ResNet50Share.infer_act16."""
    return bool(not share.training and share.precision != BWD16 and _full16(share.precision)
                and getattr(share, "infer_act16", False))


# ------------------------------------------------------------------ the conv+BN unit
class Unit:
    """What the forward of one conv+BN unit leaves for its backward.  Built by
    _TrainUnits._record only; every field is set for every unit, None where the step kind has no
    such tensor."""
    __slots__ = (
        "conv", "bn",      # the parameter containers
        "x",       # the conv's input as the wgrad reads it (bf16-bwd: its bf16 copy x16, but the
                   # stem's NHWC4 fp32 input)
        "wk",      # KRSC weights (_krsc)
        "wt",      # the dgrad's transposed CRSK copy (_dgrad_weights); None: the dgrad reads wk
        "y",       # the conv output (None: the fused frozen step never stores it)
        "z",       # the BN output of a residual unit (the ReLU mask); None without a residual,
                   # for a deferred unit, and in the bf16-bwd step once the bits replace it.  The
                   # fused frozen step: every ReLU unit's own output (fp32 z, or its bf16 copy)
        "zbits",   # the ReLU mask as bits: fp32 block outputs of a recorded step, else None
        "scale", "shift", "mean", "inv",   # BN coefficients and statistics (frozen: running)
        "stride", "pad", "relu",
        "c_real",  # real input channels per group
        "math",    # ops.MATH of the backward convs (bf16-bwd: "bf16" after a forward in "fp32")
        "groups",
        "res",     # a residual or a branch was added before the ReLU (mask from z, not from y)
        "dy16",    # the bf16-bwd step: dy is stored bf16 whatever `math` stores
        "fold")    # frozen step: wt carries scale[k], the unit's dy = g*scale is never formed

    def __init__(self, **fields):
        for name in self.__slots__:
            setattr(self, name, fields[name])

    def __getitem__(self, name):   # (resnest._splat_bwd reads bn0's operands by key)
        return getattr(self, name)


def _krsc(w, cs, s16, groups=1):
    """The forward's KRSC weights of an OIHW conv weight for an input of cs stored channels."""
    k, c, r, s = w.shape
    if r == 1 and s == 1 and c == cs and not s16:
        return w.detach().contiguous().view(k, 1, 1, c)   # OIHW == KRSC for 1x1
    # (grouped: torch's (K, C/G, R, S) -> stacked per-group KRSC blocks (K, R, S, C/G))
    return ops.weight_to_krsc(w.detach().contiguous(), cpad=cs // groups, bf16=s16)


def _conv_bn_eval(x, conv, bn, stride, pad, relu, math, residual=None, y16=False, groups=1):
    """The eval unit: running-stat BN, residual and ReLU in the conv epilogue (one launch; same
    arithmetic as conv_fwd + bn_apply) -> z.  ``y16`` (the shares' infer_act16): x and residual
    bf16, z rounded once to bf16.  ``groups``: ResNeSt's radix-2 3x3, with y16 only."""
    if groups > 1 and not y16:
        raise RuntimeError("grouped convs run in the train-mode trunk and the bf16-activation "
                           "inference trunk (y16) only")
    w = conv.weight
    wk = _krsc(w, x.shape[3], _store16(math), groups)
    scale, shift = ops.bn_eval_params(bn.weight.detach(), bn.bias.detach(), bn.running_mean,
                                      bn.running_var, bn.eps)
    return ops.conv_fwd_fused(x, wk, stride, pad, scale, shift, residual, relu,
                              c_real=w.shape[1], math=math, y16=y16, groups=groups)


def _bn_apply_form(y, scale, shift, residual, branch, relu, bits, copy16, s16):
    """The BatchNorm apply pass of a train unit -> (z, zbits, z16).  bits: also the ReLU mask as
    bits (a residual unit with ReLU); copy16: also a bf16 copy of z; branch: a deferred (y, scale,
    shift) as the residual, its BN applied on load; s16: a non-residual z is stored bf16."""
    if bits and copy16:
        if branch is not None:
            return ops.bn_apply2_bits_dual(y, scale, shift, branch[0], branch[1], branch[2])
        return ops.bn_apply_bits_dual(y, scale, shift, residual)
    if bits:
        if branch is not None:
            return ops.bn_apply2_bits(y, scale, shift, branch[0], branch[1], branch[2]) + (None,)
        return ops.bn_apply_bits(y, scale, shift, residual) + (None,)
    if branch is not None:
        z = ops.bn_apply2(y, scale, shift, branch[0], branch[1], branch[2], relu, dual=copy16)
        return (z[0], None, z[1]) if copy16 else (z, None, None)
    if copy16:
        z, z16 = ops.bn_apply_dual(y, scale, shift, residual, relu)
        return z, None, z16
    # a non-residual unit's output is only ever a conv operand (next conv's forward and wgrad; the
    # backward recomputes its ReLU mask from y): bf16 under bf16 math (with bf16 activations every
    # z is bf16: the dtype of y decides)
    return ops.bn_apply(y, scale, shift, residual, relu, bf16=s16 and residual is None), None, None


def _dgrad_weights(w, x, math, groups, bwd16, scale):
    """The transposed weight copy a unit's dgrad reads (LDS-DMA engine), or None (the dgrad takes
    the KRSC weights; the stem's 3 input channels: no dgrad).  scale: the frozen step's fold."""
    c = w.shape[1]
    if bwd16:
        if c % 8:
            return None
        if scale is not None:   # (the frozen16 step: the fp32 product w*scale rounded once)
            return ops.weight_to_crsk_scaled(w.detach().contiguous(), scale, bf16=True)
        return ops.weight_to_crsk(w.detach().contiguous())
    if scale is not None:
        return ops.weight_to_crsk_scaled(w.detach().contiguous(), scale)
    x16 = _full16(math) and x.dtype == torch.bfloat16
    if groups > 1 and (x16 or _dma32(math)):
        return ops.weight_to_crsk_grouped(w.detach().contiguous(), groups, bf16=x16)
    if x16:
        return ops.weight_to_crsk(w.detach().contiguous())
    if _dma32(math) and c % 8 == 0 and x.dtype == torch.float32:
        return ops.weight_to_crsk(w.detach().contiguous(), bf16=False)
    return None


class _TrainUnits:
    """The train-mode forward units of one step, with what is constant over the forward: ``math``
    of the forward convs, ``keep`` (record the units for a backward), ``bwd16`` (the BWD16 step: a
    bf16 copy of every z and records for a bf16-math backward), ``frozen`` (the frozen-BN step's
    {bn: (scale, shift, inv)}, _frozen_coefs: no statistics epilogue, the running statistics'
    coefficients).  ``nbt``: the units' num_batches_tracked, for one ops.counters_add_one."""

    def __init__(self, math, keep, bwd16=False, frozen=None):
        if (bwd16 or frozen is not None) and math != "fp32":
            raise RuntimeError("the bf16-bwd and the frozen-BN steps run an fp32 forward")
        self.math, self.keep, self.bwd16, self.frozen = math, keep, bwd16, frozen
        self.nbt = []

    def unit(self, x, conv, bn, stride, pad, relu, **kw):
        """conv -> BN -> (+residual | +branch) -> (ReLU) -> (z, z16, record); z16: the bf16 copy
        of z under ``dual`` (block outputs under _full16) and in the BWD16 step, else None."""
        _, z, z16, rec = self._run(x, conv, bn, stride, pad, relu, False, **kw)
        return z, z16, rec

    def deferred(self, x, conv, bn, stride, pad, relu, **kw):
        """conv and the BN coefficients only -> ((y, scale, shift), record): the consumer applies
        the BN on load (the downsample branch inside its block's BN3 pass as ``branch``, the stem
        inside the maxpool, ResNeSt's bn0 inside the split attention)."""
        branch, _, _, rec = self._run(x, conv, bn, stride, pad, relu, True, **kw)
        return branch, rec

    def fused(self, x, conv, bn, stride, pad, relu, residual=None, x16=None, fold=True,
              copy16=True):
        """A non-stem unit of the frozen step with BN folded into the conv forward
        (freeze_bn(forward="fused")): ONE launch z = [relu](fmaf(acc, scale, shift) [+ residual]),
        no y stored -> (z, z16, record).  With a bf16 backward (``bwd16``) and ``copy16`` the launch
        is the dual form, which also writes z16 = bf16(z), the next conv's wgrad operand.  The
        record's ReLU-mask source is the unit's own output (z16 where it exists, else z) -- the
        tensor the next unit keeps as its x; y and zbits are None."""
        w = conv.weight
        c = w.shape[1]
        math, bwd16 = self.math, self.bwd16
        wk = _krsc(w, x.shape[3], False)
        scale, shift, inv = self.frozen[bn]
        z16 = None
        if bwd16 and copy16:
            z, z16 = ops.conv_fwd_fused_dual(x, wk, stride, pad, scale, shift, residual, relu,
                                             c_real=c)
        else:
            z = ops.conv_fwd_fused(x, wk, stride, pad, scale, shift, residual, relu, c_real=c,
                                   math=math)
        zm = (z16 if z16 is not None else z) if relu else None
        rec = self._record(conv, bn, x, x16, wk, None, zm, None, (scale, shift, bn.running_mean,
                           inv), stride, pad, relu, 1, residual is not None, bool(fold))
        return z, z16, rec

    def _record(self, conv, bn, x, x16, wk, y, z, zbits, coefs, stride, pad, relu, groups, res,
                fold):
        """The Unit of one forward unit.  coefs: (scale, shift, mean, inv).  bwd16: the backward's
        conv views read the bf16 copies (x16, a bf16 wt) in bf16 math, dy stored bf16."""
        w = conv.weight
        bwd16 = self.bwd16
        scale, shift, mean, inv = coefs
        return Unit(conv=conv, bn=bn, x=x16 if (bwd16 and x16 is not None) else x, wk=wk,
                    wt=_dgrad_weights(w, x, self.math, groups, bwd16, scale if fold else None),
                    y=y, z=z, zbits=zbits, scale=scale, shift=shift, mean=mean, inv=inv,
                    stride=stride, pad=pad, relu=relu, c_real=w.shape[1],
                    math="bf16" if bwd16 else self.math, groups=groups, res=res, dy16=bwd16,
                    fold=fold)

    def _run(self, x, conv, bn, stride, pad, relu, defer, residual=None, branch=None, dual=False,
             groups=1, x16=None, fold=True):
        """``groups``: a grouped conv (ResNeSt's radix-2 3x3).  ``x16`` (BWD16 step): the bf16
        copy of x for the record (None: the stem's NHWC4 input).  ``fold`` (frozen step): the
        unit's masked gradient will come from a fused dgrad, so its own dgrad reads CRSK weights
        pre-scaled by scale[k]."""
        math, bwd16, frozen = self.math, self.bwd16, self.frozen
        w = conv.weight
        c = w.shape[1]
        if groups > 1 and (bwd16 or frozen is not None):
            raise RuntimeError("the bf16-bwd and the frozen-BN steps have no grouped conv")
        s16 = _store16(math)
        wk = _krsc(w, x.shape[3], s16, groups)
        if frozen is not None:
            # no statistics: the running ones, through the coefficients of the step's one launch
            y = ops.conv_fwd(x, wk, stride, pad, c_real=c, math=math)
            scale, shift, inv = frozen[bn]
            mean = bn.running_mean
        else:
            # batch statistics come out of the conv epilogue (no separate pass over y)
            y, stats, nparts = ops.conv_fwd_bnstats(x, wk, stride, pad, c_real=c * groups,
                                                    math=math, y16=_act16(math), groups=groups)
            mean, inv, scale, shift = ops.bn_finalize(
                stats, nparts, bn.weight.detach(), bn.bias.detach(), bn.running_mean,
                bn.running_var, _bn_momentum(bn), bn.eps)
            self.nbt.append(bn.num_batches_tracked)
        has_res = residual is not None or branch is not None
        # fp32 block outputs on the LDS-DMA path also record their ReLU mask as bits: the dgrad
        # that produces their gradient reads 1 bit instead of z's 4 bytes (mask 3)
        bits = (self.keep and relu and not dual and _dma32(math) and y.dtype == torch.float32
                and has_res)
        z = zbits = z16 = None
        if not defer:
            if bwd16 and has_res and not bits:
                raise RuntimeError("bwd16: a residual unit without ReLU has no dual apply")
            z, zbits, z16 = _bn_apply_form(y, scale, shift, residual, branch, relu, bits,
                                           dual or bwd16, s16)
        rec = None
        if self.keep:
            rec = self._record(conv, bn, x, x16, wk, y, z if has_res else None, zbits,
                               (scale, shift, mean, inv), stride, pad, relu, groups, has_res,
                               bool(frozen is not None and fold))
        return (y, scale, shift), z, z16, rec


def _wgrad_dy_ok(rec, g):
    """The fused wgrad (tmr_conv2d_wgrad_bnbwd) serves this unit's operands."""
    kr, ks = rec.conv.weight.shape[2:]
    return (rec.groups == 1 and
            ops.conv_wgrad_bnbwd_ok(rec.x, g, rec.y, kr, ks, rec.stride, rec.pad))


def _wgrad_dy(rec, g, coef):
    """The fused wgrad: dy = A*g + B*y + C from the masked gradient g, the unit's y and the
    coefficients of its BN backward's reductions, formed while loading -> (dy, dw)."""
    kr, ks = rec.conv.weight.shape[2:]
    dw, dy = ops.conv_wgrad_bnbwd(rec.x, g, rec.y, coef, kr, ks, rec.stride, rec.pad,
                                  c_real=rec.c_real)
    return dy, dw


def _unit_dy(rec, dz, grads, parts=None, pool=None, want_dres=False, dres_inplace=False,
             fold=False):
    """The BatchNorm backward of one unit: writes the BN gradients -> (dy, dw, dres); dw only
    where the fused wgrad formed dy, dres (the identity branch's gradient) only if wanted.
    parts: dz was produced by a fused dgrad (conv_dgrad_bnbwd): it is already ReLU-masked and
    `parts` holds its BN-backward partial sums.  Otherwise the ReLU mask comes from the saved z,
    or is recomputed from y when there was no residual.  dres_inplace: the pre-activation
    gradient overwrites dz and is returned as dres.
    pool: the argmax of the maxpool that consumed this unit's output (the stems); dz is the
    pooled gradient, gathered inside the BN backward.
    fold: with parts, the fp32 wgrad may produce dy itself (WGRAD_BNBWD) where the library serves
    the unit; the ResNet-50 trunk's units only (records of math "fp32": not the BWD16 step's)."""
    bn = rec.bn
    gamma = bn.weight.detach()
    # dy feeds only this conv's dgrad / wgrad (the BWD16 step's records always store it bf16)
    s16 = rec.dy16 or _store16(rec.math)
    dw = dres = None
    if pool is not None:
        # maxpool backward + ReLU mask + BN backward without writing dz
        dy, dg, db = ops.bn_bwd_maxpool(dz, pool, rec.y, rec.scale, rec.shift, rec.mean, rec.inv,
                                        gamma, bf16=s16)
    elif parts is None:
        dy, dres, dg, db = ops.bn_bwd(dz, rec.y, rec.z, rec.mean, rec.inv, gamma, rec.relu,
                                      want_dres=want_dres, dres_out=dz if dres_inplace else None,
                                      scale=rec.scale, shift=rec.shift, bf16=s16)
    else:
        if fold and WGRAD_BNBWD and rec.math == "fp32" and _wgrad_dy_ok(rec, dz):
            coef, dg, db = ops.bn_bwd_parts_coef(rec.y, parts[0], parts[1], rec.mean, rec.inv,
                                                 gamma)
            dy, dw = _wgrad_dy(rec, dz, coef)
        else:
            dy, dg, db = ops.bn_bwd_parts(dz, rec.y, parts[0], parts[1], rec.mean, rec.inv,
                                          gamma, bf16=s16)
        dres = dz if want_dres else None
    grads[bn.weight] = dg
    grads[bn.bias] = db
    return dy, dw, dres


def _conv_bwd(rec, dy, grads, dw=None, dx_out=None, dx_beta=0.0, need_dx=True, fuse_prev=None,
              g16=False, r16=False, g16_y32=False):
    """wgrad (unless dw came with dy, _wgrad_dy) and dgrad (optionally accumulated into dx_out)
    of one unit from its conv's output gradient dy -> (dx, fused).

    fuse_prev: the unit whose BN output gradient this unit's dgrad produces -- its mask and
    partial sums are then computed in the dgrad epilogue; `fused` = those (parts, nparts).
    g16: the fused dgrad may store fuse_prev's masked gradient as bf16 (TMR_IO_G16) when that unit
    has no residual and the dgrad runs on the bf16 LDS-DMA engine (the bf16-activation step).
    r16: the same for fuse_prev a block output (R16): the dgrad adds into dx_out (bf16 in place,
    or fp32 read and a new bf16 tensor returned).
    g16_y32 (the frozen16 step, no knob): fuse_prev's masked gradient (mask 2) stored bf16 beside
    its fp32 y; a unit whose dgrad cannot take that form raises -- no rounding moves silently."""
    x = rec.x
    r, s = rec.conv.weight.shape[2:]
    grp = rec.groups
    grads[rec.conv.weight] = dw if dw is not None else ops.conv_wgrad(
        x, dy, r, s, rec.stride, rec.pad, c_real=rec.c_real, math=rec.math, groups=grp)
    if not need_dx:
        return None, None
    hw = (x.shape[1], x.shape[2])
    wt = rec.wt is not None
    wdg = rec.wt if wt else rec.wk
    if fuse_prev is None:
        return ops.conv_dgrad(dy, wdg, hw, rec.stride, rec.pad, out=dx_out, beta=dx_beta,
                              math=rec.math, wt=wt, groups=grp), None
    p = fuse_prev
    mask = (1 if p.res else 2) if p.relu else 0
    zm = p.z
    if mask == 1 and wt and p.zbits is not None:
        mask, zm = 3, p.zbits   # the ReLU mask as bits (LDS-DMA dgrad)
    elif mask == 1 and zm is None:   # (the BWD16 step keeps only the bits)
        raise RuntimeError("a residual unit's ReLU mask needs its saved z or its bits on "
                           "the LDS-DMA dgrad")
    bf8 = wt and p.y.dtype == torch.bfloat16 and (p.y.shape[-1] // grp) % 8 == 0
    # (a grouped dgrad -- ResNeSt's radix-2 conv -- stores its per-group channel slices bf16
    # too; the residual accumulation stays ungrouped)
    gb = g16 and G16 and mask == 2 and dx_out is None and dx_beta == 0.0 and bf8
    rb = (r16 and R16 and mask in (1, 3) and dx_out is not None and dx_beta == 1.0 and bf8
          and grp == 1)
    if g16_y32:
        shape = (tuple(dy.shape), tuple(rec.conv.weight.shape), rec.stride)
        gb = (mask == 2 and dx_out is None and dx_beta == 0.0 and wt and grp == 1
              and wdg.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16
              and p.y.dtype == torch.float32 and p.y.shape[-1] % 8 == 0)
        if not gb:
            raise RuntimeError("frozen BN, bf16 backward: the fused dgrad of dy %s, weight %s, "
                               "stride %d cannot store its masked gradient bf16 (mask %d)"
                               % (shape + (mask,)))
        try:
            dx, pp, npp = ops.conv_dgrad_bnbwd(dy, wdg, hw, rec.stride, rec.pad, p.y, p.mean, mask,
                                               scale=p.scale, shift=p.shift, math=rec.math, wt=wt,
                                               g16=True)
        except RuntimeError as e:
            raise RuntimeError("frozen BN, bf16 backward: the fused dgrad of dy %s, weight %s, "
                               "stride %d refused the bf16 masked gradient: %s" % (shape + (e,)))
        return dx, (pp, npp)
    old = None
    if rb and dx_out.dtype != torch.bfloat16:   # fp32 old dx -> a new bf16 dx
        old, dx_out = dx_out, None
    dx, pp, npp = ops.conv_dgrad_bnbwd(dy, wdg, hw, rec.stride, rec.pad, p.y, p.mean, mask,
                                       z=zm, scale=p.scale, shift=p.shift, out=dx_out,
                                       beta=dx_beta, math=rec.math, wt=wt, groups=grp,
                                       g16=gb or rb, old=old)
    return dx, (pp, npp)


def _unit_bwd(rec, dz, grads, parts=None, fold=False, **conv):
    """_unit_dy then _conv_bwd (its keywords) of a unit whose dy nothing else reads."""
    dy, dw, _ = _unit_dy(rec, dz, grads, parts=parts, fold=fold)
    return _conv_bwd(rec, dy, grads, dw=dw, **conv)


# ------------------------------------------------------------------ the backward's block loop
def _backward_blocks(ctx, grads, last_unit):
    """The skeleton of a trunk backward: pops ctx.blocks' (block module, its records) last to
    first and yields (block, records, last_unit(the previous block's records) -- the unit whose
    BN output gradient is this block's dx; None for the first block).  After the loop body the
    block's gradients are final: the gradient-ready hook (get_grad_ready) starts their exchange."""
    blocks = ctx.blocks
    ready = get_grad_ready(ctx.share)
    while blocks:
        blk, recs = blocks.pop()
        prev = last_unit(blocks[-1][1]) if blocks else None
        yield blk, recs, prev
        # (this frame must not keep the popped records alive past the body: once the body's own
        # references go, the block's saved tensors die -- that bounds the step's peak memory)
        del recs, prev
        if ready is not None:
            ready([(p, grads[p]) for p in blk.parameters() if p in grads])


def _backward_head(ctx, dfeat):
    """-> the gradient at the last block's output."""
    if not ctx.keep:
        raise RuntimeError("trunk backward needs train mode and a forward with grad enabled")
    return ops.avgpool_bwd(dfeat.contiguous(), ctx.last_hw)


def _backward_tail(ctx, grads):
    """The autograd result for (x4, share, keep, *params); drops the saved records."""
    out = tuple(grads.get(p) for p in ctx.params)
    ctx.blocks = ctx.stem = None
    return (None, None, None) + out


# ------------------------------------------------------------------ frozen BatchNorm
# share -> (signature, table, buffer, {bn: (scale, shift, inv)}): the device table of
# tmr_bn_frozen_params and the coefficient buffer it fills, rebuilt when a BN tensor moves
_FROZEN = weakref.WeakKeyDictionary()


def _share_bns(share):
    return [m for m in share.modules() if isinstance(m, nn.BatchNorm2d)]


def _bn_modes(share):
    """The BN modules' common mode -> "train" / "eval"; a share whose BN modules disagree, or
    whose bn_frozen flag a BN in train mode contradicts, raises."""
    modes = {m.training for m in _share_bns(share)}
    if len(modes) > 1:
        raise RuntimeError("the trunk's BatchNorm modules disagree (some in eval mode, some in "
                           "train mode): use tmrnet_amd.freeze_bn / unfreeze_bn on the whole trunk")
    if getattr(share, "bn_frozen", False) and True in modes:
        raise RuntimeError("bn_frozen is set but the trunk's BatchNorm modules are in train mode: "
                           "call tmrnet_amd.freeze_bn again, or unfreeze_bn")
    return "train" if True in modes else "eval"


def _frozen_step(share):
    """The frozen-BN train step applies: bn_frozen on a train-mode fp32 ResNet-50 share, or -- with
    freeze_bn(backward="bf16") -- on an "fp32" or "bf16-bwd" one (_frozen16)."""
    return bool(getattr(share, "bn_frozen", False) and share.training
                and (share.precision == "fp32" or _frozen16(share)))


# freeze_bn(backward="bf16"), "frozen16": the frozen step's fp32 forward (bit for bit, plus the
# BWD16 step's bf16 operand copies through the dual apply forms on the eval coefficients) and
# every trunk conv's dgrad / wgrad in bf16 math on three roundings (RNE, each once, where the
# value is produced): the bf16 input copy x; the weights -- a folded unit's dgrad reads the bf16
# CRSK copy of the fp32 product w[k]*scale[k], the single-pass units (the last block's bn3 /
# downsample BN, the stem) the plain bf16 forms; the output-gradient operand -- bf16(g), the
# masked gradient unscaled, for a folded unit (tmr_scale_rows scales the fp32 dW), bf16(g*scale)
# for a single-pass unit.  bn1 / bn2's g is stored bf16 by the fused dgrad that produces it
# (TMR_IO_G16 beside an fp32 y; its sums are of the rounded values); a block output's g stays
# fp32 (the residual stream; sums of the fp32 values) and one pass per block writes its bf16
# copy (ops.bn_frozen_bwd(want_g16=True): the downsample BN's sums-only pass, or a plain cast).
# In the walk (TrunkFn._backward_frozen) all of this is `f16`: dy16 / want_g16 of the frozen-BN
# passes, and the bf16 store of bn1 / bn2's g in _frozen_unit_bwd.  DESIGN.md §31.
def _frozen16(share):
    return bool(getattr(share, "bn_frozen", False) and share.training
                and getattr(share, "bn_frozen_bwd", None) == "bf16"
                and share.precision in ("fp32", BWD16))


# freeze_bn(affine=False, forward="fused"), DESIGN.md §32: the frozen step with BatchNorm folded
# into the conv forward.  Every non-stem unit is ONE launch z = [relu](fmaf(acc, scale, shift)
# [+ residual]) (ops.conv_fwd_fused; with a bf16 backward ops.conv_fwd_fused_dual, which also
# writes z16 = bf16(z), rounded once) -- the values of conv_fwd + bn_apply bit for bit, but y is
# never stored and no apply pass runs.  A unit's ReLU mask is its own stored output (z > 0 is the
# predicate fmaf(y, scale, shift) > 0), the tensor the next unit keeps as x anyway; with a bf16
# backward the mask is z16 > 0, which differs from z > 0 only where a positive fp32 z rounds to
# bf16 zero (below the bf16 subnormal range).  No BN gradient exists (affine=False), so nothing in
# the backward needs y.  The stem keeps conv_fwd + maxpool_fwd_bn[_dual] and its y.  The backward
# is the frozen step's one walk: a record without y sends the dgrad that produces its unit's
# gradient to ops.conv_dgrad_relu on the stored output (_frozen_unit_bwd).
def _frozen_fused(share):
    return bool(getattr(share, "bn_frozen", False) and share.training
                and getattr(share, "bn_frozen_fwd", None) == "fused")


def _frozen_coefs(share):
    """{bn: (scale, shift, inv)} of every BN of the share, computed by ONE launch from the current
    weight / bias / running statistics (ops.bn_frozen_params)."""
    bns = _share_bns(share)
    sig = tuple(t.data_ptr() for bn in bns
                for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    ent = _FROZEN.get(share)
    if ent is None or ent[0] != sig:
        table, buf, views = ops.bn_frozen_table(bns)
        ent = _FROZEN[share] = (sig, table, buf, dict(zip(bns, views)))
    ops.bn_frozen_params(ent[1], len(bns))
    return ent[3]


def _bn_wants_grad(bn):
    return bn.weight.requires_grad or bn.bias.requires_grad


def _frozen_affine(rec, parts, grads):
    """dgamma / dbeta of a frozen unit from partial sums (its own pass's, or a fused dgrad's)."""
    if parts is not None and _bn_wants_grad(rec.bn):
        grads[rec.bn.weight], grads[rec.bn.bias] = ops.bn_frozen_finalize(
            parts[0], parts[1], rec.inv)


def _frozen_unit_bwd(rec, gy, grads, f16, real_dy=False, parts=None, prev=None, dx_out=None,
                     dx_beta=0.0, need_dx=True):
    """wgrad and dgrad of one unit of the frozen step -> (dx, the partial sums that came with it).
    gy: the unit's masked gradient g, from a fused dgrad (`parts` -> the BN gradients) -- the wgrad
    runs on g and dW's rows take scale[k], the dgrad reads the pre-scaled CRSK weights (rec.fold),
    no pass forms dy = g*scale; or (real_dy) the dy = g*scale a single-pass kernel wrote.
    prev: the unit whose output gradient this dgrad produces, masked by what that unit stored: its
    ReLU output where the forward kept no y (ops.conv_dgrad_relu; no sums), else y / z / bits with
    the partial sums (_conv_bwd).  f16 (the bf16 backward): that gradient is stored bf16 unless
    prev is a block output (the residual stream's gradient stays fp32); a dgrad that cannot
    raises with its shape."""
    _frozen_affine(rec, parts, grads)
    if real_dy and rec.fold:
        raise RuntimeError("frozen BN: a real dy meets pre-scaled dgrad weights")
    if not (real_dy or rec.fold):
        raise RuntimeError("frozen BN: a folded unit needs its pre-scaled dgrad weights")
    r, s = rec.conv.weight.shape[2:]
    dw = ops.conv_wgrad(rec.x, gy, r, s, rec.stride, rec.pad, c_real=rec.c_real, math=rec.math)
    # (dW's rows are scaled before the dgrad for a unit without y, after it otherwise: the launch
    # order scripts/step_trace.py pins)
    if rec.fold and rec.y is None:
        ops.scale_rows(dw, rec.scale)
    g16 = bool(f16 and prev is not None and not prev.res)
    if need_dx and prev is not None and prev.y is None:
        if not prev.relu or prev.z is None:
            raise RuntimeError("frozen BN, fused forward: the masked dgrad needs the previous "
                               "unit's stored ReLU output")
        grads[rec.conv.weight] = dw
        wt = rec.wt is not None
        try:
            dx, fused = ops.conv_dgrad_relu(
                gy, rec.wt if wt else rec.wk, (rec.x.shape[1], rec.x.shape[2]), rec.stride,
                rec.pad, prev.z, out=dx_out, beta=dx_beta, math=rec.math, wt=wt, g16=g16), None
        except RuntimeError as e:
            raise RuntimeError("frozen BN, fused forward: the masked dgrad of dy %s, weight %s, "
                               "stride %d refused its operands (mask source %s, beta %g): %s"
                               % (tuple(gy.shape), tuple(rec.conv.weight.shape), rec.stride,
                                  prev.z.dtype, dx_beta, e))
    else:
        dx, fused = _conv_bwd(rec, gy, grads, dw=dw, dx_out=dx_out, dx_beta=dx_beta,
                              need_dx=need_dx, fuse_prev=prev, g16_y32=g16)
    if rec.fold and rec.y is not None:
        ops.scale_rows(dw, rec.scale)
    return dx, fused


class TrunkFn(torch.autograd.Function):
    """Whole ResNet-50 trunk as one autograd node: x NHWC4 (F,224,224,4) -> (F,2048)."""

    @staticmethod
    def forward(ctx, x4, share, keep, *params):
        _bn_modes(share)
        # the frozen-BN step: every BN's coefficients in one launch, before the layout session's
        # launch scales the dgrad weights by them (a session of its own: it holds those copies)
        fz = _frozen_coefs(share) if _frozen_step(share) else None
        # every conv weight layout of the step in one launch (ops.layout_session)
        key = ("resnet50", share.training, bool(keep), share.precision, _infer16(share))
        if fz is not None:
            key += ("frozen16" if _frozen16(share) else "frozen",)
            if keep and _frozen_fused(share):
                key += ("fused",)
        with ops.layout_session(share, key):
            return TrunkFn._forward(ctx, x4, share, keep, params, fz)

    @staticmethod
    def _forward(ctx, x4, share, keep, params, fz=None):
        keep = keep and share.training
        conv1, bn1, layers = share.trunk_parts()
        mt = _fwd_math(share.precision)
        ctx.keep = keep
        ctx.frozen = fz is not None
        ctx.frozen16 = f16z = bool(fz is not None and keep and _frozen16(share))
        ctx.frozen_fused = False
        if not share.training:
            return TrunkFn._forward_eval(x4, conv1, bn1, layers, mt, _infer16(share))
        # the BWD16 step: the fp32 forward plus the bf16 copies its bf16-math backward reads
        # (without a backward to record -- no grad -- it is the fp32 path itself)
        # (frozen16: the same copies under the frozen step, whichever precision the share has)
        bw = bool(keep and share.precision == BWD16) if fz is None else f16z
        a16 = _act16(mt)                    # every activation bf16: no fp32 copies
        f16 = _full16(mt) and not a16
        st = _TrainUnits(mt, keep, bwd16=bw, frozen=fz)
        # freeze_bn(forward="fused"): a recorded frozen step whose non-stem units never store y
        # (without a backward to record the forward is the unfused one: the same bits)
        ctx.frozen_fused = fu = bool(fz is not None and keep and _frozen_fused(share))
        if fu and any(_bn_wants_grad(bn) for bn in _share_bns(share)):
            raise RuntimeError("frozen BN, forward=\"fused\": a BatchNorm weight or bias requires "
                               "grad, but dgamma needs the conv output, which this step does not "
                               "store: call tmrnet_amd.freeze_bn(..., affine=False) again")
        # bf16 activations: the stem reads an NHWC8 bf16 copy of its input (8-channel pieces: the
        # LDS-DMA engine; exact, the bf16 math rounds x anyway)
        xs = ops.nhwc4_to_bf16x8(x4) if (a16 and ops.engine_forced()) else x4
        # share.bn1 + relu applied inside the maxpool (the backward recomputes the ReLU mask from
        # y, so the stem's BN output is never needed)
        (y0, sc0, sh0), r0 = st.deferred(xs, conv1, bn1, 2, 3, True, fold=False)
        h16 = None   # (bw: the bf16 copy of the block input, the wgrads' operand)
        if bw:
            p, h16, am = ops.maxpool_fwd_bn_dual(y0, sc0, sh0)
        else:
            p, am = ops.maxpool_fwd_bn(y0, sc0, sh0, bf16=f16)
        # h: the block input as the identity residual (fp32), hx: as the conv operand (the bf16
        # copy under f16; the maxpool output is only ever a conv operand)
        h, hx = (None, p) if f16 else (p, p)
        blocks = []
        last = layers[-1][-1]
        unit = st.fused if fu else st.unit
        for layer in layers:
            for blk in layer:
                # fu: BN folded into the conv forward -- one launch per unit, no y, no apply pass
                z1, z1h, r1 = unit(hx, blk.conv1, blk.bn1, 1, 0, True, x16=h16)
                z2, z2h, r2 = unit(z1, blk.conv2, blk.bn2, blk.stride, 1, True, x16=z1h)
                # the frozen step: every unit but the last block's bn3 / downsample BN (whose g
                # arrives unmasked) folds its dy scale into its dgrad weights
                fold = blk is not last
                rd, idn, how = None, h, "residual"
                if blk.downsample is not None and fu:
                    # a fused unit without ReLU whose fp32 output (no conv operand: no bf16 copy)
                    # is conv3's residual
                    idn, _, rd = st.fused(hx, blk.downsample[0], blk.downsample[1], blk.stride, 0,
                                          False, x16=h16, fold=fold, copy16=False)
                elif blk.downsample is not None:
                    # the branch's BN is applied inside the BN3 pass (bn_apply2)
                    how = "branch"
                    idn, rd = st.deferred(hx, blk.downsample[0], blk.downsample[1], blk.stride, 0,
                                          False, x16=h16, fold=fold)
                elif h is None:
                    raise RuntimeError("identity residual of the stem output (no downsample)")
                # (fu: the last block's output is no conv operand -- fp32 only, which is also the
                # mask-1 source of its bn3's single pass)
                out = dict(copy16=fold) if fu else dict(dual=f16)
                h, hc, r3 = unit(z2, blk.conv3, blk.bn3, 1, 0, True, x16=z2h, fold=fold,
                                 **{how: idn}, **out)
                hx = hc if f16 else h
                if bw:
                    h16 = hc
                    if blocks and not fu:   # the previous block output's fp32 z: its mask is in
                        blocks[-1][1][-1].z = None   # the bits (fu: z is the mask)
                if bw or fu:   # (their fp32 z's were only this block's forward operands; with a
                    del z1, z2, idn   # bf16 backward the records hold the bf16 copies only)
                blocks.append((blk, [r1, r2, rd, r3]))
        if f16z and blocks[-1][1][-1].zbits is not None:
            blocks[-1][1][-1].z = None   # (the last block's mask is in the bits too)
        feat = ops.avgpool_fwd(h)
        if st.nbt:   # (none under frozen BN: no counter moves)
            ops.counters_add_one(st.nbt)
        if keep:
            ctx.share = share
            ctx.params = params
            ctx.stem = [r0]
            ctx.pool = (am, (y0.shape[1], y0.shape[2]))
            ctx.blocks = blocks
            ctx.last_hw = (h.shape[1], h.shape[2])
        return feat

    @staticmethod
    def _forward_eval(x4, conv1, bn1, layers, mt, i16):
        """Eval mode.  i16 (opt-in, share.infer_act16): every stored activation bf16, rounded once
        after BN (+residual) (+ReLU) by the conv's epilogue; the block output is the next block's
        operand and identity."""
        if i16:
            # the stem reads the NHWC8 bf16 copy of its input on the LDS-DMA engine; its bf16
            # output is already >= 0, so the bf16 maxpool with an identity BatchNorm is exact
            z = _conv_bn_eval(ops.nhwc4_to_bf16x8(x4), conv1, bn1, 2, 3, True, mt, y16=True)
            p, am = ops.maxpool_fwd_bn(z, torch.ones_like(bn1.running_mean),
                                       torch.zeros_like(bn1.running_mean))
        else:
            z = _conv_bn_eval(x4, conv1, bn1, 2, 3, True, mt)
            p, am = ops.maxpool_fwd(z)
        h = p
        for layer in layers:
            for blk in layer:
                z1 = _conv_bn_eval(h, blk.conv1, blk.bn1, 1, 0, True, mt, y16=i16)
                z2 = _conv_bn_eval(z1, blk.conv2, blk.bn2, blk.stride, 1, True, mt, y16=i16)
                idn = h
                if blk.downsample is not None:
                    idn = _conv_bn_eval(h, blk.downsample[0], blk.downsample[1], blk.stride, 0,
                                        False, mt, y16=i16)
                h = _conv_bn_eval(z2, blk.conv3, blk.bn3, 1, 0, True, mt, residual=idn, y16=i16)
        return ops.avgpool_fwd(h)

    @staticmethod
    def backward(ctx, dfeat):
        if ctx.frozen:
            return TrunkFn._backward_frozen(ctx, dfeat)
        grads = {}
        g = _backward_head(ctx, dfeat)   # grad at the last block output
        pending = None     # BN-backward partials of g when the dgrad that produced it was fused
        for blk, brec, prev3 in _backward_blocks(ctx, grads, lambda recs: recs[-1]):
            r1, r2, rd, r3 = brec   # (rd: None without a downsample)
            has_ds = rd is not None
            # g (owned here) becomes the masked pre-ReLU gradient = the identity-branch grad
            dw3 = dyd = dwd = cd = None
            if has_ds and _ds_dual(g, r3, rd) and pending is not None:
                # (g came masked from the next block's fused dgrad)
                bargs = (g, r3.y, pending[0], pending[1], r3.mean, r3.inv,
                         r3.bn.weight.detach(), rd.y, rd.mean, rd.inv, rd.bn.weight.detach())
                f3, fd = _ds_fold(g, r3, rd)
                if f3 or fd:
                    # the served units' wgrads produce their dy themselves (g outlives both: dres)
                    c3, dg3, db3, cd, dgd, dbd, dy3, dyd = ops.bn_bwd_parts_ds(
                        *bargs, fold3=f3, foldd=fd)
                    if f3:
                        dy3, dw3 = _wgrad_dy(r3, g, c3)
                    if not fd:
                        cd = None
                else:
                    dy3, dg3, db3, dyd, dgd, dbd = ops.bn_bwd_parts_ds(
                        *bargs, dy16=_ds_dy16(r3, rd))
                grads[r3.bn.weight], grads[r3.bn.bias] = dg3, db3
                grads[rd.bn.weight], grads[rd.bn.bias] = dgd, dbd
                dres = g
            else:
                dy3, dw3, dres = _unit_dy(r3, g, grads, parts=pending, want_dres=True,
                                          dres_inplace=True, fold=True)
            dz2, fz2 = _conv_bwd(r3, dy3, grads, dw=dw3, fuse_prev=r2, g16=True)
            del dy3
            dz1, fz1 = _unit_bwd(r2, dz2, grads, parts=fz2, fold=True, fuse_prev=r1, g16=True)
            del dz2
            if has_ds:
                # the strided downsample dgrad writes dx (its tap-less parity classes as zeros),
                # the stride-1 conv1 dgrad accumulates into it with the fused BN backward
                # (measured 51.1 vs 51.6 ms of dgrads per C2 step against the other order,
                # profiles/r3/bench_r4f/)
                if cd is not None:
                    dyd, dwd = _wgrad_dy(rd, dres, cd)
                elif dyd is None:
                    dyd, dwd, _ = _unit_dy(rd, dres, grads)
                dres, _ = _conv_bwd(rd, dyd, grads, dw=dwd)
                del dyd
            g, pending = _unit_bwd(r1, dz1, grads, parts=fz1, fold=True, dx_out=dres,
                                   dx_beta=1.0, fuse_prev=prev3, r16=True)
            del dz1, brec, dres
        am, _ = ctx.pool
        dy0, _, _ = _unit_dy(ctx.stem[0], g, grads, pool=am)
        _conv_bwd(ctx.stem[0], dy0, grads, need_dx=False)
        return _backward_tail(ctx, grads)

    @staticmethod
    def _backward_frozen(ctx, dfeat):
        """The frozen-BN step's backward, for every forward and backward of freeze_bn: no
        BN-backward projection anywhere.  The last block's bn3 (g unmasked from the avgpool) and the
        stem (g through the maxpool) take one pass of tmr_bn_frozen_bwd / _maxpool; every other
        unit's g comes masked from the dgrad that produced it (with its partial sums where the
        forward stored y), and its dy = g*scale lives in the conv operands (_frozen_unit_bwd).  A
        downsample BN that trains needs sum g*(y_ds - mean_ds) of its own: one sums-only pass over
        (g, y_ds).  The records say what the forward was: a unit of forward="fused" has no y, its
        mask source is z, and no BN of that step wants a gradient, so no sums are ever asked for.
        ctx.frozen16: the same walk on the bf16 operands of freeze_bn(backward="bf16")
        ("_frozen16" above)."""
        grads = {}
        f16 = ctx.frozen16
        g = _backward_head(ctx, dfeat)   # grad at the last block output
        masked = False     # g came masked from the next block's conv1 dgrad
        pending = None     # that dgrad's partial sums of g, where it emits them
        for blk, brec, prev3 in _backward_blocks(ctx, grads, lambda recs: recs[-1]):
            r1, r2, rd, r3 = brec   # (rd: None without a downsample)
            has_ds = rd is not None
            dyd = gop = None
            if not masked:
                # g unmasked: mask (the block output's bits, or z), dres in place, dy's and sums
                # at once
                s3 = _bn_wants_grad(r3.bn)
                bits = r3.zbits   # (without bits -- forward="fused" -- the mask is z > 0)
                mask = 1 if bits is None else 3
                if has_ds:
                    if r3.y is None:
                        raise RuntimeError("frozen BN, fused forward: a last block with a "
                                           "downsample branch has no single-pass form")
                    sums = s3 or _bn_wants_grad(rd.bn)
                    dy3, dyd, _, p3, pd, npp = ops.bn_frozen_bwd_ds(
                        g, r3.y, r3.scale, r3.shift, r3.mean, rd.y, rd.scale, rd.mean,
                        mask=mask, z=r3.z if bits is None else None, bits=bits,
                        dres_inplace=True, want_sums=sums, dy16=f16)
                else:
                    sums = s3
                    dy3, _, p3, npp = ops.bn_frozen_bwd(
                        g, r3.y, r3.scale, r3.shift, r3.mean,
                        mask=mask, z=r3.z if bits is None else None, bits=bits,
                        dres_inplace=True, want_sums=sums, dy16=f16)
                _frozen_affine(r3, (p3, npp) if sums else None, grads)
                if has_ds:
                    _frozen_affine(rd, (pd, npp) if sums else None, grads)
                dz2, fz2 = _frozen_unit_bwd(r3, dy3, grads, f16, real_dy=True, prev=r2)
                del dy3
            else:
                dsum = has_ds and _bn_wants_grad(rd.bn)
                gop = g    # the folded units' conv operand: g, or (f16) its bf16 copy
                if f16 or dsum:
                    # one pass over the block output's fp32 g: the downsample BN's sums of
                    # (g, y_ds), and / or (f16) the store of bf16(g) -- alone, a plain cast
                    u = rd if dsum else r3
                    _, g16, pd, npp = ops.bn_frozen_bwd(g, u.y, u.scale, u.shift, u.mean, mask=0,
                                                        want_dy=False, want_sums=dsum,
                                                        want_g16=f16)
                    if f16:
                        gop = g16
                    del g16, u
                    if dsum:
                        _frozen_affine(rd, (pd, npp), grads)
                dz2, fz2 = _frozen_unit_bwd(r3, gop, grads, f16, parts=pending, prev=r2)
            dres = g   # masked: the identity branch's gradient
            dz1, fz1 = _frozen_unit_bwd(r2, dz2, grads, f16, parts=fz2, prev=r1)
            del dz2
            if has_ds:
                dres, _ = _frozen_unit_bwd(rd, gop if dyd is None else dyd, grads, f16,
                                           real_dy=dyd is not None)
            del gop, dyd
            g, pending = _frozen_unit_bwd(r1, dz1, grads, f16, parts=fz1, prev=prev3, dx_out=dres,
                                          dx_beta=1.0)
            masked = True
            del dz1, brec, dres
        am, _ = ctx.pool
        st = ctx.stem[0]
        ss = _bn_wants_grad(st.bn)
        dy0, p0, np0 = ops.bn_frozen_bwd_maxpool(g, am, st.y, st.scale, st.shift, st.mean,
                                                 want_sums=ss, dy16=f16)
        _frozen_unit_bwd(st, dy0, grads, f16, real_dy=True, parts=(p0, np0) if ss else None,
                         need_dx=False)
        return _backward_tail(ctx, grads)


_CHILD_NAMES = ("conv1", "bn1", "relu", "maxpool", "layer1", "layer2", "layer3", "layer4",
                "avgpool")


class ResNet50Share(nn.Sequential):
    """The reference's `share` Sequential (keys identical to torchvision's resnet50 children).

    ``indexed=True`` names the children "0".."8" instead, which is the
    ``Sequential(*list(resnet50().children())[:-1])`` layout of code/models.py:26-28
    (keys ``res.0.weight``, ``res.4.0.conv1.weight``, ...).
    """

    def __init__(self, indexed=False, precision="fp32"):
        super().__init__()
        # conv operand precision: "fp32" | "bf16" (ops.MATH), or "bf16-bwd" (BWD16: the fp32
        # forward, bf16 operands in the backward convs only)
        if precision not in ("fp32", "bf16", BWD16):
            raise ValueError("precision must be 'fp32', 'bf16' or 'bf16-bwd', got %r" % (precision,))
        self.precision = precision
        # eval mode under precision "bf16", opt-in: bf16 activations (TrunkFn._forward_eval i16; the
        # default keeps every eval path's fp32 activations and bits)
        self.infer_act16 = False
        # frozen BatchNorm (tmrnet_amd.freeze_bn): the BN modules stay in eval mode whatever
        # train(mode) says, and a train-mode step runs on the running statistics
        self.bn_frozen = False
        self.bn_frozen_bwd = None   # "bf16": the frozen step's backward convs in bf16 math
        self.bn_frozen_fwd = None   # "fused": BN folded into the conv forward, no y stored
        mods = (nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(64),
                nn.ReLU(inplace=True), nn.MaxPool2d(3, stride=2, padding=1),
                _make_layer(64, 64, 3, 1), _make_layer(256, 128, 4, 2),
                _make_layer(512, 256, 6, 2), _make_layer(1024, 512, 3, 2),
                nn.AdaptiveAvgPool2d((1, 1)))
        for i, (name, m) in enumerate(zip(_CHILD_NAMES, mods)):
            self.add_module(str(i) if indexed else name, m)
        # torchvision init: kaiming_normal fan_out for convs, BN gamma=1 beta=0
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def trunk_parts(self):
        ch = list(self.children())
        return ch[0], ch[1], ch[4:8]

    def train(self, mode=True):
        super().train(mode)
        if getattr(self, "bn_frozen", False):
            for m in _share_bns(self):
                m.training = False
        return self

    def features_nhwc4(self, x4):
        """x4: (F,224,224,4) fp32 NHWC, 4th channel zero -> (F,2048)."""
        params = list(self.parameters())
        # grad mode is off inside autograd.Function.forward: decide here whether to save
        keep = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        return TrunkFn.apply(x4, self, keep, *params)

    def forward(self, x):
        """x: (F,3,224,224) fp32 NCHW (reference layout) -> (F,2048,1,1)."""
        x = x.reshape(-1, 3, x.shape[-2], x.shape[-1]).contiguous()
        x4 = ops.nchw_to_nhwc(x, cpad=4)
        feat = self.features_nhwc4(x4)
        return feat.view(feat.shape[0], feat.shape[1], 1, 1)


def resnet50_share():
    return ResNet50Share()


def _share_of(model):
    """The trunk of a package model: the model itself, its `share` or its `res`."""
    from .resnest import ResNeSt50Share
    kinds = (ResNet50Share, ResNeSt50Share)
    if isinstance(model, kinds):
        return model
    for name in ("share", "res"):
        m = getattr(model, name, None)
        if isinstance(m, kinds):
            return m
    raise TypeError("freeze_bn / unfreeze_bn take a ResNet50Share or a package model that holds "
                    "one as .share or .res, got %s" % type(model).__name__)


def freeze_bn(model_or_share, affine=True, backward=None, forward=None):
    """Freeze the trunk's BatchNorm: every BatchNorm2d of the share goes to eval mode and stays
    there through train() / eval() (share.bn_frozen = True); a train-mode step then normalises
    with the running statistics, writes none of them, and back-propagates dy = g*scale.
    affine=False also stops training the BN weights and biases (requires_grad=False;
    torchvision's FrozenBatchNorm2d).  ResNet-50 shares of precision "fp32" only.
    backward="bf16" (share.bn_frozen_bwd): the same fp32 forward -- logits and loss bit for bit --
    with every trunk conv's dgrad and wgrad in bf16 math on fp32 accumulation, the backward of
    precision "bf16-bwd" under frozen BatchNorm; ResNet-50 shares of precision "fp32" or
    "bf16-bwd".  backward=None or "fp32": the fp32 backward.
    forward="fused" (share.bn_frozen_fwd; needs affine=False, combines with every backward): each
    non-stem conv + BN (+ residual) (+ ReLU) unit is one launch that never stores the conv output
    and runs no BatchNorm apply pass; logits, loss and every gradient are those of the unfused
    affine=False step bit for bit (with backward="bf16" the ReLU masks are read from the bf16
    copies: they differ only where a positive output rounds to bf16 zero), with less memory.
    forward=None or "apply": conv, then the BatchNorm apply pass.  Call it after load_checkpoint
    and before the optimizer is built.  Returns its argument."""
    from .resnest import ResNeSt50Share
    if backward not in (None, "fp32", "bf16"):
        raise ValueError("freeze_bn: backward must be None, 'fp32' or 'bf16', got %r" % (backward,))
    if forward not in (None, "apply", "fused"):
        raise ValueError("freeze_bn: forward must be None, 'apply' or 'fused', got %r" % (forward,))
    share = _share_of(model_or_share)
    if backward == "bf16":
        if isinstance(share, ResNeSt50Share):
            raise ValueError("freeze_bn: backward=\"bf16\" exists for the ResNet-50 trunk only, "
                             "not for a ResNeSt-50 share")
        if share.precision not in ("fp32", BWD16):
            raise ValueError("freeze_bn: backward=\"bf16\" exists for precision 'fp32' and "
                             "'bf16-bwd' (both run the fp32 forward), not for %r"
                             % (share.precision,))
    else:
        if isinstance(share, ResNeSt50Share):
            raise ValueError("freeze_bn: frozen BatchNorm exists for the ResNet-50 trunk "
                             "(precision 'fp32') only, not for a ResNeSt-50 share")
        if share.precision != "fp32":
            raise ValueError("freeze_bn: frozen BatchNorm exists for precision 'fp32' only, not for "
                             "%r" % (share.precision,))
    if forward == "fused" and affine:
        raise ValueError("freeze_bn: forward=\"fused\" needs affine=False: dgamma needs the conv "
                         "output, which this step does not store")
    share.bn_frozen = True
    share.bn_frozen_bwd = "bf16" if backward == "bf16" else None
    share.bn_frozen_fwd = "fused" if forward == "fused" else None
    for m in _share_bns(share):
        m.training = False
        if not affine:
            m.weight.requires_grad_(False)
            m.bias.requires_grad_(False)
    return model_or_share


def unfreeze_bn(model_or_share):
    """Undo freeze_bn: clear share.bn_frozen (and bn_frozen_bwd, bn_frozen_fwd), put the BatchNorm modules back to
    share.training and their weights and biases back to requires_grad=True.  Returns its
    argument."""
    share = _share_of(model_or_share)
    share.bn_frozen = False
    share.bn_frozen_bwd = None
    share.bn_frozen_fwd = None
    for m in _share_bns(share):
        m.training = share.training
        m.weight.requires_grad_(True)
        m.bias.requires_grad_(True)
    return model_or_share
