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
            and r3["math"] == "fp32" and rd["math"] == "fp32" and g.numel() >= WGRAD_BNBWD_DS_MIN):
        return False, False

    def ok(rec):
        kr, ks = rec["conv"].weight.shape[2:]
        return (rec.get("groups", 1) == 1 and
                ops.conv_wgrad_bnbwd_ok(rec["x"], g, rec["y"], kr, ks, rec["stride"], rec["pad"]))
    return ok(r3), ok(rd)


def _ds_dual(g, r3, rd):
    """DS_DUAL applies: g, y3 and y_ds of one dtype, which is also the dy dtype the separate passes
    would write (fp32 y under bf16 storage writes bf16 dy: not this path -- except the BWD16
    step's records, whose fp32 g / y / y_ds in, bf16 dy's out form is _ds_dy16), 8-channel
    multiples."""
    y = r3["y"]
    return (DS_DUAL and g.is_contiguous() and g.dtype == y.dtype == rd["y"].dtype
            and y.shape == rd["y"].shape and y.shape[-1] % 8 == 0
            and (_ds_dy16(r3, rd) or not (_store16(r3["math"]) and y.dtype == torch.float32)))


def _ds_dy16(r3, rd):
    """The BWD16 step's downsample blocks: fp32 g, y3, y_ds, both dy's stored bf16
    (ops.bn_bwd_parts_ds(dy16=True))."""
    return bool(r3.get("dy16") and rd.get("dy16") and r3["y"].dtype == torch.float32)

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


def _conv_bn(x, conv, bn, stride, pad, relu, training, residual=None, recs=None, math="fp32",
             defer=False, branch=None, nbt=None, dual=False, groups=1, y16=False, bwd16=False,
             x16=None, frozen=None, fold=False):
    """conv (NHWC implicit GEMM) -> BN -> (+residual) -> (ReLU); returns z.

    Train mode only: ``defer`` returns (y, scale, shift) instead of applying the BN -- the
    consumer applies it on load (the downsample branch inside its block's BN3 pass, the stem
    inside the maxpool); ``branch`` = such a deferred (y, scale, shift) used as the residual.
    ``dual`` (block outputs under
    _full16): returns (z fp32, z bf16 copy).  ``groups``: a grouped conv
    (train mode, or eval mode with y16; ResNeSt's radix-2 3x3, tmr_conv_desc.groups).  ``y16``
    (eval mode, bf16 activations: the shares' infer_act16): x and residual bf16, z rounded once
    to bf16.  ``bwd16`` (train mode with recs, math "fp32": the BWD16 step): the forward of
    math "fp32", returning (z fp32, z bf16 copy) unless deferred, and a record for a bf16-math
    backward -- ``x16`` the bf16 copy of x (None: the stem's NHWC4 input), the bf16 CRSK weights.
    ``frozen`` (train mode, math "fp32": the frozen-BN step, _frozen_coefs): this BN's (scale,
    shift, inv) of the running statistics -- the conv stores y without a statistics epilogue and
    the apply forms below take the eval coefficients; ``fold``: the unit's masked gradient will
    come from a fused dgrad, so its own dgrad reads CRSK weights pre-scaled by scale[k]
    (dy = g*scale is never formed)."""
    w = conv.weight
    if frozen is not None and not (training and math == "fp32" and groups == 1 and not dual
                                   and not y16 and not bwd16):
        raise RuntimeError("frozen BatchNorm is the train-mode fp32 step of an ungrouped conv")
    k, c, r, s = w.shape
    if bwd16 and not (training and recs is not None and math == "fp32" and groups == 1
                      and not dual and not y16):
        raise RuntimeError("bwd16 is the train-mode fp32 forward of an ungrouped conv with a "
                           "recorded backward")
    cs = x.shape[3]
    s16 = _store16(math)
    if r == 1 and s == 1 and c == cs and not s16:
        wk = w.detach().contiguous().view(k, 1, 1, c)   # OIHW == KRSC for 1x1
    else:   # (grouped: torch's (K, C/G, R, S) -> stacked per-group KRSC blocks (K, R, S, C/G))
        wk = ops.weight_to_krsc(w.detach().contiguous(), cpad=cs // groups, bf16=s16)
    if groups > 1 and not training and not y16:
        raise RuntimeError("grouped convs run in the train-mode trunk and the bf16-activation "
                           "inference trunk (y16) only")
    if training and frozen is not None:
        # no statistics: the running ones, through the coefficients of the step's one launch
        y = ops.conv_fwd(x, wk, stride, pad, c_real=c, math=math)
        scale, shift, inv = frozen
        mean = bn.running_mean
    elif training:
        # batch statistics come out of the conv epilogue (no separate pass over y)
        y, stats, nparts = ops.conv_fwd_bnstats(x, wk, stride, pad, c_real=c * groups, math=math,
                                                y16=_act16(math), groups=groups)
        mean, inv, scale, shift = ops.bn_finalize(
            stats, nparts, bn.weight.detach(), bn.bias.detach(), bn.running_mean,
            bn.running_var, _bn_momentum(bn), bn.eps)
        # num_batches_tracked += 1; the trunk batches these into one launch (nbt list)
        if nbt is None:
            bn.num_batches_tracked.add_(1)
        else:
            nbt.append(bn.num_batches_tracked)
    else:
        # eval: running-stat BN, residual and ReLU in the conv epilogue (one launch, no y pass;
        # same arithmetic as conv_fwd + bn_apply)
        scale, shift = ops.bn_eval_params(bn.weight.detach(), bn.bias.detach(), bn.running_mean,
                                          bn.running_var, bn.eps)
        return ops.conv_fwd_fused(x, wk, stride, pad, scale, shift, residual, relu, c_real=c,
                                  math=math, y16=y16, groups=groups)
    # fp32 block outputs on the LDS-DMA path also record their ReLU mask as bits: the dgrad that
    # produces their gradient reads 1 bit instead of z's 4 bytes (mask 3)
    zbits = None
    # (bf16 activations too: the bits of the rounded z, tmr_bn_apply_bits_a16)
    bits = (recs is not None and relu and not dual and _dma32(math) and y.dtype == torch.float32
            and (residual is not None or branch is not None))
    z16 = None
    if defer:
        z = None
    elif bwd16 and bits and branch is not None:
        z, zbits, z16 = ops.bn_apply2_bits_dual(y, scale, shift, branch[0], branch[1], branch[2])
    elif bwd16 and bits:
        z, zbits, z16 = ops.bn_apply_bits_dual(y, scale, shift, residual)
    elif bwd16:
        if residual is not None or branch is not None:
            raise RuntimeError("bwd16: a residual unit without ReLU has no dual apply")
        z, z16 = ops.bn_apply_dual(y, scale, shift, None, relu)
    elif branch is not None and bits:
        z, zbits = ops.bn_apply2_bits(y, scale, shift, branch[0], branch[1], branch[2])
    elif bits:
        z, zbits = ops.bn_apply_bits(y, scale, shift, residual)
    elif branch is not None:
        z = ops.bn_apply2(y, scale, shift, branch[0], branch[1], branch[2], relu, dual=dual)
    elif dual:
        z = ops.bn_apply_dual(y, scale, shift, residual, relu)
    else:
        # a non-residual unit's output is only ever a conv operand (next conv's forward and
        # wgrad; the backward recomputes its ReLU mask from y): bf16 under bf16 math (with bf16
        # activations every z is bf16: the dtype of y decides)
        z = ops.bn_apply(y, scale, shift, residual, relu, bf16=s16 and residual is None)
    if recs is not None:
        # without a residual the backward recomputes the ReLU mask from y (scale/shift)
        has_res = residual is not None or branch is not None
        # the dgrad view of a bf16-operand conv reads the transposed weights (LDS-DMA engine)
        if bwd16:   # (the stem's 3 input channels: no dgrad)
            wt = ops.weight_to_crsk(w.detach().contiguous()) if c % 8 == 0 else None
        elif frozen is not None and fold:
            wt = ops.weight_to_crsk_scaled(w.detach().contiguous(), scale)
        elif groups > 1 and ((_full16(math) and x.dtype == torch.bfloat16) or _dma32(math)):
            wt = ops.weight_to_crsk_grouped(w.detach().contiguous(), groups,
                                            bf16=x.dtype == torch.bfloat16)
        elif _full16(math) and x.dtype == torch.bfloat16:
            wt = ops.weight_to_crsk(w.detach().contiguous())
        elif _dma32(math) and c % 8 == 0 and x.dtype == torch.float32:
            wt = ops.weight_to_crsk(w.detach().contiguous(), bf16=False)
        else:   # (the stem's 3 input channels: no dgrad)
            wt = None
        # bwd16: the backward's conv views read the bf16 copies in bf16 math, dy stored bf16
        recs.append({"x": x16 if (bwd16 and x16 is not None) else x, "wk": wk, "wt": wt, "y": y,
                     "z": (z[0] if dual else z) if has_res else None, "zbits": zbits,
                     "scale": scale, "shift": shift, "mean": mean, "inv": inv,
                     "stride": stride, "pad": pad, "relu": relu, "conv": conv, "bn": bn,
                     "c_real": c, "math": "bf16" if bwd16 else math, "groups": groups,
                     "res": has_res, "dy16": bwd16, "fold": bool(frozen is not None and fold)})
    if defer:
        return y, scale, shift
    return (z, z16) if bwd16 else z


def _conv_bn_bwd(rec, dz, grads, want_dres=False, dx_out=None, dx_beta=0.0, need_dx=True,
                 dres_inplace=False, parts=None, fuse_prev=None, pool=None, dy=None, g16=False,
                 r16=False, fold=False, gcoef=None):
    """BN backward, wgrad, dgrad (optionally accumulated into dx_out) of one conv+BN unit.

    parts: dz was produced by a fused dgrad (conv_dgrad_bnbwd): it is already ReLU-masked and
    `parts` holds its BN-backward partial sums.  Otherwise the ReLU mask comes from the saved z,
    or is recomputed from y when there was no residual.  dres_inplace: the pre-activation
    gradient (the identity branch's) overwrites dz and is returned as dres.
    fuse_prev: the unit whose BN output gradient this unit's dgrad produces -- its mask and
    partial sums are then computed in the dgrad epilogue; returned as the third value.
    pool: (pooled gradient, argmax) of the maxpool that consumed this unit's output (the stem);
    dz is then gathered from it inside the BN backward.
    dy: the conv's output gradient computed by the caller (ResNeSt's split-attention backward
    writes the grouped conv's dy with bn0's backward folded in): only wgrad and dgrad run here.
    g16: the fused dgrad may store fuse_prev's masked gradient as bf16 (TMR_IO_G16) when that unit
    has no residual and the dgrad runs on the bf16 LDS-DMA engine (the bf16-activation step).
    r16: the same for fuse_prev a block output (R16): the dgrad adds into dx_out (bf16 in place,
    or fp32 read and a new bf16 tensor returned).
    fold: with parts, the fp32 wgrad may produce dy itself (WGRAD_BNBWD) where the library serves
    the unit; the ResNet-50 trunk's units only (records of math "fp32": not the BWD16 step's).
    gcoef: (g, coef) in place of dy -- the caller ran the BN backward's reductions
    (ops.bn_bwd_parts_ds_coef) and the fused wgrad produces dy from the masked gradient g, this
    unit's y and its coefficients; only wgrad and dgrad run here."""
    conv, bn = rec["conv"], rec["bn"]
    # dy feeds only this conv's dgrad / wgrad (the BWD16 step's records always store it bf16)
    s16 = rec.get("dy16", False) or _store16(rec["math"])
    dy_given = dy is not None or gcoef is not None
    dw = None
    kr, ks = conv.weight.shape[2:]
    if gcoef is not None:
        dw, dy = ops.conv_wgrad_bnbwd(rec["x"], gcoef[0], rec["y"], gcoef[1], kr, ks, rec["stride"],
                                      rec["pad"], c_real=rec["c_real"])
        dres = None
    elif dy_given:
        dres = None
    elif pool is not None:
        # the stem: maxpool backward + ReLU mask + BN backward without writing dz
        dy, dg, db = ops.bn_bwd_maxpool(pool[0], pool[1], rec["y"], rec["scale"], rec["shift"],
                                        rec["mean"], rec["inv"], bn.weight.detach(), bf16=s16)
        dres = None
    elif (parts is not None and fold and WGRAD_BNBWD and rec["math"] == "fp32"
          and rec.get("groups", 1) == 1
          and ops.conv_wgrad_bnbwd_ok(rec["x"], dz, rec["y"], kr, ks, rec["stride"], rec["pad"])):
        coef, dg, db = ops.bn_bwd_parts_coef(rec["y"], parts[0], parts[1], rec["mean"],
                                             rec["inv"], bn.weight.detach())
        dw, dy = ops.conv_wgrad_bnbwd(rec["x"], dz, rec["y"], coef, kr, ks, rec["stride"],
                                      rec["pad"], c_real=rec["c_real"])
        dres = dz if want_dres else None
    elif parts is not None:
        dy, dg, db = ops.bn_bwd_parts(dz, rec["y"], parts[0], parts[1], rec["mean"], rec["inv"],
                                      bn.weight.detach(), bf16=s16)
        dres = dz if want_dres else None
    else:
        dy, dres, dg, db = ops.bn_bwd(dz, rec["y"], rec["z"], rec["mean"], rec["inv"],
                                      bn.weight.detach(), rec["relu"], want_dres=want_dres,
                                      dres_out=dz if dres_inplace else None,
                                      scale=rec["scale"], shift=rec["shift"], bf16=s16)
    if not dy_given:
        grads[bn.weight] = dg
        grads[bn.bias] = db
    x = rec["x"]
    k, c, r, s = conv.weight.shape
    grp = rec.get("groups", 1)
    grads[conv.weight] = dw if dw is not None else ops.conv_wgrad(
        x, dy, r, s, rec["stride"], rec["pad"], c_real=rec["c_real"], math=rec["math"],
        groups=grp)
    dx, fused = None, None
    if need_dx:
        hw = (x.shape[1], x.shape[2])
        wt = rec.get("wt") is not None
        wdg = rec["wt"] if wt else rec["wk"]
        if fuse_prev is not None:
            p = fuse_prev
            mask = (1 if p.get("res", p["z"] is not None) else 2) if p["relu"] else 0
            zm = p["z"]
            if mask == 1 and wt and p.get("zbits") is not None:
                mask, zm = 3, p["zbits"]   # the ReLU mask as bits (LDS-DMA dgrad)
            elif mask == 1 and zm is None:   # (the BWD16 step keeps only the bits)
                raise RuntimeError("a residual unit's ReLU mask needs its saved z or its bits on "
                                   "the LDS-DMA dgrad")
            bf8 = (wt and p["y"].dtype == torch.bfloat16 and
                   (p["y"].shape[-1] // grp) % 8 == 0)
            # (a grouped dgrad -- ResNeSt's radix-2 conv -- stores its per-group channel slices bf16
            # too; the residual accumulation stays ungrouped)
            gb = (g16 and G16 and mask == 2 and dx_out is None and dx_beta == 0.0 and bf8)
            rb = (r16 and R16 and mask in (1, 3) and dx_out is not None and dx_beta == 1.0 and bf8
                  and grp == 1)
            old = None
            if rb and dx_out.dtype != torch.bfloat16:   # fp32 old dx -> a new bf16 dx
                old, dx_out = dx_out, None
            dx, pp, npp = ops.conv_dgrad_bnbwd(dy, wdg, hw, rec["stride"], rec["pad"],
                                               p["y"], p["mean"], mask, z=zm,
                                               scale=p["scale"], shift=p["shift"], out=dx_out,
                                               beta=dx_beta, math=rec["math"],
                                               wt=wt, groups=grp, g16=gb or rb, old=old)
            fused = (pp, npp)
        else:
            dx = ops.conv_dgrad(dy, wdg, hw, rec["stride"], rec["pad"], out=dx_out,
                                beta=dx_beta, math=rec["math"], wt=wt, groups=grp)
    return dx, dres, fused


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
    """The frozen-BN train step applies: bn_frozen on a train-mode fp32 ResNet-50 share."""
    return bool(getattr(share, "bn_frozen", False) and share.training
                and share.precision == "fp32")


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
    if parts is not None and _bn_wants_grad(rec["bn"]):
        grads[rec["bn"].weight], grads[rec["bn"].bias] = ops.bn_frozen_finalize(
            parts[0], parts[1], rec["inv"])


def _frozen_unit_bwd(rec, g, grads, dy=None, parts=None, **kw):
    """wgrad and dgrad of one frozen-BN unit.  dy: its real output gradient g*scale (a unit of the
    single-pass kernels).  Otherwise g is the masked gradient from a fused dgrad (`parts` its
    partial sums -> the BN gradients): the wgrad runs on g and dW's rows take scale[k], the dgrad
    reads the pre-scaled CRSK weights (rec["fold"]) -- no elementwise pass forms dy."""
    _frozen_affine(rec, parts, grads)
    if dy is not None:
        if rec["fold"]:
            raise RuntimeError("frozen BN: a real dy meets pre-scaled dgrad weights")
        return _conv_bn_bwd(rec, None, grads, dy=dy, **kw)
    if not rec["fold"] and kw.get("need_dx", True):
        raise RuntimeError("frozen BN: a folded unit needs its pre-scaled dgrad weights")
    out = _conv_bn_bwd(rec, None, grads, dy=g, **kw)
    ops.scale_rows(grads[rec["conv"].weight], rec["scale"])
    return out


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
        with ops.layout_session(share, key + ("frozen",) if fz is not None else key):
            return TrunkFn._forward(ctx, x4, share, keep, params, fz)

    @staticmethod
    def _forward(ctx, x4, share, keep, params, fz=None):
        training = share.training
        keep = keep and training
        recs = [] if keep else None
        nbt = []   # BatchNorm num_batches_tracked counters, incremented together at the end
        conv1, bn1, layers = share.trunk_parts()
        mt = _fwd_math(share.precision)
        # the BWD16 step: the fp32 forward plus the bf16 copies its bf16-math backward reads
        # (without a backward to record -- eval, no grad -- it is the fp32 path itself)
        bw = bool(keep and share.precision == BWD16)
        a16 = training and _act16(mt)            # every activation bf16: no fp32 copies
        f16 = training and _full16(mt) and not a16
        # eval mode, opt-in (share.infer_act16): every stored activation bf16, rounded once after
        # BN (+residual) (+ReLU) by the conv's epilogue; the block output is the next block's
        # operand and identity
        i16 = _infer16(share)
        if training:
            # bf16 activations: the stem reads an NHWC8 bf16 copy of its input (8-channel
            # pieces: the LDS-DMA engine; exact, the bf16 math rounds x anyway)
            xs = ops.nhwc4_to_bf16x8(x4) if (a16 and ops.engine_forced()) else x4
            # share.bn1 + relu applied inside the maxpool (the backward recomputes the ReLU
            # mask from y, so the stem's BN output is never needed)
            y0, sc0, sh0 = _conv_bn(xs, conv1, bn1, 2, 3, True, training, recs=recs, math=mt,
                                    defer=True, nbt=nbt, bwd16=bw,
                                    frozen=fz[bn1] if fz is not None else None)
            if bw:
                p, h16, am = ops.maxpool_fwd_bn_dual(y0, sc0, sh0)
            else:
                p, am = ops.maxpool_fwd_bn(y0, sc0, sh0, bf16=f16)
            stem_hw = (y0.shape[1], y0.shape[2])
        elif i16:
            # bf16-activation inference: the stem reads the NHWC8 bf16 copy of its input on the
            # LDS-DMA engine; its bf16 output is already >= 0, so the bf16 maxpool with an
            # identity BatchNorm is exact
            z = _conv_bn(ops.nhwc4_to_bf16x8(x4), conv1, bn1, 2, 3, True, training, math=mt,
                         y16=True)
            p, am = ops.maxpool_fwd_bn(z, torch.ones_like(bn1.running_mean),
                                       torch.zeros_like(bn1.running_mean))
            stem_hw = (z.shape[1], z.shape[2])
        else:
            z = _conv_bn(x4, conv1, bn1, 2, 3, True, training, recs=recs, math=mt, nbt=nbt)
            p, am = ops.maxpool_fwd(z)
            stem_hw = (z.shape[1], z.shape[2])
        # h: the block input as the identity residual (fp32), hx: as the conv operand (the bf16
        # copy under f16; the maxpool output is only ever a conv operand)
        h, hx = (None, p) if f16 else (p, p)
        if not bw:
            h16 = None   # (bw: the bf16 copy of the block input, the wgrads' operand)
        z1h = z2h = None
        blocks = []
        last = layers[-1][-1]

        def fzk(bn, blk=None):
            # the frozen step's coefficients; every unit but the last block's bn3 / downsample BN
            # (whose g arrives unmasked) folds its dy scale into its dgrad weights
            if fz is None:
                return {}
            return {"frozen": fz[bn], "fold": blk is not last}
        for layer in layers:
            for blk in layer:
                brec = [] if keep else None
                z1 = _conv_bn(hx, blk.conv1, blk.bn1, 1, 0, True, training, recs=brec, math=mt,
                              nbt=nbt, y16=i16, bwd16=bw, x16=h16, **fzk(blk.bn1))
                if bw:
                    z1, z1h = z1
                z2 = _conv_bn(z1, blk.conv2, blk.bn2, blk.stride, 1, True, training, recs=brec,
                              math=mt, nbt=nbt, y16=i16, bwd16=bw, x16=z1h, **fzk(blk.bn2))
                if bw:
                    z2, z2h = z2
                if blk.downsample is not None:
                    # train: the branch's BN is applied inside the BN3 pass (bn_apply2)
                    idn = _conv_bn(hx, blk.downsample[0], blk.downsample[1], blk.stride, 0, False,
                                   training, recs=brec, math=mt, defer=training, nbt=nbt,
                                   y16=i16, bwd16=bw, x16=h16, **fzk(blk.downsample[1], blk))
                else:
                    if h is None:
                        raise RuntimeError("identity residual of the stem output (no downsample)")
                    idn = h
                if isinstance(idn, tuple):
                    h = _conv_bn(z2, blk.conv3, blk.bn3, 1, 0, True, training, branch=idn,
                                 recs=brec, math=mt, nbt=nbt, dual=f16, bwd16=bw, x16=z2h,
                                 **fzk(blk.bn3, blk))
                else:
                    h = _conv_bn(z2, blk.conv3, blk.bn3, 1, 0, True, training, residual=idn,
                                 recs=brec, math=mt, nbt=nbt, dual=f16, y16=i16, bwd16=bw,
                                 x16=z2h, **fzk(blk.bn3, blk))
                if bw:
                    h, h16 = h
                    hx = h
                    if blocks:   # the previous block output's fp32 z: its mask is in the bits
                        blocks[-1][1][-1]["z"] = None
                    del z1, z2, idn   # (their fp32 z's were only this block's forward operands)
                else:
                    h, hx = h if f16 else (h, h)
                blocks.append((blk, brec))
        feat = ops.avgpool_fwd(h)
        if nbt:   # (none under frozen BN: no counter moves)
            ops.counters_add_one(nbt)
        ctx.keep = keep
        ctx.frozen = fz is not None
        if keep:
            ctx.share = share
            ctx.params = params
            ctx.stem = recs
            ctx.pool = (am, stem_hw)
            ctx.blocks = blocks
            ctx.last_hw = (h.shape[1], h.shape[2])
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        if not ctx.keep:
            raise RuntimeError("trunk backward needs train mode and a forward with grad enabled")
        if ctx.frozen:
            return TrunkFn._backward_frozen(ctx, dfeat)
        grads = {}
        g = ops.avgpool_bwd(dfeat.contiguous(), ctx.last_hw)   # grad at the last block output
        blocks = ctx.blocks
        pending = None     # BN-backward partials of g when the dgrad that produced it was fused
        ready = get_grad_ready(ctx.share)   # ddp.GradAllReduce.grads_ready, or None
        while blocks:
            blk, brec = blocks.pop()
            has_ds = blk.downsample is not None
            r1, r2 = brec[0], brec[1]
            rd = brec[2] if has_ds else None
            r3 = brec[-1]
            # the previous block's last unit: its BN output gradient is this block's dx
            prev3 = blocks[-1][1][-1] if blocks else None
            # g (owned here) becomes the masked pre-ReLU gradient = the identity-branch grad
            dyd = gcd = None
            if (has_ds and _ds_dual(g, r3, rd) and pending is not None):
                # (g came masked from the next block's fused dgrad)
                bargs = (g, r3["y"], pending[0], pending[1], r3["mean"], r3["inv"],
                         r3["bn"].weight.detach(), rd["y"], rd["mean"], rd["inv"],
                         rd["bn"].weight.detach())
                f3, fd = _ds_fold(g, r3, rd)
                gc3 = None
                if f3 or fd:
                    # the served units' wgrads produce their dy themselves (g outlives both: dres)
                    c3, dg3, db3, cd, dgd, dbd, dy3, dyd = ops.bn_bwd_parts_ds(
                        *bargs, fold3=f3, foldd=fd)
                    gc3 = (g, c3) if f3 else None
                    gcd = (g, cd) if fd else None
                else:
                    dy3, dg3, db3, dyd, dgd, dbd = ops.bn_bwd_parts_ds(
                        *bargs, dy16=_ds_dy16(r3, rd))
                grads[r3["bn"].weight], grads[r3["bn"].bias] = dg3, db3
                grads[rd["bn"].weight], grads[rd["bn"].bias] = dgd, dbd
                dz2, _, fz2 = _conv_bn_bwd(r3, None, grads, fuse_prev=r2, g16=True, dy=dy3, gcoef=gc3)
                dres = g
                del dy3, gc3
            else:
                dz2, dres, fz2 = _conv_bn_bwd(r3, g, grads, want_dres=True, dres_inplace=True,
                                              parts=pending, fuse_prev=r2, g16=True, fold=True)
            dz1, _, fz1 = _conv_bn_bwd(r2, dz2, grads, parts=fz2, fuse_prev=r1, g16=True,
                                      fold=True)
            del dz2
            if has_ds:
                # the strided downsample dgrad writes dx (its tap-less parity classes as zeros),
                # the stride-1 conv1 dgrad accumulates into it with the fused BN backward
                # (measured 51.1 vs 51.6 ms of dgrads per C2 step against the other order,
                # profiles/r3/bench_r4f/)
                if dyd is not None or gcd is not None:
                    dx, _, _ = _conv_bn_bwd(rd, None, grads, dy=dyd, gcoef=gcd)
                    del dyd, gcd
                else:
                    dx, _, _ = _conv_bn_bwd(rd, dres, grads)
                dx, _, pending = _conv_bn_bwd(r1, dz1, grads, parts=fz1, dx_out=dx, dx_beta=1.0,
                                              fuse_prev=prev3, r16=True, fold=True)
            else:
                dx, _, pending = _conv_bn_bwd(r1, dz1, grads, parts=fz1, dx_out=dres, dx_beta=1.0,
                                              fuse_prev=prev3, r16=True, fold=True)
            del dz1, brec, dres
            g = dx
            if ready is not None:   # this block's parameter grads are final: start their exchange
                ready([(p, grads[p]) for p in blk.parameters() if p in grads])
        dh = g
        am, stem_hw = ctx.pool
        _conv_bn_bwd(ctx.stem[0], None, grads, need_dx=False, pool=(dh, am))
        out = [grads.get(p) for p in ctx.params]
        ctx.blocks = ctx.stem = None
        return (None, None, None) + tuple(out)

    @staticmethod
    def _backward_frozen(ctx, dfeat):
        """The frozen-BN step's backward: no BN-backward projection anywhere.  The last block's
        bn3 (g unmasked from the avgpool) and the stem (g through the maxpool) take one pass of
        tmr_bn_frozen_bwd / _maxpool; every other unit's g comes masked, with its partial sums,
        from the fused dgrad that produced it, and its dy = g*scale lives in the conv operands
        (_frozen_unit_bwd).  A downsample BN needs sum g*(y_ds - mean_ds) of its own: one
        sums-only pass over (g, y_ds), skipped with affine=False."""
        grads = {}
        g = ops.avgpool_bwd(dfeat.contiguous(), ctx.last_hw)   # grad at the last block output
        blocks = ctx.blocks
        pending = None     # the fused dgrad's partial sums of g (None: g is unmasked)
        ready = get_grad_ready(ctx.share)   # ddp.GradAllReduce.grads_ready, or None
        while blocks:
            blk, brec = blocks.pop()
            has_ds = blk.downsample is not None
            r1, r2 = brec[0], brec[1]
            rd = brec[2] if has_ds else None
            r3 = brec[-1]
            prev3 = blocks[-1][1][-1] if blocks else None
            dy3 = dyd = None
            if pending is None:
                # g unmasked: mask (the block output's bits), dres in place, dy's and sums at once
                s3 = _bn_wants_grad(r3["bn"])
                mk = dict(mask=3, bits=r3["zbits"]) if r3.get("zbits") is not None else \
                    dict(mask=1, z=r3["z"])
                if has_ds:
                    sums = s3 or _bn_wants_grad(rd["bn"])
                    dy3, dyd, p3, pd, npp = ops.bn_frozen_bwd_ds(
                        g, r3["y"], r3["scale"], r3["shift"], r3["mean"], rd["y"], rd["scale"],
                        rd["mean"], dres_inplace=True, want_sums=sums, **mk)
                    _frozen_affine(r3, (p3, npp) if sums else None, grads)
                    _frozen_affine(rd, (pd, npp) if sums else None, grads)
                else:
                    dy3, p3, npp = ops.bn_frozen_bwd(g, r3["y"], r3["scale"], r3["shift"],
                                                     r3["mean"], dres_inplace=True, want_sums=s3,
                                                     **mk)
                    _frozen_affine(r3, (p3, npp) if s3 else None, grads)
                dz2, _, fz2 = _frozen_unit_bwd(r3, None, grads, dy=dy3, fuse_prev=r2)
                del dy3
            else:
                if has_ds and _bn_wants_grad(rd["bn"]):
                    _, pd, npp = ops.bn_frozen_bwd(g, rd["y"], rd["scale"], rd["shift"],
                                                   rd["mean"], mask=0, want_dy=False)
                    _frozen_affine(rd, (pd, npp), grads)
                dz2, _, fz2 = _frozen_unit_bwd(r3, g, grads, parts=pending, fuse_prev=r2)
            dres = g   # masked: the identity branch's gradient
            dz1, _, fz1 = _frozen_unit_bwd(r2, dz2, grads, parts=fz2, fuse_prev=r1)
            del dz2
            if has_ds:
                dx, _, _ = _frozen_unit_bwd(rd, dres, grads, dy=dyd)
                del dyd
                dx, _, pending = _frozen_unit_bwd(r1, dz1, grads, parts=fz1, dx_out=dx,
                                                  dx_beta=1.0, fuse_prev=prev3)
            else:
                dx, _, pending = _frozen_unit_bwd(r1, dz1, grads, parts=fz1, dx_out=dres,
                                                  dx_beta=1.0, fuse_prev=prev3)
            del dz1, brec, dres
            g = dx
            if ready is not None:   # this block's parameter grads are final: start their exchange
                ready([(p, grads[p]) for p in blk.parameters() if p in grads])
        am, stem_hw = ctx.pool
        st = ctx.stem[0]
        ss = _bn_wants_grad(st["bn"])
        dy0, p0, np0 = ops.bn_frozen_bwd_maxpool(g, am, st["y"], st["scale"], st["shift"],
                                                 st["mean"], want_sums=ss)
        _frozen_affine(st, (p0, np0) if ss else None, grads)
        _frozen_unit_bwd(st, None, grads, dy=dy0, need_dx=False)
        out = [grads.get(p) for p in ctx.params]
        ctx.blocks = ctx.stem = None
        return (None, None, None) + tuple(out)


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
        # eval mode under precision "bf16", opt-in: bf16 activations (TrunkFn._forward i16; the
        # default keeps every eval path's fp32 activations and bits)
        self.infer_act16 = False
        # frozen BatchNorm (tmrnet_amd.freeze_bn): the BN modules stay in eval mode whatever
        # train(mode) says, and a train-mode step runs on the running statistics
        self.bn_frozen = False
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


def freeze_bn(model_or_share, affine=True):
    """Freeze the trunk's BatchNorm: every BatchNorm2d of the share goes to eval mode and stays
    there through train() / eval() (share.bn_frozen = True); a train-mode step then normalises
    with the running statistics, writes none of them, and back-propagates dy = g*scale.
    affine=False also stops training the BN weights and biases (requires_grad=False;
    torchvision's FrozenBatchNorm2d).  ResNet-50 shares of precision "fp32" only.  Call it after
    load_checkpoint and before the optimizer is built.  Returns its argument."""
    from .resnest import ResNeSt50Share
    share = _share_of(model_or_share)
    if isinstance(share, ResNeSt50Share):
        raise ValueError("freeze_bn: frozen BatchNorm exists for the ResNet-50 trunk "
                         "(precision 'fp32') only, not for a ResNeSt-50 share")
    if share.precision != "fp32":
        raise ValueError("freeze_bn: frozen BatchNorm exists for precision 'fp32' only, not for "
                         "%r" % (share.precision,))
    share.bn_frozen = True
    for m in _share_bns(share):
        m.training = False
        if not affine:
            m.weight.requires_grad_(False)
            m.bias.requires_grad_(False)
    return model_or_share


def unfreeze_bn(model_or_share):
    """Undo freeze_bn: clear share.bn_frozen, put the BatchNorm modules back to share.training
    and their weights and biases back to requires_grad=True.  Returns its argument."""
    share = _share_of(model_or_share)
    share.bn_frozen = False
    for m in _share_bns(share):
        m.training = share.training
        m.weight.requires_grad_(True)
        m.bias.requires_grad_(True)
    return model_or_share
