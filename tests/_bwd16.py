"""Shared pieces of the tests of the fp32-forward / bf16-backward train step (precision
"bf16-bwd", tmrnet_amd/trunk.py BWD16): the ResNet-50 conv geometries, a numpy emulation of the
fused elementwise passes the step adds, and the comparison helpers the GPU tests assert with.
tests/test_bwd16_cpu.py shows on planted errors that the helpers can fail.

Emulated passes (numpy, no device):
  apply   z = relu(y * scale + shift (+ residual | + yr * rscale + rshift)), its ReLU-mask bits
          (element e = bit e % 32 of word e / 32, set where z > 0) and z16 = RNE_bf16(z)
          (tmr_bn_apply_bits_dual / tmr_bn_apply2_bits_dual; the non-residual tmr_bn_apply_dual
          without the bits)
  ds      the mixed-dtype downsample BN backward: dy16 = RNE_bf16(dy), dy_ds16 = RNE_bf16(dy_ds)
          of the fp32 call's dy's, its four BN gradients unchanged (tmr_bn_bwd_parts_ds_d16)

Operands of the apply cases lie on a 2^-6 grid (scale on 2^-4) so that every product and sum is
exact in fp32: a float64 evaluation, an fp32 fmaf and an fp32 multiply-add all give the same bits,
and 1/16 of the pre-activations are planted to be exactly 0 (the boundary of the mask: bit 0)."""
import numpy as np

# ---------------------------------------------------------------- ResNet-50 conv geometries
# name -> (h, w, c_in (stored), k, r, stride, pad) at 224x224 input; the stem's input is NHWC4
def resnet50_convs():
    out = [("stem", 224, 224, 4, 64, 7, 2, 3)]
    inpl, hw = 64, 56
    for li, (planes, blocks, stride) in enumerate(((64, 3, 1), (128, 4, 2), (256, 6, 2),
                                                   (512, 3, 2)), 1):
        for b in range(blocks):
            s = stride if b == 0 else 1
            pre = "layer%d.%d." % (li, b)
            out.append((pre + "conv1", hw, hw, inpl, planes, 1, 1, 0))
            out.append((pre + "conv2", hw, hw, planes, planes, 3, s, 1))
            if b == 0:
                out.append((pre + "downsample", hw, hw, inpl, planes * 4, 1, s, 0))
            hw //= s
            out.append((pre + "conv3", hw, hw, planes, planes * 4, 1, 1, 0))
            inpl = planes * 4
    return out


# ---------------------------------------------------------------- bf16 rounding / bits (numpy)
def rne_bf16(x):
    """fp32 array -> uint16 bf16 bit patterns, round to nearest, ties to even (finite values)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def trunc_bf16(x):
    """The wrong rounding (truncation) the planted-error test uses."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def pack_bits(mask):
    """bool array (flattened) -> uint32 words, element e = bit e % 32 of word e / 32."""
    m = np.asarray(mask, dtype=bool).reshape(-1)
    pad = (-m.size) % 32
    m = np.concatenate([m, np.zeros(pad, dtype=bool)]).reshape(-1, 32)
    return (m.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


# ---------------------------------------------------------------- the apply cases
def grid_case(rows, c, seed, form):
    """Operands of one apply case, float64 arrays that fp32 holds exactly.  form: "plain"
    (no residual), "res" (identity residual) or "apply2" (the deferred downsample BN).  1/16 of the
    elements are planted so that the pre-activation is exactly 0."""
    g = np.random.default_rng(seed)
    y = g.integers(-256, 257, (rows, c)) / 64.0
    scale = g.integers(8, 25, c) / 16.0
    y0 = g.integers(-1, 2, c) / 4.0
    shift = -y0 * scale
    plant = g.random((rows, c)) < 1.0 / 16
    y = np.where(plant, y0, y)
    k = dict(y=y, scale=scale, shift=shift, res=None, yr=None, rscale=None, rshift=None,
             plant=plant)
    if form == "res":
        k["res"] = np.where(plant, 0.0, g.integers(-256, 257, (rows, c)) / 64.0)
    elif form == "apply2":
        k["rscale"] = g.integers(8, 25, c) / 16.0
        r0 = g.integers(-1, 2, c) / 4.0
        k["rshift"] = -r0 * k["rscale"]
        k["yr"] = np.where(plant, r0, g.integers(-256, 257, (rows, c)) / 64.0)
    elif form != "plain":
        raise ValueError(form)
    return k


def emu_apply(k, relu=True):
    """-> (z fp32, bits uint32 words, z16 uint16 bit patterns) of one apply case."""
    v = k["y"] * k["scale"] + k["shift"]
    assert np.array_equal(v, v.astype(np.float32).astype(np.float64))   # the fmaf is exact
    if k["res"] is not None:
        v = v + k["res"]
    elif k["yr"] is not None:
        b = k["yr"] * k["rscale"] + k["rshift"]
        assert np.array_equal(b, b.astype(np.float32).astype(np.float64))
        v = v + b
    assert np.array_equal(v, v.astype(np.float32).astype(np.float64))
    assert (v[k["plant"]] == 0).all()
    z = (np.maximum(v, 0.0) if relu else v).astype(np.float32)
    return z, pack_bits(z > 0), rne_bf16(z)


def compare_apply(z, bits, z16, ref_z=None, ref_bits=None, emu=None):
    """The outputs of a bits+dual apply (numpy: z fp32, bits uint32 words or None, z16 uint16 bit
    patterns) against the entry point it fuses (ref_z / ref_bits) and / or the emulation's
    (z, bits, z16) -> list of what differs (empty: all equal).  z16 is always held to RNE(z)."""
    bad = []
    if np.isnan(z).any():
        bad.append("z has NaN")
    if ref_z is not None and not np.array_equal(z.view(np.uint32), ref_z.view(np.uint32)):
        bad.append("z != fused entry point's z")
    if ref_bits is not None and not np.array_equal(bits, ref_bits):
        bad.append("bits != fused entry point's bits")
    if not np.array_equal(z16, rne_bf16(z)):
        bad.append("z16 != RNE(z)")
    if bits is not None and not np.array_equal(bits, pack_bits(z > 0)):
        bad.append("bits != (z > 0)")
    if emu is not None:
        ez, eb, e16 = emu
        if not np.array_equal(z.view(np.uint32), ez.view(np.uint32)):
            bad.append("z != emulation")
        if bits is not None and not np.array_equal(bits, eb):
            bad.append("bits != emulation")
        if not np.array_equal(z16, e16):
            bad.append("z16 != emulation")
    return bad


# ---------------------------------------------------------------- the mixed-dtype ds backward
def emu_ds_d16(dy32, dyd32):
    """The bf16 dy's of tmr_bn_bwd_parts_ds_d16 from the fp32 call's -> (dy16, dy_ds16) bits."""
    return rne_bf16(dy32), rne_bf16(dyd32)


def compare_ds(dy16, dyd16, grads16, dy32, dyd32, grads32):
    """Mixed-dtype call (uint16 bit patterns, 4 fp32 BN gradients) against the fp32 call's
    outputs -> list of what differs."""
    bad = []
    e3, ed = emu_ds_d16(dy32, dyd32)
    if not np.array_equal(dy16, e3):
        bad.append("dy != RNE(fp32 dy)")
    if not np.array_equal(dyd16, ed):
        bad.append("dy_ds != RNE(fp32 dy_ds)")
    for name, a, b in zip(("dgamma", "dbeta", "dgamma_ds", "dbeta_ds"), grads16, grads32):
        if not np.array_equal(np.asarray(a, np.float32).view(np.uint32),
                              np.asarray(b, np.float32).view(np.uint32)):
            bad.append(name + " != fp32 call's")
    return bad


# ---------------------------------------------------------------- the 2-frame step
STEP = dict(B=1, T=2, L=3, weight_seed=41, input_seed=42)
TRUNK_GROUPS = ("stem", "layer1", "layer2", "layer3", "layer4")
BWD_OPS = ("dy", "bx", "bw")


def step_case():
    """The 2-frame step both sides run -> (oracle model fp32 in train mode, x (B, T, 3, 224, 224),
    lt (B, L, 512), labels (B,), masks): weights and inputs from seeds; all-ones dropout masks."""
    import torch
    from oracle import tmrnet_ref as ref
    B, T, L = STEP["B"], STEP["T"], STEP["L"]
    torch.manual_seed(STEP["weight_seed"])
    r = ref.TMRNetRef(seq_len=T).train()
    g = torch.Generator().manual_seed(STEP["input_seed"])
    frames = torch.randint(0, 256, (B * T, 250, 250, 3), generator=g, dtype=torch.uint8)
    off = torch.randint(0, 27, (B, 2), generator=g, dtype=torch.int32)
    lt = torch.rand(B, L, 512, generator=g) * 2 - 1
    labels = torch.randint(0, 7, (B,), generator=g)
    x = ref.crop_normalize_ref(frames, off, T).view(B, T, 3, 224, 224)
    masks = {"nl": torch.ones(B, 512), "head": torch.ones(B, 512)}
    return r, x, lt, labels, masks


def oracle_copy(r, dtype, bwd_ops=False):
    """A copy of the oracle model r (before any forward) in `dtype`, optionally with the three
    backward roundings of the step (emulate_bf16_convs(..., ops=BWD_OPS))."""
    import copy
    from oracle import tmrnet_ref as ref
    m = copy.deepcopy(r).to(dtype)
    if bwd_ops:
        ref.emulate_bf16_convs(m.share, activations=False, grads=False, ops=BWD_OPS)
    return m.train()


def oracle_step(m, x, lt, labels, masks):
    """forward + CE-sum backward of an oracle model -> (logits, loss, {name: grad})."""
    from oracle import tmrnet_ref as ref
    dt = next(m.parameters()).dtype
    out = m(x.to(dt), lt.to(dt), masks={k: v.to(dt) for k, v in masks.items()})
    loss = ref.ce_sum_ref(out, labels)
    loss.backward()
    return out.detach(), loss.detach(), {n: p.grad for n, p in m.named_parameters()}


def group_rel(ga, gb, groups=TRUNK_GROUPS):
    """{name: grad} x 2 -> {trunk group: |ga - gb| / |gb|} over the group's parameters (torch)."""
    import torch
    from tests._bf16_grads import group_of
    num, den = {}, {}
    for n, b in gb.items():
        g = group_of(n)
        if g not in groups:
            continue
        a = ga[n].detach().double().cpu()
        b = b.detach().double().cpu()
        num[g] = num.get(g, 0.0) + float(((a - b) ** 2).sum())
        den[g] = den.get(g, 0.0) + float((b ** 2).sum())
    return {g: (num[g] / max(den[g], 1e-300)) ** 0.5 for g in num}
