"""The fp32-forward / bf16-backward train step (precision "bf16-bwd", tmrnet_amd/trunk.py BWD16) on
the device.

Elementwise passes (bn.hip, pool_layout.hip): each new entry point against the entry points it
fuses -- z, bits, argmax and the fp32 BN gradients bit for bit, every bf16 copy the RNE of the fp32
value -- and, on operands of the 2^-6 grid of tests/_bwd16.py (exact in fp32, 1/16 of the
pre-activations exactly 0), against the numpy emulation.  Outputs sit between sentinels and start
as NaN / -1.  Operands 8 bytes off a 16-B boundary are refused with a message (the new forms) or
served by the 4-wide kernel (tmr_bn_apply_dual).

The step: at 2 frames the train-mode forward (logits, loss, running statistics) and the eval-mode
logits are the "fp32" model's bit for bit; the gradients are held to the float64 emulation
(oracle.emulate_bf16_convs(activations=False, grads=False, ops=("dy", "bx", "bw"))) by the
project's criterion (tests/test_model_parity_gpu._assert_vs_fp64).  At 4 x 10 frames the gradient
ensemble statistics against the "fp32" step match the committed fixture's `bwd_ops` variant
(tests/golden/bf16_ensemble_r50.json), and 10 SGD steps track the "fp32" step's losses."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import tmrnet_amd
from tmrnet_amd import ops
from tmrnet_amd._lib import call, query, stream_ptr
from oracle import tmrnet_ref as ref
from tests import _bwd16 as H
from tests import _bf16_ensemble as E
from tests.test_head_gpu import poison  # noqa: F401
from tests.test_stem_pool8_gpu import _off8
from tests.test_bf16_ensemble_gpu import OUT   # the suite's directory of measured records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
NAN = float("nan")
SENT = 12345
GUARD = 8          # elements of sentinel on both sides: 16 B of bf16, 32 B of fp32 / int32


def guarded(shape, dev, dtype=f32):
    """(buffer, view): `view` (contiguous, `shape`, 16-B aligned) holds NaN (floats) or -1 and
    sits between sentinels"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=dev)
    view = buf[GUARD:GUARD + n].view(shape)
    view.fill_(NAN if dtype.is_floating_point else -1)
    assert view.data_ptr() % 16 == 0
    return buf, view


def guards_ok(buf):
    s = torch.full((1,), SENT, dtype=buf.dtype, device=buf.device)
    return bool((buf[:GUARD] == s).all() and (buf[-GUARD:] == s).all())


def bits16(t):
    """bf16 tensor -> numpy uint16 bit patterns"""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def words(t):
    return t.cpu().numpy().view(np.uint32)


def up(a, dev):
    return None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dev)


# ------------------------------------------------------------------ 5. the new applies
APPLY_SHAPES = [(1, 8), (33, 24), (1025, 64), (98, 2048)]   # 33 * 24: a partial last bits word


def _fused(k, d):
    """z, bits of the entry point the dual form fuses (tmr_bn_apply_bits / tmr_bn_apply2_bits)"""
    if d["yr"] is not None:
        return ops.bn_apply2_bits(d["y"], d["scale"], d["shift"], d["yr"], d["rscale"], d["rshift"])
    return ops.bn_apply_bits(d["y"], d["scale"], d["shift"], d["res"])


def _dual(d, z, z16, bits):
    rows, c = d["y"].shape
    if d["yr"] is not None:
        call("tmr_bn_apply2_bits_dual", d["y"], d["scale"], d["shift"], d["yr"], d["rscale"],
             d["rshift"], z, z16, bits, rows, c, stream_ptr())
    else:
        call("tmr_bn_apply_bits_dual", d["y"], d["scale"], d["shift"], d["res"], z, z16, bits,
             rows, c, stream_ptr())


@pytest.mark.parametrize("form", ["plain", "res", "apply2"])
@pytest.mark.parametrize("rows,c", APPLY_SHAPES)
def test_apply_bits_dual(dev, poison, rows, c, form):
    k = H.grid_case(rows, c, rows * 5 + c, form)
    emu = H.emu_apply(k)
    d = {n: up(k[n], dev) for n in ("y", "scale", "shift", "res", "yr", "rscale", "rshift")}
    rz, rbits = _fused(k, d)
    zb, z = guarded((rows, c), dev)
    hb, z16 = guarded((rows, c), dev, BF16)
    bb, bits = guarded(((rows * c + 31) // 32,), dev, I32)
    _dual(d, z, z16, bits)
    torch.cuda.synchronize()
    assert guards_ok(zb) and guards_ok(hb) and guards_ok(bb)
    assert torch.equal(z, rz) and torch.equal(bits, rbits) and torch.equal(z16, z.to(BF16))
    bad = H.compare_apply(z.cpu().numpy(), words(bits), bits16(z16), ref_z=rz.cpu().numpy(),
                          ref_bits=words(rbits), emu=emu)
    assert not bad, bad
    # the wrapper the trunk calls (its outputs handed out as NaN / -1 by `poison`)
    if form == "apply2":
        wz, wbits, w16 = ops.bn_apply2_bits_dual(d["y"], d["scale"], d["shift"], d["yr"],
                                                 d["rscale"], d["rshift"])
    else:
        wz, wbits, w16 = ops.bn_apply_bits_dual(d["y"], d["scale"], d["shift"], d["res"])
    assert torch.equal(wz, rz) and torch.equal(wbits, rbits) and torch.equal(w16, rz.to(BF16))


@pytest.mark.parametrize("form", ["res", "apply2"])
def test_apply_bits_dual_refuses_misaligned(dev, form):
    """Operands 8 bytes off a 16-B boundary, and channel counts that are no multiple of 8: refused
    with a message before any launch."""
    rows, c = 33, 24
    k = H.grid_case(rows, c, 7, form)
    d = {n: up(k[n], dev) for n in ("y", "scale", "shift", "res", "yr", "rscale", "rshift")}
    z = torch.empty(rows, c, device=dev)
    z16 = torch.empty(rows, c, device=dev, dtype=BF16)
    bits = ops.relu_bits_empty(z)
    other = "yr" if form == "apply2" else "res"
    for name in ("y", other, "z", "z16"):
        dd = dict(d)
        zz, hh = z, z16
        if name == "z":
            zz = _off8(z)
        elif name == "z16":
            hh = torch.empty(rows * c + 8, device=dev, dtype=BF16)[4:4 + rows * c].view(rows, c)
            assert hh.data_ptr() % 16 == 8
        else:
            dd[name] = _off8(d[name])
        with pytest.raises(RuntimeError, match="16-B aligned"):
            _dual(dd, zz, hh, bits)
    d12 = {n: (v[:, :12].contiguous() if v is not None and v.dim() == 2 else
               (v[:12].contiguous() if v is not None else None)) for n, v in d.items()}
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _dual(d12, z[:, :12].contiguous(), z16[:, :12].contiguous(), bits)


def test_apply_bits_dual_second_grid_trip(dev):
    """(16400, 2048): past the first trip of the grid-stride loop (8192 blocks x 256 threads x 2
    groups of 8 elements), against the fused entry point; operands made on the device."""
    rows, c = 16400, 2048
    g = torch.Generator(device=dev).manual_seed(5)
    ri = lambda lo, hi, shape, q: torch.randint(lo, hi, shape, generator=g, device=dev).float() / q
    y, res = ri(-256, 257, (rows, c), 64), ri(-256, 257, (rows, c), 64)
    scale, y0 = ri(8, 25, (c,), 16), ri(-1, 2, (c,), 4)
    shift = -y0 * scale
    plant = torch.rand(rows, c, generator=g, device=dev) < 1.0 / 16
    y = torch.where(plant, y0.expand(rows, c), y)
    res = torch.where(plant, torch.zeros_like(res), res)
    rz, rbits = ops.bn_apply_bits(y, scale, shift, res)
    del plant
    z, bits, z16 = ops.bn_apply_bits_dual(y, scale, shift, res)
    assert torch.equal(z, rz) and torch.equal(bits, rbits)
    assert torch.equal(z16, rz.to(BF16))
    assert int((rz == 0).sum()) >= rows * c // 16


@pytest.mark.parametrize("off", [False, True], ids=["aligned", "off8"])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("form", ["plain", "res"])
@pytest.mark.parametrize("rows,c", [(33, 24), (1025, 64), (77, 12)])
def test_apply_dual_8wide(dev, poison, rows, c, form, relu, off):
    """tmr_bn_apply_dual (the non-residual units' apply of the step): the 8-wide kernel (aligned,
    c % 8 == 0) and the 4-wide one (8 bytes off, c = 12) give tmr_bn_apply's z and its RNE."""
    k = H.grid_case(rows, c, rows + c, form)
    ez, _, e16 = H.emu_apply(k, relu=relu)
    y, sc, sh, res = (up(k[n], dev) for n in ("y", "scale", "shift", "res"))
    rz = ops.bn_apply(y, sc, sh, res, relu)
    if off:
        y, res = _off8(y), (None if res is None else _off8(res))
    z, z16 = ops.bn_apply_dual(y, sc, sh, res, relu)
    assert torch.equal(z, rz) and torch.equal(z16, rz.to(BF16))
    bad = H.compare_apply(z.cpu().numpy(), None, bits16(z16), ref_z=rz.cpu().numpy(),
                          emu=(ez, None, e16))
    assert not bad, bad


# ------------------------------------------------------------------ 6. the dual maxpool
@pytest.mark.parametrize("shape", [(2, 8, 8, 8), (1, 9, 7, 64)])
def test_maxpool_dual(dev, poison, shape):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(n + 3 * h + 5 * w + c)
    # a few levels (windows tie: the first maximum in scan order wins), bf16-exact
    y = (torch.randint(-6, 7, shape, generator=g).float() / 4).to(dev)
    scale = (torch.rand(c, generator=g) + 0.5).to(dev)
    shift = (torch.randn(c, generator=g) * 0.2).to(dev)
    rp, ram = ops.maxpool_fwd_bn(y, scale, shift)
    ho, wo = rp.shape[1:3]
    pb, p = guarded((n, ho, wo, c), dev)
    hb, p16 = guarded((n, ho, wo, c), dev, BF16)
    ab = torch.full((n * ho * wo * c + 32,), 77, dtype=torch.uint8, device=dev)
    am = ab[16:16 + n * ho * wo * c].view(n, ho, wo, c)
    am.fill_(255)
    call("tmr_maxpool2d_fwd_bn_dual", y, scale, shift, p, p16, am, n, h, w, c, ho, wo, stream_ptr())
    torch.cuda.synchronize()
    assert guards_ok(pb) and guards_ok(hb) and bool((ab[:16] == 77).all() and (ab[-16:] == 77).all())
    assert torch.equal(p, rp) and torch.equal(am, ram) and torch.equal(p16, rp.to(BF16))
    assert np.array_equal(bits16(p16), H.rne_bf16(rp.cpu().numpy()))
    wp, w16, wam = ops.maxpool_fwd_bn_dual(y, scale, shift)
    assert torch.equal(wp, rp) and torch.equal(wam, ram) and torch.equal(w16, rp.to(BF16))
    with pytest.raises(RuntimeError, match="16-B aligned"):
        ops.maxpool_fwd_bn_dual(_off8(y), scale, shift)
    with pytest.raises(RuntimeError, match="power of two"):
        ops.maxpool_fwd_bn_dual(torch.zeros(1, 4, 4, 24, device=dev), torch.ones(24, device=dev),
                                torch.zeros(24, device=dev))


# ------------------------------------------------------------------ 7. mixed-dtype ds backward
@pytest.mark.parametrize("c", [8, 24, 256])
@pytest.mark.parametrize("rows", [1, 98, 1025])
def test_bwd_parts_ds_d16(dev, poison, rows, c):
    """tmr_bn_bwd_parts_ds_d16 (fp32 g, y, y_ds in, bf16 dy's out) on fabricated partials, as
    tests/test_bn_gpu.py makes them: the RNE of the fp32 call's dy's, its BN gradients bit for
    bit."""
    from tests.test_bn_gpu import _bwd_case, _parts_of
    k = _bwd_case(rows, c)
    nparts = min(rows, 7)
    parts, _, _ = _parts_of(k["dz"], k["y"], k["mean"], nparts, rows + c)
    f = lambda n: k[n].float().to(dev)
    args = (f("dz"), f("y"), parts.to(dev), nparts, f("mean"), f("inv"), f("gamma"), f("yd"),
            f("mean_d"), f("inv_d"), f("gamma_d"))
    o32 = ops.bn_bwd_parts_ds(*args)
    gq, yq, pq, _, md, iv, gm, ydq, mdd, ivd, gmd = args
    b3, dy = guarded((rows, c), dev, BF16)
    bd, dyd = guarded((rows, c), dev, BF16)
    grads = [torch.full((c,), NAN, device=dev) for _ in range(4)]
    nb = query("tmr_bn_bwd_parts_ds_ws_bytes", nparts, rows, c)
    ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=dev)
    call("tmr_bn_bwd_parts_ds_d16", gq, yq, pq, nparts, md, iv, gm, dy, grads[0], grads[1], ydq,
         mdd, ivd, gmd, dyd, grads[2], grads[3], rows, c, ws, ctypes.c_size_t(ws.numel() * 8),
         stream_ptr())
    torch.cuda.synchronize()
    assert guards_ok(b3) and guards_ok(bd)
    np32 = lambda t: t.cpu().numpy()
    bad = H.compare_ds(bits16(dy), bits16(dyd), [np32(t) for t in grads], np32(o32[0]),
                       np32(o32[3]), [np32(o32[i]) for i in (1, 2, 4, 5)])
    assert not bad, bad
    assert torch.equal(dy, o32[0].to(BF16)) and torch.equal(dyd, o32[3].to(BF16))
    w = ops.bn_bwd_parts_ds(*args, dy16=True)     # the wrapper the trunk calls
    assert w[0].dtype == BF16 and torch.equal(w[0], dy) and torch.equal(w[3], dyd)
    for i, t in zip((1, 2, 4, 5), grads):
        assert torch.equal(w[i], t)
    if rows == 98 and c == 24:
        with pytest.raises(RuntimeError, match="16-B aligned"):
            ops.bn_bwd_parts_ds(_off8(args[0]), *args[1:], dy16=True)


# ------------------------------------------------------------------ 8. the step at 2 frames
def _hip_model(prec, sd, T, masks, dev, backbone="resnet50", time_conv=False):
    torch.manual_seed(0)
    m = tmrnet_amd.resnet_lstm(seq_len=T, precision=prec, backbone=backbone,
                               time_conv=time_conv).to(dev)
    m.load_state_dict(sd)
    m.train()
    m.nl_block.forced_mask = masks["nl"].to(dev)
    m.forced_head_mask = masks["head"].to(dev)
    return m


def _grads(mod):
    return {n: p.grad for n, p in mod.named_parameters()}


def test_step_two_frames(dev, monkeypatch):
    from tests.test_geometry_gpu import _head_act_spy, _trunk_out_spy
    from tests.test_model_parity_gpu import _assert_vs_fp64
    B, T, L = H.STEP["B"], H.STEP["T"], H.STEP["L"]
    r, x, lt, labels, masks = H.step_case()
    sd = {k: v.detach().clone() for k, v in r.state_dict().items()}
    x4 = E.to_nhwc4(x.view(-1, 3, 224, 224)).to(dev)
    lt_d, lab_d = lt.to(dev), labels.to(dev)
    crit = tmrnet_amd.CrossEntropyLoss(size_average=False)

    m32 = _hip_model("fp32", sd, T, masks, dev)
    out32 = m32(x4, lt_d)
    loss32 = crit(out32, lab_d)
    loss32.backward()

    # the bf16-bwd step, instrumented: the conv launches of its backward and their operand dtypes
    m = _hip_model("bf16-bwd", sd, T, masks, dev)
    acts, feats = _head_act_spy(monkeypatch), _trunk_out_spy(monkeypatch)
    seen = []
    for name in ("conv_wgrad", "conv_dgrad", "conv_dgrad_bnbwd"):
        orig = getattr(ops, name)

        def spy(a, b, *args, _orig=orig, _name=name, **kw):
            # (x, dy) of a wgrad; (dy, w) of a dgrad
            seen.append((_name, a.dtype, b.dtype, tuple(a.shape), kw.get("math", "fp32")))
            return _orig(a, b, *args, **kw)
        monkeypatch.setattr(ops, name, spy)
    folds = query("tmr_wgrad_bnbwd_launches")
    out = m(x4, lt_d)
    head_act = (acts[-1] > 0).float().cpu()                       # the step's own active sets
    zlast = (feats[-1].float() > 0).permute(0, 3, 1, 2).cpu()
    loss = crit(out, lab_d)
    monkeypatch.setattr(ops, "PROF", [])
    loss.backward()
    torch.cuda.synchronize()
    prof = ops.PROF
    monkeypatch.setattr(ops, "PROF", None)
    assert query("tmr_wgrad_bnbwd_launches") == folds      # no fp32 wgrad fold in this step

    # the forward is the fp32 step's, bit for bit
    assert torch.equal(out, out32) and torch.equal(loss, loss32)
    b32 = dict(m32.named_buffers())
    for n, b in m.named_buffers():
        assert torch.equal(b, b32[n]), n
    assert int(m.share.bn1.num_batches_tracked) == 1

    # every trunk conv of the backward ran in bf16 math on a bf16 dy; the wgrads on a bf16 x (the
    # stem's x is the fp32 NHWC4 input itself, rounded on load by the direct bf16 stem wgrad)
    kinds = [p[0] for p in prof if p[0].startswith(("conv_dgrad", "conv_wgrad"))]
    assert kinds.count("conv_wgrad_bf16") == 53 and kinds.count("conv_dgrad_bf16") == 52
    assert len(kinds) == 105
    wg = [s for s in seen if s[0] == "conv_wgrad"]
    dg = [s for s in seen if s[0] != "conv_wgrad"]
    assert len(wg) == 53 and len(dg) == 52
    for _, xdt, dydt, xshape, math in wg:
        assert math == "bf16" and dydt == BF16
        assert xdt == (f32 if xshape[-1] == 4 else BF16), xshape
    for _, dydt, wdt, _, math in dg:
        assert math == "bf16" and dydt == BF16 and wdt == BF16

    # eval mode: the fp32 path bit for bit
    m.eval(), m32.eval()
    with torch.no_grad():
        assert torch.equal(m(x4, lt_d), m32(x4, lt_d))

    # gradients against the float64 emulation, scaled by the fp32 emulation's own distance from
    # it; the HIP step's head and last-block active sets forced on the oracles
    masks = dict(masks)
    masks["head_act"] = head_act
    runs = {}
    for key, dt, emu in (("e64", torch.float64, True), ("e32", f32, True), ("f32", f32, False)):
        o = H.oracle_copy(r, dt, bwd_ops=emu)
        o.share.layer4[-1].forced_act = zlast.to(dt)
        runs[key] = H.oracle_step(o, x, lt, labels, masks)
    assert torch.equal(runs["e32"][0], runs["f32"][0])           # the emulation keeps the forward
    gm, g32 = _grads(m), _grads(m32)
    rel_dev = H.group_rel(gm, g32)
    rel_cpu = H.group_rel(runs["e32"][2], runs["f32"][2])
    rec = {"rel_dev": rel_dev, "rel_cpu": rel_cpu,
           "ratio": {g: rel_dev[g] / rel_cpu[g] for g in rel_dev}}
    print("bwd16 step, |g_bf16-bwd - g_fp32| / |g_fp32| per trunk group:", json.dumps(rec))
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "bwd16_step.json"), "w") as f:
        json.dump(rec, f, indent=1)
    _assert_vs_fp64(gm, runs["e32"][2], runs["e64"][2], "bwd16_grads")
    for g in H.TRUNK_GROUPS:
        assert rel_dev[g] <= 1.5 * rel_cpu[g], rec
    # outside the trunk the gradient never passes a trunk conv's backward: the fp32 step's bits
    for n, t in gm.items():
        if not n.startswith("share."):
            assert torch.equal(t, g32[n]), n


# ------------------------------------------------------------------ 9. the ensemble
# |HIP - emulation| of ratio and proj per group.  The bound the emulation's 1.00 called for was
# tests/test_bf16_ensemble_gpu.py's ENS_TOL["clip"] = 0.03; the worst measured gap was 1.74e-4
# (layer1's proj, profiles/bwd16/bwd16_ensemble_r50.json) -- below 0.015, so the bound is twice
# the measurement.
ENS_TOL = 3.5e-4
LOSS_TOL = 1e-5        # tests/test_bf16_ensemble_gpu.py LOSS_TOL["fp32"]


def _r50_case(dev):
    geo = "r50"
    with open(os.path.join(ROOT, "tests", "golden", "bf16_ensemble_%s.json" % geo)) as f:
        meta = json.load(f)
    sd = E.weights(geo)
    x, lt, labels, masks = E.inputs(geo)
    assert E.digest(x) == meta["x_digest"] and E.digest(lt) == meta["lt_digest"]
    assert E.digest(torch.cat([t.float().reshape(-1) for t in sd.values()
                               if t.is_floating_point()])) == meta["weights_digest"]
    return meta, sd, x, lt.to(dev), labels.to(dev), masks


def test_ensemble_r50_vs_fixture(dev):
    meta, sd, x, lt_d, lab_d, masks = _r50_case(dev)
    n, T = meta["n"], E.GEOS["r50"][3]
    crit = tmrnet_amd.CrossEntropyLoss(size_average=False)
    samples, losses = {}, {}
    for prec in ("fp32", "bf16-bwd"):
        m = _hip_model(prec, sd, T, masks, dev)
        samples[prec], losses[prec] = [], []
        for k in range(n):
            x4 = E.to_nhwc4(E.noisy(x, k)).to(dev)
            m.zero_grad(set_to_none=True)
            loss = crit(m(x4, lt_d), lab_d)
            loss.backward()
            losses[prec].append(float(loss.item()))
            samples[prec].append({g: t.float() for g, t in E.group_vectors(
                {nm: p.grad for nm, p in m.named_parameters() if p.grad is not None}).items()})
        del m
    torch.cuda.empty_cache()
    emu = meta["stats_vs_fp32"]["bwd_ops"]
    st, gaps = {}, {}
    for g in samples["fp32"][0]:
        mat = torch.stack([s[g] for s in samples["bf16-bwd"] + samples["fp32"]]).double()
        st[g] = E.stats((mat @ mat.T).numpy(), n)
        gaps[g] = {key: abs(st[g][key] - emu[g][key]) for key in ("ratio", "proj")}
    worst = max(v for d in gaps.values() for v in d.values())
    rec = {"losses": losses, "fixture_losses": meta["losses"]["bwd_ops"], "stats": st,
           "emulation": emu, "gaps": gaps, "worst_gap": worst, "tolerance": ENS_TOL}
    print("bwd16 ensemble r50: worst |HIP - emulation| over ratio / proj = %.3g" % worst)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "bwd16_ensemble_r50.json"), "w") as f:
        json.dump(rec, f, indent=1)
    # the forward is untouched: every sample's loss is the fp32 HIP sample's, and the fixture's
    assert losses["bf16-bwd"] == losses["fp32"]
    a, b = np.asarray(losses["bf16-bwd"]), np.asarray(meta["losses"]["bwd_ops"])
    assert (np.abs(a - b) <= LOSS_TOL * np.abs(b)).all(), (a.tolist(), b.tolist())
    bad = [(g, key, st[g][key], emu[g][key]) for g in gaps for key, v in gaps[g].items()
           if not v <= ENS_TOL]
    assert not bad, bad


# ------------------------------------------------------------------ 10. a short trajectory
def test_short_trajectory(dev):
    """10 SGD steps (the reference's parameter groups, lr 1e-4) on the ensemble's 40 frames,
    "bf16-bwd" beside "fp32": the loss gap stays within 0.05 x the initial loss at every step
    (DESIGN.md §2 item 4's bound) and both losses fall."""
    meta, sd, x, lt_d, lab_d, masks = _r50_case(dev)
    T = E.GEOS["r50"][3]
    x4 = E.to_nhwc4(x).to(dev)
    crit = tmrnet_amd.CrossEntropyLoss(size_average=False)
    lr = 1e-4
    traj = {}
    for prec in ("fp32", "bf16-bwd"):
        m = _hip_model(prec, sd, T, masks, dev)
        opt = tmrnet_amd.SGD(ref.sgd_param_groups(m, lr), lr=lr / 10, momentum=0.9,
                             weight_decay=5e-4)
        traj[prec] = []
        for _ in range(10):
            opt.zero_grad()
            loss = crit(m(x4, lt_d), lab_d)
            loss.backward()
            opt.step()
            traj[prec].append(float(loss.item()))
        del m, opt
    torch.cuda.empty_cache()
    a, b = np.asarray(traj["bf16-bwd"]), np.asarray(traj["fp32"])
    print("bwd16 trajectory:", json.dumps(traj))
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "bwd16_trajectory.json"), "w") as f:
        json.dump(traj, f, indent=1)
    assert a[0] == b[0]
    assert (np.abs(a - b) <= 0.05 * b[0]).all(), traj
    assert a[-1] < a[0] and b[-1] < b[0], traj
