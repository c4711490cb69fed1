"""Frozen BatchNorm on the GPU: every tmr_bn_frozen_* entry point against float64 between
sentinels, and the frozen train step of the ResNet-50 trunk against the float64 oracle
(tests/_frozen_bn.py).

Exact case of the entry points: g and y lie on the 2^-4 grid with |v| <= 2, running_mean on it
with |v| <= 1, scale, shift / scale and inv are (signed) powers of two.  Every product is then a
multiple of 2^-8, |g * (y - mean)| <= 6 and every sum of <= 1025 rows stays below 2^13, so the fp32
result is exact whatever the summation order and is compared with `torch.equal`.
Random case: normal g, arbitrary scale / shift; y and running_mean are normal values rounded to
the 2^-10 grid so that y - mean is exact in fp32 and each term g * (y - mean) carries ONE rounding
-- the bound of the sums, rows * 2^-24 * sum |terms|, is the worst case of an fp32 summation of
`rows` once-rounded terms and would not cover a second rounding at rows = 1.  dy = g * scale is one
rounding of an exact product of two fp32 values: 2^-22 relative, as the issue sets it, is loose."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import tmrnet_amd
from tmrnet_amd import ops, _lib
from tmrnet_amd._lib import stream_ptr
from tests import _frozen_bn as F
from tests._frozen_bn import SENT, guarded, intact, _buffers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SZ = ctypes.c_size_t
ROWS, CS = (1, 98, 1025), (8, 24, 256)


# ---- helpers ----------------------------------------------------------------------------------
def grid(gen, shape, lim, step=16):
    return torch.randint(-lim * step, lim * step + 1, shape, generator=gen).float() / step


def pow2(gen, shape, lo, hi):
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
    return sign * torch.pow(2.0, torch.randint(lo, hi + 1, shape, generator=gen).float())


def make_data(rows, c, exact, seed):
    """g, y, yd, residual (rows, c); scale, shift, mean, scale_d, mean_d, inv (c,) on the CPU, and
    the rows where z == 0 was planted (residual cancellation; fmaf(y, scale, shift) == 0)."""
    gen = torch.Generator().manual_seed(seed)
    d = {}
    if exact:
        d["g"], d["y"], d["yd"] = (grid(gen, (rows, c), 2) for _ in range(3))
        d["mean"], d["mean_d"] = grid(gen, (c,), 1), grid(gen, (c,), 1)
        d["scale"], d["scale_d"] = pow2(gen, (c,), -2, 1), pow2(gen, (c,), -2, 1)
        s0 = grid(gen, (c,), 2)
        d["shift"] = d["scale"] * s0
        d["res"] = grid(gen, (rows, c), 2)
        d["inv"] = pow2(gen, (c,), -1, 2).abs()
        ch = torch.arange(c)
        r_fma, r_res = ch % rows, (ch + 1) % rows
        d["g"][r_fma, ch] = 1.0
        d["g"][r_res, ch] = -1.5
        d["y"][r_fma, ch] = -s0                          # fmaf(y, scale, shift) == 0
        pre = d["y"].double() * d["scale"].double() + d["shift"].double()
        d["res"][r_res, ch] = -pre[r_res, ch].float()    # ... + residual == 0
        d["planted"] = (r_fma, r_res, ch)
    else:
        d["g"] = torch.randn(rows, c, generator=gen)
        q = lambda t: torch.round(t * 1024) / 1024
        d["y"], d["yd"] = q(torch.randn(rows, c, generator=gen)), q(torch.randn(rows, c, generator=gen))
        d["mean"], d["mean_d"] = q(0.3 * torch.randn(c, generator=gen)), q(0.3 * torch.randn(c, generator=gen))
        d["scale"], d["scale_d"] = torch.randn(c, generator=gen) * 1.7, torch.randn(c, generator=gen) * 0.6
        d["shift"] = torch.randn(c, generator=gen)
        d["res"] = torch.randn(rows, c, generator=gen)
        d["inv"] = torch.ones(c)
        d["planted"] = None
    pre = d["y"].double() * d["scale"].double() + d["shift"].double()
    d["pre2"] = pre                                       # mask 2: the forward's fmaf, exactly
    d["z"] = (pre + d["res"].double()).clamp(min=0).float() if exact else \
        torch.relu(torch.addcmul(d["shift"], d["y"], d["scale"]) + d["res"])
    return d


def reference(d, mask, y="y", scale="scale", mean="mean"):
    g, yy = d["g"].double(), d[y].double()
    if mask == 0:
        on = torch.ones_like(g, dtype=torch.bool)
    elif mask == 2:
        on = d["pre2"] > 0
    else:
        on = d["z"] > 0
    gm = torch.where(on, g, torch.zeros_like(g))
    t = gm * (yy - d[mean].double())
    return {"gm": gm, "dy": gm * d[scale].double(), "s": gm.sum(0), "q": t.sum(0),
            "s_abs": gm.abs().sum(0), "q_abs": t.abs().sum(0)}


def run_frozen(dev, d, mask, dual=False, want_sums=1, dres="none", want_dy=True, bits=None):
    """One direct call of tmr_bn_frozen_bwd(_ds) between sentinels -> dict of outputs (views) and
    the list of guarded buffers."""
    rows, c = d["g"].shape
    up = lambda k: d[k].to(dev).contiguous()
    bufs = {}
    gf, g = guarded((rows, c), dev, d["g"])
    bufs["g"] = gf
    y, yd, scale, shift, mean = up("y"), up("yd"), up("scale"), up("shift"), up("mean")
    scale_d, mean_d = up("scale_d"), up("mean_d")
    zm = None
    if mask == 1:
        zm = up("z")
    elif mask == 3:
        zm = bits
    out = {}
    for name, want in (("dy", want_dy), ("dyd", want_dy and dual), ("dres", dres == "separate")):
        if want:
            bufs[name], out[name] = guarded((rows, c), dev)
    if dres == "inplace":
        out["dres"] = g
    nparts = _lib.query("tmr_bn_frozen_bwd_parts", rows, c)
    for name in ("parts", "parts_d") if dual else ("parts",):
        bufs[name], out[name] = guarded((nparts, c, 2), dev)
    pbytes = SZ(nparts * c * 2 * 4)
    if dual:
        _lib.call("tmr_bn_frozen_bwd_ds", g, zm, mask, y, scale, shift, mean, out.get("dy"), yd,
                  scale_d, mean_d, out.get("dyd"), out.get("dres"), out["parts"], out["parts_d"],
                  pbytes, rows, c, want_sums, stream_ptr())
    else:
        _lib.call("tmr_bn_frozen_bwd", g, zm, mask, y, scale, shift, mean, out.get("dy"),
                  out.get("dres"), out["parts"], pbytes, rows, c, want_sums, stream_ptr())
    torch.cuda.synchronize()
    out["g"], out["nparts"], out["bufs"] = g, nparts, bufs
    return out


def check_sums(dev, d, parts, nparts, ref, exact, what):
    inv = d["inv"].to(dev)
    dgamma, dbeta = ops.bn_frozen_finalize(parts, nparts, inv)
    dgamma, dbeta = dgamma.double().cpu(), dbeta.double().cpu()
    rows = d["g"].shape[0]
    if exact:
        assert torch.equal(dbeta, ref["s"]), what
        assert torch.equal(dgamma, ref["q"] * d["inv"].double()), what
    else:   # inv == 1: dgamma is the sum itself
        tol = rows * 2.0 ** -24
        assert ((dbeta - ref["s"]).abs() <= tol * ref["s_abs"]).all(), what
        assert ((dgamma - ref["q"]).abs() <= tol * ref["q_abs"]).all(), what


def check_dy(got, want, exact, what):
    got = got.double().cpu()
    if exact:
        assert torch.equal(got, want), what
    else:
        assert ((got - want).abs() <= 2.0 ** -22 * want.abs()).all(), what


def gpu_bits(dev, d):
    """The ReLU-mask bits of z as the forward writes them (ops.bn_apply_bits)."""
    z, bits = ops.bn_apply_bits(d["y"].to(dev), d["scale"].to(dev), d["shift"].to(dev),
                                d["res"].to(dev))
    return z, bits


# ---- the entry points -------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("rows", ROWS)
def test_frozen_bwd_single(dev, rows, c, exact):
    d = make_data(rows, c, exact, seed=rows * 1000 + c)
    z_gpu, bits = gpu_bits(dev, d)
    if exact:
        assert torch.equal(z_gpu.cpu(), d["z"])   # (the bits below are those of this z)
    else:
        d["z"] = z_gpu.cpu()                      # mask 1 and 3 then describe one z
    for mask, dres in ((0, "none"), (1, "inplace"), (2, "separate"), (3, "separate")):
        what = "rows %d c %d mask %d" % (rows, c, mask)
        ref = reference(d, mask)
        o = run_frozen(dev, d, mask, dres=dres, bits=bits)
        assert all(intact(b) for b in o["bufs"].values()), what
        check_dy(o["dy"], ref["dy"], exact, what)
        if dres != "none":   # the masked gradient, exactly (a copy or a zero)
            assert torch.equal(o["dres"].double().cpu(), ref["gm"]), what
        else:
            assert torch.equal(o["g"].cpu(), d["g"]), what
        check_sums(dev, d, o["parts"], o["nparts"], ref, exact, what)
        if exact and mask in (1, 2, 3):
            r_fma, r_res, ch = d["planted"]
            r = r_fma if mask == 2 else r_res
            assert (d["g"][r, ch] != 0).all()
            assert (o["dy"].cpu()[r, ch] == 0).all(), what
            if dres != "none":
                assert (o["dres"].cpu()[r, ch] == 0).all(), what


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("rows", ROWS)
def test_frozen_bwd_ds_and_no_sums(dev, rows, c, exact):
    """The dual form against float64 and bit for bit against two single calls; want_sums = 0
    writes the same dy and leaves the sums buffer untouched."""
    d = make_data(rows, c, exact, seed=rows * 1000 + c + 7)
    z_gpu, bits = gpu_bits(dev, d)
    if not exact:
        d["z"] = z_gpu.cpu()
    for mask in (1, 3):
        what = "ds rows %d c %d mask %d" % (rows, c, mask)
        ref, ref_d = reference(d, mask), reference(d, mask, "yd", "scale_d", "mean_d")
        o = run_frozen(dev, d, mask, dual=True, dres="inplace", bits=bits)
        assert all(intact(b) for b in o["bufs"].values()), what
        check_dy(o["dy"], ref["dy"], exact, what)
        check_dy(o["dyd"], ref_d["dy"], exact, what)
        assert torch.equal(o["dres"].double().cpu(), ref["gm"]), what
        check_sums(dev, d, o["parts"], o["nparts"], ref, exact, what)
        check_sums(dev, d, o["parts_d"], o["nparts"], ref_d, exact, what + " ds")
        # two single calls: the same bits
        s1 = run_frozen(dev, d, mask, dres="none", bits=bits)
        d2 = dict(d, y=d["yd"], scale=d["scale_d"], mean=d["mean_d"])
        s2 = run_frozen(dev, d2, mask, dres="none", bits=bits)
        assert torch.equal(o["dy"], s1["dy"]) and torch.equal(o["dyd"], s2["dy"]), what
        assert torch.equal(o["parts"], s1["parts"]) and torch.equal(o["parts_d"], s2["parts"]), what
        # no sums
        for dual in (False, True):
            n = run_frozen(dev, d, mask, dual=dual, want_sums=0, dres="separate", bits=bits)
            assert all(intact(b) for b in n["bufs"].values()), what
            assert torch.equal(n["dy"], o["dy"]) and torch.equal(n["dres"], o["dres"]), what
            assert (n["parts"] == SENT).all(), what
            if dual:
                assert torch.equal(n["dyd"], o["dyd"]) and (n["parts_d"] == SENT).all(), what
    # sums only (the trunk's downsample BN: dy folded into the conv operands)
    o = run_frozen(dev, d, 0, want_dy=False)
    check_sums(dev, d, o["parts"], o["nparts"], reference(d, 0), exact, "sums only")
    assert torch.equal(o["g"].cpu(), d["g"])


@pytest.mark.parametrize("nparts", [1, 37, 5000])
def test_frozen_finalize_of_dgrad_style_partials(dev, nparts):
    """tmr_bn_frozen_finalize on a bare (nparts, c, 2) partials tensor -- the layout the fused
    dgrad epilogue writes -- exact on the grid."""
    c = 24
    gen = torch.Generator().manual_seed(nparts)
    parts = grid(gen, (nparts, c, 2), 1)          # |sum| <= 5000 < 2^13, multiples of 2^-4
    inv = pow2(gen, (c,), -2, 2).abs()
    full, pv = guarded((nparts, c, 2), dev, parts)
    dgamma, dbeta = ops.bn_frozen_finalize(pv, nparts, inv.to(dev))
    assert intact(full) and torch.equal(pv.cpu(), parts)
    assert torch.equal(dbeta.double().cpu(), parts[:, :, 0].double().sum(0))
    assert torch.equal(dgamma.double().cpu(), parts[:, :, 1].double().sum(0) * inv.double())


@pytest.mark.parametrize("shape", [(2, 8, 8, 8), (1, 9, 7, 64)])
@pytest.mark.parametrize("want_sums", [1, 0])
def test_frozen_bwd_maxpool(dev, shape, want_sums):
    """The stem form against tmr_maxpool2d_bwd followed by the plain form (mask 2), on the grid:
    dy bit for bit, the sums exactly those of float64."""
    n, h, w, c = shape
    gen = torch.Generator().manual_seed(h * 100 + c)
    y = grid(gen, shape, 2)
    scale, mean = pow2(gen, (c,), -2, 1), grid(gen, (c,), 1)
    s0 = grid(gen, (c,), 2)
    shift = scale * s0
    y[0, 0, 0, :] = -s0                             # fmaf(y, scale, shift) == 0 at one pixel
    inv = pow2(gen, (c,), -1, 2).abs()
    yd, sc, sh, mu = y.to(dev), scale.to(dev), shift.to(dev), mean.to(dev)
    p, am = ops.maxpool_fwd_bn(yd, sc, sh)
    dyp = grid(gen, tuple(p.shape), 2).to(dev)
    dx = ops.maxpool_bwd(dyp, am, (h, w))
    dy_ref, _, parts_ref, np_ref = ops.bn_frozen_bwd(dx, yd, sc, sh, mu, mask=2)
    ho, wo = p.shape[1:3]
    dyf, dy = guarded(shape, dev)
    nparts = _lib.query("tmr_bn_frozen_bwd_maxpool_parts", n, h, w, c)
    pf, parts = guarded((nparts, c, 2), dev)
    _lib.call("tmr_bn_frozen_bwd_maxpool", dyp, am, n, h, w, ho, wo, yd, sc, sh, mu, dy, parts,
              SZ(nparts * c * 2 * 4), c, want_sums, stream_ptr())
    torch.cuda.synchronize()
    assert intact(dyf) and intact(pf)
    assert torch.equal(dy, dy_ref)
    # float64 from the maxpool backward's dx (a gather: exact)
    gm = torch.where((y.double() * scale.double() + shift.double()) > 0, dx.double().cpu(),
                     torch.zeros((), dtype=torch.float64))
    assert torch.equal(dy.double().cpu(), gm * scale.double())
    assert (dy[0, 0, 0].cpu() == 0).all()
    if not want_sums:
        assert (parts == SENT).all()
        return
    dgamma, dbeta = ops.bn_frozen_finalize(parts, nparts, inv.to(dev))
    assert torch.equal(dbeta.double().cpu(), gm.sum((0, 1, 2)))
    assert torch.equal(dgamma.double().cpu(),
                       (gm * (y.double() - mean.double())).sum((0, 1, 2)) * inv.double())
    dg2, db2 = ops.bn_frozen_finalize(parts_ref, np_ref, inv.to(dev))
    assert torch.equal(dg2, dgamma.float().to(dev)) and torch.equal(db2, dbeta.float().to(dev))


def test_frozen_entry_points_refuse_other_shapes(dev):
    """8 channels per thread, 16-B pieces: c = 12 and misaligned operands are refused by name."""
    rows = 4
    d = make_data(rows, 16, True, seed=5)
    big = torch.zeros(rows * 16 + 8, device=dev)
    g_ok, g_off = big[:rows * 16].view(rows, 16), big[1:rows * 16 + 1].view(rows, 16)
    v = lambda k: d[k].to(dev)
    dy = torch.empty(rows, 16, device=dev)
    parts = torch.empty(_lib.query("tmr_bn_frozen_bwd_parts", rows, 16), 16, 2, device=dev)
    pb = SZ(parts.numel() * 4)
    for name, extra in (("tmr_bn_frozen_bwd", ()), ("tmr_bn_frozen_bwd_ds", None)):
        def call(g, y, dyo, c):
            if extra is None:
                _lib.call(name, g, None, 0, y, v("scale"), v("shift"), v("mean"), dyo, v("yd"),
                          v("scale_d"), v("mean_d"), None, None, parts, parts, pb, rows, c, 1,
                          stream_ptr())
            else:
                _lib.call(name, g, None, 0, y, v("scale"), v("shift"), v("mean"), dyo, None, parts,
                          pb, rows, c, 1, stream_ptr())
        with pytest.raises(RuntimeError, match=name + ": .*multiple of 8"):
            call(g_ok, v("y"), dy, 12)
        with pytest.raises(RuntimeError, match=name + ": .*16-B aligned"):
            call(g_off, v("y"), dy, 16)
        with pytest.raises(RuntimeError, match=name + ": .*16-B aligned"):
            call(g_ok, v("y"), g_off, 16)
        call(g_ok, v("y"), dy, 16)                  # the aligned call goes through
    with pytest.raises(RuntimeError, match="tmr_bn_frozen_bwd_parts"):
        _lib.query("tmr_bn_frozen_bwd_parts", rows, 12)
    # the stem form
    y = torch.zeros(1, 4, 4, 16, device=dev)
    ybig = torch.zeros(1 * 4 * 4 * 16 + 8, device=dev)
    y_off = ybig[1:257].view(1, 4, 4, 16)
    dyp = torch.zeros(1, 2, 2, 16, device=dev)
    am = torch.zeros(1, 2, 2, 16, dtype=torch.uint8, device=dev)
    args = lambda yy, c: (dyp, am, 1, 4, 4, 2, 2, yy, v("scale"), v("shift"), v("mean"),
                          torch.empty_like(y), None, SZ(0), c, 0, stream_ptr())
    with pytest.raises(RuntimeError, match="tmr_bn_frozen_bwd_maxpool: .*multiple of 8"):
        _lib.call("tmr_bn_frozen_bwd_maxpool", *args(y, 12))
    with pytest.raises(RuntimeError, match="tmr_bn_frozen_bwd_maxpool: .*16-B aligned"):
        _lib.call("tmr_bn_frozen_bwd_maxpool", *args(y_off, 16))
    torch.cuda.synchronize()


def test_scaled_weights_and_row_scale(dev):
    """ops.weight_to_crsk_scaled = weight_to_crsk * scale[k] (one rounding of an fp32 product:
    compared with torch's), inside a layout session's refresh as well; ops.scale_rows likewise."""
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(24, 16, 3, 3, generator=gen).to(dev)
    scale = torch.randn(24, generator=gen).to(dev)
    want = (w * scale.view(-1, 1, 1, 1)).permute(1, 2, 3, 0).contiguous()
    assert torch.equal(ops.weight_to_crsk_scaled(w, scale), want)
    owner = torch.nn.Conv2d(16, 24, 3, bias=False).to(dev)
    with torch.no_grad():
        owner.weight.copy_(w)
    for step in range(3):       # recorded, then refreshed from the current w and scale
        with torch.no_grad():
            owner.weight.mul_(1.5)
            scale.add_(0.25)
        with ops.layout_session(owner, ("test-frozen",)):
            got = ops.weight_to_crsk_scaled(owner.weight.detach(), scale)
            plain = ops.weight_to_krsc(owner.weight.detach(), cpad=16)
        want = (owner.weight.detach() * scale.view(-1, 1, 1, 1)).permute(1, 2, 3, 0).contiguous()
        assert torch.equal(got, want), step
        assert torch.equal(plain, owner.weight.detach().permute(0, 2, 3, 1).contiguous()), step
    ops.clear_layout_sessions(owner)
    for shape in ((24, 16, 3, 3), (8, 3, 7, 7)):    # 16-B rows and the scalar form
        dw = torch.randn(shape, generator=gen).to(dev)
        sc = torch.randn(shape[0], generator=gen).to(dev)
        want = dw * sc.view(-1, 1, 1, 1)
        assert torch.equal(ops.scale_rows(dw.clone(), sc), want)


# ---- the step ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frozen_run(dev):
    """One frozen step of the HIP model on step_case(): model, buffers before, logits, grads."""
    m = F.hip_model(dev)
    before = _buffers(m)
    logits, loss, grads = F.hip_step(m, dev)
    return {"m": m, "before": before, "logits": logits.clone(), "loss": loss,
            "grads": {n: g.detach().clone() for n, g in grads.items()}}


def test_step_against_float64_oracle(frozen_run):
    """Every gradient and the logits of the frozen 2-frame step under _assert_vs_fp64; the
    per-parameter record goes to profiles/frozen_bn/step_parity.json."""
    rows = []
    try:
        F.assert_step(frozen_run["grads"], frozen_run["logits"], what="frozen step",
                      record="frozen_step", rows_out=rows)
    finally:
        o64 = F.oracle_step(torch.float64)
        rec = {"case": "tests/_frozen_bn.step_case(): B=1, T=2, L=3", "loss_hip": frozen_run["loss"],
               "loss_fp64": o64["loss"], "params": rows}
        d = os.path.join(ROOT, "profiles", "frozen_bn")
        try:   # (a read-only checkout keeps the committed record)
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, "step_parity.json"), "w") as f:
                json.dump(rec, f, indent=1)
        except OSError:
            pass
    assert abs(frozen_run["loss"] - o64["loss"]) <= 1e-4 * max(1.0, abs(o64["loss"]))


def test_step_writes_no_statistics(frozen_run):
    after = _buffers(frozen_run["m"])
    n = 0
    for name, b in frozen_run["before"].items():
        assert torch.equal(after[name], b), name
        n += name.endswith(("running_mean", "running_var", "num_batches_tracked"))
    assert n == 3 * 53
    assert not any(b.training for b in frozen_run["m"].share.modules()
                   if isinstance(b, torch.nn.BatchNorm2d))


def test_train_features_match_eval_features(frozen_run, dev):
    """The frozen trunk in train mode against the same trunk in eval mode, by the criterion of
    tests/test_infer16_resnest_split_gpu.py with the eval features as both of its references."""
    from tests.test_infer16_resnest_split_gpu import _criterion
    m = frozen_run["m"]
    x4 = F.hip_inputs(dev)[0]
    with torch.no_grad():
        m.train()
        ft = m.share.features_nhwc4(x4).clone()
        m.eval()
        fe = m.share.features_nhwc4(x4).clone()
        m.train()
    fe = fe.cpu()
    _criterion(ft.cpu().numpy(), fe, fe.double(), "frozen train vs eval features")
    assert torch.isfinite(ft).all() and ft.abs().max() > 0


def test_step_runs_without_the_batch_statistics_ops(frozen_run, dev, monkeypatch):
    """P1 / P2: no statistics epilogue, finalize, two-pass BN backward or their variants."""
    def refuse(name):
        def f(*a, **k):
            raise AssertionError("the frozen step called ops.%s" % name)
        return f
    for name in ("bn_finalize", "bn_fwd_train", "bn_bwd", "bn_bwd_parts", "bn_bwd_parts_ds",
                 "bn_bwd_maxpool", "conv_fwd_bnstats"):
        monkeypatch.setattr(ops, name, refuse(name))
    launches = []
    real = ops.bn_frozen_params
    monkeypatch.setattr(ops, "bn_frozen_params", lambda *a: (launches.append(a[1]), real(*a))[1])
    monkeypatch.setattr(ops, "bn_eval_params", refuse("bn_eval_params"))
    logits, loss, grads = F.hip_step(frozen_run["m"], dev)
    assert launches == [53]     # one launch for all 53 BNs
    assert torch.equal(logits, frozen_run["logits"])
    for n, g in grads.items():
        assert torch.equal(g, frozen_run["grads"][n]), n


def test_affine_false_step(dev):
    m = F.hip_model(dev, affine=False)
    logits, loss, grads = F.hip_step(m, dev)
    bn = {n for n, _ in m.named_parameters()
          if n.startswith("share.") and (".bn" in n or ".downsample.1." in n)}
    assert len(bn) == 106
    F.assert_step(grads, logits, what="frozen step, affine=False", record="frozen_step_noaffine",
                  absent=bn)


def test_unfrozen_model_is_untouched(dev):
    """An fp32 model that was frozen and unfrozen steps exactly like one that never was."""
    a = F.hip_model(dev, frozen=False)
    b = tmrnet_amd.unfreeze_bn(F.hip_model(dev, frozen=True))
    la, _, ga = F.hip_step(a, dev)
    lb, _, gb = F.hip_step(b, dev)
    assert torch.equal(la, lb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    for (n, x), (_, y) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(x, y), n
    assert int(a.share.bn1.num_batches_tracked) == 1


def test_batch_independence(dev):
    """2 clips x 2 frames, the HIP step against itself: clip A's logits in the batch (A, B) and in
    (A, C), and grad(A + B) against grad(A) + grad(B) from two single-clip steps.  With frozen BN
    these differ by rounding only, so the bound is the size of fp32 rounding on the same
    quantity: the fp32 CPU oracle's distance from float64 (for the gradients, of its grad(A + B)
    from float64's grad(A) + grad(B), per parameter as l2_err) times GRAD_RATIO, no floor.
    nl_block.linear2.bias, whose exact gradient is 0, has no relative error and is held to the
    1e-5 of the largest gradient norm instead.  Also asserted: grad(A + B) taken together is no
    further from the float64 sum than AGG_RATIO x the fp32 oracle (_assert_vs_fp64's aggregate).

    Measured (this test's first form held each parameter of grad(A + B) to the float64 sum by
    _assert_vs_fp64): aggregate 0.50, but per parameter up to 6.75 x the fp32 oracle at
    layer4.2.* (3.7e-5 against 5.6e-6) -- an error those share with lstm.* (5.5e-5 against
    1.8e-5 on the single-clip step, the LSTM biases included, which no trunk kernel touches):
    it enters in the LSTM, whose inputs reach |374| under the randomised BN, not in the trunk."""
    from tests.test_model_parity_gpu import GRAD_RATIO, AGG_RATIO, l2_err
    m = F.hip_model(dev)
    keep = lambda t: (t[0].clone(), {n: g.detach().clone() for n, g in t[2].items()})
    l_ab, g_ab = keep(F.hip_step(m, dev, (0, 1)))
    l_ac, _ = keep(F.hip_step(m, dev, (0, 2)))
    l_a, g_a = keep(F.hip_step(m, dev, (0,)))
    l_b, g_b = keep(F.hip_step(m, dev, (1,)))
    o64 = {k: F.oracle_step(torch.float64, k) for k in ((0,), (1,), (0, 1))}
    o32 = {k: F.oracle_step(torch.float32, k) for k in ((0, 1), (0, 2))}
    # logits of A do not depend on the other clip
    want = o64[(0, 1)]["logits"][0]
    assert (o64[(0,)]["logits"][0] - want).abs().max() < 1e-12
    e_cpu = min((o32[k]["logits"][0].double() - want).abs().max().item() for k in o32)
    swap = max((l_ab[0] - l_ac[0]).abs().max().item(), (l_ab[0] - l_a[0]).abs().max().item(),
               (l_ab[1] - l_b[0]).abs().max().item())
    print("batch independence: logits swap %.3g, fp32 oracle vs float64 %.3g" % (swap, e_cpu))
    assert swap <= GRAD_RATIO * e_cpu
    # gradients are additive
    summed64 = {n: o64[(0,)]["grads"][n] + o64[(1,)]["grads"][n] for n in o64[(0,)]["grads"]}
    gmax = max(g.norm().item() for g in g_ab.values())
    rows, bad = [], []
    for n, g in g_ab.items():
        s = g_a[n].double() + g_b[n].double()
        e_acc = l2_err(g, summed64[n])
        e32 = l2_err(o32[(0, 1)]["grads"][n], summed64[n])
        if n.endswith("linear2.bias"):
            ok = (g.double() - s).norm().item() <= 1e-5 * gmax
            rows.append((n, (g.double() - s).norm().item(), e32, e_acc))
        else:
            e_hip = l2_err(g, s)
            ok = e_hip <= GRAD_RATIO * e32
            rows.append((n, e_hip, e32, e_acc))
        if not ok:
            bad.append(rows[-1])
    agg_rows = [r for r in rows if not r[0].endswith("linear2.bias")]
    agg = (sum(r[3] ** 2 for r in agg_rows) / sum(r[2] ** 2 for r in agg_rows)) ** 0.5
    worst = max(agg_rows, key=lambda r: r[1] / r[2])
    print("batch independence: grads worst defect %s %.3g vs fp32 oracle %.3g; accuracy vs float64 "
          "aggregate %.3g, worst per-parameter ratio %.3g"
          % (worst[0], worst[1], worst[2], agg, max(r[3] / r[2] for r in agg_rows)))
    assert not bad, bad[:5]
    assert agg <= AGG_RATIO, agg


def test_short_trajectory(dev):
    """STEPS SGD steps at lr 1e-4 on step_case(): the losses fall and stay within 5% of the
    float64 oracle trajectory's initial loss of that trajectory (tests/test_bwd16_gpu.py's bound)."""
    from oracle import tmrnet_ref as ref
    m = F.hip_model(dev)
    x4, lt, labels, masks = F.hip_inputs(dev)
    m.nl_block.forced_mask, m.forced_head_mask = masks["nl"], masks["head"]
    opt = tmrnet_amd.SGD(ref.sgd_param_groups(m, F.LR), lr=F.LR / 10, momentum=0.9,
                         weight_decay=5e-4)
    crit = tmrnet_amd.CrossEntropyLoss(size_average=False)
    before = _buffers(m)
    losses = []
    for _ in range(F.STEPS):
        opt.zero_grad()
        loss = crit(m(x4, lt), labels)
        loss.backward()
        opt.step()
        losses.append(float(loss.item()))
    want = np.asarray(F.oracle_trajectory(torch.float64))
    got = np.asarray(losses)
    print("frozen trajectory:", json.dumps({"hip": losses, "fp64": list(want)}))
    assert (np.diff(got) < 0).all(), losses
    assert (np.abs(got - want) <= 0.05 * want[0]).all(), (losses, list(want))
    after = _buffers(m)
    assert all(torch.equal(after[n], b) for n, b in before.items())
