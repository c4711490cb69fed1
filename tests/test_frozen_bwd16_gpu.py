"""freeze_bn(backward="bf16") on the GPU: the tmr_bn_frozen_bwd*_x entry points bit for bit
against their fp32 siblings, ops.weight_to_crsk_scaled(bf16=True), the fused dgrad in the step's
operand mix (bf16 dy and weights beside an fp32 y), and the 2-frame step against the float64 run
of the contract's emulation (tests/_frozen_bwd16.py)."""
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
from tests._frozen_bn import SENT, guarded, intact, _buffers, _keep
from tests import _frozen_bwd16 as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "frozen_bwd16")
SZ = ctypes.c_size_t
BF16 = torch.bfloat16
ROWS, CS = (1, 98, 1025), (8, 24, 256)


def _bits_of(dev, z):
    """int32 ReLU-mask words of z > 0 (element e = bit e % 32 of word e / 32)."""
    return torch.from_numpy(X.pack_bits(z > 0).view(np.int32)).to(dev)


def run_x(dev, k, mask, dual, want_sums, b16, want_dy=True, g16=False, inplace=True, entry="x"):
    """One call between sentinels.  entry "x": the _x entry point (b16: bf16 dy's; g16: the bf16
    masked g); "fp32": the fp32 sibling.  -> dict of numpy outputs and whether every guard zone
    survived."""
    rows, c = k["g"].shape
    up = lambda n: torch.from_numpy(k[n]).to(dev)
    bufs, out = [], {}
    gf, g = guarded((rows, c), dev, up("g"))
    bufs.append(gf)
    zm = up("z") if mask == 1 else (_bits_of(dev, k["z"]) if mask == 3 else None)
    dt = BF16 if b16 else torch.float32
    t = {}
    for name, want, d in (("dy", want_dy, dt), ("dyd", want_dy and dual, dt), ("g16", g16, BF16),
                          ("dres", not inplace, torch.float32)):
        if want:
            f, t[name] = guarded((rows, c), dev, dtype=d)
            bufs.append(f)
    if inplace:
        t["dres"] = g
    nparts = _lib.query("tmr_bn_frozen_bwd_parts", rows, c)
    for name in ("parts", "parts_d") if dual else ("parts",):
        f, t[name] = guarded((nparts, c, 2), dev)
        bufs.append(f)
    pb = SZ(nparts * c * 2 * 4)
    a = (g, zm, mask, up("y"), up("scale"), up("shift"), up("mean"), t.get("dy"))
    if dual:
        a += (up("yd"), up("scale_d"), up("mean_d"), t.get("dyd"))
    a += (t.get("dres"),)
    if entry == "x":
        a += (t.get("g16"),)
    a += (t["parts"],) + ((t["parts_d"],) if dual else ()) + (pb, rows, c, want_sums)
    if entry == "x":
        a += (int(b16),)
    name = "tmr_bn_frozen_bwd" + ("_ds" if dual else "") + ("_x" if entry == "x" else "")
    _lib.call(name, *a, stream_ptr())
    torch.cuda.synchronize()
    for n, v in t.items():
        out[n] = X.bits16(v) if v.dtype == BF16 else v.cpu().numpy()
    out["ok"] = all(intact(b) for b in bufs)
    return out


def _same(t, ref):
    """A wrapper's output tensor against run_x's numpy record of it (bf16: as bits)."""
    if t.dtype == BF16:
        return np.array_equal(X.bits16(t), ref)
    return torch.equal(t.cpu(), torch.from_numpy(ref))


@pytest.fixture
def entries(monkeypatch):
    """The names of the library entries that ops calls, in order."""
    names, real = [], ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


@pytest.mark.parametrize("rows,c", [(ROWS[0], CS[0]), (ROWS[1], CS[1])])
def test_merged_wrappers_are_the_direct_calls(dev, entries, rows, c):
    """ops.bn_frozen_bwd / _ds for masks 0..3, dy16, want_g16 and want_sums on and off, dres in
    place: every output torch.equal to the same call through _lib.call (run_x; bf16 as bits); with
    neither dy16 nor want_g16 the fp32 entry is the one called, else the _x entry."""
    k = X.x_case(rows, c, rows * 1000 + c + 7)
    v = lambda n: torch.from_numpy(k[n]).to(dev)
    for mask in range(4):
        mk = dict(z=v("z")) if mask == 1 else \
            (dict(bits=_bits_of(dev, k["z"])) if mask == 3 else {})
        for dual in (False, True):
            for dy16 in (False, True):
                for g16 in (False, True):
                    for sums in (False, True):
                        what = (rows, c, mask, dual, dy16, g16, sums)
                        x = dy16 or g16
                        ref = run_x(dev, k, mask, dual, int(sums), dy16, g16=g16,
                                    entry="x" if x else "fp32")
                        assert ref["ok"], what
                        g = v("g")
                        a = (g, v("y"), v("scale"), v("shift"), v("mean"))
                        kw = dict(mask=mask, dres_inplace=True, want_sums=sums, dy16=dy16,
                                  want_g16=g16, **mk)
                        del entries[:]
                        if dual:
                            dy, dyd, gb, parts, parts_d, nparts = ops.bn_frozen_bwd_ds(
                                *a, v("yd"), v("scale_d"), v("mean_d"), **kw)
                            assert _same(dyd, ref["dyd"]), what
                            assert dyd.dtype == (BF16 if dy16 else torch.float32), what
                        else:
                            dy, gb, parts, nparts = ops.bn_frozen_bwd(*a, **kw)
                            parts_d = None
                        torch.cuda.synchronize()
                        name = "tmr_bn_frozen_bwd" + ("_ds" if dual else "") + ("_x" if x else "")
                        assert [n for n in entries if "frozen" in n] == [name], (what, entries)
                        assert dy.dtype == (BF16 if dy16 else torch.float32), what
                        assert _same(dy, ref["dy"]) and _same(g, ref["dres"]), what
                        assert (gb is None) == (not g16), what
                        assert gb is None or _same(gb, ref["g16"]), what
                        if sums:
                            assert nparts == _lib.query("tmr_bn_frozen_bwd_parts", rows, c)
                            assert _same(parts, ref["parts"]), what
                            assert parts_d is None or _same(parts_d, ref["parts_d"]), what
                            assert (parts_d is not None) == dual, what
                        else:
                            assert parts is None and parts_d is None and nparts == 0, what


@pytest.mark.parametrize("dy16", [False, True])
@pytest.mark.parametrize("want_sums", [True, False])
def test_merged_maxpool_wrapper_is_the_direct_call(dev, entries, dy16, want_sums):
    """ops.bn_frozen_bwd_maxpool at (1, 9, 7, 64): dy and the partials torch.equal to the direct
    call of the entry it must take -- the fp32 one without dy16."""
    shape = n, h, w, c = (1, 9, 7, 64)
    gen = torch.Generator().manual_seed(97)
    yd = torch.randn(shape, generator=gen).to(dev)
    sc = (0.5 + torch.rand(c, generator=gen)).to(dev)
    sh = (0.1 * torch.randn(c, generator=gen)).to(dev)
    mu = (0.2 * torch.randn(c, generator=gen)).to(dev)
    p, am = ops.maxpool_fwd_bn(yd, sc, sh)
    dyp = torch.randn(tuple(p.shape), generator=gen).to(dev)
    name = "tmr_bn_frozen_bwd_maxpool" + ("_x" if dy16 else "")
    nparts = _lib.query("tmr_bn_frozen_bwd_maxpool_parts", n, h, w, c)
    dyf, dy_ref = guarded(shape, dev, dtype=BF16 if dy16 else torch.float32)
    pf, parts_ref = guarded((nparts, c, 2), dev)
    _lib.call(name, dyp, am, n, h, w, p.shape[1], p.shape[2], yd, sc, sh, mu, dy_ref, parts_ref,
              SZ(nparts * c * 2 * 4), c, int(want_sums), *((1,) if dy16 else ()), stream_ptr())
    torch.cuda.synchronize()
    assert intact(dyf) and intact(pf)
    del entries[:]
    dy, parts, npp = ops.bn_frozen_bwd_maxpool(dyp, am, yd, sc, sh, mu, want_sums=want_sums,
                                               dy16=dy16)
    torch.cuda.synchronize()
    assert [e for e in entries if "frozen" in e and not e.endswith("_parts")] == [name], entries
    assert dy.dtype == dy_ref.dtype
    assert torch.equal(dy.view(torch.int16) if dy16 else dy,
                       dy_ref.view(torch.int16) if dy16 else dy_ref)
    if want_sums:
        assert npp == nparts and torch.equal(parts, parts_ref)
    else:
        assert parts is None and npp == 0


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("rows", ROWS)
def test_frozen_bwd_x(dev, rows, c):
    """tmr_bn_frozen_bwd_x / _ds_x, masks 0..3, single and dual, want_sums 0 / 1, dres in place:
    bf16 dy / dy_ds = RNE of the fp32 entry point's, g16 = RNE(dres), partials and dres bit for
    bit the fp32 call's; out_bf16 = 0, g16 = NULL is the fp32 entry point itself."""
    k = X.x_case(rows, c, rows * 1000 + c)
    u = X.bits32(k["g"][:, 0])
    assert ((u & 0xFFFF) == 0x8000).all()               # the planted ties
    for mask in range(4):
        for dual in (False, True):
            for sums in (1, 0):
                what = "rows %d c %d mask %d dual %s sums %d" % (rows, c, mask, dual, sums)
                ref = run_x(dev, k, mask, dual, sums, False, entry="fp32")
                assert ref["ok"], what
                emu = X.emu_x(k, mask, dual)            # the fp32 call is what the emulation says
                assert np.array_equal(X.bits32(ref["dres"]), X.bits32(emu["dres"])), what
                assert np.array_equal(X.bits32(ref["dy"]), X.bits32(emu["dy"])), what
                got = run_x(dev, k, mask, dual, sums, True, g16=True)
                assert got["ok"], what
                want = dict(ref)
                got16 = dict(dy16=got["dy"], dyd16=got.get("dyd"), g16=got["g16"],
                             dres=got["dres"], parts=got["parts"], parts_d=got.get("parts_d"))
                assert X.compare_x(got16, want) == [], what
                if not sums:
                    assert (got["parts"] == SENT).all(), what
                # the fp32 form of the _x entry point: the fp32 entry point's bits
                same = run_x(dev, k, mask, dual, sums, False)
                for n in ("dy", "dyd", "dres", "parts", "parts_d"):
                    if n in ref:
                        assert np.array_equal(X.bits32(same[n]), X.bits32(ref[n])), (what, n)
                assert same["ok"], what
    # the planted zeros of the mask's argument pass nothing
    z0 = k["zero"] & (k["g"] != 0)
    got = run_x(dev, k, 1, False, 0, True, g16=True)
    assert z0.any() and (got["g16"][z0] & 0x7FFF == 0).all() and (got["dy"][z0] & 0x7FFF == 0).all()
    got = run_x(dev, k, 2, False, 0, True, g16=True)
    assert (got["g16"][:, 1][k["zero"][:, 1]] & 0x7FFF == 0).all()


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("rows", ROWS)
def test_block_output_pass(dev, rows, c):
    """dy = NULL, g16, mask 0, want_sums 0 / 1 -- the step's pass over a block output's gradient:
    g untouched, g16 = RNE(g), the partials those of the fp32 sums-only call."""
    k = X.x_case(rows, c, rows * 1000 + c + 3)
    ref = run_x(dev, k, 0, False, 1, False, want_dy=False, inplace=False, entry="fp32")
    for sums in (1, 0):
        got = run_x(dev, k, 0, False, sums, True, want_dy=False, g16=True, inplace=False)
        assert got["ok"]
        assert np.array_equal(got["g16"], X.rne_bf16(k["g"]))
        assert np.array_equal(X.bits32(got["dres"]), X.bits32(k["g"]))
        if sums:
            assert np.array_equal(X.bits32(got["parts"]), X.bits32(ref["parts"]))
        else:
            assert (got["parts"] == SENT).all()
    g = torch.from_numpy(k["g"]).to(dev)
    v = lambda n: torch.from_numpy(k[n]).to(dev)
    _, g16, parts, nparts = ops.bn_frozen_bwd(g, v("y"), v("scale"), v("shift"), v("mean"),
                                              mask=0, want_dy=False, want_g16=True)
    assert torch.equal(g16, g.to(BF16)) and np.array_equal(X.bits32(parts.cpu().numpy()),
                                                           X.bits32(ref["parts"]))


@pytest.mark.parametrize("shape", [(2, 8, 8, 8), (1, 9, 7, 64)])
@pytest.mark.parametrize("want_sums", [1, 0])
def test_frozen_bwd_maxpool_x(dev, shape, want_sums):
    """The stem form: bf16 dy = RNE of the fp32 entry point's dy, the same partials; odd h / w."""
    n, h, w, c = shape
    gen = torch.Generator().manual_seed(h * 100 + c)
    y = torch.randn(shape, generator=gen)
    scale = 0.5 + torch.rand(c, generator=gen)
    shift, mean = 0.1 * torch.randn(c, generator=gen), 0.2 * torch.randn(c, generator=gen)
    scale[0], shift[1] = 0.5, 0.0
    y[0, 0, 0, 1] = 0.0                               # fmaf(y, scale, shift) == 0
    yd, sc, sh, mu = y.to(dev), scale.to(dev), shift.to(dev), mean.to(dev)
    p, am = ops.maxpool_fwd_bn(yd, sc, sh)
    dyp = torch.randn(tuple(p.shape), generator=gen)
    g = np.random.default_rng(c)
    dyp[..., 0] = torch.from_numpy(X.ties(g, dyp[..., 0].numel(), 0)).view(dyp.shape[:-1])
    dyp = dyp.to(dev)
    ho, wo = p.shape[1:3]
    nparts = _lib.query("tmr_bn_frozen_bwd_maxpool_parts", n, h, w, c)
    res = {}
    for key, name, dt, extra in (("f32", "tmr_bn_frozen_bwd_maxpool", torch.float32, ()),
                                 ("x32", "tmr_bn_frozen_bwd_maxpool_x", torch.float32, (0,)),
                                 ("x16", "tmr_bn_frozen_bwd_maxpool_x", BF16, (1,))):
        dyf, dy = guarded(shape, dev, dtype=dt)
        pf, parts = guarded((nparts, c, 2), dev)
        _lib.call(name, dyp, am, n, h, w, ho, wo, yd, sc, sh, mu, dy, parts,
                  SZ(nparts * c * 2 * 4), c, want_sums, *extra, stream_ptr())
        torch.cuda.synchronize()
        assert intact(dyf) and intact(pf), key
        res[key] = (dy, parts)
    assert torch.equal(res["x32"][0], res["f32"][0])
    assert np.array_equal(X.bits16(res["x16"][0]), X.rne_bf16(res["f32"][0].cpu().numpy()))
    assert (res["x16"][0][0, 0, 0, 1] == 0).all()
    for key in ("x32", "x16"):
        assert torch.equal(res[key][1], res["f32"][1]), key
    if not want_sums:
        assert (res["x16"][1] == SENT).all()
    dy, parts, npp = ops.bn_frozen_bwd_maxpool(dyp, am, yd, sc, sh, mu, want_sums=bool(want_sums),
                                               dy16=True)
    assert dy.dtype == BF16 and torch.equal(dy, res["x16"][0])
    assert (parts is None) == (not want_sums)


def test_x_entry_points_refuse_other_shapes(dev):
    """c = 12 and a misaligned bf16 output are refused by name."""
    rows = 4
    k = X.x_case(rows, 16, 5)
    v = lambda n: torch.from_numpy(k[n]).to(dev)
    g, y = v("g"), v("y")
    big = torch.zeros(rows * 16 + 8, dtype=BF16, device=dev)
    o_ok, o_off = big[:rows * 16].view(rows, 16), big[1:rows * 16 + 1].view(rows, 16)
    parts = torch.empty(_lib.query("tmr_bn_frozen_bwd_parts", rows, 16), 16, 2, device=dev)
    pb = SZ(parts.numel() * 4)

    def single(dy, g16, c):
        _lib.call("tmr_bn_frozen_bwd_x", g, None, 0, y, v("scale"), v("shift"), v("mean"), dy, None,
                  g16, parts, pb, rows, c, 1, 1, stream_ptr())

    def dual(dy, dyd, g16, c):
        _lib.call("tmr_bn_frozen_bwd_ds_x", g, None, 0, y, v("scale"), v("shift"), v("mean"), dy,
                  v("yd"), v("scale_d"), v("mean_d"), dyd, None, g16, parts, parts, pb, rows, c, 1,
                  1, stream_ptr())
    with pytest.raises(RuntimeError, match="tmr_bn_frozen_bwd_x: .*multiple of 8"):
        single(o_ok, None, 12)
    with pytest.raises(RuntimeError, match="tmr_bn_frozen_bwd_x: .*16-B aligned"):
        single(o_off, None, 16)
    with pytest.raises(RuntimeError, match="tmr_bn_frozen_bwd_x: .*16-B aligned"):
        single(None, o_off, 16)
    with pytest.raises(RuntimeError, match="tmr_bn_frozen_bwd_ds_x: .*multiple of 8"):
        dual(o_ok, o_ok.clone(), None, 12)
    with pytest.raises(RuntimeError, match="tmr_bn_frozen_bwd_ds_x: .*16-B aligned"):
        dual(o_ok, o_off, None, 16)
    with pytest.raises(RuntimeError, match="tmr_bn_frozen_bwd_ds_x: .*16-B aligned"):
        dual(o_ok, o_ok.clone(), o_off, 16)
    single(o_ok, o_ok.clone(), 16)                    # the aligned calls go through
    dual(o_ok, o_ok.clone(), o_ok.clone(), 16)
    # the stem form
    yy = torch.zeros(1, 4, 4, 16, device=dev)
    dyp = torch.zeros(1, 2, 2, 16, device=dev)
    am = torch.zeros(1, 2, 2, 16, dtype=torch.uint8, device=dev)
    obig = torch.zeros(256 + 8, dtype=BF16, device=dev)
    args = lambda out, c: (dyp, am, 1, 4, 4, 2, 2, yy, v("scale"), v("shift"), v("mean"), out, None,
                           SZ(0), c, 0, 1, stream_ptr())
    with pytest.raises(RuntimeError, match="tmr_bn_frozen_bwd_maxpool_x: .*multiple of 8"):
        _lib.call("tmr_bn_frozen_bwd_maxpool_x", *args(obig[:256], 12))
    with pytest.raises(RuntimeError, match="tmr_bn_frozen_bwd_maxpool_x: .*16-B aligned"):
        _lib.call("tmr_bn_frozen_bwd_maxpool_x", *args(obig[1:257], 16))
    _lib.call("tmr_bn_frozen_bwd_maxpool_x", *args(obig[:256], 16))
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(24, 16, 3, 3), (256, 64, 1, 1)])
def test_scaled_weights_bf16(dev, shape):
    """ops.weight_to_crsk_scaled(bf16=True) = RNE(crsk(w) * scale[k]), the product in fp32: alone,
    and recorded then refreshed by a layout session after w and scale change; the fp32 request
    beside it keeps its own copy."""
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(shape, generator=gen)
    scale = 0.5 + torch.rand(shape[0], generator=gen)
    got = ops.weight_to_crsk_scaled(w.to(dev), scale.to(dev), bf16=True)
    assert got.dtype == BF16 and tuple(got.shape) == (shape[1], shape[2], shape[3], shape[0])
    assert X.compare_wscaled(X.bits16(got), w.numpy(), scale.numpy()) == []
    want = (w.to(dev) * scale.to(dev).view(-1, 1, 1, 1)).permute(1, 2, 3, 0).contiguous().to(BF16)
    assert torch.equal(got, want)
    owner = torch.nn.Conv2d(shape[1], shape[0], shape[2], bias=False).to(dev)
    sc = scale.to(dev)
    with torch.no_grad():
        owner.weight.copy_(w)
    for step in range(3):
        with torch.no_grad():
            owner.weight.mul_(1.5)
            sc.add_(0.25)
        with ops.layout_session(owner, ("test-frozen16",)):
            g16 = ops.weight_to_crsk_scaled(owner.weight.detach(), sc, bf16=True)
            g32 = ops.weight_to_crsk_scaled(owner.weight.detach(), sc)
        assert X.compare_wscaled(X.bits16(g16), owner.weight.detach().cpu().numpy(),
                                 sc.cpu().numpy()) == [], step
        assert g32.dtype == torch.float32 and torch.equal(g32.to(BF16), g16), step
    ops.clear_layout_sessions(owner)


# ---- the fused dgrad in the step's mix --------------------------------------------------------
@pytest.mark.parametrize("kind", ["1x1", "3x3"])
def test_fused_dgrad_g16_beside_fp32_y(dev, kind):
    """bf16 dy and CRSK weights, fp32 y, mask 2: with TMR_IO_G16 the bf16 g is the RNE of the
    same call's fp32 g and the partials are the sums of the rounded values, within the 1e-5 that
    tests/test_conv_engine_gpu.py holds the fused dgrad's partials to (its _rel).  Mask 3 with
    beta = 1 into fp32 (the block outputs' unchanged call): a sanity run."""
    from tests.test_conv_engine_gpu import _rel
    n, h = 2, 14
    cin, k, r = (64, 256, 1) if kind == "1x1" else (64, 64, 3)
    gen = torch.Generator().manual_seed(17)
    dy = (torch.randn(n, h, h, k, generator=gen) * 0.5).to(dev).to(BF16)
    w = (torch.randn(k, cin, r, r, generator=gen) / np.sqrt(k * r * r)).to(dev)
    wt = ops.weight_to_crsk(w)
    y = torch.randn(n, h, h, cin, generator=gen).to(dev)
    mean = 0.2 * torch.randn(cin, generator=gen).to(dev)
    scale = (0.5 + torch.rand(cin, generator=gen)).to(dev)
    shift = (0.1 * torch.randn(cin, generator=gen)).to(dev)
    kw = dict(scale=scale, shift=shift, math="bf16", wt=True)
    g32, p32, n32 = ops.conv_dgrad_bnbwd(dy, wt, (h, h), 1, r // 2, y, mean, 2, **kw)
    g16, p16, n16 = ops.conv_dgrad_bnbwd(dy, wt, (h, h), 1, r // 2, y, mean, 2, g16=True, **kw)
    torch.cuda.synchronize()
    assert g16.dtype == BF16 and g32.dtype == torch.float32
    on = (y.double() * scale.double() + shift.double()) > 0    # the fmaf's sign, exactly
    assert (g32[~on] == 0).all() and (g32[on] != 0).any()
    assert torch.equal(g16, g32.to(BF16))
    gr = g16.double().view(-1, cin)
    s0, s1 = gr.sum(0), (gr * (y.double().view(-1, cin) - mean.double())).sum(0)
    p = p16[:n16].double().sum(0)
    assert _rel(p[:, 0], s0) < 1e-5 and _rel(p[:, 1], s1) < 1e-5
    # against float64 on the rounded operands
    wd = wt.double().permute(3, 0, 1, 2)    # (K, C, R, S)
    full = torch.nn.grad.conv2d_input((n, cin, h, h), wd, dy.double().permute(0, 3, 1, 2), 1,
                                      r // 2).permute(0, 2, 3, 1)
    assert _rel(g32, full * on) < 1e-5
    # mask 3, beta 1, fp32 out
    bits = _bits_of(dev, on.cpu().numpy())
    old = torch.randn(n, h, h, cin, generator=gen).to(dev)
    g3, p3, n3 = ops.conv_dgrad_bnbwd(dy, wt, (h, h), 1, r // 2, y, mean, 3, z=bits,
                                      out=old.clone(), beta=1.0, math="bf16", wt=True)
    torch.cuda.synchronize()
    assert g3.dtype == torch.float32 and (g3[~on] == 0).all()
    assert _rel(g3, (old.double() + full) * on) < 1e-5


# ---- the step ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(dev):
    """One step of the fp32 frozen model and of the frozen16 model (share kind "fp32")."""
    m32 = F.hip_model(dev)
    l32, loss32, g32 = _keep(F.hip_step(m32, dev))
    m = F.hip_model(dev, backward="bf16")
    before = _buffers(m)
    torch.cuda.reset_peak_memory_stats()
    l16, loss16, g16 = _keep(F.hip_step(m, dev))
    return {"m": m, "before": before, "l32": l32, "loss32": loss32, "g32": g32, "l16": l16,
            "loss16": loss16, "g16": g16, "peak": torch.cuda.max_memory_allocated()}


def test_step_forward_is_the_fp32_frozen_step(runs):
    assert torch.equal(runs["l16"], runs["l32"]) and runs["loss16"] == runs["loss32"]
    after = _buffers(runs["m"])
    n = 0
    for name, b in runs["before"].items():
        assert torch.equal(after[name], b), name
        n += name.endswith(("running_mean", "running_var", "num_batches_tracked"))
    assert n == 3 * 53
    # outside the trunk no gradient passes a trunk conv's backward: the fp32 step's bits
    for name, g in runs["g16"].items():
        if not name.startswith("share."):
            assert torch.equal(g, runs["g32"][name]), name
    assert any(not torch.equal(g, runs["g32"][n]) for n, g in runs["g16"].items())


def test_step_gradients_against_the_float64_emulation(runs):
    """Every gradient under tests/test_model_parity_gpu._assert_vs_fp64 (the criterion and
    constants of tests/test_bwd16_gpu.py's step test) against the float64 run of the emulation,
    the fp32 run of the emulation as the yardstick; per trunk group |g_frozen16 - g_frozen32| /
    |g_frozen32| on the device within 1.5 x the CPU emulation pair's.  The aggregates go to
    profiles/frozen_bwd16/step_parity.json."""
    from tests.test_model_parity_gpu import _assert_vs_fp64, l2_err
    e64, e32 = X.emu_step(torch.float64), X.emu_step(torch.float32)
    o32 = F.oracle_step(torch.float32)
    assert torch.equal(e32["logits"], o32["logits"])
    rel_dev = X.trunk_rel(runs["g16"], runs["g32"])
    rel_cpu = X.trunk_rel(e32["grads"], o32["grads"])
    rows = [(n, l2_err(g, e64["grads"][n]), l2_err(e32["grads"][n], e64["grads"][n]))
            for n, g in runs["g16"].items()]
    agg_rows = [r for r in rows if not r[0].endswith("linear2.bias")]
    agg = (sum(r[1] ** 2 for r in agg_rows) / sum(r[2] ** 2 for r in agg_rows)) ** 0.5
    rec = {"case": "tests/_frozen_bn.step_case(): B=1, T=2, L=3", "loss": runs["loss16"],
           "rel_dev": rel_dev, "rel_cpu": rel_cpu,
           "ratio": {g: rel_dev[g] / rel_cpu[g] for g in rel_dev}, "agg_ratio_vs_fp64": agg,
           "max_ratio_vs_fp64": max(r[1] / max(r[2], 1e-12) for r in agg_rows),
           "max_memory_allocated": runs["peak"]}
    print("frozen16 step:", json.dumps(rec))
    try:   # (a read-only checkout keeps the committed record)
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, "step_parity.json"), "w") as f:
            json.dump(rec, f, indent=1)
    except OSError:
        pass
    assert all(g is not None for g in runs["g16"].values())
    _assert_vs_fp64(runs["g16"], e32["grads"], e64["grads"], "frozen16_grads")
    for g in X.H.TRUNK_GROUPS:
        assert rel_dev[g] <= 1.5 * rel_cpu[g], rec


def test_step_runs_without_the_batch_statistics_ops(runs, dev, monkeypatch):
    """No statistics epilogue, finalize, two-pass BN backward or their variants (the fp32 frozen
    test's set plus tmr_bn_bwd_parts_x / _ds_d16), no fp32 wgrad fold; every backward conv in
    bf16 math on bf16 dy / CRSK weights, the wgrads on bf16 x (the stem: its fp32 NHWC4 input)."""
    def refuse(name):
        def f(*a, **k):
            raise AssertionError("the frozen16 step called ops.%s" % name)
        return f
    for name in ("bn_finalize", "bn_fwd_train", "bn_bwd", "bn_bwd_parts", "bn_bwd_parts_ds",
                 "bn_bwd_maxpool", "conv_fwd_bnstats", "bn_bwd_parts_coef", "bn_eval_params",
                 "conv_wgrad_bnbwd"):
        monkeypatch.setattr(ops, name, refuse(name))
    real_call = ops.call

    def call(name, *a):
        assert name not in ("tmr_bn_bwd_parts_x", "tmr_bn_bwd_parts_ds_d16"), name
        return real_call(name, *a)
    monkeypatch.setattr(ops, "call", call)
    launches = []
    real = ops.bn_frozen_params
    monkeypatch.setattr(ops, "bn_frozen_params", lambda *a: (launches.append(a[1]), real(*a))[1])
    seen = []
    for name in ("conv_wgrad", "conv_dgrad", "conv_dgrad_bnbwd"):
        orig = getattr(ops, name)

        def spy(a, b, *args, _orig=orig, _name=name, **kw):
            seen.append((_name, a.dtype, b.dtype, tuple(a.shape), kw.get("math", "fp32"),
                         bool(kw.get("g16"))))
            return _orig(a, b, *args, **kw)
        monkeypatch.setattr(ops, name, spy)
    folds = _lib.query("tmr_wgrad_bnbwd_launches")
    logits, loss, grads = F.hip_step(runs["m"], dev)
    assert _lib.query("tmr_wgrad_bnbwd_launches") == folds
    assert launches == [53]
    assert torch.equal(logits, runs["l16"])
    for n, g in grads.items():
        assert torch.equal(g, runs["g16"][n]), n
    wg = [s for s in seen if s[0] == "conv_wgrad"]
    dg = [s for s in seen if s[0] != "conv_wgrad"]
    assert len(wg) == 53 and len(dg) == 52
    for _, xdt, dydt, xshape, math, _g in wg:
        assert math == "bf16" and dydt == BF16
        assert xdt == (torch.float32 if xshape[-1] == 4 else BF16), xshape
    for _, dydt, wdt, _s, math, _g in dg:
        assert math == "bf16" and dydt == BF16 and wdt == BF16
    assert sum(s[5] for s in dg) == 32              # conv3 and conv2 of the 16 blocks store g bf16


def test_affine_false_step(dev, runs):
    m = F.hip_model(dev, affine=False, backward="bf16")
    logits, loss, grads = F.hip_step(m, dev)
    bn = {n for n, _ in m.named_parameters()
          if n.startswith("share.") and (".bn" in n or ".downsample.1." in n)}
    assert len(bn) == 106
    assert torch.equal(logits, runs["l16"])
    for n, g in grads.items():
        if n in bn:
            assert g is None, n
        else:   # without the sums the other gradients are the affine step's bits
            assert torch.equal(g, runs["g16"][n]), n


@pytest.mark.parametrize("precision", ["fp32", "bf16-bwd"])
def test_both_share_kinds_and_unfreeze(dev, runs, precision):
    """The frozen16 step is the same on an "fp32" and a "bf16-bwd" share; unfreeze_bn gives back
    the share's own step, torch.equal to a never-frozen model's."""
    m = F.hip_model(dev, backward="bf16", precision=precision)
    logits, _, grads = F.hip_step(m, dev)
    assert torch.equal(logits, runs["l16"])
    for n, g in grads.items():
        assert torch.equal(g, runs["g16"][n]), n
    a = F.hip_model(dev, frozen=False, precision=precision)
    b = tmrnet_amd.unfreeze_bn(m)
    la, _, ga = F.hip_step(a, dev)
    lb, _, gb = F.hip_step(b, dev)
    assert torch.equal(la, lb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    # (b's statistics were not written by its frozen step: one update on each side)
    for (n, x), (_, y) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(x, y), n
    assert int(b.share.bn1.num_batches_tracked) == 1


def test_batch_independence(dev, runs):
    """2 clips x 2 frames: clip A's logits bit-identical in (A, B), (A, C) and alone; grad(A + B)
    against grad(A) + grad(B) bounded as tests/test_frozen_bn_gpu.py::test_batch_independence
    bounds the fp32 frozen step (GRAD_RATIO x the fp32 run's distance of grad(A + B) from the
    float64 sum, here both of the emulation; linear2.bias 1e-5 of the largest norm)."""
    from tests.test_model_parity_gpu import GRAD_RATIO, AGG_RATIO, l2_err
    m = runs["m"]
    keep = lambda t: (t[0].clone(), {n: g.detach().clone() for n, g in t[2].items()})
    l_ab, g_ab = keep(F.hip_step(m, dev, (0, 1)))
    l_ac, _ = keep(F.hip_step(m, dev, (0, 2)))
    l_b, g_b = keep(F.hip_step(m, dev, (1,)))
    l_a, g_a = runs["l16"], runs["g16"]
    swap = max((l_ab[0] - l_ac[0]).abs().max().item(), (l_ab[0] - l_a[0]).abs().max().item(),
               (l_ab[1] - l_b[0]).abs().max().item())
    print("frozen16 batch independence: logits swap %.3g" % swap)
    assert torch.equal(l_ab[0], l_ac[0]) and torch.equal(l_ab[0], l_a[0])
    assert torch.equal(l_ab[1], l_b[0])
    e64 = {k: X.emu_step(torch.float64, k) for k in ((0,), (1,))}
    e32 = X.emu_step(torch.float32, (0, 1))
    summed64 = {n: e64[(0,)]["grads"][n] + e64[(1,)]["grads"][n] for n in e64[(0,)]["grads"]}
    gmax = max(g.norm().item() for g in g_ab.values())
    rows, bad = [], []
    for n, g in g_ab.items():
        s = g_a[n].double() + g_b[n].double()
        e_acc = l2_err(g, summed64[n])
        e_cpu = l2_err(e32["grads"][n], summed64[n])
        if n.endswith("linear2.bias"):
            ok = (g.double() - s).norm().item() <= 1e-5 * gmax
        else:
            e_hip = l2_err(g, s)
            ok = e_hip <= GRAD_RATIO * e_cpu
            rows.append((n, e_hip, e_cpu, e_acc))
        if not ok:
            bad.append((n, l2_err(g, s), e_cpu))
    agg = (sum(r[3] ** 2 for r in rows) / sum(r[2] ** 2 for r in rows)) ** 0.5
    worst = max(rows, key=lambda r: r[1] / r[2])
    print("frozen16 batch independence: worst defect %s %.3g vs fp32 emulation %.3g; aggregate vs "
          "float64 %.3g" % (worst[0], worst[1], worst[2], agg))
    assert not bad, bad[:5]
    assert agg <= AGG_RATIO, agg


def test_short_trajectory(dev):
    """STEPS SGD steps at lr 1e-4 on step_case(): the frozen16 losses fall and stay within 5% of
    the initial loss of the fp32 frozen step's trajectory."""
    from oracle import tmrnet_ref as ref
    x4, lt, labels, masks = F.hip_inputs(dev)
    crit = tmrnet_amd.CrossEntropyLoss(size_average=False)
    traj = {}
    for key, m in (("frozen32", F.hip_model(dev)),
                   ("frozen16", F.hip_model(dev, backward="bf16", precision="bf16-bwd"))):
        m.nl_block.forced_mask, m.forced_head_mask = masks["nl"], masks["head"]
        opt = tmrnet_amd.SGD(ref.sgd_param_groups(m, F.LR), lr=F.LR / 10, momentum=0.9,
                             weight_decay=5e-4)
        before = _buffers(m)
        losses = []
        for _ in range(F.STEPS):
            opt.zero_grad()
            loss = crit(m(x4, lt), labels)
            loss.backward()
            opt.step()
            losses.append(float(loss.item()))
        traj[key] = losses
        after = _buffers(m)
        assert all(torch.equal(after[n], b) for n, b in before.items())
    print("frozen16 trajectory:", json.dumps(traj))
    got, want = np.asarray(traj["frozen16"]), np.asarray(traj["frozen32"])
    assert got[0] == want[0]
    assert (np.diff(got) < 0).all(), traj
    assert (np.abs(got - want) <= 0.05 * want[0]).all(), traj
