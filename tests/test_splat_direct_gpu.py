"""Every entry point of csrc/resnest.hip -- the training split attention, column centring, axpy and
the general AvgPool2d -- against the float64 references of tests/_splat_ref.py, elementwise within
the bounds derived there (tests/test_splat_direct_cpu.py shows them fair and sharp).  Each check
prints `ratio <entry point> <max error / bound>`; the assertion is ratio <= 1.

Outputs go to NaN-filled buffers between sentinels (`guarded` / `guarded16`), or come from wrappers
whose torch.empty hands out NaN (`poison`).  bf16 operands run 16-B aligned and 8 bytes off; both
results are held to float64.

Shapes (n, h, w, C):
  (1, 1, 1, 4)       hw = 1 and C/4 = 1: both FastDivs with d = 1, one frame, 255 / 1023 idle rows
  (3, 5, 3, 12)      C/4 = 3: non-power-of-two division; red_shape cols 2, ragged last chunk;
                     C % 8 != 0: bf16 stays 4-wide
  (2, 4, 5, 24)      C/8 = 3 does not divide 256: aligned bf16 still takes the 4-wide kernels
  (5, 7, 7, 40)      C/8 = 5 likewise; C/4 = 10: cols 8, 2 chunks, ragged
  (6, 7, 7, 64)      8-wide, C/8 = 8
  (3, 10, 30, 264)   C/4 = 66: a full 64-column chunk and one of 2 columns; hw = 300 (ragged rows)
  (4, 7, 7, 512)     layer4's shape, 2 full chunks, C/8 = 64
  (2, 3, 1, 2048)    C/8 = 256 = the block; hw = 3 < the row count
  BIG (the second trip of the grid-stride loops, grid cap 8192 blocks), one per loop form:
  (5, 29, 29, 512) scalar unfused kernels; (5, 29, 29, 2048) 4-wide _bn kernels, fp32 and bf16 8
  bytes off; (10, 29, 29, 2048) 8-wide, where a thread's second pixel lies in another frame (the
  att / dgap register cache); (1025, 2048) tmr_splat_att; 2^21 + 3 tmr_axpy.
tmr_splat_bn0_coefs and tmr_center_cols also run at n / rows in {1, 5, 16, 17, 33} (16 row groups:
idle, exact, second trip) x 8, 48, 64, 80, 1024 columns (partial, exact, second partial block).
Average pools (n, h, w, c, k, s, p, count_include_pad, ceil_mode): three windows that hang over the
padded extent with count_include_pad (nn.AvgPool2d divides by the clipped window), avg_down at
stride 1 with c/4 = 1, h = 1 and w = 1 (FastDiv d = 1 in the backward), the runtime-window backward
with c/4 = 3, and one BIG case each way.  The index-type `long` instances need 2^31 element groups
(32 GiB of fp32) and are out of reach at test size.

Entry point -> kernels / template instances reached:
  tmr_splat_gap            splat_gap_k
  tmr_splat_combine        splat_combine_k, att written and att = NULL
  tmr_splat_bwd            splat_bwd_reduce_k
  tmr_splat_bwd_apply      splat_bwd_apply_k
  tmr_splat_gap_bn         splat_gap_bn_k<float>, splat_gap_bn_k<__bf16, 1024>
  tmr_splat_att            splat_att_k
  tmr_splat_combine_bn     splat_combine_bn_k<float>, splat_combine_bn_k<__bf16> (C % 8, C/8 not
                           dividing 256, or 8 bytes off), splat_combine_bn8_k
  tmr_splat_bwd_reduce_bn  splat_bwd_reduce_bn_k<float>, splat_bwd_reduce_bn_k<__bf16>
  tmr_splat_bn0_coefs      splat_bn0_coefs_k
  tmr_splat_bwd_apply_bn   splat_bwd_apply_bn_k<float>, splat_bwd_apply_bn_k<__bf16>,
                           splat_bwd_apply_bn8_k
  tmr_center_cols          center_cols_k
  tmr_axpy                 axpy_k
  tmr_avgpool2d_fwd        avgpool2d_fwd_k<uint32_t>
  tmr_avgpool2d_bwd        avgpool2d_bwd_fd_k<3, 2, 1>, <2, 2, 0>, <0, 0, 0>
  tmr_avgpool2d_fwd_a16    avgpool2d_fwd_a16_fd_k<3, 2, 1>, <2, 2, 0>, avgpool2d_fwd_a16_k<uint32_t>
  not reached: avgpool2d_fwd_k<long>, avgpool2d_bwd_k<long>, avgpool2d_fwd_a16_k<long>
"""
import numpy as np
import pytest
import torch

from tmrnet_amd import ops
from tmrnet_amd._lib import call, stream_ptr
from tests import _splat_ref as R
from tests._splat_ref import BF16, U, f32
from tests.test_bn_gpu import bf16_excess, up
from tests.test_head_gpu import guarded, guards_ok, no_nan, poison, rel_err  # noqa: F401

gpu = pytest.mark.gpu

NAN = float("nan")
SENT16 = 1024.0        # a sentinel bf16 holds exactly
MODES = [(False, False), (True, False), (True, True)]
MODE_IDS = ["fp32", "bf16", "bf16_off8"]


def guarded16(shape, dev, off):
    """`guarded` for bf16: the NaN-filled view 16-B aligned, or 8 bytes off -> (buffer, view, lead)"""
    n, lead = int(np.prod(shape)), 12 if off else 8
    buf = torch.full((lead + n + 8,), SENT16, dtype=BF16, device=dev)
    view = buf[lead:lead + n].view(shape)
    view.fill_(NAN)
    assert view.data_ptr() % 16 == (8 if off else 0)
    return buf, view, lead


def out_buf(shape, dev, bf16=False, off=False):
    """-> (view, ok): ok() tells whether the sentinels around the view survived"""
    if not bf16:
        buf, view = guarded(shape, dev)
        return view, lambda: guards_ok(buf)
    buf, view, lead = guarded16(shape, dev, off)
    n = view.numel()
    return view, lambda: bool((buf[:lead] == SENT16).all() and (buf[lead + n:] == SENT16).all())


def check(name, out, ref, bound):
    assert no_nan(out), name
    r = R.ratio(out, ref, bound)
    print("ratio %s %.4f" % (name, r))
    assert r <= 1.0, (name, r)


def att_sum_ok(att, C):
    a = att.double().cpu()
    return (a[:, :C] + a[:, C:] - 1).abs().max().item() <= 2 * U


def _case(shape, need="xy"):
    k = R.splat_case(*shape, need)
    return k, k["n"], k["hw"], k["C"]


# ------------------------------------------------------------------ unfused fp32 kernels
def _combine(dev, k, n, hw, C, x, with_att=True):
    out, ok = out_buf((n, hw, C), dev)
    att, ok_a = out_buf((n, 2 * C), dev)
    call("tmr_splat_combine", x, up(k["z"], dev), att if with_att else None, out, n, hw, C, stream_ptr())
    assert ok() and ok_a()
    return att, out


@gpu
@pytest.mark.parametrize("shape", R.SMALL)
def test_unfused(dev, shape):
    """tmr_splat_gap, tmr_splat_combine (att written and NULL), tmr_splat_bwd, tmr_splat_bwd_apply"""
    k, n, hw, C = _case(shape)
    x, att_in, dout, dgap = (up(k[name], dev) for name in ("x", "att", "dout", "dgap"))
    gap, ok = out_buf((n, C), dev)
    call("tmr_splat_gap", x, gap, n, hw, C, stream_ptr())
    assert ok()
    check("tmr_splat_gap", gap, *R.ref_gap(k["x"], C))
    ra, ro = R.ref_combine(k["x"], k["z"], C)
    att, out = _combine(dev, k, n, hw, C, x)
    check("tmr_splat_combine.att", att, *ra)
    check("tmr_splat_combine.out", out, *ro)
    assert att_sum_ok(att, C)
    untouched, out2 = _combine(dev, k, n, hw, C, x, with_att=False)
    assert torch.equal(out2, out) and bool(torch.isnan(untouched).all())
    dz, ok = out_buf((n, 2 * C), dev)
    call("tmr_splat_bwd", dout, x, att_in, dz, n, hw, C, stream_ptr())
    assert ok()
    check("tmr_splat_bwd", dz, *R.ref_bwd(k["dout"], k["x"], k["att"], C))
    dx, ok = out_buf((n, hw, 2 * C), dev)
    call("tmr_splat_bwd_apply", dout, att_in, dgap, dx, n, hw, C, stream_ptr())
    assert ok()
    check("tmr_splat_bwd_apply", dx, *R.ref_bwd_apply(k["dout"], k["att"], k["dgap"], hw))


@gpu
def test_unfused_big(dev):
    """splat_combine_k and splat_bwd_apply_k at (5, 29, 29, 512): the loops' second trip"""
    k, n, hw, C = _case(R.BIG_SCALAR, "x")
    x = up(k["x"], dev)
    _, ro = R.ref_combine(k["x"], k["z"], C)
    _, out = _combine(dev, k, n, hw, C, x)
    check("tmr_splat_combine.out", out, *ro)
    del ro
    dx, ok = out_buf((n, hw, 2 * C), dev)
    call("tmr_splat_bwd_apply", up(k["dout"], dev), up(k["att"], dev), up(k["dgap"], dev), dx, n, hw, C,
         stream_ptr())
    assert ok()
    check("tmr_splat_bwd_apply", dx, *R.ref_bwd_apply(k["dout"], k["att"], k["dgap"], hw))


@gpu
@pytest.mark.parametrize("n,C", [(s[0], s[3]) for s in R.SMALL] + [(7, 36), R.BIG_ATT])
def test_att(dev, poison, n, C):
    """tmr_splat_att: N(0, 3) logits with pairs that are equal, +-30 and +-100 apart (n C >= 36)"""
    z = R.logits(n, C, torch.Generator().manual_seed(n * 4099 + C))
    att = ops.splat_att(up(z, dev))
    check("tmr_splat_att", att, *R.ref_att(z, C))
    assert att_sum_ok(att, C)


# ------------------------------------------------------------------ bn0 + ReLU applied on load
def _bn_operands(dev, k, bf16, off):
    f = lambda name: up(k[name], dev)
    y = up(k["y"], dev, BF16 if bf16 else f32, off=off)
    return y, f("scale"), f("shift"), f("mean"), f("att"), f("dout"), f("dgap"), f("coef")


def _combine_bn(dev, k, n, hw, C, bf16, off):
    y, sc, sh, _, att, _, _, _ = _bn_operands(dev, k, bf16, off)
    out, ok = out_buf((n, hw, C), dev, bf16, off)
    call("tmr_splat_combine_bn", y, sc, sh, att, out, n, hw, C, int(bf16), stream_ptr())
    assert ok()
    check("tmr_splat_combine_bn." + ("bf16" if bf16 else "fp32"), out,
          *R.ref_combine_bn(k["y"], k["scale"], k["shift"], k["att"], C, bf16))


def _apply_bn(dev, k, n, hw, C, bf16, off):
    y, sc, sh, mean, att, dout, dgap, coef = _bn_operands(dev, k, bf16, off)
    dy, ok = out_buf((n, hw, 2 * C), dev, bf16, off)
    call("tmr_splat_bwd_apply_bn", dout, y, sc, sh, mean, att, dgap, coef, dy, n, hw, C, int(bf16),
         stream_ptr())
    assert ok()
    check("tmr_splat_bwd_apply_bn." + ("bf16" if bf16 else "fp32"), dy,
          *R.ref_bwd_apply_bn(k["dout"], k["y"], k["scale"], k["shift"], k["mean"], k["att"], k["dgap"],
                              k["coef"], hw, bf16))


def _coefs(dev, k, n, hw, C):
    """tmr_splat_bn0_coefs on the arbitrary sums of the case"""
    f = lambda name: up(k[name], dev)
    coef, ok = out_buf((3, 2 * C), dev)
    dgamma, ok_g = out_buf((2 * C,), dev)
    dbeta, ok_b = out_buf((2 * C,), dev)
    call("tmr_splat_bn0_coefs", f("att"), f("dgap"), f("sums"), f("mean"), f("invstd"), f("gamma"), coef,
         dgamma, dbeta, n, hw, C, stream_ptr())
    assert ok() and ok_g() and ok_b()
    ref = R.ref_bn0_coefs(k["att"], k["dgap"], k["sums"], k["invstd"], k["gamma"], n, hw, C)
    got = {"dgamma": dgamma, "dbeta": dbeta, "coef0": coef[0], "coef1": coef[1], "coef2": coef[2]}
    for name, rb in ref.items():
        check("tmr_splat_bn0_coefs." + name, got[name], *rb)


@gpu
@pytest.mark.parametrize("bf16,off", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", R.SMALL)
def test_bn_on_load(dev, shape, bf16, off):
    """tmr_splat_gap_bn, _combine_bn, _bwd_reduce_bn, _bn0_coefs, _bwd_apply_bn, each on the same y
    (a share of the pre-activations exactly 0) and otherwise arbitrary operands"""
    k, n, hw, C = _case(shape)
    y, sc, sh, mean, att, dout, _, _ = _bn_operands(dev, k, bf16, off)
    tag = "bf16" if bf16 else "fp32"
    gap, ok = out_buf((n, C), dev)
    call("tmr_splat_gap_bn", y, sc, sh, gap, n, hw, C, int(bf16), stream_ptr())
    assert ok()
    check("tmr_splat_gap_bn." + tag, gap, *R.ref_gap_bn(k["y"], k["scale"], k["shift"], C, bf16))
    _combine_bn(dev, k, n, hw, C, bf16, off)
    dzl, ok = out_buf((n, 2 * C), dev)
    sums, ok_s = out_buf((4, n, 2 * C), dev)
    call("tmr_splat_bwd_reduce_bn", dout, y, sc, sh, mean, att, dzl, sums, n, hw, C, int(bf16),
         stream_ptr())
    assert ok() and ok_s()
    rd, (rs, bs) = R.ref_bwd_reduce_bn(k["dout"], k["y"], k["scale"], k["shift"], k["mean"], k["att"], C,
                                       bf16)
    check("tmr_splat_bwd_reduce_bn.dzl." + tag, dzl, *rd)
    assert torch.equal(sums[1].double().cpu(), rs[1])
    for i in (0, 2, 3):
        check("tmr_splat_bwd_reduce_bn.S%d.%s" % (i + 1, tag), sums[i], rs[i], bs[i])
    if not off:
        _coefs(dev, k, n, hw, C)
    _apply_bn(dev, k, n, hw, C, bf16, off)


@gpu
@pytest.mark.parametrize("shape,bf16,off", [(R.BIG_4WIDE, False, False), (R.BIG_4WIDE, True, True),
                                            (R.BIG_8WIDE, True, False)],
                         ids=["4wide_fp32", "4wide_bf16_off8", "8wide"])
def test_bn_on_load_big(dev, shape, bf16, off):
    """the grid-stride kernels' second trip: splat_combine_bn_k / splat_bwd_apply_bn_k<float | __bf16>
    at (5, 29, 29, 2048), the 8-wide pair at (10, 29, 29, 2048), where the pixel a thread takes on its
    second trip lies in another frame than its first"""
    k, n, hw, C = _case(shape, "y")
    _combine_bn(dev, k, n, hw, C, bf16, off)
    _apply_bn(dev, k, n, hw, C, bf16, off)


@gpu
@pytest.mark.parametrize("n", R.ROWS)
@pytest.mark.parametrize("c2", R.COLS)
def test_bn0_coefs_rows_cols(dev, n, c2):
    """16 row groups: n = 1, 5 leave groups idle, 16 fills them, 17 and 33 take further trips; 2C = 8,
    48 a partial block of the 64 columns, 64 an exact one, 80 and 1024 more than one"""
    C, hw = c2 // 2, 49
    g = torch.Generator().manual_seed(n * 2000 + c2)
    k = dict(att=R.rnd(n, c2, g=g, scale=0.3, shift=0.5), dgap=R.rnd(n, C, g=g, scale=2.0),
             sums=R.rnd(4, n, c2, g=g, scale=float(hw)), mean=R.rnd(c2, g=g), invstd=R.pos(c2, g=g),
             gamma=R.rnd(c2, g=g, shift=0.3))
    _coefs(dev, k, n, hw, C)


@gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(5, 7, 7, 40), (6, 7, 7, 64)])
def test_closed_loop(dev, poison, shape, bf16):
    """reduce -> coefs -> apply with the true batch statistics of y, against float64 autograd through
    BatchNorm2d(train) -> ReLU of L = sum dout (att0 x0 + att1 x1) + sum dgap gap, att and dgap fixed:
    the S1..S4 decomposition without bn1's few-row amplification.  dy, dgamma, dbeta within the
    BatchNorm-backward bound of tests/test_bn_gpu.py (rel_err < 1e-5; bf16 dy: bf16_excess <= 1)."""
    k, n, hw, C = _case(shape)
    h, w = shape[1], shape[2]
    g = torch.Generator().manual_seed(sum(shape))
    gamma, beta = R.rnd(2 * C, g=g, shift=1.0), R.rnd(2 * C, g=g, scale=0.3)
    yr = k["y"].view(n, h, w, 2 * C).permute(0, 3, 1, 2).clone().requires_grad_(True)
    bn = torch.nn.BatchNorm2d(2 * C, eps=1e-5).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    x = torch.relu(bn(yr)).permute(0, 2, 3, 1).reshape(n, hw, 2 * C)
    a0, a1 = (t.unsqueeze(1) for t in R.halves(k["att"], C))
    gap = (x[..., :C] + x[..., C:]).mean(1)
    ((k["dout"] * (a0 * x[..., :C] + a1 * x[..., C:])).sum() + (k["dgap"] * gap).sum()).backward()
    dy64 = yr.grad.permute(0, 2, 3, 1).reshape(n, hw, 2 * C)

    f = lambda name: up(k[name], dev)
    mean, inv, scale, shift = ops.bn_fwd_train(f("y").view(n * hw, 2 * C), up(gamma, dev), up(beta, dev),
                                               None, None, 0.1, 1e-5)
    y = up(k["y"], dev, BF16 if bf16 else f32).view(n, h, w, 2 * C)
    dout = f("dout").view(n, h, w, C)
    _, sums = ops.splat_bwd_reduce_bn(dout, y, scale, shift, mean, f("att"))
    coef, dgamma, dbeta = ops.splat_bn0_coefs(f("att"), f("dgap"), sums, mean, inv, up(gamma, dev), hw)
    dy = ops.splat_bwd_apply_bn(dout, y, scale, shift, mean, f("att"), f("dgap"), coef)
    assert no_nan(dy) and dy.dtype == (BF16 if bf16 else f32)
    errs = rel_err(dgamma, bn.weight.grad), rel_err(dbeta, bn.bias.grad)
    if bf16:
        ex = bf16_excess(dy.view(n, hw, 2 * C), dy64, 1e-5)
        print("closed loop bf16 %s: dy excess %.4f dgamma %.3g dbeta %.3g" % (shape, ex, *errs))
        assert ex <= 1.0
    else:
        e = rel_err(dy.view(n, hw, 2 * C), dy64)
        print("closed loop fp32 %s: dy %.3g dgamma %.3g dbeta %.3g" % (shape, e, *errs))
        assert e < 1e-5
    assert max(errs) < 1e-5


# ------------------------------------------------------------------ centring, axpy
@gpu
@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("cols", R.COLS)
def test_center_cols(dev, rows, cols):
    """tmr_center_cols on rows = base + 1 % spread: center against the float64 mean, xc bitwise
    x - center (one fp32 subtraction)"""
    x = R.center_case(rows, cols)
    xd = up(x, dev)
    center, ok = out_buf((cols,), dev)
    xc, ok_x = out_buf((rows, cols), dev)
    call("tmr_center_cols", xd, rows, cols, center, xc, stream_ptr())
    assert ok() and ok_x()
    check("tmr_center_cols", center, *R.ref_center_cols(x))
    assert no_nan(xc) and torch.equal(xc, xd - center)


@gpu
@pytest.mark.parametrize("n", R.AXPY_N)
def test_axpy(dev, n):
    """tmr_axpy; n = 2^21 + 3 is three elements into the loop's second trip"""
    g = torch.Generator().manual_seed(n)
    x, y = R.rnd(n, g=g), R.rnd(n, g=g)
    alpha = float(torch.tensor(0.37, dtype=f32))
    buf, yd = guarded((n,), dev)
    yd.copy_(up(y, dev))
    call("tmr_axpy", n, alpha, up(x, dev), yd, stream_ptr())
    assert guards_ok(buf)
    check("tmr_axpy", yd, *R.ref_axpy(alpha, x, y))


@gpu
def test_axpy_nothing(dev):
    """n = 0 leaves y untouched"""
    y = torch.arange(8, dtype=f32, device=dev)
    call("tmr_axpy", 0, 2.0, torch.ones(8, device=dev), y, stream_ptr())
    assert torch.equal(y.cpu(), torch.arange(8, dtype=f32))


# ------------------------------------------------------------------ AvgPool2d
def _pool_fwd(dev, case, x64, bf16):
    n, h, w, c, k, s, p, incl, ceil = case
    ref, bound = R.ref_avgpool2d_fwd(x64, k, s, p, incl, ceil, bf16)
    y = ops.avgpool2d_fwd(up(x64, dev, BF16 if bf16 else f32), k, s, p, incl, ceil)
    assert tuple(y.shape) == tuple(ref.shape) and y.dtype == (BF16 if bf16 else f32)
    check("tmr_avgpool2d_fwd" + ("_a16" if bf16 else ""), y, ref, bound)
    return ref.shape[1:3]


def _pool_bwd(dev, case, dy64):
    n, h, w, c, k, s, p, incl, ceil = case
    dx = ops.avgpool2d_bwd(up(dy64, dev), (h, w), k, s, p, incl)
    check("tmr_avgpool2d_bwd", dx, *R.ref_avgpool2d_bwd(dy64, (h, w), k, s, p, incl, ceil))


@gpu
@pytest.mark.parametrize("case", R.POOL_SMALL)
def test_avgpool2d(dev, poison, case):
    """tmr_avgpool2d_fwd, _fwd_a16 and _bwd against F.avg_pool2d in float64 and its autograd"""
    x, x16, g = R.pool_case(case)
    ho, wo = _pool_fwd(dev, case, x, False)
    _pool_fwd(dev, case, x16, True)
    _pool_bwd(dev, case, R.rnd(case[0], ho, wo, case[3], g=g))


@gpu
def test_avgpool2d_big_fwd(dev, poison):
    """avgpool2d_fwd_k<uint32_t> and avgpool2d_fwd_a16_fd_k<2, 2, 0> at (33, 64, 64, 256): the
    second trip"""
    n, h, w, c = R.POOL_BIG_FWD[:4]
    x16 = R.rnd16(n, h, w, c, g=torch.Generator().manual_seed(1))      # bf16-exact: serves both
    _pool_fwd(dev, R.POOL_BIG_FWD, x16, False)
    _pool_fwd(dev, R.POOL_BIG_FWD, x16, True)


@gpu
def test_avgpool2d_big_bwd(dev, poison):
    """avgpool2d_bwd_fd_k<2, 2, 0> at (33, 32, 32, 256): the second trip"""
    n, h, w, c = R.POOL_BIG_BWD[:4]
    _pool_bwd(dev, R.POOL_BIG_BWD, R.rnd(n, h // 2, w // 2, c, g=torch.Generator().manual_seed(2)))


# ------------------------------------------------------------------ refused arguments
@gpu
def test_refused_arguments(dev):
    """C % 4 != 0 where the entry point checks it, n = 0 or hw = 0 on the `_bn` entry points,
    rows = 0 on tmr_center_cols: each fails with tmr_last_error's message, nothing is launched"""
    t = torch.zeros(64, device=dev)
    s = stream_ptr()
    with pytest.raises(RuntimeError, match="tmr_splat_gap: channels 6 must be a multiple of 4"):
        call("tmr_splat_gap", t, t, 1, 1, 6, s)
    with pytest.raises(RuntimeError, match="tmr_splat_bwd: channels 6 must be a multiple of 4"):
        call("tmr_splat_bwd", t, t, t, t, 1, 1, 6, s)
    for name in ("tmr_avgpool2d_fwd", "tmr_avgpool2d_bwd", "tmr_avgpool2d_fwd_a16"):
        with pytest.raises(RuntimeError, match=name + ": channels 6 must be a multiple of 4"):
            call(name, t, t, 1, 2, 2, 6, 1, 1, 2, 2, 0, 0, s)
    for n, hw, c in ((1, 1, 6), (0, 1, 4), (1, 0, 4)):
        for name, ptrs in (("tmr_splat_gap_bn", 4), ("tmr_splat_combine_bn", 5),
                           ("tmr_splat_bwd_reduce_bn", 8), ("tmr_splat_bwd_apply_bn", 9)):
            with pytest.raises(RuntimeError, match="%s: bad shape n %d hw %d c %d" % (name, n, hw, c)):
                call(name, *([t] * ptrs), n, hw, c, 0, s)
    for n, hw in ((0, 1), (1, 0)):
        with pytest.raises(RuntimeError, match="tmr_splat_bn0_coefs: bad shape n %d hw %d c 4" % (n, hw)):
            call("tmr_splat_bn0_coefs", t, t, t, t, t, t, t, t, t, n, hw, 4, s)
    with pytest.raises(RuntimeError, match="tmr_splat_att: bad shape n 0 c 4"):
        call("tmr_splat_att", t, t, 0, 4, s)
    with pytest.raises(RuntimeError, match="tmr_center_cols: bad shape 0x8"):
        call("tmr_center_cols", t, 0, 8, t, t, s)
    assert bool((t == 0).all())
