"""The clip-head kernels of csrc/head.hip, each entry point against a plain float64 CPU
computation of the same operation (torch / numpy, written here), at shapes other than the models'
own: odd sizes, more than one block, one step past the grid cap of the grid-stride kernels, the
tail switches of the column sums, every optional-pointer form, and tie rules on data that ties.

Bounds (stated per test): forward outputs of fp32 kernels rel_err < 3e-6 and backward outputs
rel_err < 1e-5 (max |a - b| / max |b|, the bounds of tests/test_kernels_gpu.py); operations that
only select or copy are compared with torch.equal.  Backward kernels are fed the float64
reference's saved tensors rounded to fp32, so their `> 0` masks equal the reference's by
construction.  Outputs a kernel must fully overwrite start as NaN; memory it must not touch holds
a sentinel that must survive.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tmrnet_amd import ops
from tmrnet_amd._lib import call, stream_ptr

gpu = pytest.mark.gpu

f64 = torch.float64
NAN = float("nan")
SENT = 12345.0
GUARD = 4                      # floats of sentinel on both sides (keeps 16-byte alignment)
LARGE = 8192 * 256 + 1000      # one step past the 8192-block cap of blocks_for (head.hip)
U = 2.0 ** -24                 # fp32 unit roundoff


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def rnd(*shape, g, scale=1.0, shift=0.0):
    """float64 values that fp32 holds exactly (both sides of a comparison see the same numbers)"""
    return (torch.randn(*shape, generator=g, dtype=f64) * scale + shift).float().double()


def guarded(shape, dev, fill=NAN, dtype=torch.float32, sent=SENT):
    """(buffer, view): `view` (contiguous, `shape`) holds `fill` and sits between sentinels"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), sent, dtype=dtype, device=dev)
    view = buf[GUARD:GUARD + n].view(shape)
    view.fill_(fill)
    return buf, view


def guards_ok(buf, sent=SENT):
    return bool((buf[:GUARD] == sent).all() and (buf[-GUARD:] == sent).all())


def strided(b, n, pad, dev, payload=None):
    """(wide, view): rows of n floats inside rows of n + pad; NaN everywhere but the payload"""
    wide = torch.full((b, n + pad), NAN, device=dev)
    view = wide[:, :n]
    if payload is not None:
        view.copy_(payload)
    return wide, view


def no_nan(t):
    return not bool(torch.isnan(t).any())


@pytest.fixture
def poison(monkeypatch):
    """The ops wrappers allocate their outputs with torch.empty / empty_like, which hand back
    whatever the caching allocator's block last held -- possibly the right answer of the previous
    case.  Within the test they hand out NaN (floats), 0xff bytes or -1 instead, so an element a
    kernel skips is seen."""
    real_empty, real_like = torch.empty, torch.empty_like

    def fill(t):
        if t.is_floating_point():
            t.fill_(NAN)
        elif t.dtype == torch.uint8:
            t.fill_(255)
        elif t.dtype != torch.bool:
            t.fill_(-1)
        return t

    monkeypatch.setattr(torch, "empty", lambda *a, **k: fill(real_empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: fill(real_like(*a, **k)))


# ------------------------------------------------------------------ 1. LayerNorm + ReLU
LN_CASES = [(1, 512), (5, 512), (7, 64), (3, 100), (9, 33), (6, 1024)]
LN_EPS = 1e-5


def _ln_ref(rows, D):
    g = torch.Generator().manual_seed(rows * 10000 + D)
    x = rnd(rows, D, g=g, scale=3.0, shift=5.0)     # row offset: the mean matters
    gamma, beta, dy = rnd(D, g=g), rnd(D, g=g), rnd(rows, D, g=g)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    y = torch.relu(F.layer_norm(xr, (D,), gr, br, LN_EPS))
    y.backward(dy)
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False) + LN_EPS)
    return x, gamma, beta, dy, y.detach(), mean, rstd, xr.grad, gr.grad, br.grad


@gpu
@pytest.mark.parametrize("rows,D", LN_CASES)
def test_layernorm_relu(dev, poison, rows, D):
    """tmr_layernorm_relu_fwd/bwd vs F.layer_norm + relu in float64 (autograd): D not a multiple
    of 64 (100, 33), rows not a multiple of the 4 rows of a workgroup.  y, mean, rstd < 3e-6;
    dx, dgamma, dbeta < 1e-5, the backward reading the reference's y, mean, rstd."""
    x, gamma, beta, dy, y64, mean64, rstd64, dx64, dg64, db64 = _ln_ref(rows, D)
    d = lambda t: t.float().to(dev)
    y, mean, rstd = ops.layernorm_relu_fwd(d(x), d(gamma), d(beta), LN_EPS)
    assert no_nan(y) and no_nan(mean) and no_nan(rstd)
    assert rel_err(y, y64) < 3e-6
    assert rel_err(mean, mean64) < 3e-6
    assert rel_err(rstd, rstd64) < 3e-6
    assert torch.equal(y.cpu() > 0, y64 > 0)
    dx, dg, db = ops.layernorm_relu_bwd(d(dy), d(x), d(y64), d(gamma), d(mean64), d(rstd64))
    assert no_nan(dx) and no_nan(dg) and no_nan(db)
    assert rel_err(dx, dx64) < 1e-5
    assert rel_err(dg, dg64) < 1e-5
    assert rel_err(db, db64) < 1e-5


@gpu
def test_layernorm_relu_bwd_without_param_grads(dev):
    """dgamma = dbeta = NULL: dx bit for bit that of the full call; dgamma alone / dbeta alone
    equal the full call's."""
    rows, D = 9, 33
    x, gamma, beta, dy, y64, mean64, rstd64, dx64, _, _ = _ln_ref(rows, D)
    d = lambda t: t.float().to(dev)
    args = [d(dy), d(x), d(y64), d(gamma), d(mean64), d(rstd64)]
    dx, dg, db = ops.layernorm_relu_bwd(*args)
    buf, dx2 = guarded((rows, D), dev)
    call("tmr_layernorm_relu_bwd", *args, dx2, None, None, rows, D, stream_ptr())
    assert no_nan(dx2) and guards_ok(buf)
    assert torch.equal(dx2, dx)
    assert rel_err(dx2, dx64) < 1e-5
    bg, dg2 = guarded((D,), dev)
    bb, db2 = guarded((D,), dev)
    call("tmr_layernorm_relu_bwd", *args, dx2, dg2, None, rows, D, stream_ptr())
    call("tmr_layernorm_relu_bwd", *args, dx2, None, db2, rows, D, stream_ptr())
    assert torch.equal(dg2, dg) and torch.equal(db2, db)
    assert guards_ok(bg) and guards_ok(bb)


# ------------------------------------------------------------------ 2. column sums
@gpu
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 112, 113, 127, 128, 129, 1000])
def test_col_sum(dev, rows):
    """tmr_col_sum around the edges of its loops (16 row lanes; the 8-deep unrolled loop runs
    while r + 112 < rows), ld = cols + 3 with NaN in the padding columns.  beta = 0 must not read
    the NaN-filled `out`; beta = 1, 0.5 against beta*out + colsum.  rel_err < 3e-6 (the entries
    have mean 1, so a sum of `rows` of them does not cancel)."""
    for cols in (1, 7, 16, 17, 512):
        g = torch.Generator().manual_seed(rows * 1000 + cols)
        ld = cols + 3
        x = rnd(rows, ld, g=g, shift=1.0)
        s64 = x[:, :cols].sum(0)
        x[:, cols:] = NAN
        xd = x.float().to(dev)
        buf, out = guarded((cols,), dev)
        ops.col_sum(xd, rows, cols, ld, out=out, beta=0.0)
        assert bool(torch.isfinite(out).all()), cols
        assert guards_ok(buf), cols
        assert rel_err(out, s64) < 3e-6, cols
        for beta in (1.0, 0.5):
            o0 = rnd(cols, g=g)
            buf, out = guarded((cols,), dev)
            out.copy_(o0)
            ops.col_sum(xd, rows, cols, ld, out=out, beta=beta)
            assert guards_ok(buf), (cols, beta)
            assert rel_err(out, beta * o0 + s64) < 3e-6, (cols, beta)


# ------------------------------------------------------------------ 3. dropout mask
def _mask_ref(n, p, seed, offset):
    """The generator documented at dropout_mask_k: h = splitmix64 finaliser of
    seed*0x9e3779b97f4a7c15 + offset + i; u = (h >> 40) * 2^-24 as fp32; keep iff u >= fp32(p);
    kept elements hold fp32 1/(1-p), the others 0.  All arithmetic modulo 2^64."""
    u64 = np.uint64
    i = np.arange(n, dtype=np.uint64)
    z = np.array([seed], dtype=np.uint64) * u64(0x9e3779b97f4a7c15) + u64(offset) + i
    z = (z ^ (z >> u64(30))) * u64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> u64(27))) * u64(0x94d049bb133111eb)
    h = z ^ (z >> u64(31))
    u = (h >> u64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert scale == np.float32(1.0 / (1.0 - p))
    return np.where(u >= np.float32(p), scale, np.float32(0.0)).astype(np.float32)


def _keep_count_ok(m, n, p):
    """|kept - n(1-p)| <= 6 sqrt(n p (1-p)): six standard deviations of the binomial count"""
    return abs(int(np.count_nonzero(m)) - n * (1.0 - p)) <= 6.0 * (n * p * (1.0 - p)) ** 0.5


SEEDS = (0, 1, 2 ** 63 + 5)


def test_dropout_mask_replica_statistics():
    """The numpy replica alone: values and keep counts (needs no device)."""
    n = 1 << 20
    for p in (0.2, 0.5):
        for seed in SEEDS:
            m = _mask_ref(n, p, seed, 0)
            assert set(np.unique(m).tolist()) == {0.0, float(np.float32(1.0 / (1.0 - p)))}
            assert _keep_count_ok(m, n, p), (p, seed)
    assert (_mask_ref(1000, 0.0, 7, 0) == 1.0).all()


def _mask_gpu(dev, n, p, seed, offset):
    like = torch.empty(1, device=dev)
    return ops.dropout_mask(n, p, seed, offset, like).cpu().numpy()


@gpu
def test_dropout_mask_bits(dev, poison):
    """Bit equality with the replica over p, seed (one past 2^63) and n (one element, one past a
    block, one step past the grid cap); only the values 0 and fp32 1/(1-p) occur."""
    for n in (1, 257):
        for p in (0.0, 0.2, 0.5):
            for seed in SEEDS:
                m = _mask_gpu(dev, n, p, seed, 0)
                assert np.array_equal(m, _mask_ref(n, p, seed, 0)), (n, p, seed)
    for p, seed in ((0.0, 1), (0.2, 2 ** 63 + 5), (0.5, 0)):
        m = _mask_gpu(dev, LARGE, p, seed, 0)
        assert np.array_equal(m, _mask_ref(LARGE, p, seed, 0)), (p, seed)
        assert np.isin(m, [0.0, np.float32(1.0 / (1.0 - p))]).all()


@gpu
def test_dropout_mask_offset_and_count(dev, poison):
    """mask(n, offset=k)[i] == mask(n + k, offset=0)[i + k] (also for an offset past 2^32, against
    the replica), and the keep count over 2^20 elements within six binomial sigmas."""
    n, k = 5000, 1000
    for p, seed in ((0.2, 3), (0.5, 2 ** 63 + 5)):
        a = _mask_gpu(dev, n, p, seed, k)
        b = _mask_gpu(dev, n + k, p, seed, 0)
        assert np.array_equal(a, b[k:])
        big = 2 ** 40 + 3
        assert np.array_equal(_mask_gpu(dev, n, p, seed, big), _mask_ref(n, p, seed, big))
    n = 1 << 20
    for p in (0.2, 0.5):
        m = _mask_gpu(dev, n, p, 11, 0)
        assert _keep_count_ok(_mask_ref(n, p, 11, 0), n, p)
        assert _keep_count_ok(m, n, p), p
    assert (_mask_gpu(dev, n, 0.0, 11, 0) == 1.0).all()


# ------------------------------------------------------------------ 4. elementwise glue
def _within_ulp(out, ref64):
    """|out - ref| <= 2^-23 |ref|: at most two fp32 roundings, each within 2^-24/(1 + 2^-24)
    relative (one if the compiler contracts base + z*m into an fma); no operand cancels (see the
    data) and none is subnormal"""
    o = out.detach().double().cpu()
    return bool(((o - ref64).abs() <= 2.0 ** -23 * ref64.abs()).all())


def _glue_data(n, seed):
    """base and z share their sign element by element and the mask is >= 0, so base + z*mask
    never cancels: its two roundings stay within 2^-23 of the result"""
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    base = ((rnd(n, g=g).abs() + 2.0 ** -10) * sign).float().double()
    z = ((rnd(n, g=g).abs() + 2.0 ** -10) * sign).float().double()
    mask = torch.randint(0, 2, (n,), generator=g).double() * 2.0     # dropout(0.5): 0 or 2
    return base, z, mask


@gpu
@pytest.mark.parametrize("n", [1, 255, 257, LARGE])
def test_residual_mask_and_mask_relu(dev, poison, n):
    """tmr_residual_mask, tmr_mask_relu_fwd/bwd with and without the mask, vs float64 within one
    fp32 ulp (2^-23) of the result's magnitude; LARGE runs the grid-stride loops a second time.
    mask_relu_bwd reads the reference's `a`, exact zeros included: a == 0 passes no gradient."""
    base, z, mask = _glue_data(n, n)
    d = lambda t: t.float().to(dev)
    for m in (None, mask):
        mm = 1.0 if m is None else m
        md = None if m is None else d(m)
        out = ops.residual_mask(d(base), d(z), md)
        assert no_nan(out) and _within_ulp(out, base + z * mm)
        h = z                                       # both signs
        a64 = torch.relu(h * mm)
        a = ops.mask_relu_fwd(d(h), md)
        assert no_nan(a) and _within_ulp(a, a64)
        assert torch.equal(a.cpu() > 0, a64 > 0)
        da = base
        dh = ops.mask_relu_bwd(d(da), d(a64), md)
        assert bool((a64 == 0).any()) or n == 1
        assert no_nan(dh) and _within_ulp(dh, torch.where(a64 > 0, da * mm, torch.zeros_like(da)))


@gpu
@pytest.mark.parametrize("n", [1, 255, 257, LARGE])
def test_mul(dev, n):
    """tmr_mul: a, a*b, a*s, a*b*s vs float64 within 2^-23 of the result (two roundings); the
    output sits between sentinels."""
    g = torch.Generator().manual_seed(n + 1)
    a, b = rnd(n, g=g), rnd(n, g=g)
    s = rnd(1, g=g, shift=3.0)
    d = lambda t: t.float().to(dev)
    for bb in (None, b):
        for ss in (None, s):
            buf, out = guarded((n,), dev)
            ops.mul(d(a), None if bb is None else d(bb), None if ss is None else d(ss), out=out)
            ref = a * (1.0 if bb is None else bb) * (1.0 if ss is None else ss)
            assert no_nan(out) and guards_ok(buf)
            assert _within_ulp(out, ref), (bb is None, ss is None)


# ------------------------------------------------------------------ 5. last step of each clip
@gpu
@pytest.mark.parametrize("b,t,h", [(3, 1, 8), (5, 7, 512), (64, 10, 512)])
def test_seq_last(dev, b, t, h):
    """tmr_seq_last == y[:, -1]; tmr_seq_last_bwd == d1 (+ d2) scattered to the last step, zeros
    elsewhere, over a NaN-filled dy -- exact (one fp32 add at most)."""
    g = torch.Generator().manual_seed(b * 100 + t)
    y = torch.randn(b, t, h, generator=g)
    d1, d2 = torch.randn(b, h, generator=g), torch.randn(b, h, generator=g)
    buf, out = guarded((b, h), dev)
    call("tmr_seq_last", y.to(dev), out, b, t, h, stream_ptr())
    assert guards_ok(buf)
    assert torch.equal(out.cpu(), y[:, -1])
    for dd in (None, d2):
        buf, dy = guarded((b, t, h), dev)
        call("tmr_seq_last_bwd", d1.to(dev), None if dd is None else dd.to(dev), dy, b, t, h,
             stream_ptr())
        ref = torch.zeros(b, t, h)
        ref[:, -1] = d1 if dd is None else d1 + dd
        assert guards_ok(buf)
        assert torch.equal(dy.cpu(), ref)


# ------------------------------------------------------------------ 6. LSTM cell
def _lstm_cell_ref(b, h, first, with_rec, with_dcn):
    g = torch.Generator().manual_seed(b * 1000 + h + 7 * first + 3 * with_rec + with_dcn)
    gx = rnd(b, 4 * h, g=g, scale=2.0)
    ghh = None if first else rnd(b, 4 * h, g=g)
    cp = None if first else rnd(b, h, g=g)
    dho = rnd(b, h, g=g)
    dhr = rnd(b, h, g=g) if with_rec else None
    dcn = rnd(b, h, g=g) if with_dcn else None
    pre = (gx if first else gx + ghh).clone().requires_grad_(True)
    cpr = (torch.zeros(b, h, dtype=f64) if first else cp.clone()).requires_grad_(True)
    i, f, gg, o = pre.split(h, dim=1)
    i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
    c = f * cpr + i * gg
    hh = o * torch.tanh(c)
    loss = (hh * (dho if dhr is None else dho + dhr)).sum()
    if dcn is not None:
        loss = loss + (c * dcn).sum()
    loss.backward()
    act = torch.cat([i, f, gg, o], 1).detach()
    return dict(gx=gx, ghh=ghh, cp=cp, dho=dho, dhr=dhr, dcn=dcn, h=hh.detach(), c=c.detach(),
                act=act, dg=pre.grad, dcp=cpr.grad)


@gpu
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("b,h", [(1, 32), (5, 100), (3, 512)])
def test_lstm_cell_fwd(dev, b, h, first):
    """tmr_lstm_cell_fwd vs the i,f,g,o equations in float64: first-step form (ghh, c_prev NULL)
    and later-step form, act saved and NULL (inference).  gx and h_out are row-strided views of
    wider tensors whose gaps hold NaN: the gaps keep it, the payload loses it.  < 3e-6."""
    r = _lstm_cell_ref(b, h, first, False, False)
    d = lambda t: None if t is None else t.float().to(dev)
    gxw, gx = strided(b, 4 * h, 5, dev, r["gx"].float())
    outs = []
    for save in (True, False):
        hw, hv = strided(b, h, 3, dev)
        bc, c = guarded((b, h), dev)
        ba, act = guarded((b, 4 * h), dev, fill=NAN if save else SENT)
        ops.lstm_cell_fwd(gx, d(r["ghh"]), d(r["cp"]), hv, c, act if save else None)
        assert no_nan(hv) and bool(torch.isnan(hw[:, h:]).all())
        assert bool(torch.isnan(gxw[:, 4 * h:]).all())
        assert no_nan(c) and guards_ok(bc) and guards_ok(ba)
        assert rel_err(hv, r["h"]) < 3e-6
        assert rel_err(c, r["c"]) < 3e-6
        if save:
            assert no_nan(act) and rel_err(act, r["act"]) < 3e-6
        else:
            assert bool((act == SENT).all())
        outs.append((hv.clone(), c.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@gpu
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("with_rec,with_dcn", [(False, False), (True, False), (False, True),
                                               (True, True)])
@pytest.mark.parametrize("b,h", [(1, 32), (5, 100), (3, 512)])
def test_lstm_cell_bwd(dev, b, h, first, with_rec, with_dcn):
    """tmr_lstm_cell_bwd vs float64 autograd of the cell, reading the reference's act and c
    rounded to fp32: dh_rec / dc_next / c_prev NULL and given; dh_out and dgates row-strided with
    NaN gaps that must survive.  dgates, dc_prev < 1e-5."""
    r = _lstm_cell_ref(b, h, first, with_rec, with_dcn)
    d = lambda t: None if t is None else t.float().to(dev)
    dhw, dho = strided(b, h, 3, dev, r["dho"].float())
    dgw, dg = strided(b, 4 * h, 5, dev)
    buf, dcp = guarded((b, h), dev)
    ops.lstm_cell_bwd(dho, d(r["dhr"]), d(r["dcn"]), d(r["act"]), d(r["c"]), d(r["cp"]), dg, dcp)
    assert no_nan(dg) and bool(torch.isnan(dgw[:, 4 * h:]).all())
    assert bool(torch.isnan(dhw[:, h:]).all())
    assert no_nan(dcp) and guards_ok(buf)
    assert rel_err(dg, r["dg"]) < 1e-5
    assert rel_err(dcp, r["dcp"]) < 1e-5
    if first:
        assert bool((dg[:, h:2 * h] == 0).all())     # no previous cell state: no forget-gate grad


# ------------------------------------------------------------------ 7. cross-entropy sum
def _ce_data(b, k):
    g = torch.Generator().manual_seed(b * 10 + k)
    x = torch.randn(b, k, generator=g, dtype=f64) * 3
    r = torch.arange(b)
    x[r % 3 == 1] += 1e4                      # the max subtraction must carry these
    x[r % 3 == 2] -= 1e4
    x = x.float().double()
    if k >= 2:
        for i in range(0, b, 5):              # the maximum twice, the second copy anywhere else
            j = int(x[i].argmax())
            x[i, (j + 1 + (i // 5) % (k - 1)) % k] = x[i, j]
    for i in range(3, b, 7):                  # all-equal rows
        x[i] = x[i, 0]
    y = torch.randint(0, k, (b,), generator=g)
    w = (torch.rand(k, generator=g, dtype=f64) + 0.5).float().double()
    return x, y, w


@gpu
@pytest.mark.parametrize("k", [1, 2, 7])
@pytest.mark.parametrize("b", [1, 255, 257, 1000])
def test_ce_sum_shapes(dev, poison, b, k):
    """tmr_ce_sum vs float64 F.cross_entropy(reduction='sum') with autograd: b past the 256
    threads of its one workgroup (the i += blockDim.x loop), logits offset by +-1e4, repeated
    maxima and all-equal rows (preds = the first maximum, numpy argmax), weight / no weight,
    gscale 1 and 0.25; want_grad=False gives the same loss and preds.
    Loss bound, derived: the kernel adds b fp32 terms serially, each w*(lse - x_label) itself a
    few roundings of numbers of size |lse|, |x_label|:
        |loss - loss64| <= (b + 16) * 2^-24 * sum_i w_i (|lse_i| + |x_i,label|).
    dlogits: rel_err < 1e-5."""
    x, y, w = _ce_data(b, k)
    xd, yd = x.float().to(dev), y.to(dev)
    preds64 = torch.from_numpy(np.argmax(x.numpy(), axis=1))
    lse = torch.logsumexp(x, 1)
    xlab = x.gather(1, y[:, None])[:, 0]
    if k >= 2 and b >= 10:
        srt = x.sort(1, descending=True).values
        assert int((srt[:, 0] == srt[:, 1]).sum()) >= b // 5      # the data does tie
        assert int((preds64 > 0).sum()) > 0
    for wt in (None, w):
        wi = torch.ones(b, dtype=f64) if wt is None else wt[y]
        bound = (b + 16) * U * float((wi * (lse.abs() + xlab.abs())).sum())
        for gscale in (1.0, 0.25):
            xr = x.clone().requires_grad_(True)
            l64 = F.cross_entropy(xr, y, weight=wt, reduction="sum")
            (l64 * gscale).backward()
            wd = None if wt is None else wt.float().to(dev)
            loss, dl, preds = ops.ce_sum(xd, yd, wd, gscale=gscale)
            err = abs(loss.item() - l64.item())
            print("ce_sum b=%d k=%d w=%s g=%g: |dloss| %.3g bound %.3g dl %.3g"
                  % (b, k, wt is not None, gscale, err, bound, rel_err(dl, xr.grad)))
            assert err <= bound
            assert no_nan(dl) and rel_err(dl, xr.grad) < 1e-5
            assert torch.equal(preds.cpu(), preds64)
            loss2, dl2, preds2 = ops.ce_sum(xd, yd, wd, gscale=gscale, want_grad=False)
            assert dl2 is None
            assert torch.equal(loss2, loss) and torch.equal(preds2, preds)


# ------------------------------------------------------------------ 8. TimeConv max-of-5
def _max5_ref(x, y1, y2, y3):
    """(out, code, prev): stack order (x, y1, y2, y3, pooled), argmax takes the first maximum;
    the pooled branch is prev unless x > prev (then it is x, and ties with the identity, which
    comes first).  prev = x[t-1], the zero pad at t = 0."""
    prev = np.concatenate([np.zeros_like(x[:, :1]), x[:, :-1]], axis=1)
    pooled = np.where(x > prev, x, prev)
    st = np.stack([x, y1, y2, y3, pooled])
    return st.max(0), st.argmax(0).astype(np.uint8), prev


def _max5_bwd_ref(dy, code, x, prev):
    """branches 1-3 -> d1..d3; identity -> dx[t]; pooled -> dx[t] if x > prev else dx[t-1],
    dropped at t = 0.  fp32 throughout: dx[t] is one IEEE add of two routed values."""
    zero = np.float32(0)
    d = [np.where(code == c, dy, zero) for c in (1, 2, 3)]
    pool = np.where(code == 4, dy, zero)
    to_t = np.where(x > prev, pool, zero)
    to_prev = np.where(x > prev, zero, pool)
    dx = np.where(code == 0, dy, zero) + to_t
    dx[:, :-1] = dx[:, :-1] + to_prev[:, 1:]
    return d[0], d[1], d[2], dx


def _max5_data(b, L, C):
    rng = np.random.default_rng(b * 100 + L * 10 + C)
    x, y1, y2, y3 = (rng.integers(-2, 3, (b, L, C)).astype(np.float32) for _ in range(4))
    dy = rng.standard_normal((b, L, C)).astype(np.float32)
    return x, y1, y2, y3, dy


MAX5_CASES = [(2, 1, 3), (2, 2, 8), (3, 5, 512)]


def _tie_share(x, y1, y2, y3, prev):
    top = np.sort(np.stack([x, y1, y2, y3, prev]), axis=0)
    return float((top[-1] == top[-2]).mean())


def test_max5_reference_ties():
    """The integer data ties (needs no device): the top two of (x, y1, y2, y3, prev) are equal in
    at least 10% of the elements of every case; x[t] == x[t-1] and x[0] <= 0 both occur."""
    for b, L, C in MAX5_CASES:
        x, y1, y2, y3, _ = _max5_data(b, L, C)
        _, code, prev = _max5_ref(x, y1, y2, y3)
        assert _tie_share(x, y1, y2, y3, prev) >= 0.10
        assert (x[:, 0] <= 0).any()
        assert not ((code == 4) & (x > prev)).any()
    x, _, _, _, _ = _max5_data(3, 5, 512)
    assert (x[:, 1:] == x[:, :-1]).mean() > 0.1


@gpu
@pytest.mark.parametrize("b,L,C", MAX5_CASES)
def test_timeconv_max5(dev, b, L, C):
    """tmr_timeconv_max5_fwd/bwd on inputs drawn from the integers -2..2, so every pair of
    branches ties often: out, the branch code, d1..d3 and dx equal the numpy reference exactly;
    dx == NULL leaves d1..d3 identical."""
    x, y1, y2, y3, dy = _max5_data(b, L, C)
    out64, code_ref, prev = _max5_ref(x, y1, y2, y3)
    assert _tie_share(x, y1, y2, y3, prev) >= 0.10
    t = lambda a: torch.from_numpy(a).to(dev)
    bo, out = guarded((b, L, C), dev)
    bc, code = guarded((b, L, C), dev, fill=255, dtype=torch.uint8, sent=77)
    call("tmr_timeconv_max5_fwd", t(x), t(y1), t(y2), t(y3), out, code, b, L, C, stream_ptr())
    assert guards_ok(bo) and guards_ok(bc, 77)
    assert torch.equal(out.cpu(), torch.from_numpy(out64))
    assert torch.equal(code.cpu(), torch.from_numpy(code_ref))
    refs = _max5_bwd_ref(dy, code_ref, x, prev)
    got = []
    for want_dx in (True, False):
        bufs = [guarded((b, L, C), dev) for _ in range(4)]
        d1, d2, d3, dx = (v for _, v in bufs)
        call("tmr_timeconv_max5_bwd", t(dy), t(code_ref), d1, d2, d3, dx if want_dx else None,
             b, L, C, stream_ptr())
        assert all(guards_ok(bf) for bf, _ in bufs)
        for v, r in zip((d1, d2, d3), refs[:3]):
            assert torch.equal(v.cpu(), torch.from_numpy(r))
        if want_dx:
            assert torch.equal(dx.cpu(), torch.from_numpy(refs[3]))
        else:
            assert bool(torch.isnan(dx).all())
        got.append((d1, d2, d3))
    for a, c in zip(*got):
        assert torch.equal(a, c)


# ------------------------------------------------------------------ 11. small ones
SGD_CASES = [
    # n, momentum, dampening, weight decay, nesterov
    (1000, 0.0, 0.0, 0.0, False),
    (1000, 0.0, 0.0, 5e-4, False),
    (1000, 0.9, 0.0, 0.0, False),
    (1000, 0.9, 0.1, 0.0, False),
    (1000, 0.9, 0.0, 5e-4, True),
    (LARGE, 0.9, 0.1, 5e-4, False),
]


@gpu
@pytest.mark.parametrize("n,mom,damp,wd,nesterov", SGD_CASES)
def test_sgd_step_single_tensor(dev, n, mom, damp, wd, nesterov):
    """tmr_sgd_step (the single-tensor kernel) over three steps -- the first (buf = d) and two
    later ones -- vs torch.optim.SGD on a float64 parameter; momentum 0 passes buf = NULL.
    p and the momentum buffer rel_err < 1e-6 (tests/test_kernels_gpu.py::test_sgd_matches_torch)."""
    g = torch.Generator().manual_seed(n + int(mom * 10) + int(damp * 100) + nesterov)
    p0 = rnd(n, g=g)
    grads = [rnd(n, g=g) for _ in range(3)]
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([pr], lr=0.1, momentum=mom, dampening=damp, weight_decay=wd,
                          nesterov=nesterov)
    bp, p = guarded((n,), dev)
    p.copy_(p0)
    bb, buf = guarded((n,), dev)
    for step, gr in enumerate(grads):
        pr.grad = gr.clone()
        opt.step()
        ops.sgd_step(p, gr.float().to(dev), buf if mom else None, 0.1, mom, damp, wd, nesterov,
                     step == 0)
    assert guards_ok(bp) and guards_ok(bb)
    assert rel_err(p, pr) < 1e-6
    if mom:
        assert rel_err(buf, opt.state[pr]["momentum_buffer"]) < 1e-6
    else:
        assert bool(torch.isnan(buf).all())


@gpu
@pytest.mark.parametrize("nrows,d", [(37, 4), (300, 512), (5000, 2048)])
def test_lfb_gather_shapes(dev, poison, nrows, d):
    """tmr_lfb_gather == bank[rows] for repeated and out-of-order rows; 5000 x 2048 puts
    nrows*d/4 past the grid cap."""
    g = torch.Generator().manual_seed(nrows + d)
    bank = torch.randn(211, d, generator=g)
    rows = torch.randint(0, 211, (nrows,), generator=g, dtype=torch.int32)
    rows[:3] = 210
    rows[-2:] = 0
    out = ops.lfb_gather(bank.to(dev), rows.to(dev))
    assert torch.equal(out.cpu(), bank[rows.long()])


@gpu
def test_lfb_gather_rejects_odd_width(dev):
    bank = torch.zeros(8, 6, device=dev)
    rows = torch.zeros(2, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError):
        ops.lfb_gather(bank, rows)


@gpu
@pytest.mark.parametrize("n", [1, 257])
def test_fill_f32(dev, n):
    buf, x = guarded((n,), dev)
    call("tmr_fill_f32", x, ctypes.c_long(n), 2.5, stream_ptr())
    assert guards_ok(buf) and bool((x == 2.5).all())
    call("tmr_fill_f32", x, ctypes.c_long(0), 7.0, stream_ptr())
    assert bool((x == 2.5).all())


@gpu
def test_counters_add(dev):
    """tmr_counters_add over 300 counters (past one 256-thread block), v = 1 (the wrapper) and
    v = 5; the counters after the table's end keep their values."""
    c = torch.arange(304, dtype=torch.int64, device=dev) * 3
    ops.counters_add_one([c[i] for i in range(300)])
    torch.cuda.synchronize()
    exp = torch.arange(304, dtype=torch.int64) * 3
    exp[:300] += 1
    assert torch.equal(c.cpu(), exp)
    tab = (c.data_ptr() + 8 * torch.arange(300, dtype=torch.int64)).to(dev)
    call("tmr_counters_add", tab, 300, 5, stream_ptr())
    exp[:300] += 5
    assert torch.equal(c.cpu(), exp)
