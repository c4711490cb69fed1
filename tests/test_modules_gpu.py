"""Module-level C entry points (include/tmr.h: tmr_lstm_*, tmr_nlblock_*, tmr_timeconv_*,
tmr_linear_*) against float64 torch, and their two execution paths.

* tmr_lstm_fwd/bwd: the persistent one-launch recurrence (hidden 512; grid 64 x ceil(B/16)
  workgroups behind a grid barrier) and the per-step path it falls back to (TMR_LSTM_PERSIST=0,
  other hidden sizes, or a grid the cooperative launch refuses: B > 64 at one workgroup per CU)
  -- both against nn.LSTM in float64 (train_only_non-local_pretrained.py:215, :230-231), and the
  barrier's timeout word must read 0; a barrier give-up (forced, or caused by a kernel resident
  on another stream) is recomputed by the solo kernels, bit-identical.
* tmr_nl_attn split over 32-row chunks at the C5 shape (B=64, L=300, bank rows) against float64,
  at every advertised width (256, 512, 1024), with scores spanning +-60 (the online-softmax
  rescale) and with all scores equal.
* tmr_timeconv_fwd/wgrad at L = 1, 2, 7 against TimeConvRef in float64 under autograd.
* tmr_linear_fwd/bwd against float64 nn.Linear.
"""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import tmrnet_ref as ref
from tmrnet_amd import ops
from tmrnet_amd._lib import call, stream_ptr
from tmrnet_amd.lstm import LSTM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _lstm_case(dev, B, T, I, H, seed):
    torch.manual_seed(seed)
    ref = torch.nn.LSTM(I, H, batch_first=True).double()
    m = LSTM(I, H).to(dev)
    m.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    x = torch.randn(B, T, I, dtype=torch.float64)
    dy = torch.randn(B, T, H, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    yr, (hr, cr) = ref(xr)
    yr.backward(dy)
    xd = x.float().to(dev).requires_grad_(True)
    y, (hn, cn) = m(xd)
    y.backward(dy.float().to(dev))
    torch.cuda.synchronize()
    assert rel(y, yr) < 5e-6
    assert rel(hn, hr) < 5e-6 and rel(cn, cr) < 5e-6
    assert rel(xd.grad, xr.grad) < 2e-5
    for (n1, p1), (n2, p2) in zip(m.named_parameters(), ref.named_parameters()):
        assert n1 == n2
        assert rel(p1.grad, p2.grad) < 2e-5, n1


@pytest.mark.parametrize("persist", ["1", "0"])
@pytest.mark.parametrize("B,T", [(64, 10), (5, 30), (1, 1), (100, 3)])
def test_lstm_entry_points(dev, monkeypatch, persist, B, T):
    """Hidden 512 as in the reference; B=64 x T=10 is C2's clip batch (4 workgroup rows of 16
    clips, the persistent grid fills 256 CUs), B=100 needs 7 rows (448 > 256 workgroups): the
    cooperative launch refuses it and the per-step path runs."""
    monkeypatch.setenv("TMR_LSTM_PERSIST", persist)
    _lstm_case(dev, B, T, 256, 512, seed=B * 100 + T)


def test_lstm_persistent_barrier_status(dev):
    """The timeout word of the grid barrier stays 0 over a full C2-shaped forward + backward, and
    the persistent and per-step paths agree to fp32 summation order."""
    torch.manual_seed(3)
    B, T, I, H = 64, 10, 2048, 512
    x = torch.randn(B, T, I, device=dev)
    w_ih = torch.randn(4 * H, I, device=dev) * (2.0 / (I + 4 * H)) ** 0.5
    w_hh = torch.randn(4 * H, H, device=dev) * (2.0 / (H + 4 * H)) ** 0.5
    b_ih = torch.rand(4 * H, device=dev) * 0.08 - 0.04
    b_hh = torch.rand(4 * H, device=dev) * 0.08 - 0.04
    os.environ["TMR_LSTM_PERSIST"] = "1"
    try:
        y1, h1, c1, saved1, ws1 = ops.lstm_fwd(x, w_ih, w_hh, b_ih, b_hh)
        assert ops.lstm_sync_status(ws1) == 0
        dy = torch.randn_like(y1)
        g1 = ops.lstm_bwd(dy, x, w_ih, w_hh, y1, saved1)
        assert ops.lstm_sync_status(g1[-1]) == 0
        os.environ["TMR_LSTM_PERSIST"] = "0"
        y0, h0, c0, saved0, _ = ops.lstm_fwd(x, w_ih, w_hh, b_ih, b_hh)
        g0 = ops.lstm_bwd(dy, x, w_ih, w_hh, y0, saved0)
    finally:
        os.environ.pop("TMR_LSTM_PERSIST", None)
    assert rel(y1, y0) < 1e-5 and rel(c1, c0) < 1e-5
    for a, b in zip(g1[:5], g0[:5]):
        assert rel(a, b) < 1e-4


def _lstm_operands(dev, B=64, T=10, seed=3):
    torch.manual_seed(seed)
    I, H = 2048, 512
    x = torch.randn(B, T, I, device=dev)
    w_ih = torch.randn(4 * H, I, device=dev) * (2.0 / (I + 4 * H)) ** 0.5
    w_hh = torch.randn(4 * H, H, device=dev) * (2.0 / (H + 4 * H)) ** 0.5
    b_ih = torch.rand(4 * H, device=dev) * 0.08 - 0.04
    b_hh = torch.rand(4 * H, device=dev) * 0.08 - 0.04
    return x, w_ih, w_hh, b_ih, b_hh


def _lstm_fwd_bwd(ops_args, dy):
    x, w_ih, w_hh, b_ih, b_hh = ops_args
    y, hn, cn, saved, ws = ops.lstm_fwd(x, w_ih, w_hh, b_ih, b_hh)
    st_f = ops.lstm_sync_status(ws)
    g = ops.lstm_bwd(dy, x, w_ih, w_hh, y, saved)
    st_b = ops.lstm_sync_status(g[-1])
    return [y, hn, cn, saved] + list(g[:5]), st_f, st_b


@pytest.mark.parametrize("B,T", [(64, 10), (64, 30), (5, 7)])
def test_lstm_giveup_recovers(dev, monkeypatch, B, T):
    """A persistent launch that gives up a grid barrier (forced: TMR_LSTM_SPIN_LIMIT=1, so the
    first wait on another workgroup fails) is recomputed on the same stream by the barrier-free
    solo kernels (lstm.hip lstm_rec_{fwd,bwd}_solo_k): every output -- y, h_n, c_n, the saved cell
    states / gate activations, dx, dW, db -- is bit-identical to the run whose barriers all
    completed, the timeout word reads 2 ("recovered") and the health word stays clear."""
    from tmrnet_amd import health
    health.reset()
    monkeypatch.setenv("TMR_LSTM_PERSIST", "1")
    args = _lstm_operands(dev, B, T, seed=B + T)
    dy = torch.randn(B, T, 512, device=dev)
    ref, s0f, s0b = _lstm_fwd_bwd(args, dy)
    assert (s0f, s0b) == (0, 0)
    monkeypatch.setenv("TMR_LSTM_SPIN_LIMIT", "1")
    out, s1f, s1b = _lstm_fwd_bwd(args, dy)
    monkeypatch.delenv("TMR_LSTM_SPIN_LIMIT")
    assert (s1f, s1b) == (2, 2), (s1f, s1b)
    for i, (a, b) in enumerate(zip(out, ref)):
        assert torch.equal(a, b), i
    health.check(sync=True)          # recovered: nothing to report


def test_lstm_next_to_resident_kernel(dev, monkeypatch):
    """the persistent LSTM while another stream holds most of the device's wave
    slots (tmr_test_hold_cus: ~1.5 s of resident workgroups on a side stream, launched first).
    Whether the grid barrier gives up depends on how the dispatcher places the workgroups; either
    way the step must return the same bits as on an idle device and raise nothing -- the recovery
    above is what makes that hold on a shared device.  The status seen is recorded."""
    from tmrnet_amd import health
    health.reset()
    monkeypatch.setenv("TMR_LSTM_PERSIST", "1")
    args = _lstm_operands(dev, 64, 10, seed=77)
    dy = torch.randn(64, 10, 512, device=dev)
    ref, _, _ = _lstm_fwd_bwd(args, dy)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        # two 1024-thread workgroups fill a CU's 32 wave slots; leave 16 CUs free
        call("tmr_test_hold_cus", 2 * (cus - 16), 1500.0, stream_ptr())
    # the LSTM's stream first waits 50 ms (one sleeping workgroup), so the side stream's
    # workgroups are resident when the persistent grid is dispatched
    call("tmr_test_hold_cus", 1, 50.0, stream_ptr())
    out, sf, sb = _lstm_fwd_bwd(args, dy)
    torch.cuda.synchronize()
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "lstm_resident_kernel.json"), "w") as f:
        json.dump({"status_fwd": sf, "status_bwd": sb, "cus": cus}, f)
    assert sf in (0, 2) and sb in (0, 2), (sf, sb)
    for i, (a, b) in enumerate(zip(out, ref)):
        assert torch.equal(a, b), i
    health.check(sync=True)


def test_lstm_giveup_is_loud(dev, monkeypatch):
    """An unrecovered give-up (TMR_LSTM_RECOVER=0 skips the solo re-computation; forced:
    TMR_LSTM_SPIN_LIMIT=1) is reported: the train step's optimizer raises RuntimeError at its next
    step (tmrnet_amd/health.py), and health.check(sync=True) at once -- instead of training on a
    garbage recurrence."""
    import tmrnet_amd
    from tmrnet_amd import health
    health.reset()
    try:
        _giveup_steps(dev, monkeypatch)
    finally:
        health.reset()      # never leave a set health word to the tests that follow


def _giveup_steps(dev, monkeypatch):
    import tmrnet_amd
    from tmrnet_amd import health
    monkeypatch.setenv("TMR_LSTM_PERSIST", "1")
    monkeypatch.setenv("TMR_LSTM_SPIN_LIMIT", "1")
    monkeypatch.setenv("TMR_LSTM_RECOVER", "0")
    torch.manual_seed(5)
    m = tmrnet_amd.LSTM(2048, 512).to(dev)
    opt = tmrnet_amd.SGD(m.parameters(), lr=1e-3, momentum=0.9)
    x = torch.randn(64, 10, 2048, device=dev)
    w0 = [p.detach().clone() for p in m.parameters()]
    y, _ = m(x)
    y.sum().backward()
    opt.step()                      # schedules the status copy of this step
    torch.cuda.synchronize()
    # the failed step's update was skipped on the device (the kernel reads the health word)
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), w0))
    with pytest.raises(RuntimeError, match="gave up a grid barrier"):
        opt.step()                  # ... and raises on it one step later, without a sync
    health.check(sync=True)         # a raised failure clears the word (reported once)
    # inference (no grad): the forward itself waits for the launch and raises at once
    with torch.no_grad(), pytest.raises(RuntimeError, match="gave up a grid barrier"):
        m(x)
    monkeypatch.delenv("TMR_LSTM_SPIN_LIMIT")
    with torch.no_grad():
        m(x)                        # a retry on the healthy device succeeds (no reset needed)
    y, _ = m(x)                     # default limit: no give-up, nothing raised
    y.sum().backward()
    opt.step()
    health.check(sync=True)
    assert not all(torch.equal(p, q) for p, q in zip(m.parameters(), w0))
    with torch.no_grad():
        m(x)


@pytest.mark.parametrize("B,L,rows,D", [
    pytest.param(64, 300, True, 512, id="64-300-True"),
    pytest.param(3, 40, False, 512, id="3-40-False"),
    pytest.param(2, 1, False, 512, id="2-1-False"),
    pytest.param(4, 33, True, 512, id="4-33-True"),
    (3, 40, False, 256), (2, 33, True, 1024), (2, 1, False, 1024), (4, 70, True, 256)])
def test_nl_attn_split(dev, B, L, rows, D):
    """Chunked attention core (32-row chunks + ordered combine) vs float64, incl. a ragged last
    chunk (L=33), L=1 and C5's B=64, L=300 read from a bank through the row table; every
    advertised width (D = 256, 512, 1024: one template instantiation each)."""
    g = torch.Generator().manual_seed(B * 1000 + L)
    u = torch.randn(B, D, generator=g, dtype=torch.float64)
    dctx = torch.randn(B, D, generator=g, dtype=torch.float64)
    if rows:
        bank = torch.rand(5 * L + 7, D, generator=g, dtype=torch.float64) * 2 - 1
        idx = torch.randint(0, bank.shape[0], (B, L), generator=g)
        lt64 = bank[idx]
        lt_d, rows_d = bank.float().to(dev), idx.to(torch.int32).to(dev)
    else:
        lt64 = torch.rand(B, L, D, generator=g, dtype=torch.float64) * 2 - 1
        lt_d, rows_d = lt64.float().to(dev), None
    scale = (1.0 / 512) ** 0.5
    s = torch.einsum("bld,bd->bl", lt64, u) * scale
    p64 = torch.softmax(s, 1)
    ctx64 = torch.einsum("bl,bld->bd", p64, lt64)
    dp = torch.einsum("bld,bd->bl", lt64, dctx)
    ds = scale * p64 * (dp - (p64 * dp).sum(1, keepdim=True))
    ut64 = torch.einsum("bl,bld->bd", ds, lt64)
    dlt64 = p64[:, :, None] * dctx[:, None, :] + ds[:, :, None] * u[:, None, :]
    p, ctx = ops.nl_attn_fwd(lt_d, rows_d, u.float().to(dev), B, L, scale)
    assert rel(p, p64) < 1e-5 and rel(ctx, ctx64) < 1e-5
    ut, dlt = ops.nl_attn_bwd(lt_d, rows_d, u.float().to(dev), p, dctx.float().to(dev), B, L,
                              scale, rows_d is None)
    assert rel(ut, ut64) < 2e-5
    if rows_d is None:
        assert rel(dlt, dlt64) < 2e-5


def _attn_ref(lt64, u, dctx, scale):
    """float64 attention core and its backward (include/tmr.h, tmr_nl_attn_fwd / _bwd)"""
    s = torch.einsum("bld,bd->bl", lt64, u) * scale
    p = torch.softmax(s, 1)
    ctx = torch.einsum("bl,bld->bd", p, lt64)
    dp = torch.einsum("bld,bd->bl", lt64, dctx)
    ds = scale * p * (dp - (p * dp).sum(1, keepdim=True))
    ut = torch.einsum("bl,bld->bd", ds, lt64)
    return s, p, ctx, dp, ut


ATTN_PEAK_MARGIN = 4.0


def _attn_large_score_case(D):
    """(lt, u, dctx), fp32-exact float64: B = 2 clips of L = 77 rows (chunks of 32, 32 and a
    ragged 13 = one full wave + 5 rows) whose scores span about +-60, the clip maximum in the
    last row.  The peak row is the clip's best row moved to the end and shrunk until its score is
    ATTN_PEAK_MARGIN above the runner-up: far above the typical score, so every other chunk is
    rescaled by exp(-4) ... exp(-120) in the combine, yet 1 - p_peak stays near 2e-2.  (ut is
    proportional to 1 - p_peak while the fp32 rounding of dp_peak - sum_k p_k dp_k is not: a
    peak e.g. 12 above the runner-up would leave ut with a relative fp32 error of 1e-3 in any
    implementation.)"""
    B, L = 2, 77
    g = torch.Generator().manual_seed(D)
    u = (torch.randn(B, D, generator=g, dtype=torch.float64) * 45).float().double()
    dctx = torch.randn(B, D, generator=g, dtype=torch.float64).float().double()
    lt = (torch.rand(B, L, D, generator=g, dtype=torch.float64) * 2 - 1).float().double()
    scale = (1.0 / D) ** 0.5
    for _ in range(2):          # the second pass absorbs the fp32 rounding of the shrunk row
        s = torch.einsum("bld,bd->bl", lt, u) * scale
        for b in range(B):
            j = int(s[b].argmax())
            if j != L - 1:
                lt[b, [j, L - 1]] = lt[b, [L - 1, j]]
                s[b, [j, L - 1]] = s[b, [L - 1, j]]
            top, second = s[b, L - 1], s[b, :L - 1].max()
            lt[b, L - 1] = (lt[b, L - 1] * ((second + ATTN_PEAK_MARGIN) / top)).float().double()
    return lt, u, dctx, scale


@pytest.mark.parametrize("D,rows", [(256, False), (512, True), (1024, False)])
def test_nl_attn_large_scores(dev, D, rows):
    """The online-softmax rescale between waves and chunks under stress: scores spanning about
    +-60 with the clip maximum in the last, ragged chunk, at every width.  p, ctx < 1e-5 (the
    bounds of test_nl_attn_split), |sum_l p_l - 1| < 1e-6, ut < 2e-5 of its own magnitude; the
    backward reads the reference's p rounded to fp32."""
    lt64, u, dctx, scale = _attn_large_score_case(D)
    B, L, _ = lt64.shape
    s, p64, ctx64, _, ut64 = _attn_ref(lt64, u, dctx, scale)
    # conditions on the data, from the float64 reference alone
    assert bool((s.argmax(1) == L - 1).all())
    assert float((s.max(1).values - s.min(1).values).min()) > 100.0
    margin = s[:, L - 1] - s[:, :L - 1].max(1).values
    assert bool(((margin - ATTN_PEAK_MARGIN).abs() < 0.05).all())
    assert float((s[:, L - 1] - s[:, :64].max(1).values).min()) > ATTN_PEAK_MARGIN - 0.05
    if rows:
        perm = torch.randperm(B * L, generator=torch.Generator().manual_seed(1))
        bank = torch.empty(B * L, D)
        bank[perm] = lt64.float().view(B * L, D)
        lt_d, rows_d = bank.to(dev), perm.view(B, L).to(torch.int32).to(dev)
    else:
        lt_d, rows_d = lt64.float().to(dev), None
    ud = u.float().to(dev)
    p, ctx = ops.nl_attn_fwd(lt_d, rows_d, ud, B, L, scale)
    assert rel(p, p64) < 1e-5 and rel(ctx, ctx64) < 1e-5
    assert (p.double().sum(1) - 1).abs().max().item() < 1e-6
    ut, dlt = ops.nl_attn_bwd(lt_d, rows_d, ud, p64.float().to(dev), dctx.float().to(dev), B, L,
                              scale, rows_d is None)
    assert rel(ut, ut64) < 2e-5
    if rows_d is None:
        assert bool(torch.isfinite(dlt).all())


def test_nl_attn_equal_scores(dev):
    """Every bank index of a clip is the same row: all scores equal, p = 1/L (L = 50: 1/L is not
    an fp32 number), ctx = that row.  ut vanishes in exact arithmetic (ds_l = scale p_l (dp_l -
    sum_k p_k dp_k) = 0); in fp32 it is bounded by the rounding of the sum against dp, so it is
    held to 2e-5 of the size of its terms, scale * max|dp| * max|row|."""
    B, L, D = 3, 50, 512
    g = torch.Generator().manual_seed(50)
    bank = (torch.rand(20, D, generator=g, dtype=torch.float64) * 2 - 1).float().double()
    u = torch.randn(B, D, generator=g, dtype=torch.float64).float().double()
    dctx = torch.randn(B, D, generator=g, dtype=torch.float64).float().double()
    which = torch.tensor([7, 0, 19])
    idx = which[:, None].expand(B, L).contiguous()
    scale = (1.0 / D) ** 0.5
    _, p64, ctx64, dp, _ = _attn_ref(bank[idx], u, dctx, scale)
    assert (p64 - 1.0 / L).abs().max().item() < 1e-15
    bank_d, rows_d = bank.float().to(dev), idx.to(torch.int32).to(dev)
    p, ctx = ops.nl_attn_fwd(bank_d, rows_d, u.float().to(dev), B, L, scale)
    assert rel(p, p64) < 1e-5 and rel(ctx, ctx64) < 1e-5
    assert (p.double().sum(1) - 1).abs().max().item() < 1e-6
    ut, _ = ops.nl_attn_bwd(bank_d, rows_d, u.float().to(dev), p, dctx.float().to(dev), B, L,
                            scale, False)
    size = scale * dp.abs().max().item() * bank[which].abs().max().item()
    assert ut.abs().max().item() < 2e-5 * size


# seeds 100*L + s, s = 0..3, whose inputs meet the gap condition below (smallest gaps 1.8e-5 ..
# 3.7e-4); L = 7, s = 3 does not (5.7e-7 between x and conv3 at one element) and is left out
TC_SMALL_L = [(L, s) for L in (1, 2, 7) for s in range(4) if (L, s) != (7, 3)]


@pytest.mark.parametrize("L,s", TC_SMALL_L)
def test_timeconv_backward_small_L(dev, L, s):
    """TimeConv forward, x.grad and the six parameter gradients vs TimeConvRef in float64 under
    autograd, where the 7-tap window is mostly padding (L = 1, 2) -- the only rectangular-filter
    (k x 1) use of the conv engine's dgrad / wgrad.  Forward 1e-5 absolute
    (test_timeconv_generalised_L), gradients rel_err < 1e-5 (test_timeconv_golden).
    amax splits the gradient of the structural x / maxpool tie evenly and both shares land on
    x[t], so the float64 gradients agree with the first-maximum rule -- provided no other two
    branches come close: the smallest gap between the top two of (x, y1, y2, y3, prev) is asserted
    to be >= 1e-5 in float64, ten times the forward bound."""
    from tmrnet_amd.timeconv import TimeConv
    torch.manual_seed(100 * L + s)
    r = ref.TimeConvRef()
    x = torch.rand(2, L, 512) * 2 - 1
    dy = torch.randn(2, L, 512)
    m = TimeConv().to(dev)
    m.load_state_dict(r.state_dict())
    r = r.double()
    with torch.no_grad():
        xt = x.double().transpose(1, 2)
        prev = F.pad(xt, (1, 0))[..., :-1]
        top = torch.stack((xt, r.timeconv1(xt), r.timeconv2(xt), r.timeconv3(xt), prev)
                          ).sort(0).values
        assert (top[-1] - top[-2]).min().item() >= 1e-5
    xr = x.double().requires_grad_(True)
    yr = r(xr)
    yr.backward(dy.double())
    xd = x.to(dev).requires_grad_(True)
    y = m(xd)
    y.backward(dy.to(dev))
    assert (y.detach().cpu().double() - yr.detach()).abs().max().item() < 1e-5
    assert rel(xd.grad, xr.grad) < 1e-5
    grads = dict(r.named_parameters())
    for name, p in m.named_parameters():
        assert rel(p.grad, grads[name].grad) < 1e-5, name


def test_linear_bwd_single_row(dev):
    """rows = 1, out = 7: the bias gradient is the column sum of one row (tmr_col_sum's tail
    alone), dW an outer product."""
    g = torch.Generator().manual_seed(17)
    x = torch.randn(1, 1024, generator=g, dtype=torch.float64).float().double()
    w = torch.randn(7, 1024, generator=g, dtype=torch.float64).float().double()
    dy = torch.randn(1, 7, generator=g, dtype=torch.float64).float().double()
    dx, dw, db = ops.linear_bwd(dy.float().to(dev), x.float().to(dev), w.float().to(dev))
    assert rel(db, dy[0]) < 2e-6
    assert rel(dw, dy.t() @ x) < 2e-6
    assert rel(dx, dy @ w) < 2e-6


def test_linear_entry_points(dev):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(37, 1024, generator=g, dtype=torch.float64)
    lin = torch.nn.Linear(1024, 7).double()
    dy = torch.randn(37, 7, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    lin(xr).backward(dy)
    w, b = lin.weight.detach().float().to(dev), lin.bias.detach().float().to(dev)
    y = ops.linear_fwd(x.float().to(dev), w, b)
    assert rel(y, lin(x)) < 2e-6
    dx, dw, db = ops.linear_bwd(dy.float().to(dev), x.float().to(dev), w)
    assert rel(dx, xr.grad) < 2e-6
    assert rel(dw, lin.weight.grad) < 2e-6 and rel(db, lin.bias.grad) < 2e-6
