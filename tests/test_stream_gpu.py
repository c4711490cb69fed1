"""Online recognition (tmrnet_amd/stream.OnlineRecognizer) and its sliding-window recurrence
(tmr_lstm_window_fwd).

* The kernel against a float64 recurrence over the same gate rows, bit-identity across the ways
  the same clips can lie in a gate table (rotated / wrapped rings, ring capacity, shared rows,
  scattered output), its per-step path and its bounded give-up.
* One stream against the offline path (lfb_build.build_lfb + evaluate.evaluate_split on a split
  that is this one video) and against the oracle's restatement of the reference loops; several
  streams out of lockstep against their single-stream runs; TimeConv, resize, the bf16-activation
  trunk and the restored module flags.
"""
import numpy as np
import pytest
import torch

import tmrnet_amd
from tmrnet_amd import evaluate, frames as tframes, ops
from tmrnet_amd.lfb import LongFeatureBank
from tmrnet_amd.lfb_build import build_lfb
from tmrnet_amd.stream import OnlineRecognizer
from oracle import tmrnet_ref as ref
from tests._infer16_emu import randomize_bn

pytestmark = pytest.mark.gpu

T, L, N = 3, 5, 11
# seeds chosen on the CPU oracle for clear top-2 margins (asserted in the tests that need them)
SEED = 15
SEED_TC = 12
SEED_BF16 = 15


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


# ------------------------------------------------------------------ tmr_lstm_window_fwd
def _operands(dev, nrows, seed, H=512):
    """A gate table and W_hh scaled as test_modules_gpu._lstm_operands: x ~ N(0,1), xavier-normal
    weights, biases in +-0.04; gate rows = x W_ih^T + b_ih + b_hh."""
    torch.manual_seed(seed)
    I = 2048
    x = torch.randn(nrows, I, device=dev)
    w_ih = torch.randn(4 * H, I, device=dev) * (2.0 / (I + 4 * H)) ** 0.5
    w_hh = torch.randn(4 * H, H, device=dev) * (2.0 / (H + 4 * H)) ** 0.5
    b_ih = torch.rand(4 * H, device=dev) * 0.08 - 0.04
    b_hh = torch.rand(4 * H, device=dev) * 0.08 - 0.04
    gates = ops.gemm_nt(x, w_ih, bias=b_ih + b_hh)
    return gates, w_hh


def _recur64(gates, rows, w_hh):
    """float64 nn.LSTM recurrence (gates i,f,g,o; h_0 = c_0 = 0) over gates[rows[b, s]]."""
    g = gates.double().cpu()
    w = w_hh.double().cpu()
    rows = rows.cpu().long()
    B, Tn = rows.shape
    H = w.shape[1]
    h = torch.zeros(B, H, dtype=torch.float64)
    c = torch.zeros(B, H, dtype=torch.float64)
    for s in range(Tn):
        z = g[rows[:, s]] + h @ w.t()
        i, f, gg, o = z.chunk(4, 1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
    return h


def _i32(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32).to(dev)


def _run(gates, rows, w_hh, **kw):
    out, ws = ops.lstm_window_fwd(gates, rows, w_hh, **kw)
    return out, ops.lstm_sync_status(ws)


@pytest.mark.parametrize("B,Tn", [(1, 1), (1, 3), (5, 10), (17, 3)])
def test_window_kernel(dev, monkeypatch, B, Tn):
    """h = 512: 17 clips cross the 16-clip workgroup row.  Clip b is frames b .. b+Tn-1 of one
    video (overlapping clips share gate rows, as in a split's gate table)."""
    monkeypatch.setenv("TMR_LSTM_PERSIST", "1")
    nf = B + Tn - 1
    gates, w_hh = _operands(dev, nf, seed=100 * B + Tn)
    fr = np.arange(B)[:, None] + np.arange(Tn)[None, :]            # frame of (clip, step)
    shared, st = _run(gates, _i32(fr, dev), w_hh)
    assert st == 0
    assert rel(shared, _recur64(gates, torch.from_numpy(fr), w_hh)) < 5e-6
    # every clip with private copies of its rows, densely: the layout tmr_lstm_fwd reads
    dense_g = gates[torch.from_numpy(fr.reshape(-1)).to(dev)].contiguous()
    dense, st = _run(dense_g, _i32(np.arange(B * Tn).reshape(B, Tn), dev), w_hh)
    assert st == 0 and torch.equal(dense, shared)
    # the table rotated: frame f at row (f + shift) % nf, so clips wrap around its end
    shift = nf // 2 + 1
    perm = (np.arange(nf) + shift) % nf
    rot_g = torch.empty_like(gates)
    rot_g[torch.from_numpy(perm).to(dev)] = gates
    rot, st = _run(rot_g, _i32(perm[fr], dev), w_hh)
    assert st == 0 and torch.equal(rot, shared)
    # one ring of Tcap rows per clip, as the recognizer keeps per stream: frame f of clip b at
    # b * Tcap + f % Tcap, for Tcap = Tn (every later clip wraps) and Tn + 3
    for tcap in (Tn, Tn + 3):
        ring_rows = np.arange(B)[:, None] * tcap + fr % tcap
        ring_g = torch.zeros((B * tcap, gates.shape[1]), device=dev)
        ring_g[torch.from_numpy(ring_rows.reshape(-1)).to(dev)] = dense_g
        ring, st = _run(ring_g, _i32(ring_rows, dev), w_hh)
        assert st == 0 and torch.equal(ring, shared), tcap
    # scattered output rows, the rest of the buffer untouched
    orow = (np.arange(B) * 3 + 1) % (B + 3)
    assert np.unique(orow).size == B
    buf = torch.full((B + 3, 512), 7.0, device=dev)
    _, st = _run(gates, _i32(fr, dev), w_hh, out=buf, out_rows=_i32(orow, dev))
    assert st == 0 and torch.equal(buf[torch.from_numpy(orow).to(dev)], shared)
    rest = np.setdiff1d(np.arange(B + 3), orow)
    assert (buf[torch.from_numpy(rest).to(dev)] == 7.0).all()


def test_window_per_step_other_hidden_size(dev):
    """h = 64 has no persistent kernel: gather + gate GEMM + cell kernel per step."""
    B, Tn, H = 2, 3, 64
    torch.manual_seed(5)
    gates = torch.randn(B + Tn - 1, 4 * H, device=dev)
    w_hh = torch.randn(4 * H, H, device=dev) * (2.0 / (5 * H)) ** 0.5
    fr = np.arange(B)[:, None] + np.arange(Tn)[None, :]
    out, st = _run(gates, _i32(fr, dev), w_hh)
    assert st == 0
    assert rel(out, _recur64(gates, torch.from_numpy(fr), w_hh)) < 5e-6
    buf = torch.zeros((4, H), device=dev)
    _run(gates, _i32(fr, dev), w_hh, out=buf, out_rows=_i32([3, 1], dev))
    assert torch.equal(buf[[3, 1]], out) and (buf[[0, 2]] == 0).all()


@pytest.mark.parametrize("B,Tn", [(5, 10), (17, 3)])
def test_window_persistent_vs_per_step(dev, monkeypatch, B, Tn):
    gates, w_hh = _operands(dev, B + Tn - 1, seed=B + Tn)
    rows = _i32(np.arange(B)[:, None] + np.arange(Tn)[None, :], dev)
    monkeypatch.setenv("TMR_LSTM_PERSIST", "1")
    one, st1 = _run(gates, rows, w_hh)
    monkeypatch.setenv("TMR_LSTM_PERSIST", "0")
    steps, st0 = _run(gates, rows, w_hh)
    assert (st1, st0) == (0, 0)
    assert rel(one, steps) < 1e-5
    assert rel(steps, _recur64(gates, rows, w_hh)) < 5e-6


def test_window_giveup_recovers(dev, monkeypatch):
    """After test_modules_gpu.test_lstm_giveup_recovers: a forced give-up of the grid barrier
    (TMR_LSTM_SPIN_LIMIT=1; the kernel exits normally) is recomputed by the solo kernel on the
    same stream: word 2, the same bits, nothing for the health word."""
    from tmrnet_amd import health
    health.reset()
    B, Tn = 5, 10
    monkeypatch.setenv("TMR_LSTM_PERSIST", "1")
    gates, w_hh = _operands(dev, B + Tn - 1, seed=B + Tn)
    rows = _i32(np.arange(B)[:, None] + np.arange(Tn)[None, :], dev)
    orow = _i32([4, 0, 3, 1, 2], dev)
    ref_out, s0 = _run(gates, rows, w_hh, out=torch.zeros((B, 512), device=dev), out_rows=orow)
    monkeypatch.setenv("TMR_LSTM_SPIN_LIMIT", "1")
    out, ws = ops.lstm_window_fwd(gates, rows, w_hh, out=torch.zeros((B, 512), device=dev),
                                  out_rows=orow)
    health.note_lstm(ws)
    s1 = ops.lstm_sync_status(ws)
    monkeypatch.delenv("TMR_LSTM_SPIN_LIMIT")
    assert (s0, s1) == (0, 2), (s0, s1)
    assert torch.equal(out, ref_out)
    health.check(sync=True)


# ------------------------------------------------------------------ OnlineRecognizer
def make_pair(seed, n=N, lfb_len=L, precision="fp32", **model_kw):
    """CPU-side case: a resnet_lstm and a resnet_lstm_LFB of seq_len T with randomised BN, one
    video of n 250 x 250 noise frames (as test_evaluate_split_gpu.make_case) and labels."""
    torch.manual_seed(seed)
    m = tmrnet_amd.resnet_lstm(seq_len=T, precision=precision, **model_kw)
    randomize_bn(m, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    fr = torch.randint(0, 256, (n, 250, 250, 3), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 7, (n,), generator=g)
    torch.manual_seed(seed + 3)
    f = tmrnet_amd.resnet_lstm_LFB(seq_len=T, precision=precision)
    randomize_bn(f, seed + 4)
    return {"model": m, "model_lfb": f, "frames": fr, "labels": labels, "n": n, "L": lfb_len}


def offline(c, dev, activations="fp32"):
    """The offline answer for the case's one video: device-built bank, then evaluate_split."""
    c["model"].to(dev).eval()
    c["model_lfb"].to(dev).eval()
    bank, valid = build_lfb(c["model_lfb"], c["frames"], [c["n"]], activations=activations)
    c["bank"] = bank
    c["res"] = evaluate.evaluate_split(c["model"], LongFeatureBank(bank, valid, c["L"], dev),
                                       c["frames"], [c["n"]], c["labels"],
                                       activations=activations)
    return c


def stream_video(rec, video, stream=0):
    """Push a video frame by frame into one stream -> (ready flags, per-clip outputs stacked)."""
    ready, keep = [], {k: [] for k in ("preds", "scores", "probs", "logits", "lfb_rows")}
    for i in range(video.shape[0]):
        out = rec.push(video[i:i + 1], streams=[stream])
        ready.append(bool(out["ready"][0]))
        if ready[-1]:
            for k in keep:
                keep[k].append(out[k][0])
    return ready, {k: torch.stack(v) for k, v in keep.items()}


@pytest.fixture(scope="module")
def case(dev):
    c = offline(make_pair(SEED), dev)
    rec = OnlineRecognizer(c["model"], c["model_lfb"], L, window="kernel")
    c["ready"], c["online"] = stream_video(rec, c["frames"])
    c["history"] = rec.history(0)
    c["rec"] = rec
    return c


def test_stream_matches_offline(case):
    res, on = case["res"], case["online"]
    assert case["ready"] == [False] * (T - 1) + [True] * (N - T + 1)
    assert case["rec"].age(0) == N
    assert case["history"].dtype == np.int64
    assert case["history"].tolist() == res["preds"].tolist()
    assert on["preds"].cpu().numpy().tolist() == res["preds"].tolist()
    d = np.abs(on["scores"].cpu().numpy() - res["scores"]).max()
    db = (on["lfb_rows"] - case["bank"]).abs().max().item()
    print("stream vs evaluate_split: max score diff %.3g, max bank row diff %.3g" % (d, db))
    assert d < 1e-5
    assert db < 1e-5
    case["rec"].health()


def test_stream_matches_oracle(case):
    """End to end against the reference loops: the oracle's bank (build_lfb_ref) and logits
    (TMRNetRef over lfb_index_table rows) for clips 0 (own-row fallback), 1 (first distinct
    row), 6 and 8 (both sides of the bank ring's wrap at C = L + 1 = 6)."""
    clips = [0, 1, 6, 8]
    rl = ref.LFBModelRef(seq_len=T)
    rl.load_state_dict({k: v.detach().cpu() for k, v in case["model_lfb"].state_dict().items()})
    bank_ref, valid = ref.build_lfb_ref(rl, case["frames"], [N])
    r = ref.TMRNetRef(seq_len=T).eval()
    r.load_state_dict({k: v.detach().cpu() for k, v in case["model"].state_dict().items()})
    idx = torch.tensor([s + t for s in clips for t in range(T)])
    off = torch.full((len(clips), 2), 13, dtype=torch.int32)
    lt = torch.from_numpy(bank_ref).float()[torch.tensor(ref.lfb_index_table(clips, valid, L))]
    with torch.no_grad():
        out = r(ref.crop_normalize_ref(case["frames"][idx], off, T).view(len(clips), T, 3, 224, 224),
                lt)
    probs = torch.softmax(out, 1)
    score, pred = torch.max(probs, 1)
    top2 = probs.topk(2, 1).values
    assert (top2[:, 0] - top2[:, 1]).min().item() > 1e-3, top2
    on = case["online"]
    assert on["preds"].cpu()[clips].tolist() == pred.tolist()
    d = (on["scores"].cpu()[clips] - score).abs().max().item()
    print("stream vs oracle: max score diff %.3g" % d)
    assert d < 1e-5


def test_stream_steps_vs_kernel(case):
    rec = OnlineRecognizer(case["model"], case["model_lfb"], L, window="steps")
    ready, on = stream_video(rec, case["frames"])
    assert ready == case["ready"]
    assert torch.equal(on["preds"], case["online"]["preds"])
    d = (on["scores"] - case["online"]["scores"]).abs().max().item()
    print("window steps vs kernel: max score diff %.3g" % d)
    assert d < 1e-6
    assert rec.history(0).tolist() == case["history"].tolist()


def test_two_streams_out_of_lockstep(case, dev):
    """Stream 0 carries the 11-frame video; stream 1 starts two ticks later with a 6-frame
    video, is reset, then carries a 4-frame video; pushes carry one or both streams, in either
    order.  Every video's outputs are those of its own single-stream run."""
    g = torch.Generator().manual_seed(SEED + 9)
    vb = torch.randint(0, 256, (6, 250, 250, 3), generator=g, dtype=torch.uint8)
    vc = torch.randint(0, 256, (4, 250, 250, 3), generator=g, dtype=torch.uint8)
    va = case["frames"]
    single = {"a": case["online"]}
    for name, v in (("b", vb), ("c", vc)):
        _, single[name] = stream_video(
            OnlineRecognizer(case["model"], case["model_lfb"], L, window="kernel"), v)
    rec = OnlineRecognizer(case["model"], case["model_lfb"], L, streams=2, window="kernel")
    plan = [[0], [0], [0, 1], [1, 0], [0, 1], [1], [0, 1], [1], "reset",
            [0, 1], [0, 1], [1, 0], [0, 1], [0]]
    nxt = {0: 0, 1: 0}
    vid = {0: ("a", va), 1: ("b", vb)}
    got = {k: {"preds": [], "scores": []} for k in "abc"}
    for ids in plan:
        if ids == "reset":
            assert rec.age(1) == 6
            rec.reset(1)
            assert rec.age(1) == 0 and rec.age(0) == 6
            vid[1], nxt[1] = ("c", vc), 0
            continue
        batch = torch.stack([vid[i][1][nxt[i]] for i in ids])
        out = rec.push(batch, streams=ids)
        for k, i in enumerate(ids):
            assert bool(out["ready"][k]) == (nxt[i] + 1 >= T)
            if out["ready"][k]:
                got[vid[i][0]]["preds"].append(out["preds"][k])
                got[vid[i][0]]["scores"].append(out["scores"][k])
            nxt[i] += 1
    assert nxt == {0: 11, 1: 4}
    for name in "abc":
        p, s = torch.stack(got[name]["preds"]), torch.stack(got[name]["scores"])
        assert torch.equal(p, single[name]["preds"]), name
        d = (s - single[name]["scores"]).abs().max().item()
        print("two streams, video %s: max score diff %.3g" % (name, d))
        assert d < 1e-6, name
    # history runs across the reset, video after video: what export_phase takes
    assert rec.history(0).tolist() == case["history"].tolist()
    assert rec.history(1).tolist() == (single["b"]["preds"].cpu().tolist()
                                       + single["c"]["preds"].cpu().tolist())


def test_stream_time_conv(dev):
    """TimeConv at its fixed L = 30: one 34-frame video (test_split_time_conv's geometry)."""
    c = offline(make_pair(SEED_TC, n=34, lfb_len=30, time_conv=True), dev)
    rec = OnlineRecognizer(c["model"], c["model_lfb"], 30, window="kernel")
    ready, on = stream_video(rec, c["frames"])
    assert sum(ready) == 32 and c["res"]["clips"] == 32
    assert on["preds"].cpu().numpy().tolist() == c["res"]["preds"].tolist()
    d = np.abs(on["scores"].cpu().numpy() - c["res"]["scores"]).max()
    print("time_conv stream vs evaluate_split: max score diff %.3g" % d)
    assert d < 1e-5


def test_stream_resizes_frames(case, dev):
    """Frames of another size go through frames.resize_frames: the same bits as resizing first."""
    g = torch.Generator().manual_seed(SEED + 5)
    small = torch.randint(0, 256, (4, 48, 64, 3), generator=g, dtype=torch.uint8)
    big = tframes.resize_frames(small.to(dev), tframes.RESIZE)
    assert tuple(big.shape) == (4, 250, 250, 3)
    _, a = stream_video(OnlineRecognizer(case["model"], case["model_lfb"], L, window="kernel"),
                        small)
    _, b = stream_video(OnlineRecognizer(case["model"], case["model_lfb"], L, window="kernel"),
                        big)
    assert a["preds"].shape[0] == 2
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def case16(dev):
    return offline(make_pair(SEED_BF16, precision="bf16"), dev, activations="bf16")


def test_stream_restores_flags(case16, dev):
    m, f = case16["model"], case16["model_lfb"]
    rec = OnlineRecognizer(m, f, L, activations="bf16", window="kernel")

    def bad_loader(ids):
        raise OSError("decoder failed")

    m.train()
    try:
        with pytest.raises(OSError):
            rec.push(bad_loader)
        assert m.training and m.share.training and not f.training
        assert m.share.infer_act16 is False and f.share.infer_act16 is False
        assert rec.age(0) == 0
        rec.push(case16["frames"][:1])
        assert m.training and not f.training and rec.age(0) == 1
        assert m.share.infer_act16 is False and f.share.infer_act16 is False
        m.eval()
        rec.push(lambda ids: case16["frames"][1:2])
        assert not m.training and m.share.infer_act16 is False and rec.age(0) == 2
    finally:
        m.eval()


def test_stream_bf16_activations(case16, dev):
    """activations='bf16' against evaluate_split(activations='bf16') on the bank built the same
    way: equal predictions wherever the offline margin exceeds 2e-2 (the "sure" rule of
    test_split_bf16_activations)."""
    res = case16["res"]
    rec = OnlineRecognizer(case16["model"], case16["model_lfb"], L, activations="bf16",
                           window="kernel")
    ready, on = stream_video(rec, case16["frames"])
    assert sum(ready) == N - T + 1
    top2 = -np.sort(-res["probs"], axis=1)[:, :2]
    sure = (top2[:, 0] - top2[:, 1]) > 2e-2
    print("bf16 stream: offline margins", top2[:, 0] - top2[:, 1])
    assert sure.any(), top2
    assert on["preds"].cpu().numpy()[sure].tolist() == res["preds"][sure].tolist()
    assert case16["model"].share.infer_act16 is False
