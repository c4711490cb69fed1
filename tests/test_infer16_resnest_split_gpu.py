"""activations="bf16-resnest" end to end: evaluate_split, build_lfb and OnlineRecognizer on
ResNeSt-50 models of precision "bf16" against the float64 emulation of the trunk
(tests/_infer16_resnest_emu.py) + the oracle's heads."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tmrnet_amd
from tmrnet_amd import evaluate
from tmrnet_amd.lfb import LongFeatureBank
from tmrnet_amd.lfb_build import build_lfb, clip_plan
from tmrnet_amd.stream import OnlineRecognizer
from oracle import tmrnet_ref as ref
from tests._infer16_resnest_emu import randomize_bn, hooked_share, features

pytestmark = pytest.mark.gpu

T, L, LENGTHS = 3, 5, [4, 3]      # 7 frames, 3 valid clips (starts 0, 1, 4), every frame in use
SEED = 15
ACT = "bf16-resnest"


@pytest.fixture(scope="module")
def case(dev):
    torch.manual_seed(SEED)
    m = tmrnet_amd.resnet_lstm(seq_len=T, backbone="resnest50", precision="bf16")
    randomize_bn(m, SEED + 1)
    g = torch.Generator().manual_seed(SEED + 2)
    n = sum(LENGTHS)
    frames = torch.randint(0, 256, (n, 250, 250, 3), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 7, (n,), generator=g)
    torch.manual_seed(SEED + 3)
    f = tmrnet_amd.resnet_lstm_LFB(seq_len=T, backbone="resnest50", precision="bf16")
    randomize_bn(f, SEED + 4)
    valid, used, grow = clip_plan(T, LENGTHS)
    assert list(valid) == [0, 1, 4] and used.size == n
    # the frames as the centre-cropped, normalised network input, once for both emulations
    off = torch.full((1, 2), 13, dtype=torch.int32)
    x = ref.crop_normalize_ref(frames, off, n).view(-1, 3, 224, 224)
    c = {"model": m, "model_lfb": f, "frames": frames, "labels": labels, "valid": list(valid),
         "grow": grow, "x": x}
    m.to(dev).eval()
    f.to(dev).eval()
    return c


def _emulated_feats(model, x):
    """(fp32, float64) features of the 7 frames from the hooked emulation of model.share."""
    e32, e64 = hooked_share(model.state_dict(), "share.")
    return features(e32, x), features(e64, x.double())


def _lstm_rows(model, feat, grow):
    """The oracle LSTM's last-step outputs of the clips (rows `grow` of feat), in feat's dtype."""
    lstm = torch.nn.LSTM(2048, 512, batch_first=True)
    lstm.load_state_dict({k[len("lstm."):]: v.detach().cpu() for k, v in model.state_dict().items()
                          if k.startswith("lstm.")})
    lstm = lstm.to(feat.dtype)
    seq = torch.stack([feat[g:g + T] for g in grow])
    with torch.no_grad():
        y, _ = lstm(seq)
    return y[:, T - 1]


def _criterion(got, out32, out64, what):
    """The bound of test_split_bf16_activations / test_infer16_trunk."""
    e_hip = np.abs(np.asarray(got, dtype=np.float64) - out64.numpy()).max()
    e_cpu = (out32.double() - out64).abs().max().item()
    print("%s: e_hip %.3g e_cpu %.3g max|f64| %.3g" % (what, e_hip, e_cpu, out64.abs().max().item()))
    assert e_hip < max(5e-4 * max(1.0, out64.abs().max().item()), 3 * e_cpu), (what, e_hip, e_cpu)


def test_build_lfb_rows(case, dev):
    """The bank rows against the emulated trunk + the oracle LSTM, and not the default route's."""
    f = case["model_lfb"]
    bank, valid = build_lfb(f, case["frames"], LENGTHS, activations=ACT)
    assert f.share.infer_act16 is False and not f.training
    assert list(valid) == case["valid"] and tuple(bank.shape) == (3, 512)
    bank32, _ = build_lfb(f, case["frames"], LENGTHS)
    assert not torch.equal(bank, bank32)
    f32, f64 = _emulated_feats(f, case["x"])
    _criterion(bank.cpu().numpy(), _lstm_rows(f, f32, case["grow"]),
               _lstm_rows(f, f64, case["grow"]), "bf16-resnest bank rows")
    case["bank"] = bank


def test_split_and_stream(case, dev):
    """evaluate_split's logits against the emulation + the oracle head; one OnlineRecognizer stream
    over the 4-frame video against build_lfb + evaluate_split on that video alone by the rule of
    test_stream_matches_offline (equal predictions, scores and bank rows within 1e-5; the logits
    too), and farther than that from the fp32-activation stream."""
    m, f = case["model"], case["model_lfb"]
    if "bank" not in case:
        case["bank"], _ = build_lfb(f, case["frames"], LENGTHS, activations=ACT)
    bank = LongFeatureBank(case["bank"], case["valid"], L, dev)
    res = evaluate.evaluate_split(m, bank, case["frames"], LENGTHS, case["labels"], activations=ACT)
    assert res["clips"] == 3 and res["frames_encoded"] == 7
    assert m.share.infer_act16 is False and not m.training
    r32 = evaluate.evaluate_split(m, bank, case["frames"], LENGTHS, case["labels"])
    assert not np.array_equal(res["logits"], r32["logits"])   # the switch took effect

    # the emulated logits: hooked trunk, oracle LSTM / non-local block / head, the device's bank
    r = ref.TMRNetRef(seq_len=T, backbone="resnest50").eval()
    r.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    rows = torch.tensor(ref.lfb_index_table(case["valid"], case["valid"], L))
    lt = case["bank"].cpu()[rows]
    f32, f64 = _emulated_feats(m, case["x"])

    def logits(feat):
        rr = r.to(feat.dtype)
        y = _lstm_rows(m, feat, case["grow"])
        with torch.no_grad():
            y1 = rr.nl_block(y, lt.to(feat.dtype))
            return rr.fc_c(F.relu(rr.fc_h_c(torch.cat([y, y1], 1))))

    out32, out64 = logits(f32), logits(f64)
    _criterion(res["logits"], out32, out64, "bf16-resnest split logits")

    # the 4-frame video alone: offline, then streamed frame by frame
    video = case["frames"][:4]
    bank_v, valid_v = build_lfb(f, video, [4], activations=ACT)
    res_v = evaluate.evaluate_split(m, LongFeatureBank(bank_v, valid_v, L, dev), video, [4],
                                    case["labels"][:4], activations=ACT)

    def stream(activations):
        rec = OnlineRecognizer(m, f, L, activations=activations, window="kernel")
        ready, keep = [], {"preds": [], "scores": [], "logits": [], "lfb_rows": []}
        for i in range(4):
            out = rec.push(video[i:i + 1], streams=[0])
            ready.append(bool(out["ready"][0]))
            if ready[-1]:
                for k in keep:
                    keep[k].append(out[k][0].double().cpu())
        assert ready == [False, False, True, True]
        rec.health()
        return {k: torch.stack(v).numpy() for k, v in keep.items()}

    on = stream(ACT)
    assert m.share.infer_act16 is False and f.share.infer_act16 is False
    # no kernel of the route sums over frames, so a frame encoded alone has the bits it has in a
    # batch (test_infer16_resnest_batch_of_one); what is left between the stream and the offline
    # pass is the fp32 heads' summation order: the 1e-5 of test_stream_matches_offline
    d = np.abs(on["scores"] - res_v["scores"]).max()
    dl = np.abs(on["logits"] - res_v["logits"].astype(np.float64)).max()
    db = np.abs(on["lfb_rows"] - bank_v.double().cpu().numpy()).max()
    print("bf16-resnest stream vs evaluate_split: max score diff %.3g, logit diff %.3g, bank row "
          "diff %.3g" % (d, dl, db))
    top2 = -np.sort(-res_v["probs"], axis=1)[:, :2]
    print("bf16-resnest stream: offline margins", top2[:, 0] - top2[:, 1])
    assert on["preds"].tolist() == res_v["preds"].tolist()
    assert d < 1e-5 and dl < 1e-5 and db < 1e-5
    # and the stream took the switch: the fp32-activation stream is farther away than the bound
    on32 = stream("fp32")
    d32 = np.abs(on["logits"] - on32["logits"]).max()
    print("bf16-resnest stream vs fp32-activation stream: max logit diff %.3g" % d32)
    assert d32 > 1e-5
