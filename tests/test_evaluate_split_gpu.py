"""Single-pass split evaluation (tmrnet_amd/evaluate.SplitEvaluator / evaluate_split): every frame
encoded once, against the oracle's restatement of the reference loop
(eval/python/test_singlenet_phase_non-local_pretrained_2fc_copy_mutiConv6_3.py:449-492 and the
validation loss of Training TMRNet/train_only_non-local_pretrained.py:816), against the per-clip
PhaseEvaluator, and the bf16-activation trunk against its float64 emulation."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tmrnet_amd
from tmrnet_amd import ops, evaluate
from tmrnet_amd.lfb import LongFeatureBank
from oracle import tmrnet_ref as ref
from tests._infer16_emu import randomize_bn, hooked_share, features

pytestmark = pytest.mark.gpu

T, L, LENGTHS = 3, 5, [6, 2, 5]          # 13 frames, 7 valid clips, 11 frames in use
WEIGHT = torch.tensor([0.5, 1.0, 2.0, 1.5, 0.7, 1.2, 0.9])   # tests/test_evaluate_gpu.py's
# seeds chosen on the CPU oracle for clear top-2 margins (asserted in the tests that need them)
SEED = 15
SEED_TC = 12
SEED_BF16 = 15


def make_case(seed, lengths=LENGTHS, seq_len=T, lfb_len=L, **model_kw):
    """CPU-side case: model (on the CPU), uint8 frames, labels, valid starts and bank rows."""
    torch.manual_seed(seed)
    m = tmrnet_amd.resnet_lstm(seq_len=seq_len, **model_kw)
    randomize_bn(m, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    n = int(sum(lengths))
    frames = torch.randint(0, 256, (n, 250, 250, 3), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 7, (n,), generator=g)
    valid = ref.get_useful_start_idx(seq_len, lengths)
    bank_np = torch.rand(len(valid), 512, generator=g) * 2 - 1
    return {"model": m, "frames": frames, "labels": labels, "valid": valid, "bank_np": bank_np,
            "T": seq_len, "L": lfb_len, "lengths": list(lengths)}


def clip_inputs(case, clips):
    """The reference loader's view of clips (indices into valid): frames (B*T, ...), centre-crop
    offsets, clip labels labels[s + T - 1], dense long features."""
    Tc = case["T"]
    starts = [case["valid"][i] for i in clips]
    idx = torch.tensor([s + t for s in starts for t in range(Tc)])
    off = torch.full((len(starts), 2), 13, dtype=torch.int32)   # CenterCrop(224) of 250
    lab = case["labels"][idx][Tc - 1::Tc]
    lt = case["bank_np"][torch.tensor(ref.lfb_index_table(starts, case["valid"], case["L"]))]
    return starts, case["frames"][idx], off, lab, lt


def oracle_loop(case, clips, **ref_kw):
    """The reference eval loop on `clips`, restated with the oracle."""
    Tc = case["T"]
    r = ref.TMRNetRef(seq_len=Tc, **ref_kw).eval()
    r.load_state_dict({k: v.detach().cpu() for k, v in case["model"].state_dict().items()})
    _, fr, off, lab, lt = clip_inputs(case, clips)
    with torch.no_grad():
        out = r(ref.crop_normalize_ref(fr, off, Tc).view(len(clips), Tc, 3, 224, 224), lt)
    probs = torch.softmax(out, 1)
    score, pred = torch.max(probs, 1)
    top2 = probs.topk(2, 1).values
    return {"logits": out, "probs": probs, "scores": score.numpy(), "preds": pred.numpy(),
            "labels": lab.numpy(), "margin": (top2[:, 0] - top2[:, 1]).numpy(),
            "loss_sum": F.cross_entropy(probs, lab, weight=WEIGHT, reduction="sum").item(),
            "logit_loss_sum": F.cross_entropy(out, lab, weight=WEIGHT, reduction="sum").item()}


def _on_device(case, dev):
    case["model"].to(dev).eval()
    case["bank"] = LongFeatureBank(case["bank_np"], case["valid"], case["L"], dev)
    return case


@pytest.fixture(scope="module")
def case(dev):
    c = _on_device(make_case(SEED), dev)
    c["res"] = evaluate.evaluate_split(c["model"], c["bank"], c["frames"], LENGTHS, c["labels"],
                                       weight=WEIGHT.to(dev))
    return c


def test_split_matches_reference_loop(case):
    o = oracle_loop(case, range(7))
    res = case["res"]
    assert o["margin"].min() > 1e-3, o["margin"]   # no near-tie behind (or against) the equality
    assert list(res["preds"]) == list(o["preds"])
    print("split vs oracle: max score diff", np.abs(res["scores"] - o["scores"]).max())
    assert np.abs(res["scores"] - o["scores"]).max() < 1e-5
    assert list(res["labels"]) == list(o["labels"])
    assert res["loss_sum"] == pytest.approx(o["loss_sum"], rel=1e-5)
    assert res["logit_loss_sum"] == pytest.approx(o["logit_loss_sum"], rel=1e-5)
    assert res["accuracy"] == pytest.approx(np.mean(o["preds"] == o["labels"]))
    assert res["average_loss"] == pytest.approx(o["loss_sum"] / 7, rel=1e-5)


def test_split_matches_phase_evaluator(case, dev):
    """The per-clip loop on the same 7 clips, fed as two batches; 11 frames encoded, not 21."""
    evl = evaluate.PhaseEvaluator(case["model"], case["bank"], weight=WEIGHT.to(dev))
    for clips in (range(0, 4), range(4, 7)):
        starts, fr, off, lab, _ = clip_inputs(case, clips)
        x4 = ops.crop_normalize(fr.to(dev), off.to(dev), T)
        evl.step(x4, lab.to(dev), clip_starts=starts)
    pe, res = evl.result(), case["res"]
    assert list(res["preds"]) == list(pe["preds"])
    print("split vs PhaseEvaluator: max score diff", np.abs(res["scores"] - pe["scores"]).max())
    assert np.abs(res["scores"] - pe["scores"]).max() < 1e-6
    assert res["loss_sum"] == pytest.approx(pe["loss_sum"], rel=1e-5)
    assert res["frames_encoded"] == 11 and res["clips"] == 7
    assert set(pe) | {"logit_loss_sum", "frames_encoded", "clips"} <= set(res)


def test_split_loader_and_small_chunks(case, dev):
    asked = []

    def loader(first, count):
        asked.append((first, count))
        return case["frames"][first:first + count]

    r2 = evaluate.evaluate_split(case["model"], case["bank"], loader, LENGTHS, case["labels"],
                                 weight=WEIGHT.to(dev), frames_per_launch=4, clips_per_launch=3)
    assert asked == [(0, 4), (4, 2), (8, 4), (12, 1)]   # video 1 (2 frames < T) is never read
    assert list(r2["preds"]) == list(case["res"]["preds"])
    assert np.abs(r2["scores"] - case["res"]["scores"]).max() < 1e-6


def test_split_shards_merge(case, dev):
    """world = 3 by hand; the third shard (clips 5, 6) starts inside video 2: the halo case."""
    parts = [evaluate.evaluate_split(case["model"], case["bank"], case["frames"], LENGTHS,
                                     case["labels"], weight=WEIGHT.to(dev), rank=r, world=3)
             for r in range(3)]
    assert [p["clips"] for p in parts] == [3, 2, 2]
    assert [p["frames_encoded"] for p in parts] == [5, 6, 4]
    full, m = case["res"], evaluate.merge_results(parts)
    assert list(m["preds"]) == list(full["preds"]) and list(m["labels"]) == list(full["labels"])
    assert np.abs(m["scores"] - full["scores"]).max() < 1e-6
    assert m["loss_sum"] == pytest.approx(full["loss_sum"], rel=1e-6)
    assert m["logit_loss_sum"] == pytest.approx(full["logit_loss_sum"], rel=1e-6)
    assert m["corrects"] == full["corrects"] and m["clips"] == 7


def test_split_time_conv(dev):
    """TimeConv variant at its fixed L = 30: one 34-frame video, 32 clips, 4 of them against the
    oracle (the tolerances of the reference-loop test)."""
    c = _on_device(make_case(SEED_TC, lengths=[34], lfb_len=30, time_conv=True), dev)
    res = evaluate.evaluate_split(c["model"], c["bank"], c["frames"], [34], c["labels"],
                                  weight=WEIGHT.to(dev))
    assert res["clips"] == 32 and res["frames_encoded"] == 34
    clips = [0, 9, 20, 31]
    o = oracle_loop(c, clips, time_conv=True)
    assert o["margin"].min() > 1e-3, o["margin"]
    assert list(res["preds"][clips]) == list(o["preds"])
    print("time_conv split vs oracle: max score diff", np.abs(res["scores"][clips] - o["scores"]).max())
    assert np.abs(res["scores"][clips] - o["scores"]).max() < 1e-5
    assert list(res["labels"][clips]) == list(o["labels"])


@pytest.fixture(scope="module")
def case16(dev):
    return _on_device(make_case(SEED_BF16, precision="bf16"), dev)


def _emulated_logits(case, share):
    """Logits of the 7 clips with the trunk replaced by the hooked emulation `share` (the 11 used
    frames encoded once; per-frame in eval mode), the rest of the model the oracle's, in the
    share's dtype."""
    dt = next(share.parameters()).dtype
    r = ref.TMRNetRef(seq_len=T).eval()
    r.load_state_dict({k: v.detach().cpu() for k, v in case["model"].state_dict().items()})
    r = r.to(dt)
    _, used, grow = evaluate.clip_plan(T, LENGTHS)
    off = torch.full((1, 2), 13, dtype=torch.int32)
    x = ref.crop_normalize_ref(case["frames"][torch.from_numpy(used)], off, len(used)).to(dt)
    feat = features(share, x.view(-1, 3, 224, 224))
    _, _, _, _, lt = clip_inputs(case, range(7))
    seq = torch.stack([feat[g:g + T] for g in grow])
    with torch.no_grad():
        y, _ = r.lstm(seq)
        y = y[:, T - 1]
        y1 = r.nl_block(y, lt.to(dt))
        return r.fc_c(F.relu(r.fc_h_c(torch.cat([y, y1], 1))))


def test_split_bf16_activations(case16, dev):
    """activations='bf16' against the same run with bf16 math and fp32 activations (preds, where
    the latter's margin allows) and against the float64 hooked emulation (logits, the bound of
    test_bf16_gpu.test_tmrnet_bf16_eval_logits)."""
    c = case16
    args = (c["model"], c["bank"], c["frames"], LENGTHS, c["labels"])
    r32 = evaluate.evaluate_split(*args, weight=WEIGHT.to(dev))
    r16 = evaluate.evaluate_split(*args, weight=WEIGHT.to(dev), activations="bf16")
    assert r16["frames_encoded"] == 11 and r16["clips"] == 7
    top2 = -np.sort(-r32["probs"], axis=1)[:, :2]
    sure = (top2[:, 0] - top2[:, 1]) > 2e-2
    print("bf16 activations: fp32-activation margins", top2[:, 0] - top2[:, 1])
    assert sure.sum() >= 6, top2
    assert list(r16["preds"][sure]) == list(r32["preds"][sure])
    assert not np.array_equal(r16["logits"], r32["logits"])   # the switch took effect
    e32, e64 = hooked_share(c["model"].state_dict(), "share.")
    out64 = _emulated_logits(c, e64)
    out32 = _emulated_logits(c, e32).double()
    e_hip = np.abs(r16["logits"].astype(np.float64) - out64.numpy()).max()
    e_cpu = (out32 - out64).abs().max().item()
    print("bf16 activations: e_hip %.3g e_cpu %.3g max|out64| %.3g"
          % (e_hip, e_cpu, out64.abs().max().item()))
    assert e_hip < max(5e-4 * max(1.0, out64.abs().max().item()), 3 * e_cpu), (e_hip, e_cpu)


def test_split_restores_flags(case16, dev):
    m = case16["model"]

    def bad_loader(first, count):
        raise OSError("decoder failed")

    m.train()
    try:
        with pytest.raises(OSError):
            evaluate.evaluate_split(m, case16["bank"], bad_loader, LENGTHS, case16["labels"],
                                    activations="bf16")
        assert m.training and m.share.training and m.share.infer_act16 is False
        evaluate.evaluate_split(m, case16["bank"], case16["frames"], LENGTHS, case16["labels"],
                                activations="bf16")
        assert m.training and m.share.infer_act16 is False
        m.eval()
        evaluate.evaluate_split(m, case16["bank"], case16["frames"], LENGTHS, case16["labels"],
                                activations="bf16")
        assert not m.training and m.share.infer_act16 is False
    finally:
        m.eval()


def test_lfb_builder_bf16_activations(case16, dev):
    """LFBBuilder(activations='bf16') runs the switched trunk: its rows are bit-equal to encode +
    recur called by hand with the switch on, differ from the fp32-activation rows, and the
    switch is off again afterwards."""
    from tmrnet_amd import lfb_build
    m = case16["model"]
    b16 = lfb_build.LFBBuilder(m, activations="bf16")
    bank16, valid = b16.build(case16["frames"], LENGTHS)
    assert m.share.infer_act16 is False and not m.training
    bank32, _ = lfb_build.LFBBuilder(m).build(case16["frames"], LENGTHS)
    _, used, grow = lfb_build.clip_plan(T, LENGTHS)
    m.share.infer_act16 = True
    try:
        gates = torch.empty((used.size, 2048), device=dev)
        b16.encode(case16["frames"], used, gates)
        rows = b16.recur(gates, grow, torch.empty((grow.size, 512), device=dev))
    finally:
        m.share.infer_act16 = False
    assert list(valid) == list(case16["valid"])
    assert torch.equal(bank16, rows) and not torch.equal(bank16, bank32)
    assert (bank16 - bank32).abs().max().item() < 0.1   # the same rows, bf16 rounding apart
